// What the kernels between the volumes and the token rows share (misc.hip, token_select.hip, mae.hip, mix.hip): the patch order in both
// directions, typed runs of VEC elements, the ordered compaction round, the row mover and the (row, column) decode of a row walk.
#pragma once
#include "volume_io.h"

namespace xvit {

// ---- the patch order ---------------------------------------------------------------------------------------------------------------------
// A contiguous [B, M, 1, D, H, W] volume tensor with patch (dp, hp, wp) has Dn Hn Wn patches per volume, Dn = D / dp and so on.  Voxel
// (d dp + p1, h hp + p2, w wp + p3) is feature f of patch (token) t with
//     t = (h Wn + w) Dn + d,    f = (p1 hp + p2) wp + p3      (reference model_cross.py:193)
// and sequence s = m B + b holds the patches of modality m of sample b.  A run of VEC features from f on (VEC divides wp, and f) stays
// inside one W-run of the volume and inside one patch row.  The two functions below are the only statements of this order outside
// gemm.hip's gather loaders.

// Volume and patch, and how many rows of a sequence the caller selects (K kept, or Rm dropped)
struct TokenGeom { int B, M, D, H, W, dp, hp, wp, n; };
__device__ __forceinline__ int patch_count(const TokenGeom& g) { return (g.D / g.dp) * (g.H / g.hp) * (g.W / g.wp); }

// (s, t, f) -> element index in the volume tensor
__device__ __forceinline__ int64_t voxel_index(const TokenGeom& g, int s, int t, int f) {
  const int Dn = g.D / g.dp, Wn = g.W / g.wp;
  const int m = s / g.B, b = s - m * g.B;
  const int d = t % Dn, hw = t / Dn, w = hw % Wn, h = hw / Wn;
  const int p3 = f % g.wp, p12 = f / g.wp, p2 = p12 % g.hp, p1 = p12 / g.hp;
  return ((((int64_t)b * g.M + m) * g.D + (d * g.dp + p1)) * g.H + (h * g.hp + p2)) * g.W + (w * g.wp + p3);
}

// The other direction, for a whole-volume walk: the VEC voxels at linear volume index idx * VEC -> element index of the first in a patch
// matrix whose row (b, m, t) is row b stride_b + m stride_m + t + row_off.
struct PatchGeom { int M, D, H, W, dp, hp, wp; int64_t stride_b, stride_m; int row_off; };
template <int VEC>
__device__ __forceinline__ int64_t patch_elem(const PatchGeom& g, int64_t idx) {
  const int Wv = g.W / VEC;
  const int Dn = g.D / g.dp, Wn = g.W / g.wp;
  const int wv = (int)(idx % Wv);
  int64_t r = idx / Wv;
  const int hh = (int)(r % g.H); r /= g.H;
  const int dd = (int)(r % g.D); r /= g.D;
  const int vol = (int)r;  // b*M + m
  const int b = vol / g.M, m = vol - b * g.M;
  const int w0 = wv * VEC;
  const int w = w0 / g.wp, p3 = w0 - w * g.wp;
  const int h = hh / g.hp, p2 = hh - h * g.hp;
  const int d = dd / g.dp, p1 = dd - d * g.dp;
  const int t = (h * Wn + w) * Dn + d;
  const int f = (p1 * g.hp + p2) * g.wp + p3;
  return ((int64_t)b * g.stride_b + (int64_t)m * g.stride_m + t + g.row_off) * (g.dp * g.hp * g.wp) + f;
}

// ---- runs of VEC = 8 | 1 elements (volume_io.h); the 8-element forms need 16-byte aligned addresses ---------------------------------------
template <int VEC, typename S>
__device__ __forceinline__ void load_run(const S* p, float (&v)[VEC]) {
  if constexpr (VEC == 8) load_run8_aligned(p, v);
  else v[0] = src_f(*p);
}
template <int VEC, typename D>
__device__ __forceinline__ void store_run(D* p, const float (&v)[VEC]) {
  if constexpr (VEC == 8) store_run8(p, v);
  else store_one(p, v[0]);
}
template <int VEC, typename D, typename S>
__device__ __forceinline__ void copy_run(D* dst, const S* src) {
  if constexpr (VEC == 8) copy_run8(dst, src);
  else store_one(dst, src_f(*src));
}

// ---- one round of an ordered compaction -----------------------------------------------------------------------------------------------
// Every thread of a BLOCK-thread workgroup brings one flag.  Returns base + the number of set flags in the threads below this one (the
// ascending position of this thread's element, if its flag is set) and advances base, the same in every thread, by the round's total:
// a ballot prefix inside each wave, the waves' totals through wave_tot[BLOCK / kWave] in LDS.  The trailing barrier keeps the next
// round from rewriting wave_tot while it is read.
template <int BLOCK>
__device__ __forceinline__ int compact_round(bool flag, int* wave_tot, int& base) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const uint64_t vote = __ballot(flag);
  const int in_wave = __popcll(vote & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[wave] = __popcll(vote);
  __syncthreads();
  int before = 0, round = 0;
  for (int w = 0; w < BLOCK / kWave; ++w) {
    const int t = wave_tot[w];
    before += w < wave ? t : 0;
    round += t;
  }
  const int pos = base + before + in_wave;
  base += round;
  __syncthreads();
  return pos;
}

// ---- fp32 token rows, 4 features (16 bytes) per thread --------------------------------------------------------------------------------
// Work item i of a walk over [rows, 4 dv] -> its row and first column
struct RowCol { int64_t row; int c; };
__device__ __forceinline__ RowCol row_col(int64_t i, int dv) { return {i / dv, (int)(i % dv) * 4}; }

// out[row] = in[map(row)], or a zero row where map(row) < 0: every output row written once.  Map: int64_t operator()(int64_t row) const.
template <class Map>
__global__ void move_rows_kernel(const float* __restrict__ in, float* __restrict__ out, const Map map, int dd, int64_t total) {
  const int dv = dd >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const auto [row, c] = row_col(i, dv);
    const int64_t from = map(row);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (from >= 0) v = *(const f32x4*)(in + from * dd + c);
    *(f32x4*)(out + row * dd + c) = v;
  }
}

}  // namespace xvit
