// The per-lane body of xvit_augment_apply (include/xvit.h, "Augmenting input stage"), shared by augment.hip and elastic.hip: where a lane
// sits in its brick, the exact copy, the trilinear tap at a source coordinate, and what follows the sample (clamp window, a v + b, noise,
// one rounding, the store).  xvit_augment_apply_elastic runs a sample whose flag is 0 through aug_apply_lane, the very code of
// augment_apply_kernel, and a deformed sample through aug_trilinear and aug_finish_run with its own coordinates.
#pragma once
#include <math.h>

#include "volume_io.h"

namespace xvit {

struct AugGeom {
  int Ds, Hs, Ws, D, H, W;
  int od, oh, ow;   // the pad / crop offsets of xvit_resize_pad_crop_i16: source index = destination index + offset
};

// standard normal for voxel `idx` of a volume: Box-Muller on two 24-bit draws
__device__ __forceinline__ float normal_at(uint32_t noise_seed, uint32_t idx) {
  const float u1 = (float)(draw24(noise_seed, 2ull * idx) + 1u) * kInv24;        // (0, 1]
  const float u2 = uniform01(noise_seed, 2ull * idx + 1);
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// A 256-thread workgroup owns a brick of (8 << lx) x (64 >> lx) x 4 destination voxels (x, y, z): a wave is one z-slice of it, 1 << lx
// lanes along x with 8 voxels each.  Neighbouring lanes and waves read neighbouring source voxels, so the 8 taps of the general path hit
// lines the brick has already pulled into L1 / L2.
struct AugLane {
  int vol, bx, by, bz;   // the volume and the brick inside it: workgroup-uniform
  int x0, y, z, n;       // the lane's run: n of its 8 voxels lie inside the destination
  bool inside;           // false: the lane has no voxel
};

__device__ __forceinline__ AugLane aug_locate(const AugGeom& g, int lx, int nbx, int nby, int nbz) {
  AugLane L;
  const int per_vol = nbx * nby * nbz;
  const int logical = xcd_logical(blockIdx.x, gridDim.x);   // consecutive bricks (shared source halos) on one XCD's L2
  L.vol = logical / per_vol;
  int brick = logical - L.vol * per_vol;
  L.bx = brick % nbx;
  brick /= nbx;
  L.by = brick % nby, L.bz = brick / nby;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  L.x0 = ((L.bx << lx) + (lane & ((1 << lx) - 1))) * 8;
  L.y = L.by * (64 >> lx) + (lane >> lx);
  L.z = L.bz * 4 + wave;
  L.inside = !(L.x0 >= g.W || L.y >= g.H || L.z >= g.D);
  L.n = min(8, g.W - L.x0);
  return L;
}

// exact path: the source voxel at the integer index (a flip is a reversed run)
template <typename S>
__device__ __forceinline__ void aug_exact_run(const S* __restrict__ sv, const float* __restrict__ P, const AugGeom& g, const AugLane& L, float pad_value,
                                              float (&v)[8]) {
  const int fz = (int)P[0], fy = (int)P[5], fx = (int)P[10];   // +-1
  const int sz = fz * L.z + (int)P[3], sy = fy * L.y + (int)P[7];
  const int sx_first = fx * L.x0 + (int)P[11];
  const bool row_in = sz >= 0 && sz < g.Ds && sy >= 0 && sy < g.Hs;
  const S* __restrict__ row = sv + ((int64_t)(row_in ? sz : 0) * g.Hs + (row_in ? sy : 0)) * g.Ws;
  const int lo = fx > 0 ? sx_first : sx_first - 7;   // lowest source x of a full run
  if (row_in && lo >= 0 && lo <= g.Ws - 8) {
    float t[8];
    load_run8(row + lo, t);
    for (int i = 0; i < 8; ++i) v[i] = fx > 0 ? t[i] : t[7 - i];
  } else {
    for (int i = 0; i < 8; ++i) {
      const int sx = sx_first + fx * i;
      const bool in = row_in && sx >= 0 && sx < g.Ws;
      const float t = src_f(row[in ? sx : 0]);   // always a valid address: the load needs no branch
      v[i] = in ? t : pad_value;
    }
  }
}

// general path: trilinear interpolation at the source coordinate (qz, qy, qx), voxels outside the volume counting as pad_value
template <typename S>
__device__ __forceinline__ float aug_trilinear(const S* __restrict__ sv, const AugGeom& g, float qz, float qy, float qx, float pad_value) {
  // beyond [-2, size + 1] every tap is outside: clamping there changes no result and keeps the integer conversion defined
  const float hz = (float)g.Ds + 1.f, hy = (float)g.Hs + 1.f, hx = (float)g.Ws + 1.f;
  const float pz = fminf(fmaxf(qz, -2.f), hz), py = fminf(fmaxf(qy, -2.f), hy);
  const float px = fminf(fmaxf(qx, -2.f), hx);
  const float flz = floorf(pz), fly = floorf(py), flx = floorf(px);
  const float wz = pz - flz, wy = py - fly, wx = px - flx;
  const int iz = (int)flz, iy = (int)fly, ix = (int)flx;
  float tap[8];
  for (int k = 0; k < 8; ++k) {
    const int tz = iz + (k >> 2), ty = iy + ((k >> 1) & 1), tx = ix + (k & 1);
    const bool in = tz >= 0 && tz < g.Ds && ty >= 0 && ty < g.Hs && tx >= 0 && tx < g.Ws;
    const float t = src_f(sv[in ? ((uint32_t)tz * g.Hs + ty) * g.Ws + tx : 0u]);   // < 2^31 inside the volume; a valid address either way
    tap[k] = in ? t : pad_value;
  }
  const float c00 = fmaf(wx, tap[1] - tap[0], tap[0]), c01 = fmaf(wx, tap[3] - tap[2], tap[2]);
  const float c10 = fmaf(wx, tap[5] - tap[4], tap[4]), c11 = fmaf(wx, tap[7] - tap[6], tap[6]);
  const float c0 = fmaf(wy, c01 - c00, c00), c1 = fmaf(wy, c11 - c10, c10);
  return fmaf(wz, c1 - c0, c0);
}

// The affine source coordinate of a lane's run, p = A (z, y, x) + t: the x-independent part of every row once, then one fmaf per voxel.
struct AugAffine {
  float bz0, by0, bx0, az, ay, ax;
  __device__ __forceinline__ AugAffine(const float* __restrict__ P, const AugLane& L) {
    const float fzc = (float)L.z, fyc = (float)L.y;
    bz0 = fmaf(P[0], fzc, fmaf(P[1], fyc, P[3])), by0 = fmaf(P[4], fzc, fmaf(P[5], fyc, P[7])), bx0 = fmaf(P[8], fzc, fmaf(P[9], fyc, P[11]));
    az = P[2], ay = P[6], ax = P[10];
  }
  __device__ __forceinline__ void at(float xf, float& pz, float& py, float& px) const {
    pz = fmaf(az, xf, bz0), py = fmaf(ay, xf, by0), px = fmaf(ax, xf, bx0);
  }
};

template <typename S>
__device__ __forceinline__ void aug_general_run(const S* __restrict__ sv, const float* __restrict__ P, const AugGeom& g, const AugLane& L, float pad_value,
                                                float (&v)[8]) {
  const AugAffine aff(P, L);
  for (int i = 0; i < 8; ++i) {
    float pz, py, px;
    aff.at((float)(L.x0 + i), pz, py, px);
    v[i] = aug_trilinear(sv, g, pz, py, px, pad_value);
  }
}

// behind the sample: the optional clamp window, a v + b, noise, one rounding, the store
template <typename T>
__device__ __forceinline__ void aug_finish_run(const float* __restrict__ P, int flags, const AugGeom& g, const AugLane& L, T* __restrict__ dst, float (&v)[8]) {
  const float a = P[XVIT_AUG_SCALE], b = P[XVIT_AUG_SHIFT], sigma = P[XVIT_AUG_SIGMA];
  const uint32_t noise_seed = __builtin_bit_cast(uint32_t, P[XVIT_AUG_NOISE_SEED]);
  const uint32_t vox0 = ((uint32_t)L.z * g.H + L.y) * g.W + L.x0;   // < 2^31 by the host check
  T* __restrict__ out = dst + (int64_t)L.vol * g.D * g.H * g.W + vox0;

  if ((flags & XVIT_AUG_FLAG_CLAMP) != 0) {   // xvit_volume_stats' window, in source units: padding lands on its floor
    const float lo = P[XVIT_AUG_CLAMP_LO], hi = P[XVIT_AUG_CLAMP_HI];
    for (int i = 0; i < 8; ++i) v[i] = fminf(fmaxf(v[i], lo), hi);
  }
  for (int i = 0; i < 8; ++i) v[i] = fmaf(a, v[i], b);
  if (sigma > 0.f)
    for (int i = 0; i < 8; ++i) v[i] = fmaf(sigma, normal_at(noise_seed, vox0 + i), v[i]);

  if (L.n == 8 && ((uintptr_t)out & 15) == 0) {
    store_run8(out, v);
  } else {
    for (int i = 0; i < 8; ++i)
      if (i < L.n) store_one(out + i, v[i]);
  }
}

// one lane of xvit_augment_apply: L.inside holds
template <typename S, typename T>
__device__ __forceinline__ void aug_apply_lane(const S* __restrict__ src, T* __restrict__ dst, const float* __restrict__ P, const AugGeom& g, const AugLane& L,
                                               float pad_value) {
  const int flags = (int)P[XVIT_AUG_FLAGS];
  const S* __restrict__ sv = src + (int64_t)L.vol * g.Ds * g.Hs * g.Ws;
  float v[8];
  if ((flags & XVIT_AUG_FLAG_EXACT) != 0)
    aug_exact_run(sv, P, g, L, pad_value, v);
  else
    aug_general_run(sv, P, g, L, pad_value, v);
  aug_finish_run(P, flags, g, L, dst, v);
}

// ---- host side: geometry, the argument checks and the launch shape both entry points share ----
static inline AugGeom make_geom(int Ds, int Hs, int Ws, int D, int H, int W) {
  // per dimension: size < target -> pad, before = (target - size) / 2; size > target -> crop, start = size / 2 - target / 2
  auto offset = [](int size, int target) { return size >= target ? size / 2 - target / 2 : -((target - size) / 2); };
  return AugGeom{Ds, Hs, Ws, D, H, W, offset(Ds, D), offset(Hs, H), offset(Ws, W)};
}

static inline bool sizes_ok(int Ds, int Hs, int Ws, int D, int H, int W) { return Ds > 0 && Hs > 0 && Ws > 0 && D > 0 && H > 0 && W > 0; }
static inline bool volume_ok(int d, int h, int w) { return (int64_t)d * h * w < (1ll << 31); }

struct AugBricks {
  int lx, nbx, nby, nbz;
  explicit AugBricks(const AugGeom& g) {
    lx = g.W > 64 ? 4 : g.W > 32 ? 3 : 2;   // 16, 8 or 4 lanes along x
    nbx = (g.W + (8 << lx) - 1) / (8 << lx), nby = (g.H + (64 >> lx) - 1) / (64 >> lx), nbz = (g.D + 3) / 4;
  }
  unsigned blocks(int nvol) const { return (unsigned)(nbx * nby * nbz * nvol); }
};

// The refusals of xvit_augment_apply, under the caller's name.
#define XVIT_AUG_APPLY_REQUIRE(who)                                                                                                                          \
  XVIT_REQUIRE(src && dst && params, who ": null source, destination or parameter table");                                                                   \
  XVIT_REQUIRE(src_dtype == XVIT_I16 || src_dtype == XVIT_BF16 || src_dtype == XVIT_F32, who ": unknown source dtype %d", src_dtype);                        \
  XVIT_REQUIRE(dst_dtype == XVIT_BF16 || dst_dtype == XVIT_F32, who ": unknown destination dtype %d", dst_dtype);                                            \
  XVIT_REQUIRE(nvol > 0 && xvit::sizes_ok(Ds, Hs, Ws, D, H, W), who ": non-positive size (nvol %d, source %d x %d x %d, destination %d x %d x %d)", nvol, Ds, \
               Hs, Ws, D, H, W);                                                                                                                             \
  XVIT_REQUIRE(xvit::volume_ok(Ds, Hs, Ws) && xvit::volume_ok(D, H, W), who ": a volume must have fewer than 2^31 voxels");                                  \
  XVIT_REQUIRE(((uintptr_t)params & 15) == 0, who ": the parameter table must be 16-byte aligned");                                                          \
  XVIT_REQUIRE((uintptr_t)src % (src_dtype == XVIT_F32 ? 4 : 2) == 0 && (uintptr_t)dst % (dst_dtype == XVIT_F32 ? 4 : 2) == 0,                               \
               who ": source or destination not aligned to its element size");                                                                               \
  /* bricks are at least 32 x 4 x 4 voxels, so the block count stays far below 2^31 for any table the draw kernel accepts */                                 \
  XVIT_REQUIRE((int64_t)nvol * ((W + 31) / 32) * ((H + 3) / 4) * ((D + 3) / 4) < (1ll << 31), who ": too many bricks for one launch")

}  // namespace xvit
