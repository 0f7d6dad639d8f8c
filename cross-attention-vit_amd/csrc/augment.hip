// Augmenting input stage (include/xvit.h, "Augmenting input stage"): xvit_augment_draw fills one 32-float record per volume from a
// config and a seed; xvit_augment_apply resamples every volume through its record.  The random numbers live in the table only, so the
// kernel that touches the voxels is a pure function of (src, table).
#include <math.h>

#include "xvit_common.h"

namespace xvit {

constexpr uint64_t kCounterStride = 0xD1B54A32D192ED03ull;   // the odd constant of drop_seed_at
constexpr float kInv24 = 1.0f / kTwo24;

__device__ __forceinline__ float uniform01(uint64_t seed, uint64_t idx) { return (float)draw24(seed, idx) * kInv24; }   // [0, 1), exact

struct AugGeom {
  int Ds, Hs, Ws, D, H, W;
  int od, oh, ow;   // the pad / crop offsets of xvit_resize_pad_crop_i16: source index = destination index + offset
};

// ------------------------------------------------------------------------------------------
// draw: one block; thread i serves volumes i, i + 256, ...  Every thread reads the counter before the barrier, one thread advances it
// after it (a plain store), so all records of a launch see the same call index.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) augment_draw_kernel(xvit_augment_config c, float* __restrict__ params, int B, int M, AugGeom g, uint64_t seed,
                                                           uint64_t* counter, int advance) {
  const uint64_t count = counter ? *counter : 0;
  const uint64_t s = seed + count * kCounterStride;
  __syncthreads();
  if (advance && threadIdx.x == 0) *counter = count + 1;

  for (int vol = threadIdx.x; vol < B * M; vol += blockDim.x) {
    const uint64_t sp = 64ull * (uint64_t)(vol / M);   // spatial draws: by sample, never by modality
    const uint64_t in = 64ull * (uint64_t)vol + 32;    // intensity draws: by volume
    auto range = [&](uint64_t i, float lo, float hi) { return fminf(fmaxf(fmaf(uniform01(s, i), hi - lo, lo), lo), hi); };

    float flip[3], ang[3] = {0.f, 0.f, 0.f}, zoom[3] = {1.f, 1.f, 1.f}, tr[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k) flip[k] = uniform01(s, sp + k) < c.flip_prob[k] ? 1.f : 0.f;
    if (uniform01(s, sp + 3) < c.rotate_prob)
      for (int k = 0; k < 3; ++k) ang[k] = range(sp + 4 + k, -c.rotate_range[k], c.rotate_range[k]);
    if (uniform01(s, sp + 7) < c.zoom_prob)
      for (int k = 0; k < 3; ++k) zoom[k] = range(sp + 8 + k, c.zoom_range[0], c.zoom_range[1]);
    if (uniform01(s, sp + 11) < c.translate_prob)
      for (int k = 0; k < 3; ++k) tr[k] = range(sp + 12 + k, -c.translate_range[k], c.translate_range[k]);

    float fac = 1.f, shift = 0.f, sigma = 0.f;
    if (uniform01(s, in + 0) < c.scale_prob) fac = range(in + 1, c.scale_range[0], c.scale_range[1]);
    if (uniform01(s, in + 2) < c.shift_prob) shift = range(in + 3, c.shift_range[0], c.shift_range[1]);
    if (uniform01(s, in + 4) < c.noise_prob) sigma = c.noise_std * ((float)(draw24(s, in + 5) + 1u) * kInv24);
    const uint32_t noise_seed = hash32(s, in + 6);

    // L = F Rz Ry Rx diag(1 / zoom) in double from the recorded fp32 draws, rounded once
    const double cz = cos((double)ang[0]), sz = sin((double)ang[0]), cy = cos((double)ang[1]), sy = sin((double)ang[1]);
    const double cx = cos((double)ang[2]), sx = sin((double)ang[2]);
    const double Rz[3][3] = {{1, 0, 0}, {0, cz, -sz}, {0, sz, cz}}, Ry[3][3] = {{cy, 0, sy}, {0, 1, 0}, {-sy, 0, cy}};
    const double Rx[3][3] = {{cx, -sx, 0}, {sx, cx, 0}, {0, 0, 1}};
    double T[3][3], L[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) T[i][j] = Ry[i][0] * Rx[0][j] + Ry[i][1] * Rx[1][j] + Ry[i][2] * Rx[2][j];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        L[i][j] = (flip[i] != 0.f ? -1.0 : 1.0) * (Rz[i][0] * T[0][j] + Rz[i][1] * T[1][j] + Rz[i][2] * T[2][j]) / (double)zoom[j];
    const double ctr[3] = {0.5 * (g.D - 1), 0.5 * (g.H - 1), 0.5 * (g.W - 1)};
    const int off[3] = {g.od, g.oh, g.ow};

    float* __restrict__ P = params + (int64_t)vol * XVIT_AUG_NPARAM;
    bool exact = true;
    for (int i = 0; i < 3; ++i) {
      const double t = ctr[i] + off[i] + (double)tr[i] - (L[i][0] * ctr[0] + L[i][1] * ctr[1] + L[i][2] * ctr[2]);
      for (int j = 0; j < 3; ++j) {
        const float a = (float)L[i][j];
        P[XVIT_AUG_MATRIX + 4 * i + j] = a;
        exact = exact && (i == j ? fabsf(a) == 1.f : a == 0.f);
      }
      const float tf = (float)t;
      P[XVIT_AUG_MATRIX + 4 * i + 3] = tf;
      exact = exact && tf == rintf(tf) && fabsf(tf) < 1e9f;
    }
    P[XVIT_AUG_SCALE] = fac * c.intensity_scale;
    P[XVIT_AUG_SHIFT] = fmaf(fac, c.intensity_shift, shift);
    P[XVIT_AUG_SIGMA] = sigma;
    P[XVIT_AUG_NOISE_SEED] = __builtin_bit_cast(float, noise_seed);
    P[XVIT_AUG_FLAGS] = exact ? (float)XVIT_AUG_FLAG_EXACT : 0.f;
    for (int k = 0; k < 3; ++k) {
      P[XVIT_AUG_FLIPS + k] = flip[k];
      P[XVIT_AUG_ANGLES + k] = ang[k];
      P[XVIT_AUG_ZOOMS + k] = zoom[k];
      P[XVIT_AUG_TRANSLATION + k] = tr[k];
      P[29 + k] = 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------
// apply
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float src_f(int16_t v) { return (float)v; }
__device__ __forceinline__ float src_f(bf16 v) { return bf2f(v); }
__device__ __forceinline__ float src_f(float v) { return v; }

// 8 consecutive source elements at any element-aligned address (the crop offset decides the alignment, not the kernel)
template <typename S>
__device__ __forceinline__ void load_run8(const S* p, float (&v)[8]) {
  struct Run { S e[8]; } r;
  __builtin_memcpy(&r, __builtin_assume_aligned(p, sizeof(S)), sizeof(r));
  for (int i = 0; i < 8; ++i) v[i] = src_f(r.e[i]);
}

__device__ __forceinline__ void store_run8(bf16* p, const float (&v)[8]) {
  bf16x8 o;
  for (int i = 0; i < 8; ++i) o[i] = f2bf(v[i]);
  *(bf16x8*)p = o;
}
__device__ __forceinline__ void store_run8(float* p, const float (&v)[8]) {
  *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
  *(f32x4*)(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
}
__device__ __forceinline__ void store_one(bf16* p, float v) { *p = f2bf(v); }
__device__ __forceinline__ void store_one(float* p, float v) { *p = v; }

// standard normal for voxel `idx` of a volume: Box-Muller on two 24-bit draws
__device__ __forceinline__ float normal_at(uint32_t noise_seed, uint32_t idx) {
  const float u1 = (float)(draw24(noise_seed, 2ull * idx) + 1u) * kInv24;        // (0, 1]
  const float u2 = (float)draw24(noise_seed, 2ull * idx + 1) * kInv24;           // [0, 1)
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// A 256-thread workgroup owns a brick of (8 << lx) x (64 >> lx) x 4 destination voxels (x, y, z): a wave is one z-slice of it, 1 << lx
// lanes along x with 8 voxels each.  Neighbouring lanes and waves read neighbouring source voxels, so the 8 taps of the general path hit
// lines the brick has already pulled into L1 / L2.
template <typename S, typename T>
__global__ void __launch_bounds__(256) augment_apply_kernel(const S* __restrict__ src, T* __restrict__ dst, const float* __restrict__ params, AugGeom g,
                                                            int lx, int nbx, int nby, int nbz, float pad_value) {
  const int per_vol = nbx * nby * nbz;
  const int logical = xcd_logical(blockIdx.x, gridDim.x);   // consecutive bricks (shared source halos) on one XCD's L2
  const int vol = logical / per_vol;
  int brick = logical - vol * per_vol;
  const int bx = brick % nbx;
  brick /= nbx;
  const int by = brick % nby, bz = brick / nby;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = ((bx << lx) + (lane & ((1 << lx) - 1))) * 8;
  const int y = by * (64 >> lx) + (lane >> lx);
  const int z = bz * 4 + wave;
  if (x0 >= g.W || y >= g.H || z >= g.D) return;   // no barrier below
  const int n = min(8, g.W - x0);

  const float* __restrict__ P = params + (int64_t)vol * XVIT_AUG_NPARAM;   // wave-uniform: scalar loads
  const float a = P[XVIT_AUG_SCALE], b = P[XVIT_AUG_SHIFT], sigma = P[XVIT_AUG_SIGMA];
  const uint32_t noise_seed = __builtin_bit_cast(uint32_t, P[XVIT_AUG_NOISE_SEED]);
  const int flags = (int)P[XVIT_AUG_FLAGS];
  const bool exact = (flags & XVIT_AUG_FLAG_EXACT) != 0, clamp = (flags & XVIT_AUG_FLAG_CLAMP) != 0;

  const S* __restrict__ sv = src + (int64_t)vol * g.Ds * g.Hs * g.Ws;
  const uint32_t vox0 = ((uint32_t)z * g.H + y) * g.W + x0;   // < 2^31 by the host check
  T* __restrict__ out = dst + (int64_t)vol * g.D * g.H * g.W + vox0;

  float v[8];
  if (exact) {
    const int fz = (int)P[0], fy = (int)P[5], fx = (int)P[10];   // +-1
    const int sz = fz * z + (int)P[3], sy = fy * y + (int)P[7];
    const int sx_first = fx * x0 + (int)P[11];
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
  } else {
    const float fzc = (float)z, fyc = (float)y;
    // the x-independent part of every row of A (z, y, x) + t
    const float bz0 = fmaf(P[0], fzc, fmaf(P[1], fyc, P[3])), by0 = fmaf(P[4], fzc, fmaf(P[5], fyc, P[7])), bx0 = fmaf(P[8], fzc, fmaf(P[9], fyc, P[11]));
    const float az = P[2], ay = P[6], ax = P[10];
    // beyond [-2, size + 1] every tap is outside: clamping there changes no result and keeps the integer conversion defined
    const float hz = (float)g.Ds + 1.f, hy = (float)g.Hs + 1.f, hx = (float)g.Ws + 1.f;
    for (int i = 0; i < 8; ++i) {
      const float xf = (float)(x0 + i);
      const float pz = fminf(fmaxf(fmaf(az, xf, bz0), -2.f), hz), py = fminf(fmaxf(fmaf(ay, xf, by0), -2.f), hy);
      const float px = fminf(fmaxf(fmaf(ax, xf, bx0), -2.f), hx);
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
      v[i] = fmaf(wz, c1 - c0, c0);
    }
  }

  if (clamp) {   // xvit_volume_stats' window, in source units: padding lands on its floor
    const float lo = P[XVIT_AUG_CLAMP_LO], hi = P[XVIT_AUG_CLAMP_HI];
    for (int i = 0; i < 8; ++i) v[i] = fminf(fmaxf(v[i], lo), hi);
  }
  for (int i = 0; i < 8; ++i) v[i] = fmaf(a, v[i], b);
  if (sigma > 0.f)
    for (int i = 0; i < 8; ++i) v[i] = fmaf(sigma, normal_at(noise_seed, vox0 + i), v[i]);

  if (n == 8 && ((uintptr_t)out & 15) == 0) {
    store_run8(out, v);
  } else {
    for (int i = 0; i < 8; ++i)
      if (i < n) store_one(out + i, v[i]);
  }
}

template <typename S, typename T>
static void launch_apply(const void* src, void* dst, const float* params, int nvol, const AugGeom& g, float pad_value, hipStream_t s) {
  const int lx = g.W > 64 ? 4 : g.W > 32 ? 3 : 2;   // 16, 8 or 4 lanes along x
  const int nbx = (g.W + (8 << lx) - 1) / (8 << lx), nby = (g.H + (64 >> lx) - 1) / (64 >> lx), nbz = (g.D + 3) / 4;
  hipLaunchKernelGGL((augment_apply_kernel<S, T>), dim3((unsigned)(nbx * nby * nbz * nvol)), dim3(256), 0, s, (const S*)src, (T*)dst, params, g, lx, nbx,
                     nby, nbz, pad_value);
}

static AugGeom make_geom(int Ds, int Hs, int Ws, int D, int H, int W) {
  // per dimension: size < target -> pad, before = (target - size) / 2; size > target -> crop, start = size / 2 - target / 2
  auto offset = [](int size, int target) { return size >= target ? size / 2 - target / 2 : -((target - size) / 2); };
  return AugGeom{Ds, Hs, Ws, D, H, W, offset(Ds, D), offset(Hs, H), offset(Ws, W)};
}

static bool sizes_ok(int Ds, int Hs, int Ws, int D, int H, int W) { return Ds > 0 && Hs > 0 && Ws > 0 && D > 0 && H > 0 && W > 0; }
static bool volume_ok(int d, int h, int w) { return (int64_t)d * h * w < (1ll << 31); }

}  // namespace xvit

extern "C" int xvit_augment_draw(const xvit_augment_config* config, float* params, int B, int M, int Ds, int Hs, int Ws, int D, int H, int W, uint64_t seed,
                                 uint64_t* counter, int advance, xvit_stream_t stream) {
  XVIT_REQUIRE(config && params, "xvit_augment_draw: null config or parameter table");
  XVIT_REQUIRE(B > 0 && M > 0 && (int64_t)B * M < (1 << 24), "xvit_augment_draw: B=%d, M=%d must be positive (and B M < 2^24)", B, M);
  XVIT_REQUIRE(xvit::sizes_ok(Ds, Hs, Ws, D, H, W), "xvit_augment_draw: non-positive size (source %d x %d x %d, destination %d x %d x %d)", Ds, Hs, Ws, D, H, W);
  XVIT_REQUIRE(((uintptr_t)params & 15) == 0, "xvit_augment_draw: the parameter table must be 16-byte aligned");
  XVIT_REQUIRE(((uintptr_t)counter & 7) == 0, "xvit_augment_draw: the counter must be 8-byte aligned");
  XVIT_REQUIRE(counter || !advance, "xvit_augment_draw: advance needs a counter");
  const xvit_augment_config& c = *config;
  auto prob = [](float p) { return p >= 0.f && p <= 1.f; };   // false for NaN
  XVIT_REQUIRE(prob(c.flip_prob[0]) && prob(c.flip_prob[1]) && prob(c.flip_prob[2]) && prob(c.rotate_prob) && prob(c.zoom_prob) && prob(c.translate_prob) &&
                   prob(c.scale_prob) && prob(c.shift_prob) && prob(c.noise_prob),
               "xvit_augment_draw: every probability must lie in [0, 1]");
  for (int k = 0; k < 3; ++k)
    XVIT_REQUIRE(c.rotate_range[k] >= 0.f && c.translate_range[k] >= 0.f && isfinite(c.rotate_range[k]) && isfinite(c.translate_range[k]),
                 "xvit_augment_draw: rotate_range and translate_range are half-widths: finite and >= 0");
  XVIT_REQUIRE(c.zoom_range[0] > 0.f && c.zoom_range[0] <= c.zoom_range[1] && isfinite(c.zoom_range[1]),
               "xvit_augment_draw: zoom_range (%g, %g) is reversed or not positive", c.zoom_range[0], c.zoom_range[1]);
  XVIT_REQUIRE(c.scale_range[0] <= c.scale_range[1] && isfinite(c.scale_range[0]) && isfinite(c.scale_range[1]),
               "xvit_augment_draw: scale_range (%g, %g) is reversed", c.scale_range[0], c.scale_range[1]);
  XVIT_REQUIRE(c.shift_range[0] <= c.shift_range[1] && isfinite(c.shift_range[0]) && isfinite(c.shift_range[1]),
               "xvit_augment_draw: shift_range (%g, %g) is reversed", c.shift_range[0], c.shift_range[1]);
  XVIT_REQUIRE(c.noise_std >= 0.f && isfinite(c.noise_std), "xvit_augment_draw: noise_std=%g must be finite and >= 0", c.noise_std);
  XVIT_REQUIRE(isfinite(c.intensity_scale) && isfinite(c.intensity_shift), "xvit_augment_draw: the fixed intensity affine must be finite");
  hipLaunchKernelGGL(xvit::augment_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, c, params, B, M, xvit::make_geom(Ds, Hs, Ws, D, H, W), seed, counter,
                     advance);
  return xvit::check_launch("xvit_augment_draw");
}

extern "C" int xvit_augment_apply(const void* src, int src_dtype, void* dst, int dst_dtype, const float* params, int nvol, int Ds, int Hs, int Ws, int D, int H,
                                  int W, float pad_value, xvit_stream_t stream) {
  XVIT_REQUIRE(src && dst && params, "xvit_augment_apply: null source, destination or parameter table");
  XVIT_REQUIRE(src_dtype == XVIT_I16 || src_dtype == XVIT_BF16 || src_dtype == XVIT_F32, "xvit_augment_apply: unknown source dtype %d", src_dtype);
  XVIT_REQUIRE(dst_dtype == XVIT_BF16 || dst_dtype == XVIT_F32, "xvit_augment_apply: unknown destination dtype %d", dst_dtype);
  XVIT_REQUIRE(nvol > 0 && xvit::sizes_ok(Ds, Hs, Ws, D, H, W), "xvit_augment_apply: non-positive size (nvol %d, source %d x %d x %d, destination %d x %d x %d)",
               nvol, Ds, Hs, Ws, D, H, W);
  XVIT_REQUIRE(xvit::volume_ok(Ds, Hs, Ws) && xvit::volume_ok(D, H, W), "xvit_augment_apply: a volume must have fewer than 2^31 voxels");
  XVIT_REQUIRE(((uintptr_t)params & 15) == 0, "xvit_augment_apply: the parameter table must be 16-byte aligned");
  const int src_size = src_dtype == XVIT_F32 ? 4 : 2, dst_size = dst_dtype == XVIT_F32 ? 4 : 2;
  XVIT_REQUIRE((uintptr_t)src % src_size == 0 && (uintptr_t)dst % dst_size == 0, "xvit_augment_apply: source or destination not aligned to its element size");
  const xvit::AugGeom g = xvit::make_geom(Ds, Hs, Ws, D, H, W);
  // bricks are at least 32 x 4 x 4 voxels, so the block count stays far below 2^31 for any table the draw kernel accepts
  XVIT_REQUIRE((int64_t)nvol * ((W + 31) / 32) * ((H + 3) / 4) * ((D + 3) / 4) < (1ll << 31), "xvit_augment_apply: too many bricks for one launch");
  hipStream_t s = (hipStream_t)stream;
#define XVIT_AUG_CASE(SD, S, DD, T) \
  if (src_dtype == SD && dst_dtype == DD) xvit::launch_apply<S, T>(src, dst, params, nvol, g, pad_value, s)
  XVIT_AUG_CASE(XVIT_I16, int16_t, XVIT_BF16, xvit::bf16);
  XVIT_AUG_CASE(XVIT_I16, int16_t, XVIT_F32, float);
  XVIT_AUG_CASE(XVIT_BF16, xvit::bf16, XVIT_BF16, xvit::bf16);
  XVIT_AUG_CASE(XVIT_BF16, xvit::bf16, XVIT_F32, float);
  XVIT_AUG_CASE(XVIT_F32, float, XVIT_BF16, xvit::bf16);
  XVIT_AUG_CASE(XVIT_F32, float, XVIT_F32, float);
#undef XVIT_AUG_CASE
  return xvit::check_launch("xvit_augment_apply");
}
