// Augmenting input stage (include/xvit.h, "Augmenting input stage"): xvit_augment_draw fills one 32-float record per volume from a
// config and a seed; xvit_augment_apply resamples every volume through its record.  The random numbers live in the table only, so the
// kernel that touches the voxels is a pure function of (src, table).
#include <math.h>

#include "augment_apply.h"

namespace xvit {

// ------------------------------------------------------------------------------------------
// draw: one block; thread i serves volumes i, i + 256, ...  Every thread reads the counter before the barrier, one thread advances it
// after it (a plain store), so all records of a launch see the same call index.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) augment_draw_kernel(xvit_augment_config c, float* __restrict__ params, int B, int M, AugGeom g, uint64_t seed,
                                                           uint64_t* counter, int advance) {
  const uint64_t count = counter ? *counter : 0;
  const uint64_t s = draw_seed(seed, count, 0);   // the first stream under a seed: no salt
  __syncthreads();
  if (advance && threadIdx.x == 0) *counter = count + 1;

  for (int vol = threadIdx.x; vol < B * M; vol += blockDim.x) {
    const uint64_t sp = 64ull * (uint64_t)(vol / M);   // spatial draws: by sample, never by modality
    const uint64_t in = 64ull * (uint64_t)vol + 32;    // intensity draws: by volume

    float flip[3], ang[3] = {0.f, 0.f, 0.f}, zoom[3] = {1.f, 1.f, 1.f}, tr[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k) flip[k] = uniform01(s, sp + k) < c.flip_prob[k] ? 1.f : 0.f;
    if (uniform01(s, sp + 3) < c.rotate_prob)
      for (int k = 0; k < 3; ++k) ang[k] = uniform_in(s, sp + 4 + k, -c.rotate_range[k], c.rotate_range[k]);
    if (uniform01(s, sp + 7) < c.zoom_prob)
      for (int k = 0; k < 3; ++k) zoom[k] = uniform_in(s, sp + 8 + k, c.zoom_range[0], c.zoom_range[1]);
    if (uniform01(s, sp + 11) < c.translate_prob)
      for (int k = 0; k < 3; ++k) tr[k] = uniform_in(s, sp + 12 + k, -c.translate_range[k], c.translate_range[k]);

    float fac = 1.f, shift = 0.f, sigma = 0.f;
    if (uniform01(s, in + 0) < c.scale_prob) fac = uniform_in(s, in + 1, c.scale_range[0], c.scale_range[1]);
    if (uniform01(s, in + 2) < c.shift_prob) shift = uniform_in(s, in + 3, c.shift_range[0], c.shift_range[1]);
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
template <typename S, typename T>
__global__ void __launch_bounds__(256) augment_apply_kernel(const S* __restrict__ src, T* __restrict__ dst, const float* __restrict__ params, AugGeom g,
                                                            int lx, int nbx, int nby, int nbz, float pad_value) {
  const AugLane L = aug_locate(g, lx, nbx, nby, nbz);
  if (!L.inside) return;   // no barrier below
  aug_apply_lane(src, dst, params + (int64_t)L.vol * XVIT_AUG_NPARAM, g, L, pad_value);   // the record is wave-uniform: scalar loads
}

}  // namespace xvit

extern "C" int xvit_augment_draw(const xvit_augment_config* config, float* params, int B, int M, int Ds, int Hs, int Ws, int D, int H, int W, uint64_t seed,
                                 uint64_t* counter, int advance, xvit_stream_t stream) {
  XVIT_REQUIRE(config && params, "xvit_augment_draw: null config or parameter table");
  XVIT_REQUIRE(B > 0 && M > 0 && (int64_t)B * M < (1 << 24), "xvit_augment_draw: B=%d, M=%d must be positive (and B M < 2^24)", B, M);
  XVIT_REQUIRE(xvit::sizes_ok(Ds, Hs, Ws, D, H, W), "xvit_augment_draw: non-positive size (source %d x %d x %d, destination %d x %d x %d)", Ds, Hs, Ws, D, H, W);
  XVIT_REQUIRE(((uintptr_t)params & 15) == 0, "xvit_augment_draw: the parameter table must be 16-byte aligned");
  XVIT_REQUIRE_COUNTER("xvit_augment_draw", counter, advance);
  const xvit_augment_config& c = *config;
  const auto prob = xvit::prob_ok;
  XVIT_REQUIRE(prob(c.flip_prob[0]) && prob(c.flip_prob[1]) && prob(c.flip_prob[2]) && prob(c.rotate_prob) && prob(c.zoom_prob) && prob(c.translate_prob) &&
                   prob(c.scale_prob) && prob(c.shift_prob) && prob(c.noise_prob),
               "xvit_augment_draw: every probability must lie in [0, 1]");
  for (int k = 0; k < 3; ++k)
    XVIT_REQUIRE(c.rotate_range[k] >= 0.f && c.translate_range[k] >= 0.f && isfinite(c.rotate_range[k]) && isfinite(c.translate_range[k]),
                 "xvit_augment_draw: rotate_range and translate_range are half-widths: finite and >= 0");
  XVIT_REQUIRE(c.zoom_range[0] > 0.f && xvit::range_ok(c.zoom_range[0], c.zoom_range[1]), "xvit_augment_draw: zoom_range (%g, %g) is reversed or not positive",
               c.zoom_range[0], c.zoom_range[1]);
  XVIT_REQUIRE(xvit::range_ok(c.scale_range[0], c.scale_range[1]), "xvit_augment_draw: scale_range (%g, %g) is reversed", c.scale_range[0], c.scale_range[1]);
  XVIT_REQUIRE(xvit::range_ok(c.shift_range[0], c.shift_range[1]), "xvit_augment_draw: shift_range (%g, %g) is reversed", c.shift_range[0], c.shift_range[1]);
  XVIT_REQUIRE(c.noise_std >= 0.f && isfinite(c.noise_std), "xvit_augment_draw: noise_std=%g must be finite and >= 0", c.noise_std);
  XVIT_REQUIRE(isfinite(c.intensity_scale) && isfinite(c.intensity_shift), "xvit_augment_draw: the fixed intensity affine must be finite");
  hipLaunchKernelGGL(xvit::augment_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, c, params, B, M, xvit::make_geom(Ds, Hs, Ws, D, H, W), seed, counter,
                     advance);
  return xvit::check_launch("xvit_augment_draw");
}

extern "C" int xvit_augment_apply(const void* src, int src_dtype, void* dst, int dst_dtype, const float* params, int nvol, int Ds, int Hs, int Ws, int D, int H,
                                  int W, float pad_value, xvit_stream_t stream) {
  XVIT_AUG_APPLY_REQUIRE("xvit_augment_apply");
  const xvit::AugGeom g = xvit::make_geom(Ds, Hs, Ws, D, H, W);
  const xvit::AugBricks b(g);
  xvit::by_src_dtype(src_dtype, [&](auto sd) {
    xvit::by_dtype(dst_dtype, [&](auto dd) {
      using S = decltype(sd);
      using T = decltype(dd);
      hipLaunchKernelGGL((xvit::augment_apply_kernel<S, T>), dim3(b.blocks(nvol)), dim3(256), 0, (hipStream_t)stream, (const S*)src, (T*)dst, params, g, b.lx,
                         b.nbx, b.nby, b.nbz, pad_value);
    });
  });
  return xvit::check_launch("xvit_augment_apply");
}
