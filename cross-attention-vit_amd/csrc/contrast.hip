// Contrast stage (include/xvit.h, "Contrast augmentations"): xvit_contrast_draw fills one 32-float record per volume from a config and a
// seed; xvit_contrast_apply runs every volume through its record: separable Gaussian blur, multiplicative bias field, gamma, one rounding.
// As in augment.hip the random numbers live in the table only: the kernel that touches the voxels is a pure function of (src, table).
#include <math.h>

#include "volume_io.h"

namespace xvit {

constexpr uint64_t kConSalt = 0x434F4E5452415354ull;     // "CONTRAST": keeps this stream apart from xvit_augment_draw's under one seed

constexpr int TX = 64, TY = 16;                          // destination tile of a workgroup (x, y); it marches along z
constexpr int RMAX = XVIT_CON_MAX_RADIUS, NRING = 2 * RMAX + 1;
constexpr int RAW_H = TY + 2 * RMAX, RAW_W = TX + 16;    // source plane tile: a halo of RMAX rows, and of one 8-voxel run either side
constexpr int LDS_RAW = 0, LDS_XB = LDS_RAW + RAW_H * RAW_W, LDS_RING = LDS_XB + RAW_H * TX, LDS_WGT = LDS_RING + NRING * TX * TY;
constexpr int LDS_FLOATS = LDS_WGT + 3 * 16;
constexpr int LDS_BYTES = LDS_FLOATS * 4;                // 69 568
constexpr int POINT_UNROLL = 4;                          // 16-byte runs a lane keeps in flight on the pointwise path

// ------------------------------------------------------------------------------------------
// draw: one block; thread i serves volumes i, i + 256, ...  The counter is read by every thread before the barrier and advanced by one
// thread after it, as in augment_draw_kernel.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) contrast_draw_kernel(xvit_contrast_config c, float* __restrict__ params, int nvol, uint64_t seed, uint64_t* counter,
                                                            int advance) {
  const uint64_t count = counter ? *counter : 0;
  const uint64_t s = draw_seed(seed, count, kConSalt);
  __syncthreads();
  if (advance && threadIdx.x == 0) *counter = count + 1;

  for (int vol = threadIdx.x; vol < nvol; vol += blockDim.x) {
    const uint64_t i0 = 64ull * (uint64_t)vol;

    float* __restrict__ P = params + (int64_t)vol * XVIT_CON_NPARAM;
    int flags = 0;
    const float ublur = uniform01(s, i0 + 0), ubias = uniform01(s, i0 + 4), ugamma = uniform01(s, i0 + 14);
    float sigma[3] = {0.f, 0.f, 0.f}, beta = 0.f, coeff[9];
    for (int k = 0; k < 9; ++k) coeff[k] = 0.f;
    if (ublur < c.blur_prob) {
      flags |= XVIT_CON_FLAG_BLUR;
      for (int k = 0; k < 3; ++k) sigma[k] = uniform_in(s, i0 + (c.blur_isotropic ? 1 : 1 + k), c.blur_sigma_range[0], c.blur_sigma_range[1]);
    }
    if (ubias < c.bias_prob) {
      flags |= XVIT_CON_FLAG_BIAS;
      for (int k = 0; k < 9; ++k) coeff[k] = uniform_in(s, i0 + 5 + k, -c.bias_coeff, c.bias_coeff);
    }
    if (ugamma < c.gamma_prob) {
      flags |= XVIT_CON_FLAG_GAMMA;
      beta = uniform_in(s, i0 + 15, c.log_gamma_range[0], c.log_gamma_range[1]);
    }
    P[XVIT_CON_FLAGS] = (float)flags;
    for (int k = 0; k < 3; ++k) {
      P[XVIT_CON_SIGMA + k] = sigma[k];
      P[XVIT_CON_RADIUS + k] = sigma[k] > 0.f ? fminf(ceilf(3.f * sigma[k]), (float)RMAX) : 0.f;
    }
    P[XVIT_CON_GAMMA] = (float)exp((double)beta);   // 1 when not drawn
    P[XVIT_CON_WINDOW_LO] = c.gamma_window[0];
    P[XVIT_CON_WINDOW_HI] = c.gamma_window[1];
    for (int k = 0; k < 9; ++k) P[XVIT_CON_BIAS + k] = coeff[k];
    P[XVIT_CON_U_BLUR] = ublur;
    P[XVIT_CON_U_BIAS] = ubias;
    P[XVIT_CON_U_GAMMA] = ugamma;
    P[XVIT_CON_BETA] = beta;
    for (int k = XVIT_CON_BETA + 1; k < XVIT_CON_NPARAM; ++k) P[k] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------
// apply
// ------------------------------------------------------------------------------------------
// t^g for t in [0, 1], g > 0, without powf: measured against float64, powf(1e-30f, 0.74f) was 19 ulp off, and a power's relative error
// is its exponent's absolute one.  So: t = m 2^e with m in [2^-1/2, 2^1/2), the exponent g (e + log2f(m)) formed in double (log2f's 1 ulp
// of |log2 m| <= 0.5 is all that is lost), split into n + f, 2^f from exp2f and 2^n from ldexpf.  t = 1: m = 1, e = 0, exactly 1.
__device__ __forceinline__ float pow_unit(float t, float g) {
  if (t == 0.f) return 0.f;
  int e;
  float m = frexpf(t, &e);
  if (m < 0.70710678f) m *= 2.f, --e;
  const double E = (double)g * ((double)e + (double)log2f(m));
  const double n = fmin(fmax(rint(E), -400.0), 400.0);
  return ldexpf(exp2f((float)(E - n)), (int)n);
}

// What follows the blur, per voxel: v exp(c . m(u)), then the gamma curve inside the window.  Everything here is wave-uniform but v and u.
struct PointOps {
  int flags;
  float c[9];            // z, y, x, z^2, y^2, x^2, zy, zx, yx
  float g, lo, span;     // gamma, window floor, hi - lo
  float kz, ky, kx;      // 2 / (n - 1), or 0 when n = 1 (u = 0 there)

  __device__ __forceinline__ static float coord(int i, float k) { return k != 0.f ? fmaf((float)i, k, -1.f) : 0.f; }
  // the part of the exponent that one row (z, y) shares
  __device__ __forceinline__ float row_part(float uz, float uy) const {
    return fmaf(uz, fmaf(c[3], uz, c[0]), uy * fmaf(c[4], uy, fmaf(c[6], uz, c[1])));
  }
  __device__ __forceinline__ float apply(float v, float row_e, float uz, float uy, float ux) const {
    if (flags & XVIT_CON_FLAG_BIAS) {
      const float e = fmaf(ux, fmaf(c[5], ux, fmaf(c[7], uz, fmaf(c[8], uy, c[2]))), row_e);
      v *= expf(e);
    }
    if (flags & XVIT_CON_FLAG_GAMMA) {
      const float t = (v - lo) / span;
      if (t >= 0.f && t <= 1.f) v = fmaf(span, pow_unit(t, g), lo);   // false for NaN: it passes through
    }
    return v;
  }
};

template <typename S, typename T>
__global__ void __launch_bounds__(256) contrast_apply_kernel(const S* __restrict__ src, T* __restrict__ dst, const float* __restrict__ params, int D, int H, int W,
                                                             int ntx, int nty, int nseg) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int ntile = ntx * nty * nseg;
  const int logical = xcd_logical(blockIdx.x, gridDim.x);   // neighbouring tiles of one volume (shared halos) on one XCD's L2
  const int vol = logical / ntile;
  int tile = logical - vol * ntile;
  const int tid = threadIdx.x;
  const uint32_t nvox = (uint32_t)D * H * W;                 // < 2^31 by the host check

  const float* __restrict__ P = params + (int64_t)vol * XVIT_CON_NPARAM;   // wave-uniform: scalar loads
  PointOps ops;
  ops.flags = (int)fminf(fmaxf(P[XVIT_CON_FLAGS], 0.f), 1048576.f) & 7;    // NaN -> 0
  for (int k = 0; k < 9; ++k) ops.c[k] = P[XVIT_CON_BIAS + k];
  ops.g = P[XVIT_CON_GAMMA], ops.lo = P[XVIT_CON_WINDOW_LO], ops.span = P[XVIT_CON_WINDOW_HI] - ops.lo;
  ops.kz = D > 1 ? 2.f / (float)(D - 1) : 0.f, ops.ky = H > 1 ? 2.f / (float)(H - 1) : 0.f, ops.kx = W > 1 ? 2.f / (float)(W - 1) : 0.f;

  const S* __restrict__ sv = src + (int64_t)vol * nvox;
  T* __restrict__ dv = dst + (int64_t)vol * nvox;

  if (!(ops.flags & XVIT_CON_FLAG_BLUR)) {
    // ---- pointwise: the volume as one flat array, cut into ntile contiguous shares of 8-voxel runs; no LDS, 16 bytes per lane and access
    const bool aligned = (((uintptr_t)sv | (uintptr_t)dv) & 15) == 0;
    const uint32_t runs = (nvox + 7) >> 3, share = (runs + ntile - 1) / ntile;
    const uint32_t first = (uint32_t)tile * share, last = min(first + share, runs);
    for (uint32_t base = first + tid; base < last; base += POINT_UNROLL * 256) {
      float v[POINT_UNROLL][8];
#pragma unroll
      for (int u = 0; u < POINT_UNROLL; ++u) {
        const uint32_t r = base + u * 256;
        if (r >= last) break;
        const uint32_t i = r << 3;
        if (aligned && i + 8 <= nvox) {
          load_run8_aligned(sv + i, v[u]);
        } else {
          for (int e = 0; e < 8; ++e) v[u][e] = src_f(sv[min(i + e, nvox - 1)]);
        }
      }
#pragma unroll
      for (int u = 0; u < POINT_UNROLL; ++u) {
        const uint32_t r = base + u * 256;
        if (r >= last) break;
        const uint32_t i = r << 3;
        if (ops.flags) {
          uint32_t x = i % (uint32_t)W, rest = i / (uint32_t)W;
          uint32_t y = rest % (uint32_t)H, z = rest / (uint32_t)H;
          float uz = PointOps::coord((int)z, ops.kz), uy = PointOps::coord((int)y, ops.ky), row_e = ops.row_part(uz, uy);
          for (int e = 0; e < 8; ++e) {
            v[u][e] = ops.apply(v[u][e], row_e, uz, uy, PointOps::coord((int)x, ops.kx));
            if (++x == (uint32_t)W) {   // the run crosses into the next row (beyond the volume's end nothing is stored)
              x = 0;
              if (++y == (uint32_t)H) y = 0, ++z;
              uz = PointOps::coord((int)z, ops.kz), uy = PointOps::coord((int)y, ops.ky), row_e = ops.row_part(uz, uy);
            }
          }
        }
        if (aligned && i + 8 <= nvox) {
          store_run8(dv + i, v[u]);
        } else {
          for (int e = 0; e < 8; ++e)
            if (i + e < nvox) store_one(dv + i + e, v[u][e]);
        }
      }
    }
    return;
  }

  // ---- blur: the (x, y) tile marches along its z-segment.  Per source plane: tile + halo -> raw (LDS), blurred along x -> xb, along y ->
  // one slot of a ring of 2 Rz + 1 planes; a destination plane is the z-sum over the ring, then bias, gamma and the store.  A thread owns
  // the same 4 voxels (y, x4 .. x4 + 3) of every plane, so the ring is private to it: only raw and xb need barriers.
  const int tx = tile % ntx;
  tile /= ntx;
  const int ty = tile % nty, seg = tile / nty;
  const int x0 = tx * TX, y0 = ty * TY;
  const int seg_len = (D + nseg - 1) / nseg;
  const int zs = seg * seg_len, ze = min(zs + seg_len, D);
  if (zs >= ze) return;   // uniform: before any barrier

  int R[3];               // z, y, x: clamped into [0, RMAX] whatever the table holds; an axis without a positive sigma is skipped
  float sigma[3];
  for (int a = 0; a < 3; ++a) {
    sigma[a] = P[XVIT_CON_SIGMA + a];
    R[a] = sigma[a] > 0.f ? (int)fminf(fmaxf(P[XVIT_CON_RADIUS + a], 0.f), (float)RMAX) : 0;
  }
  const int Rz = R[0], Ry = R[1], Rx = R[2], NR = 2 * Rz + 1;

  float* __restrict__ raw = lds + LDS_RAW;
  float* __restrict__ xb = lds + LDS_XB;
  f32x4* __restrict__ ring = (f32x4*)(lds + LDS_RING);
  float* __restrict__ wgt = lds + LDS_WGT;   // [3][16]: normalised weights w[a][k + R[a]]
  if (tid < 3 * 16) {
    const int a = tid >> 4, k = (tid & 15) - R[a];
    if (k <= R[a]) {
      const float inv = 1.f / (2.f * sigma[a] * sigma[a]);   // unused when R[a] = 0
      float sum = 0.f;
      for (int j = -R[a]; j <= R[a]; ++j) sum += j == 0 ? 1.f : expf(-(float)(j * j) * inv);
      wgt[tid] = (k == 0 ? 1.f : expf(-(float)(k * k) * inv)) / sum;
    }
  }

  const int nrows = TY + 2 * Ry, nruns = Rx > 0 ? TX / 8 + 2 : TX / 8, run0 = Rx > 0 ? -1 : 0;
  const int nfetch = nrows * nruns;                     // <= 280: at most 2 runs per thread
  const bool vec = (W & 7) == 0 && ((uintptr_t)sv & 15) == 0;
  float pre[2][8];

  auto fetch = [&](int p) {   // plane p (inside the volume) -> registers; every index clamped into the volume
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int q = tid + u * 256;
      if (q >= nfetch) break;
      const int row = q / nruns, run = q - row * nruns + run0;
      const int gy = min(max(y0 - Ry + row, 0), H - 1), gx = x0 + run * 8;
      const S* __restrict__ line = sv + ((uint32_t)p * H + gy) * (uint32_t)W;
      if (vec && gx >= 0 && gx + 8 <= W) {
        load_run8_aligned(line + gx, pre[u]);
      } else {
        for (int e = 0; e < 8; ++e) pre[u][e] = src_f(line[min(max(gx + e, 0), W - 1)]);
      }
    }
  };

  const int x4 = (tid & 15) * 4, yl = tid >> 4;
  const int gy_out = y0 + yl, gx_out = x0 + x4;
  const float uy = PointOps::coord(gy_out, ops.ky);
  const bool store_vec = (W & 3) == 0 && ((uintptr_t)dv & 15) == 0;

  const int p_first = max(zs - Rz, 0), p_last = min(ze - 1 + Rz, D - 1);
  int zo = zs;
  fetch(p_first);
  for (int p = p_first; p <= p_last; ++p) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {   // the previous plane's x-pass is behind the last barrier: raw is free
      const int q = tid + u * 256;
      if (q >= nfetch) break;
      const int row = q / nruns, run = q - row * nruns + run0;
      float* o = raw + row * RAW_W + (run + 1) * 8;
      *(f32x4*)o = f32x4{pre[u][0], pre[u][1], pre[u][2], pre[u][3]};
      *(f32x4*)(o + 4) = f32x4{pre[u][4], pre[u][5], pre[u][6], pre[u][7]};
    }
    if (p < p_last) fetch(p + 1);   // in flight during this plane's passes
    __syncthreads();
    for (int j = tid; j < nrows * TX; j += 256) {   // along x: a wave is one row of 64
      const int row = j >> 6, x = j & 63;
      const float* in = raw + row * RAW_W + 8 + x - Rx;
      float acc = wgt[32] * in[0];
      for (int k = 1; k <= 2 * Rx; ++k) acc = fmaf(wgt[32 + k], in[k], acc);
      xb[row * TX + x] = acc;
    }
    __syncthreads();
    {   // along y: the thread's 4 voxels
      const float* in = xb + yl * TX + x4;
      f32x4 acc = *(const f32x4*)in * wgt[16];
      for (int k = 1; k <= 2 * Ry; ++k) {
        const f32x4 t = *(const f32x4*)(in + k * TX);
        const float w = wgt[16 + k];
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(w, t[e], acc[e]);
      }
      ring[(p % NR) * 256 + tid] = acc;
    }
    for (; zo < ze && min(zo + Rz, D - 1) <= p; ++zo) {   // every destination plane whose last source plane is now in the ring
      f32x4 acc = ring[(min(max(zo - Rz, 0), D - 1) % NR) * 256 + tid] * wgt[0];
      for (int k = 1; k <= 2 * Rz; ++k) {
        const f32x4 t = ring[(min(max(zo - Rz + k, 0), D - 1) % NR) * 256 + tid];
        const float w = wgt[k];
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(w, t[e], acc[e]);
      }
      if (gy_out >= H || gx_out >= W) continue;
      if (ops.flags & (XVIT_CON_FLAG_BIAS | XVIT_CON_FLAG_GAMMA)) {
        const float uz = PointOps::coord(zo, ops.kz), row_e = ops.row_part(uz, uy);
        for (int e = 0; e < 4; ++e) acc[e] = ops.apply(acc[e], row_e, uz, uy, PointOps::coord(gx_out + e, ops.kx));
      }
      T* __restrict__ out = dv + ((uint32_t)zo * H + gy_out) * (uint32_t)W + gx_out;
      if (store_vec) {   // W % 4 == 0: the run of 4 is inside the row and its address a multiple of 4 elements
        store_run4(out, acc);
      } else {
        for (int e = 0; e < 4; ++e)
          if (gx_out + e < W) store_one(out + e, acc[e]);
      }
    }
  }
}

// z-segments per tile column: one, unless the grid would leave CUs idle and the segments stay long against the 2 RMAX planes each re-reads
static int contrast_segments(int64_t columns, int D) {
  int nseg = 1;
  while (columns * nseg < 512 && D / (nseg + 1) >= 32) ++nseg;
  return nseg;
}

}  // namespace xvit

extern "C" int xvit_contrast_draw(const xvit_contrast_config* config, float* params, int nvol, uint64_t seed, uint64_t* counter, int advance,
                                  xvit_stream_t stream) {
  XVIT_REQUIRE(config && params, "xvit_contrast_draw: null config or parameter table");
  XVIT_REQUIRE(nvol > 0 && nvol < (1 << 24), "xvit_contrast_draw: nvol=%d must be positive (and below 2^24)", nvol);
  XVIT_REQUIRE(((uintptr_t)params & 15) == 0, "xvit_contrast_draw: the parameter table must be 16-byte aligned");
  XVIT_REQUIRE_COUNTER("xvit_contrast_draw", counter, advance);
  const xvit_contrast_config& c = *config;
  XVIT_REQUIRE(xvit::prob_ok(c.blur_prob) && xvit::prob_ok(c.bias_prob) && xvit::prob_ok(c.gamma_prob),
               "xvit_contrast_draw: every probability must lie in [0, 1]");
  XVIT_REQUIRE(c.blur_sigma_range[0] > 0.f && c.blur_sigma_range[0] <= c.blur_sigma_range[1] && c.blur_sigma_range[1] <= 2.0f,
               "xvit_contrast_draw: blur_sigma_range (%g, %g) needs 0 < lo <= hi <= 2.0 (radius ceil(3 sigma) <= %d)", c.blur_sigma_range[0],
               c.blur_sigma_range[1], XVIT_CON_MAX_RADIUS);
  XVIT_REQUIRE(c.bias_coeff >= 0.f && isfinite(c.bias_coeff), "xvit_contrast_draw: bias_coeff=%g must be finite and >= 0", c.bias_coeff);
  XVIT_REQUIRE(xvit::range_ok(c.log_gamma_range[0], c.log_gamma_range[1]), "xvit_contrast_draw: log_gamma_range (%g, %g) is reversed or not finite",
               c.log_gamma_range[0], c.log_gamma_range[1]);
  XVIT_REQUIRE(c.gamma_window[0] != c.gamma_window[1] && xvit::range_ok(c.gamma_window[0], c.gamma_window[1]),
               "xvit_contrast_draw: gamma_window (%g, %g) needs finite lo < hi", c.gamma_window[0], c.gamma_window[1]);
  hipLaunchKernelGGL(xvit::contrast_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, c, params, nvol, seed, counter, advance);
  return xvit::check_launch("xvit_contrast_draw");
}

extern "C" int xvit_contrast_apply(const void* src, void* dst, int src_dtype, int dst_dtype, const float* params, int nvol, int D, int H, int W,
                                   xvit_stream_t stream) {
  XVIT_REQUIRE(src && dst && params, "xvit_contrast_apply: null source, destination or parameter table");
  XVIT_REQUIRE(src_dtype == XVIT_BF16 || src_dtype == XVIT_F32, "xvit_contrast_apply: unknown source dtype %d", src_dtype);
  XVIT_REQUIRE(dst_dtype == XVIT_BF16 || dst_dtype == XVIT_F32, "xvit_contrast_apply: unknown destination dtype %d", dst_dtype);
  XVIT_REQUIRE(nvol > 0 && D > 0 && H > 0 && W > 0, "xvit_contrast_apply: non-positive size (nvol %d, volume %d x %d x %d)", nvol, D, H, W);
  XVIT_REQUIRE((int64_t)D * H * W < (1ll << 31), "xvit_contrast_apply: a volume must have fewer than 2^31 voxels");
  XVIT_REQUIRE((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)params) & 15) == 0,
               "xvit_contrast_apply: source, destination and parameter table must be 16-byte aligned");
  XVIT_REQUIRE(src != dst, "xvit_contrast_apply: out of place only (the blur reads neighbours of voxels already written)");
  const int ntx = (W + xvit::TX - 1) / xvit::TX, nty = (H + xvit::TY - 1) / xvit::TY;
  const int nseg = xvit::contrast_segments((int64_t)ntx * nty * nvol, D);
  XVIT_REQUIRE((int64_t)ntx * nty * nseg * nvol < (1ll << 31), "xvit_contrast_apply: too many tiles for one launch");
  const dim3 grid((unsigned)(ntx * nty * nseg * nvol));
  hipStream_t s = (hipStream_t)stream;
  xvit::by_dtype(src_dtype, [&](auto sd) {
    xvit::by_dtype(dst_dtype, [&](auto dd) {
      using S = decltype(sd);
      using T = decltype(dd);
      xvit::launch_lds<xvit::contrast_apply_kernel<S, T>, xvit::LDS_BYTES, 256>(grid, s, (const S*)src, (T*)dst, params, D, H, W, ntx, nty, nseg);
    });
  });
  return xvit::check_launch("xvit_contrast_apply");
}
