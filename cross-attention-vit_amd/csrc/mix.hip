// Mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019) on the volumes, with the soft-target loss (include/xvit.h, "Mixup / CutMix"):
//   xvit_mix_draw      one readable record per sample from (config, seed, dropout epoch): capturable, no host read-back
//   xvit_mix_apply     dst = the volumes of src mixed through the records: a pure function of (src, table)
//   xvit_mean_ce       the mean over the modalities and the cross-entropy tail, forward and backward in one launch
//   xvit_mean_ce_mix   the same with the target lam smooth(y_b) + oml smooth(y_partner[b]), read from the same table
// The random numbers live in the table only.
#include <math.h>

#include "xvit_common.h"

namespace xvit {

// ------------------------------------------------------------------------------------------
// draw: one thread per record, everything in fp64 so that a float64 restatement on the host takes the same accept / reject and floor
// decisions (tests/_mix_check.py).  Uniform i of decision block r is (hash32(seed', r * XVIT_MIX_DRAW_STRIDE + i) + 0.5) / 2^32, in (0, 1).
// Block r belongs to sample r under per_sample, block 0 serves the whole batch otherwise; block B holds the batch's partner shift.
// ------------------------------------------------------------------------------------------
constexpr int kMixAttempts = 16;                                      // Marsaglia-Tsang rounds per gamma draw before the fallback
enum { kMixUMix = 0, kMixUSwitch = 1, kMixUCentre = 2, kMixUBoost = 8, kMixUGamma = 16 };   // kMixUGamma + 64 g + 4 k + {0, 1, 2}: gamma g, round k

__device__ __forceinline__ double mix_uniform(uint64_t seed, uint64_t idx) { return ((double)hash32(seed, idx) + 0.5) * (1.0 / 4294967296.0); }

// Gamma(alpha, 1) by Marsaglia-Tsang (2000) with Box-Muller normals; alpha < 1 through Gamma(alpha + 1) U^(1 / alpha).  false: no round accepted.
__device__ bool mix_gamma(uint64_t seed, uint64_t base, int g, double alpha, double* out) {
  const double a = alpha < 1.0 ? alpha + 1.0 : alpha;
  const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  for (int k = 0; k < kMixAttempts; ++k) {
    const uint64_t i = base + kMixUGamma + 64 * g + 4 * k;
    const double x = sqrt(-2.0 * log(mix_uniform(seed, i))) * cos(6.283185307179586 * mix_uniform(seed, i + 1));
    const double t = 1.0 + c * x, v = t * t * t;
    if (!(v > 0.0)) continue;
    if (log(mix_uniform(seed, i + 2)) < 0.5 * x * x + d - d * v + d * log(v)) {
      *out = alpha < 1.0 ? d * v * pow(mix_uniform(seed, base + kMixUBoost + g), 1.0 / alpha) : d * v;
      return true;
    }
  }
  return false;
}

__global__ void __launch_bounds__(256) mix_draw_kernel(xvit_mix_config c, float* __restrict__ table, int B, int D, int H, int W, uint64_t seed,
                                                       const uint64_t* __restrict__ epoch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint64_t sd = drop_seed_at(seed, epoch);
  const uint64_t base = (uint64_t)(c.per_sample ? b : 0) * XVIT_MIX_DRAW_STRIDE;
  float rec[XVIT_MIX_NPARAM];
  for (int k = 0; k < XVIT_MIX_NPARAM; ++k) rec[k] = 0.f;
  rec[XVIT_MIX_MODE] = 0.f;
  rec[XVIT_MIX_PARTNER] = (float)b;
  rec[XVIT_MIX_LAM] = 1.f;
  rec[XVIT_MIX_LAM0] = 1.f;

  const bool any = c.mixup_alpha > 0.f || c.cutmix_alpha > 0.f;
  if (B > 1 && any && mix_uniform(sd, base + kMixUMix) < (double)c.prob) {
    const bool both = c.mixup_alpha > 0.f && c.cutmix_alpha > 0.f;
    const bool cut = both ? mix_uniform(sd, base + kMixUSwitch) < (double)c.switch_prob : c.cutmix_alpha > 0.f;
    const double alpha = (double)(cut ? c.cutmix_alpha : c.mixup_alpha);
    double g1, g2, lam0 = 0.5;
    if (mix_gamma(sd, base, 0, alpha, &g1) && mix_gamma(sd, base, 1, alpha, &g2) && g1 + g2 > 0.0) lam0 = g1 / (g1 + g2);
    const int shift = 1 + (int)floor(mix_uniform(sd, (uint64_t)B * XVIT_MIX_DRAW_STRIDE) * (double)(B - 1));   // 1 .. B - 1: nobody meets themself
    double lam = lam0;
    if (cut) {
      const double r = cbrt(1.0 - lam0);
      const int size[3] = {D, H, W};
      double vox = 1.0;
      for (int k = 0; k < 3; ++k) {
        const int ext = (int)floor((double)size[k] * r);
        const int ctr = (int)floor(mix_uniform(sd, base + kMixUCentre + k) * (double)size[k]);
        const int lo = ctr - ext / 2, hi = lo + ext;                  // `ext` voxels around the centre, then clipped to the volume
        const int lo_c = lo < 0 ? 0 : lo, hi_c = hi > size[k] ? size[k] : hi;
        rec[XVIT_MIX_BOX + 2 * k] = (float)lo_c;
        rec[XVIT_MIX_BOX + 2 * k + 1] = (float)hi_c;
        vox *= (double)(hi_c - lo_c);
      }
      lam = 1.0 - vox / ((double)D * (double)H * (double)W);
    }
    rec[XVIT_MIX_MODE] = cut ? (float)XVIT_MIX_MODE_CUTMIX : (float)XVIT_MIX_MODE_MIXUP;
    rec[XVIT_MIX_PARTNER] = (float)((b + shift) % B);
    rec[XVIT_MIX_LAM] = (float)lam;
    rec[XVIT_MIX_LAM0] = (float)lam0;
  }
  rec[XVIT_MIX_OML] = 1.f - rec[XVIT_MIX_LAM];
  f32x4* out = (f32x4*)(table + (int64_t)b * XVIT_MIX_NPARAM);
  for (int k = 0; k < XVIT_MIX_NPARAM / 4; ++k) out[k] = f32x4{rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]};
}

// ------------------------------------------------------------------------------------------
// The record as the apply and the loss kernel read it: `mixed` only for mode 1 / 2, an integral partner in [0, B) and lam != 1.
// ------------------------------------------------------------------------------------------
struct MixRecord {
  int mode, partner;   // mode 0: a copy record (the partner is never read)
  float lam, oml;
};
__device__ __forceinline__ MixRecord mix_record(const float* __restrict__ rec, int B) {
  MixRecord r;
  const float mode = rec[XVIT_MIX_MODE], p = rec[XVIT_MIX_PARTNER];
  r.lam = rec[XVIT_MIX_LAM];
  r.oml = rec[XVIT_MIX_OML];
  const bool ok = (mode == (float)XVIT_MIX_MODE_MIXUP || mode == (float)XVIT_MIX_MODE_CUTMIX) && p >= 0.f && p < (float)B && p == floorf(p) && r.lam != 1.f;
  r.mode = ok ? (int)mode : 0;
  r.partner = ok ? (int)p : 0;
  return r;
}
__device__ __forceinline__ int box_edge(float v, int size) { return (int)fminf(fmaxf(v, 0.f), (float)size); }   // NaN -> 0

// ------------------------------------------------------------------------------------------
// apply.  A 256-thread workgroup owns kMixItems * 256 consecutive vectors (VEC voxels each) of ONE volume; its sample's record goes
// through LDS, read from the table once.  VEC = 16 bytes of T where W, the strides and the pointers allow it (a vector then never
// crosses a row), else 1.  CutMix reads every voxel from exactly one source: whole vectors where the vector lies inside or outside the
// box, element by element where it straddles w0 or w1.
// ------------------------------------------------------------------------------------------
constexpr int kMixItems = 4;

template <typename T, int VEC> struct MixVec;
template <> struct MixVec<bf16, 8> { typedef bf16x8 type; };
template <> struct MixVec<float, 4> { typedef f32x4 type; };
template <> struct MixVec<bf16, 1> { typedef bf16 type; };
template <> struct MixVec<float, 1> { typedef float type; };

__device__ __forceinline__ float mix_one(float lam, float a, float oml, float b) { return fmaf(lam, a, oml * b); }
__device__ __forceinline__ float mix_blend(float lam, float oml, float a, float b) { return mix_one(lam, a, oml, b); }
__device__ __forceinline__ bf16 mix_blend(float lam, float oml, bf16 a, bf16 b) { return f2bf(mix_one(lam, bf2f(a), oml, bf2f(b))); }

template <typename T, int VEC>
__global__ void __launch_bounds__(256) mix_apply_kernel(const T* __restrict__ src, T* __restrict__ dst, const float* __restrict__ table, int B, int M, int D, int H,
                                                        int W, int64_t stride_b, int64_t stride_m, int blocks_per_vol) {
  typedef typename MixVec<T, VEC>::type V;
  __shared__ float rec_s[XVIT_MIX_NPARAM];
  const int vol = blockIdx.x / blocks_per_vol, chunk = blockIdx.x - vol * blocks_per_vol;
  const int b = vol / M, m = vol - b * M;
  if (threadIdx.x < XVIT_MIX_NPARAM) rec_s[threadIdx.x] = table[(int64_t)b * XVIT_MIX_NPARAM + threadIdx.x];
  __syncthreads();
  const MixRecord r = mix_record(rec_s, B);
  const int nvox = D * H * W, nvec = nvox / VEC;                     // < 2^31 (host check); VEC divides W
  const T* __restrict__ own = src + b * stride_b + m * stride_m;
  const T* __restrict__ other = src + r.partner * stride_b + m * stride_m;   // partner 0 for a copy record: valid, and never read
  T* __restrict__ out = dst + (int64_t)vol * nvox;
  const int v0 = chunk * (kMixItems * 256) + threadIdx.x;

  if (r.mode == 0) {
#pragma unroll
    for (int i = 0; i < kMixItems; ++i) {
      const int v = v0 + i * 256;
      if (v < nvec) ((V*)out)[v] = ((const V*)own)[v];
    }
  } else if (r.mode == XVIT_MIX_MODE_MIXUP) {
#pragma unroll
    for (int i = 0; i < kMixItems; ++i) {
      const int v = v0 + i * 256;
      if (v >= nvec) continue;
      const V a = ((const V*)own)[v], c = ((const V*)other)[v];
      V o;
      if constexpr (VEC == 1) {
        o = mix_blend(r.lam, r.oml, a, c);
      } else {
        for (int j = 0; j < VEC; ++j) o[j] = mix_blend(r.lam, r.oml, a[j], c[j]);
      }
      ((V*)out)[v] = o;
    }
  } else {
    const int d0 = box_edge(rec_s[XVIT_MIX_BOX + 0], D), d1 = box_edge(rec_s[XVIT_MIX_BOX + 1], D);
    const int h0 = box_edge(rec_s[XVIT_MIX_BOX + 2], H), h1 = box_edge(rec_s[XVIT_MIX_BOX + 3], H);
    const int w0 = box_edge(rec_s[XVIT_MIX_BOX + 4], W), w1 = box_edge(rec_s[XVIT_MIX_BOX + 5], W);
    const int wv = W / VEC;
#pragma unroll
    for (int i = 0; i < kMixItems; ++i) {
      const int v = v0 + i * 256;
      if (v >= nvec) continue;
      const int row = v / wv, x = (v - row * wv) * VEC;
      const int z = row / H, y = row - z * H;
      const bool row_in = z >= d0 && z < d1 && y >= h0 && y < h1;
      const int lo = max(x, w0), hi = min(x + VEC, w1);              // the part of the vector inside the box along x: [lo, hi)
      if (!row_in || lo >= hi) {
        ((V*)out)[v] = ((const V*)own)[v];
      } else if (lo == x && hi == x + VEC) {
        ((V*)out)[v] = ((const V*)other)[v];
      } else if constexpr (VEC > 1) {
        V o;
        const int e = v * VEC;
        for (int j = 0; j < VEC; ++j) {
          const bool in = x + j >= lo && x + j < hi;
          o[j] = (in ? other : own)[e + j];
        }
        ((V*)out)[v] = o;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// loss.  logits = mean_m logits_m; loss = mean_b CE(logits_b, target_b); dlogits_m = (softmax - target) / (B * M).  One block; B*C small.
// target_b is the smoothed label of sample b and, with MIX, lam times it plus oml times the smoothed label of the partner the record names
// (a copy record: the label alone).  Without MIX neither the table nor a second label is read.
// ------------------------------------------------------------------------------------------
template <bool MIX>
__global__ void mean_ce_kernel(const float* __restrict__ logits_m, const int64_t* __restrict__ labels, const float* __restrict__ table, float eps,
                               float* __restrict__ logits, float* __restrict__ loss, float* __restrict__ dlogits_m, int M, int B, int C) {
  __shared__ float red[4];
  float part = 0.f;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) {
      float s = 0.f;
      for (int m = 0; m < M; ++m) s += logits_m[((int64_t)m * B + b) * C + c];
      s /= (float)M;
      logits[b * C + c] = s;
      mx = fmaxf(mx, s);
    }
    float z = 0.f;
    for (int c = 0; c < C; ++c) z += expf(logits[b * C + c] - mx);
    const float lz = mx + logf(z);
    const int y = (int)labels[b];
    MixRecord r = {0, 0, 1.f, 0.f};
    int yp = y;
    if constexpr (MIX) {
      r = mix_record(table + (int64_t)b * XVIT_MIX_NPARAM, B);
      if (r.mode != 0) yp = (int)labels[r.partner];
    }
    float l = 0.f;
    for (int c = 0; c < C; ++c) {
      const float logp = logits[b * C + c] - lz;
      float tgt = (c == y ? 1.0f - eps : 0.f) + eps / (float)C;
      if (MIX && r.mode != 0) tgt = fmaf(r.lam, tgt, r.oml * ((c == yp ? 1.0f - eps : 0.f) + eps / (float)C));
      l -= tgt * logp;
      const float g = (expf(logp) - tgt) / (float)(B * M);
      for (int m = 0; m < M; ++m) dlogits_m[((int64_t)m * B + b) * C + c] = g;
    }
    part += l;
  }
  part = wave_sum(part);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    *loss = t / (float)B;
  }
}

}  // namespace xvit

using namespace xvit;

extern "C" int xvit_mix_draw(const xvit_mix_config* config, float* table, int B, int D, int H, int W, uint64_t seed, xvit_stream_t stream) {
  XVIT_REQUIRE(config && table, "xvit_mix_draw: null config or record table");
  XVIT_REQUIRE(B > 0 && B < (1 << 24), "xvit_mix_draw: B=%d must be positive and below 2^24 (the partner index is stored as a float)", B);
  XVIT_REQUIRE(D > 0 && H > 0 && W > 0 && (int64_t)D * H * W < (1ll << 31), "xvit_mix_draw: bad volume %d x %d x %d (positive, fewer than 2^31 voxels)", D, H, W);
  XVIT_REQUIRE(aligned16({table}), "xvit_mix_draw: the record table must be 16-byte aligned");
  const xvit_mix_config& c = *config;
  XVIT_REQUIRE(c.mixup_alpha >= 0.f && c.cutmix_alpha >= 0.f && isfinite(c.mixup_alpha) && isfinite(c.cutmix_alpha),
               "xvit_mix_draw: mixup_alpha=%g and cutmix_alpha=%g must be finite and >= 0", c.mixup_alpha, c.cutmix_alpha);
  XVIT_REQUIRE(c.prob >= 0.f && c.prob <= 1.f && c.switch_prob >= 0.f && c.switch_prob <= 1.f, "xvit_mix_draw: prob=%g and switch_prob=%g must lie in [0, 1]", c.prob,
               c.switch_prob);
  hipLaunchKernelGGL(mix_draw_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c, table, B, D, H, W, seed, drop_epoch_ptr());
  return check_launch("xvit_mix_draw");
}

extern "C" int xvit_mix_apply(const void* src, void* dst, int dtype, const float* table, int B, int M, int D, int H, int W, int64_t stride_b, int64_t stride_m,
                              xvit_stream_t stream) {
  XVIT_REQUIRE(src && dst && table, "xvit_mix_apply: null source, destination or record table");
  XVIT_REQUIRE(dtype == XVIT_BF16 || dtype == XVIT_F32, "xvit_mix_apply: bad dtype %d", dtype);
  XVIT_REQUIRE(B > 0 && M > 0 && D > 0 && H > 0 && W > 0, "xvit_mix_apply: bad sizes (B=%d M=%d volume %d x %d x %d)", B, M, D, H, W);
  const int64_t nvox = (int64_t)D * H * W;
  XVIT_REQUIRE(nvox < (1ll << 31), "xvit_mix_apply: a volume must have fewer than 2^31 voxels");
  XVIT_REQUIRE(stride_b > 0 && stride_m > 0, "xvit_mix_apply: the batch and modality strides must be positive");
  const int64_t size = dtype == XVIT_F32 ? 4 : 2;
  XVIT_REQUIRE((uintptr_t)src % size == 0 && (uintptr_t)dst % size == 0 && ((uintptr_t)table & 3) == 0, "xvit_mix_apply: a pointer is not aligned to its element size");
  // out of place: a sample's voxels are read after its partner's destination has been written
  const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)(((B - 1) * stride_b + (M - 1) * stride_m + nvox) * size);
  const uintptr_t t0 = (uintptr_t)dst, t1 = t0 + (uintptr_t)((int64_t)B * M * nvox * size);
  XVIT_REQUIRE(s1 <= t0 || t1 <= s0, "xvit_mix_apply: dst aliases src (the mix is out of place: dst != src, no overlap)");
  const int vec = (int)(16 / size);
  const bool wide = W % vec == 0 && stride_b % vec == 0 && stride_m % vec == 0 && aligned16({src, dst});
  const int64_t nvec = wide ? nvox / vec : nvox;
  const int64_t per_vol = (nvec + kMixItems * 256 - 1) / (kMixItems * 256);
  XVIT_REQUIRE(per_vol * B * M < (1ll << 31), "xvit_mix_apply: too many workgroups for one launch");
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    auto launch = [&](auto v) {
      hipLaunchKernelGGL((mix_apply_kernel<T, decltype(v)::value>), dim3((unsigned)(per_vol * B * M)), dim3(256), 0, (hipStream_t)stream, (const T*)src, (T*)dst, table, B,
                         M, D, H, W, stride_b, stride_m, (int)per_vol);
    };
    if (wide) launch(Int<(int)(16 / sizeof(T))>{});
    else launch(Int<1>{});
  });
  return check_launch("xvit_mix_apply");
}

extern "C" int xvit_mean_ce(const float* logits_m, const int64_t* labels, float label_smoothing, float* logits, float* loss, float* dlogits_m, int M,
                            int B, int C, xvit_stream_t stream) {
  XVIT_REQUIRE(logits_m && labels && logits && loss && dlogits_m && M > 0 && B > 0 && C > 0, "xvit_mean_ce: bad arguments");
  hipLaunchKernelGGL(mean_ce_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, logits_m, labels, (const float*)nullptr, label_smoothing, logits, loss, dlogits_m, M, B, C);
  return check_launch("xvit_mean_ce");
}

extern "C" int xvit_mean_ce_mix(const float* logits_m, const int64_t* labels, const float* table, float label_smoothing, float* logits, float* loss,
                                float* dlogits_m, int M, int B, int C, xvit_stream_t stream) {
  XVIT_REQUIRE(table, "xvit_mean_ce_mix: null record table (xvit_mean_ce is the loss without mixing)");
  XVIT_REQUIRE(logits_m && labels && logits && loss && dlogits_m && M > 0 && B > 0 && C > 0, "xvit_mean_ce_mix: bad arguments");
  hipLaunchKernelGGL(mean_ce_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, logits_m, labels, table, label_smoothing, logits, loss, dlogits_m, M, B, C);
  return check_launch("xvit_mean_ce_mix");
}
