// Per-volume intensity statistics (include/xvit.h, "Per-volume intensity statistics"): an exact 65 536-bin histogram of the foreground
// voxels of every volume, then one workgroup per volume that turns its histogram into the stats record, folds the normalisation into the
// augmentation table and leaves the histogram zeroed.  Integer counters only, so the result does not depend on the execution order.
#include <math.h>

#include "xvit_common.h"

namespace xvit {

constexpr int kBins = 65536;
constexpr uint32_t kWinLo = XVIT_STATS_WINDOW_LO, kWinBins = XVIT_STATS_WINDOW_BINS;
constexpr int kStatThreads = 1024;
constexpr int kBinsPerThread = kBins / kStatThreads;   // 64 consecutive bins per thread of the scan
static_assert(kWinLo + kWinBins <= (uint32_t)kBins && kWinBins % (4 * kStatThreads) == 0, "the LDS window lies inside the key space");

// Key order is value order.  int16: v + 32768 (the bit pattern with its sign bit flipped).  bf16: negative patterns with all bits flipped,
// the others with the sign bit set.
template <bool BF>
__device__ __forceinline__ uint32_t key_of(uint32_t bits) {
  if constexpr (BF) return (bits & 0x8000u) ? (~bits & 0xFFFFu) : (bits | 0x8000u);
  else return bits ^ 0x8000u;
}
template <bool BF>
__device__ __forceinline__ float value_of_bits(uint32_t bits) {   // exact in fp32 for either source
  if constexpr (BF) return __builtin_bit_cast(float, bits << 16);
  else return (float)(int16_t)bits;
}
template <bool BF>
__device__ __forceinline__ double value_of_key(uint32_t key) {
  if constexpr (BF) return (double)value_of_bits<true>((key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu));
  else return (double)((int)key - 32768);
}

// ------------------------------------------------------------------------------------------
// (a) histogram.  A workgroup owns `chunk` consecutive voxels of one volume.  Keys inside [kWinLo, kWinLo + kWinBins) are counted in LDS
// and flushed once; the others go straight to global memory.  Where a key is counted never changes what is counted.
// ------------------------------------------------------------------------------------------
template <bool BF>
__device__ __forceinline__ void count_one(uint32_t bits, float fg, uint32_t* win, uint32_t* __restrict__ hist) {
  if (!(value_of_bits<BF>(bits) > fg)) return;   // NaN compares false: never foreground
  const uint32_t key = key_of<BF>(bits), w = key - kWinLo;   // unsigned: one compare serves both window edges
  if (w < kWinBins) atomicAdd(&win[w], 1u);
  else atomicAdd(&hist[key], 1u);
}
template <bool BF>
__device__ __forceinline__ void count_run8(const uint4& r, float fg, uint32_t* win, uint32_t* __restrict__ hist) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
  for (int i = 0; i < 4; ++i) {
    count_one<BF>(w[i] & 0xFFFFu, fg, win, hist);
    count_one<BF>(w[i] >> 16, fg, win, hist);
  }
}

template <bool BF>
__global__ void __launch_bounds__(kStatThreads) volume_hist_kernel(const uint16_t* __restrict__ src, uint32_t* __restrict__ hist, int64_t nvox, int per_vol,
                                                                   int64_t chunk, float fg) {
  extern __shared__ uint32_t win[];   // kWinBins counters
  const int tid = threadIdx.x;
  const int vol = blockIdx.x / per_vol, part = blockIdx.x - vol * per_vol;
  for (int i = tid; i < (int)kWinBins / 4; i += kStatThreads) ((uint4*)win)[i] = uint4{0u, 0u, 0u, 0u};
  __syncthreads();

  const int64_t beg = (int64_t)part * chunk;
  const int64_t len = max((int64_t)0, min(nvox, beg + chunk) - beg);
  const uint16_t* __restrict__ p = src + (int64_t)vol * nvox + beg;
  uint32_t* __restrict__ h = hist + (int64_t)vol * kBins;

  // a volume's base is only 2-byte aligned when nvox is odd: scalar head up to the first 16-byte boundary, 16-byte runs, scalar tail
  const int head = (int)min(len, (int64_t)(((0 - (uintptr_t)p) & 15) >> 1));
  if (tid < head) count_one<BF>(p[tid], fg, win, h);
  const uint4* __restrict__ pv = (const uint4*)(p + head);
  const int64_t nvec = (len - head) >> 3;
  int64_t i = tid;
  for (; i + 3 * kStatThreads < nvec; i += 4 * kStatThreads) {   // four loads in flight per lane
    const uint4 r0 = pv[i], r1 = pv[i + kStatThreads], r2 = pv[i + 2 * kStatThreads], r3 = pv[i + 3 * kStatThreads];
    count_run8<BF>(r0, fg, win, h);
    count_run8<BF>(r1, fg, win, h);
    count_run8<BF>(r2, fg, win, h);
    count_run8<BF>(r3, fg, win, h);
  }
  for (; i < nvec; i += kStatThreads) count_run8<BF>(pv[i], fg, win, h);
  const int64_t done = head + nvec * 8;
  if (tid < (int)(len - done)) count_one<BF>(p[done + tid], fg, win, h);
  __syncthreads();

  for (int b = tid; b < (int)kWinBins; b += kStatThreads) {
    const uint32_t c = win[b];
    if (c) atomicAdd(&h[kWinLo + b], c);
  }
}

// ------------------------------------------------------------------------------------------
// (b) scan.  One workgroup per volume; thread t owns bins [64 t, 64 t + 64) in every pass and zeroes them at the end.
// ------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T block_sum(T v, T* buf) {   // fixed order: bit-reproducible for double, exact for int64
  const int tid = threadIdx.x;
  __syncthreads();
  buf[tid] = v;
  __syncthreads();
  for (int s = kStatThreads / 2; s > 0; s >>= 1) {
    if (tid < s) buf[tid] += buf[tid + s];
    __syncthreads();
  }
  return buf[0];
}

enum { kRankMin = 0, kRankMax = 1, kRankLo = 2, kRankHi = 3 };

template <bool BF>
__global__ void __launch_bounds__(kStatThreads) volume_scan_kernel(uint32_t* __restrict__ hist, xvit_norm_config cfg, double* __restrict__ stats,
                                                                   float* __restrict__ params) {
  __shared__ uint32_t wave_total[kStatThreads / 64];
  __shared__ uint32_t found_key[4], found_below[4], found_upto[4];
  __shared__ double sum_d[kStatThreads];
  __shared__ long long sum_i[kStatThreads];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, vol = blockIdx.x;
  uint32_t* __restrict__ h = hist + (int64_t)vol * kBins + tid * kBinsPerThread;
  const uint32_t key0 = (uint32_t)tid * kBinsPerThread;
  double* __restrict__ out = stats + (int64_t)vol * XVIT_STATS_NSTAT;

  uint32_t c = 0;   // a volume has fewer than 2^31 voxels: every count and prefix fits
  for (int j = 0; j < kBinsPerThread / 4; ++j) {
    const uint4 r = ((const uint4*)h)[j];
    c += r.x + r.y + r.z + r.w;
  }
  uint32_t inc = c;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wave_total[wave] = inc;
  __syncthreads();
  uint32_t below = inc - c, n = 0;
  for (int w = 0; w < kStatThreads / 64; ++w) {
    if (w < wave) below += wave_total[w];
    n += wave_total[w];
  }
  if (n == 0) {   // no foreground: a record of zeros, the table untouched (a_n = 1, b_n = 0, no clamp); the histogram is already zero
    if (tid < XVIT_STATS_NSTAT) out[tid] = 0.0;
    return;
  }

  // nearest rank: k = max(1, ceil(q n)) in double from the fp32 q
  uint32_t rank[4] = {1u, n, 1u, n};
  if (cfg.q_lo >= 0.f) {
    const double dn = (double)n;
    rank[kRankLo] = min(n, max(1u, (uint32_t)ceil((double)cfg.q_lo * dn)));
    rank[kRankHi] = min(n, max(1u, (uint32_t)ceil((double)cfg.q_hi * dn)));
  }
  for (int j = 0; j < 4; ++j) {
    if (rank[j] > below && rank[j] <= below + c) {   // exactly one thread per rank
      uint32_t cum = below;
      for (int b = 0; b < kBinsPerThread; ++b) {
        const uint32_t cnt = h[b];
        if (rank[j] <= cum + cnt) {
          found_key[j] = key0 + b;
          found_below[j] = cum;
          found_upto[j] = cum + cnt;
          break;
        }
        cum += cnt;
      }
    }
  }
  __syncthreads();
  const uint32_t key_lo = found_key[kRankLo], key_hi = found_key[kRankHi];
  const uint32_t n_w = found_upto[kRankHi] - found_below[kRankLo];   // every value equal to lo or hi belongs to W
  const double dn_w = (double)n_w;

  // this thread's bins inside [key_lo, key_hi]
  const int b_beg = key_lo > key0 ? (int)(key_lo - key0) : 0;
  const int b_end = c == 0 ? 0 : key_hi < key0 ? 0 : min(kBinsPerThread, (int)(key_hi - key0) + 1);

  double mu;
  if constexpr (BF) {
    double s = 0.0;
    for (int b = b_beg; b < b_end; ++b) s += (double)h[b] * value_of_key<true>(key0 + b);
    mu = block_sum(s, sum_d) / dn_w;
  } else {
    long long s = 0;   // exact: |sum| < 2^31 2^15
    for (int b = b_beg; b < b_end; ++b) s += (long long)h[b] * ((int)(key0 + b) - 32768);
    mu = (double)block_sum(s, sum_i) / dn_w;   // rounded once
  }
  double s2 = 0.0;
  for (int b = b_beg; b < b_end; ++b) {
    const double d = value_of_key<BF>(key0 + b) - mu;
    s2 += (double)h[b] * (d * d);
  }
  const double sigma = sqrt(block_sum(s2, sum_d) / dn_w);

  if (c != 0)
    for (int j = 0; j < kBinsPerThread / 4; ++j) ((uint4*)h)[j] = uint4{0u, 0u, 0u, 0u};   // zero on entry of the next call

  if (tid == 0) {
    const double lo = value_of_key<BF>(key_lo), hi = value_of_key<BF>(key_hi);
    out[0] = (double)n;
    out[1] = dn_w;
    out[2] = mu;
    out[3] = sigma;
    out[4] = lo;
    out[5] = hi;
    out[6] = value_of_key<BF>(found_key[kRankMin]);
    out[7] = value_of_key<BF>(found_key[kRankMax]);
    if (params && cfg.mode != XVIT_NORM_STATS_ONLY) {
      float* __restrict__ P = params + (int64_t)vol * XVIT_AUG_NPARAM;
      double a_n, b_n;
      if (cfg.mode == XVIT_NORM_ZSCORE) {
        const double sp = sigma > 0.0 ? sigma : 1.0;
        a_n = 1.0 / sp;
        b_n = -mu / sp;
      } else {
        const double r = hi - lo > 0.0 ? hi - lo : 1.0;
        a_n = 1.0 / r;
        b_n = -lo / r;
      }
      const double a = (double)P[XVIT_AUG_SCALE], b = (double)P[XVIT_AUG_SHIFT];   // as the draw wrote them
      P[XVIT_AUG_SCALE] = (float)(a * a_n);
      P[XVIT_AUG_SHIFT] = (float)(a * b_n + b);
      if (cfg.clip) {
        P[XVIT_AUG_CLAMP_LO] = (float)lo;
        P[XVIT_AUG_CLAMP_HI] = (float)hi;
        P[XVIT_AUG_FLAGS] = (float)((int)P[XVIT_AUG_FLAGS] | XVIT_AUG_FLAG_CLAMP);
      }
    }
  }
}

template <bool BF>
static void launch_stats(const void* src, int nvol, int64_t nvox, const xvit_norm_config& cfg, double* stats, float* params, void* workspace, hipStream_t s) {
  // at least 64 Ki voxels per workgroup (it zeroes and flushes a 128 KiB window), about one workgroup per CU when there is enough work
  const int cap = nvol >= 256 ? 1 : 256 / nvol;
  int per_vol = (int)min((int64_t)cap, (nvox + 65535) / 65536);
  const int64_t chunk = ((nvox + per_vol - 1) / per_vol + 7) & ~(int64_t)7;
  per_vol = (int)((nvox + chunk - 1) / chunk);   // no empty workgroup
  launch_lds<volume_hist_kernel<BF>, (int)(kWinBins * sizeof(uint32_t)), kStatThreads>(dim3((unsigned)(nvol * per_vol)), s, (const uint16_t*)src,
                                                                                       (uint32_t*)workspace, nvox, per_vol, chunk, cfg.foreground_above);
  hipLaunchKernelGGL(volume_scan_kernel<BF>, dim3((unsigned)nvol), dim3(kStatThreads), 0, s, (uint32_t*)workspace, cfg, stats, params);
}

}  // namespace xvit

extern "C" int64_t xvit_volume_stats_workspace_bytes(int nvol) { return nvol > 0 ? (int64_t)nvol * xvit::kBins * (int64_t)sizeof(uint32_t) : 0; }

extern "C" int xvit_volume_stats(const void* src, int src_dtype, int nvol, int64_t nvox, const xvit_norm_config* cfg, double* stats, float* params,
                                 void* workspace, int64_t workspace_bytes, xvit_stream_t stream) {
  XVIT_REQUIRE(src && cfg && stats && workspace, "xvit_volume_stats: null source, config, stats or workspace");
  XVIT_REQUIRE(src_dtype != XVIT_F32, "xvit_volume_stats: fp32 sources are not supported (the histogram has 2^16 bins): cast to bf16 or normalise beforehand");
  XVIT_REQUIRE(src_dtype == XVIT_I16 || src_dtype == XVIT_BF16, "xvit_volume_stats: unknown source dtype %d", src_dtype);
  XVIT_REQUIRE(nvol > 0 && nvol < (1 << 24), "xvit_volume_stats: nvol=%d must be positive (and < 2^24)", nvol);
  XVIT_REQUIRE(nvox > 0 && nvox < (1ll << 31), "xvit_volume_stats: nvox=%lld: a volume must have at least one and fewer than 2^31 voxels", (long long)nvox);
  XVIT_REQUIRE(cfg->mode == XVIT_NORM_STATS_ONLY || cfg->mode == XVIT_NORM_ZSCORE || cfg->mode == XVIT_NORM_WINDOW, "xvit_volume_stats: unknown mode %d",
               cfg->mode);
  XVIT_REQUIRE(!isnan(cfg->foreground_above), "xvit_volume_stats: foreground_above is NaN");
  XVIT_REQUIRE(cfg->q_lo < 0.f || (cfg->q_lo >= 0.f && cfg->q_lo <= cfg->q_hi && cfg->q_hi <= 1.f),
               "xvit_volume_stats: percentiles (%g, %g) need 0 <= q_lo <= q_hi <= 1 (q_lo < 0: none)", cfg->q_lo, cfg->q_hi);
  XVIT_REQUIRE(((uintptr_t)src & 1) == 0, "xvit_volume_stats: the source is not aligned to its element size");
  XVIT_REQUIRE(((uintptr_t)stats & 7) == 0, "xvit_volume_stats: stats must be 8-byte aligned");
  XVIT_REQUIRE(((uintptr_t)params & 15) == 0, "xvit_volume_stats: the parameter table must be 16-byte aligned");
  XVIT_REQUIRE(((uintptr_t)workspace & 15) == 0, "xvit_volume_stats: the workspace must be 16-byte aligned");
  XVIT_REQUIRE(workspace_bytes >= xvit_volume_stats_workspace_bytes(nvol), "xvit_volume_stats: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)xvit_volume_stats_workspace_bytes(nvol));
  if (src_dtype == XVIT_BF16) xvit::launch_stats<true>(src, nvol, nvox, *cfg, stats, params, workspace, (hipStream_t)stream);
  else xvit::launch_stats<false>(src, nvol, nvox, *cfg, stats, params, workspace, (hipStream_t)stream);
  return xvit::check_launch("xvit_volume_stats");
}
