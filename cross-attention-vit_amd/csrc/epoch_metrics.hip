// Pooled multi-class epoch metrics (include/xvit.h, "Pooled epoch metrics").
//
// xvit_epoch_metrics_update appends a step's softmax rows, labels and predictions to caller-owned epoch buffers at a device-side cursor
// and folds the step into an integer confusion matrix: one single-workgroup launch per step, no host read, capturable.
// xvit_epoch_rank_stats turns the stored epoch into exact integer rank statistics, one workgroup per (bootstrap replicate, class): the
// replicate's multiplicities are drawn into 16-bit LDS counters, then one tie-aware walk of the class's sorted order yields the pair count
// behind the one-vs-rest AUROC, the average precision and the replicate's confusion row.
//
// What bounds them.  Update: launch latency (a step is at most 8192 x 64 floats).  Rank statistics: the LDS pipe and the barriers of the
// two block scans per pass of kRankPass sorted elements, plus one 4-byte gather per element; no floating-point work outside the AP terms.
#include <math.h>

#include "xvit_common.h"

namespace xvit {

constexpr int kEpochThreads = 1024, kEpochWaves = kEpochThreads / 64;
constexpr int kEpochMaxC = XVIT_EPOCH_MAX_C, kEpochMaxB = XVIT_EPOCH_MAX_B, kHead = XVIT_EPOCH_STATE_HEAD;
constexpr int kRankPass = XVIT_EPOCH_RANK_PASS;
static_assert(kRankPass == kEpochThreads, "the walk takes one sorted element per thread and pass");

// ------------------------------------------------------------------------------------------
// (a) update.  Thread t takes rows t, t + 1024, ...; kept rows are compacted in row order (ballot + wave counts), so the stored epoch
// is the concatenation of the steps' kept rows whatever the batch split.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kEpochThreads) void epoch_update_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, int B, int C,
                                                                     float* __restrict__ scores, int32_t* __restrict__ labels32, int32_t* __restrict__ preds,
                                                                     int64_t cap, int64_t* __restrict__ state) {
  __shared__ uint32_t conf[kEpochMaxC * kEpochMaxC];
  __shared__ uint32_t wave_cnt[kEpochWaves];
  __shared__ uint32_t dropped[2];   // ignored, nonfinite
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < C * C; i += kEpochThreads) conf[i] = 0u;
  if (tid < 2) dropped[tid] = 0u;
  // every thread reads the cursor here; it is written once, by thread 0, after the last barrier
  const int64_t cursor = min(max(state[XVIT_EPOCH_STORED], (int64_t)0), cap);
  int64_t kept = 0;
  __syncthreads();

  for (int base = 0; base < B; base += kEpochThreads) {
    const int b = base + tid;
    bool keep = false;
    int lab = 0, pred = 0;
    float mx = 0.f;
    const float* __restrict__ row = logits + (int64_t)(b < B ? b : 0) * ld;
    if (b < B) {
      const int64_t l64 = labels[b];
      if (l64 < 0 || l64 >= C) atomicAdd(&dropped[0], 1u);
      else {
        lab = (int)l64;
        mx = row[0];
        bool finite = isfinite(mx);
        for (int c = 1; c < C; ++c) {
          const float v = row[c];
          finite = finite && isfinite(v);
          if (v > mx) { mx = v; pred = c; }   // first maximum on ties
        }
        if (finite) keep = true;
        else atomicAdd(&dropped[1], 1u);
      }
    }
    const unsigned long long vote = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(vote);
    __syncthreads();
    uint32_t before = (uint32_t)__popcll(vote & ((1ull << lane) - 1ull)), total = 0u;
    for (int w = 0; w < kEpochWaves; ++w) {
      const uint32_t c = wave_cnt[w];
      if (w < wave) before += c;
      total += c;
    }
    __syncthreads();   // wave_cnt is rewritten by the next pass
    if (keep) {
      atomicAdd(&conf[lab * C + pred], 1u);
      const int64_t pos = cursor + kept + before;
      if (pos < cap) {   // a row past the capacity is counted (confusion, overflow) and not stored
        float sum = 0.f;
        for (int c = 0; c < C; ++c) sum += expf(row[c] - mx);   // class order
        float* __restrict__ out = scores + pos * C;
        for (int c = 0; c < C; ++c) out[c] = expf(row[c] - mx) / sum;
        labels32[pos] = lab;
        preds[pos] = pred;
      }
    }
    kept += total;
  }
  __syncthreads();
  // one workgroup per launch and launches of one stream in order: plain read-modify-write, no atomics needed
  for (int i = tid; i < C * C; i += kEpochThreads) {
    const uint32_t c = conf[i];
    if (c) state[kHead + i] += (int64_t)c;
  }
  if (tid == 0) {
    const int64_t end = cursor + kept;
    state[XVIT_EPOCH_STORED] = min(end, cap);
    state[XVIT_EPOCH_SEEN] += B;
    state[XVIT_EPOCH_STEPS] += 1;
    state[XVIT_EPOCH_IGNORED] += dropped[0];
    state[XVIT_EPOCH_NONFINITE] += dropped[1];
    state[XVIT_EPOCH_OVERFLOW] += end > cap ? end - cap : 0;
  }
}

// ------------------------------------------------------------------------------------------
// (b) rank statistics.  blockIdx.x = replicate r, blockIdx.y = class c.
// ------------------------------------------------------------------------------------------
typedef unsigned long long u64;

struct RankScratch {          // the fixed head of the dynamic LDS region; the 16-bit multiplicities follow it
  u64 wave_sum[kEpochWaves];
  u64 wave_max[kEpochWaves];
  u64 red_u[kEpochWaves];
  double red_d[kEpochWaves];
  uint32_t conf[kEpochMaxC];
  float s[kRankPass + 4];     // this pass's scores in sorted order
};
static_assert(sizeof(RankScratch) % 16 == 0, "the multiplicities start 16-byte aligned");
constexpr int64_t kRankMaxN = XVIT_EPOCH_RANK_MAX_N;   // 16-bit counters: at most 65 535 draws can land on one sample
static_assert(sizeof(RankScratch) + (kRankMaxN + 1) * 2 <= 160 * 1024, "scratch and counters fit the LDS of one CU");

__device__ __forceinline__ u64 wave_scan_sum(u64 v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}
__device__ __forceinline__ u64 wave_scan_max(u64 v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = __shfl_up(v, d);
    if (lane >= d) v = max(v, o);
  }
  return v;
}

__global__ __launch_bounds__(kEpochThreads) void epoch_rank_kernel(const float* __restrict__ scores, const int32_t* __restrict__ labels32,
                                                                   const int32_t* __restrict__ preds, const int64_t* __restrict__ perm, int64_t ldp,
                                                                   const int64_t* __restrict__ n_dev, int64_t n_max, int C, uint64_t seed,
                                                                   int64_t* __restrict__ ranks, double* __restrict__ ap, int64_t* __restrict__ conf) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  RankScratch& S = *reinterpret_cast<RankScratch*>(smem);
  uint32_t* __restrict__ w2 = reinterpret_cast<uint32_t*>(smem + sizeof(RankScratch));   // two 16-bit counters per word, by sample

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x, c = blockIdx.y;
  const int n = (int)min(max(*n_dev, (int64_t)0), n_max);   // n_max < 2^31 (host-checked); with r > 0 also <= kRankMaxN
  const bool boot = r > 0;

  if (tid < C) S.conf[tid] = 0u;
  if (boot) {
    for (int i = tid; i < (n + 1) / 2; i += kEpochThreads) w2[i] = 0u;
    __syncthreads();
    const uint64_t rs = seed + (uint64_t)r * 0x9E3779B97F4A7C15ull;
    for (int k = tid; k < n; k += kEpochThreads) {
      const uint32_t i = (uint32_t)(((uint64_t)hash32(rs, (uint64_t)k) * (uint64_t)n) >> 32);   // < n
      atomicAdd(&w2[i >> 1], 1u << (16 * (i & 1)));   // n <= 65 535: the low half never carries into the high one
    }
  }
  __syncthreads();
  auto weight = [&](int i) -> uint32_t { return boot ? (w2[i >> 1] >> (16 * (i & 1))) & 0xFFFFu : 1u; };

  // totals by sample: Wpos, W and the confusion row of class c
  u64 tot = 0;   // Wpos << 32 | W
  for (int i = tid; i < n; i += kEpochThreads) {
    const uint32_t w = weight(i);
    tot += w;
    if (labels32[i] == c) {
      tot += (u64)w << 32;
      const int p = preds[i];
      if (w && (unsigned)p < (unsigned)C) atomicAdd(&S.conf[p], w);
    }
  }
  for (int d = 32; d > 0; d >>= 1) tot += __shfl_down(tot, d);
  if (lane == 0) S.red_u[wave] = tot;
  __syncthreads();
  tot = 0;
  for (int w = 0; w < kEpochWaves; ++w) tot += S.red_u[w];
  const u64 Wpos = tot >> 32, Wneg = (tot & 0xFFFFFFFFull) - Wpos;
  if (tid < C) conf[((int64_t)r * C + c) * C + tid] = (int64_t)S.conf[tid];

  // the walk: cumulative (positive << 32 | negative) weight in sorted order and, per element, the cumulative weight in front of its tie
  // group (a running maximum over the group heads: cumulative weights never decrease).  A group contributes where it ends.
  const int64_t* __restrict__ order = perm + (int64_t)c * ldp;
  auto score_at = [&](int j) -> float {
    const int64_t i = order[j];
    return (uint64_t)i < (uint64_t)n ? scores[i * C + c] : 0.f;
  };
  u64 carry_sum = 0, carry_head = 0, u2 = 0;
  double ap_sum = 0.0;
  for (int base = 0; base < n; base += kRankPass) {
    const int j = base + tid;
    const bool in = j < n;
    float s = 0.f;
    u64 mine = 0;
    if (in) {
      const int64_t i = order[j];
      if ((uint64_t)i < (uint64_t)n) {   // an index outside the epoch carries no weight
        s = scores[i * C + c];
        const uint32_t w = weight((int)i);
        mine = labels32[i] == c ? (u64)w << 32 : (u64)w;
      }
    }
    S.s[tid + 1] = s;
    if (tid == 0) S.s[0] = base > 0 ? score_at(base - 1) : 0.f;
    if (tid == kRankPass - 1) S.s[kRankPass + 1] = base + kRankPass < n ? score_at(base + kRankPass) : 0.f;
    const u64 incl_w = wave_scan_sum(mine, lane);
    if (lane == 63) S.wave_sum[wave] = incl_w;
    __syncthreads();
    u64 incl = carry_sum + incl_w, pass_total = 0;
#pragma unroll 4   // fully unrolled, the 16 totals sit in registers at once: 122 VGPRs, one workgroup per CU; by fours: 58, two
    for (int w = 0; w < kEpochWaves; ++w) {
      const u64 t = S.wave_sum[w];
      if (w < wave) incl += t;
      pass_total += t;
    }
    const bool head = in && (j == 0 || S.s[tid] != s);
    const bool tail = in && (j == n - 1 || S.s[tid + 2] != s);
    const u64 head_w = wave_scan_max(head ? incl - mine : 0ull, lane);
    if (lane == 63) S.wave_max[wave] = head_w;
    __syncthreads();
    u64 before = max(carry_head, head_w), pass_head = carry_head;
#pragma unroll 4
    for (int w = 0; w < kEpochWaves; ++w) {
      const u64 t = S.wave_max[w];
      if (w < wave) before = max(before, t);
      pass_head = max(pass_head, t);
    }
    if (tail) {
      const u64 cp = incl >> 32, cn = incl & 0xFFFFFFFFull;
      const u64 gp = cp - (before >> 32), gn = cn - (before & 0xFFFFFFFFull);
      u2 += gp * (2ull * (Wneg - cn) + gn);
      if (gp) ap_sum += (double)(gp * cp) / (double)(cp + cn);
    }
    carry_sum += pass_total;
    carry_head = pass_head;
  }

  // fixed-order reductions: lanes by halving, waves in order
  for (int d = 32; d > 0; d >>= 1) {
    u2 += __shfl_down(u2, d);
    ap_sum += __shfl_down(ap_sum, d);
  }
  __syncthreads();   // red_u was read above
  if (lane == 0) {
    S.red_u[wave] = u2;
    S.red_d[wave] = ap_sum;
  }
  __syncthreads();
  if (tid == 0) {
    u64 u = 0;
    double a = 0.0;
    for (int w = 0; w < kEpochWaves; ++w) {
      u += S.red_u[w];
      a += S.red_d[w];
    }
    int64_t* __restrict__ out = ranks + ((int64_t)r * C + c) * XVIT_EPOCH_RANK_NSTAT;
    out[XVIT_EPOCH_RANK_U2] = (int64_t)u;
    out[XVIT_EPOCH_RANK_WPOS] = (int64_t)Wpos;
    out[XVIT_EPOCH_RANK_WNEG] = (int64_t)Wneg;
    ap[(int64_t)r * C + c] = Wpos ? a / (double)Wpos : 0.0;
  }
}

}  // namespace xvit

extern "C" int xvit_epoch_metrics_update(const float* logits, int64_t ld, const int64_t* labels, int B, int C, float* scores, int32_t* labels32, int32_t* preds,
                                         int64_t cap, int64_t* state, xvit_stream_t stream) {
  XVIT_REQUIRE(logits && labels && scores && labels32 && preds && state, "xvit_epoch_metrics_update: null pointer");
  XVIT_REQUIRE(C >= 2 && C <= xvit::kEpochMaxC, "xvit_epoch_metrics_update: %d classes outside 2..%d", C, xvit::kEpochMaxC);
  XVIT_REQUIRE(B >= 1 && B <= xvit::kEpochMaxB, "xvit_epoch_metrics_update: batch %d outside 1..%d", B, xvit::kEpochMaxB);
  XVIT_REQUIRE(ld >= C, "xvit_epoch_metrics_update: row stride %lld shorter than the %d classes", (long long)ld, C);
  XVIT_REQUIRE(cap >= 1 && cap < (1ll << 31), "xvit_epoch_metrics_update: capacity %lld outside 1..2^31-1", (long long)cap);
  XVIT_REQUIRE(((uintptr_t)state & 7) == 0, "xvit_epoch_metrics_update: state must be 8-byte aligned");
  hipLaunchKernelGGL(xvit::epoch_update_kernel, dim3(1), dim3(xvit::kEpochThreads), 0, (hipStream_t)stream, logits, ld, labels, B, C, scores, labels32, preds, cap,
                     state);
  return xvit::check_launch("xvit_epoch_metrics_update");
}

extern "C" int64_t xvit_epoch_rank_stats_max_n(void) { return xvit::kRankMaxN; }

extern "C" int xvit_epoch_rank_stats(const float* scores, const int32_t* labels32, const int32_t* preds, const int64_t* perm, int64_t ldp, const int64_t* n_dev,
                                     int64_t n_max, int C, int R, uint64_t seed, int64_t* ranks, double* ap, int64_t* conf, xvit_stream_t stream) {
  XVIT_REQUIRE(ranks && ap && conf, "xvit_epoch_rank_stats: null output pointer");
  XVIT_REQUIRE(C >= 2 && C <= xvit::kEpochMaxC, "xvit_epoch_rank_stats: %d classes outside 2..%d", C, xvit::kEpochMaxC);
  XVIT_REQUIRE(R >= 0 && R <= 65534, "xvit_epoch_rank_stats: %d bootstrap replicates outside 0..65534", R);
  XVIT_REQUIRE(n_max >= 0 && n_max < (1ll << 31), "xvit_epoch_rank_stats: n_max = %lld outside 0..2^31-1", (long long)n_max);
  XVIT_REQUIRE(R == 0 || n_max <= xvit::kRankMaxN,
               "xvit_epoch_rank_stats: n_max = %lld with %d bootstrap replicates: the 16-bit LDS multiplicities hold at most %lld samples (R = 0 has no limit)",
               (long long)n_max, R, (long long)xvit::kRankMaxN);
  XVIT_REQUIRE(((uintptr_t)ranks & 7) == 0 && ((uintptr_t)ap & 7) == 0 && ((uintptr_t)conf & 7) == 0, "xvit_epoch_rank_stats: outputs must be 8-byte aligned");
  const int64_t cells = (int64_t)(R + 1) * C;
  if (n_max == 0) {   // an empty epoch: nothing is launched, the outputs are zero
    hipError_t e = hipMemsetAsync(ranks, 0, cells * XVIT_EPOCH_RANK_NSTAT * sizeof(int64_t), (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(ap, 0, cells * sizeof(double), (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(conf, 0, cells * C * sizeof(int64_t), (hipStream_t)stream);
    if (e != hipSuccess) {
      xvit::set_error("xvit_epoch_rank_stats: hipMemsetAsync: %s", hipGetErrorString(e));
      return (int)e;
    }
    return XVIT_OK;
  }
  XVIT_REQUIRE(scores && labels32 && preds && perm && n_dev, "xvit_epoch_rank_stats: null input pointer");
  XVIT_REQUIRE(ldp >= n_max, "xvit_epoch_rank_stats: permutation row stride %lld shorter than n_max = %lld", (long long)ldp, (long long)n_max);
  const size_t lds = sizeof(xvit::RankScratch) + (R > 0 ? (size_t)((n_max + 1) / 2 * 4 + 15) / 16 * 16 : 0);
  const hipError_t e = xvit::launch_dyn_lds<xvit::epoch_rank_kernel>(dim3((unsigned)(R + 1), (unsigned)C), dim3(xvit::kEpochThreads), lds, (hipStream_t)stream, scores,
                                                                     labels32, preds, perm, ldp, n_dev, n_max, C, seed, ranks, ap, conf);
  if (e != hipSuccess) {
    xvit::set_error("xvit_epoch_rank_stats: hipFuncSetAttribute(%zu bytes of LDS): %s", lds, hipGetErrorString(e));
    return (int)e;
  }
  return xvit::check_launch("xvit_epoch_rank_stats");
}
