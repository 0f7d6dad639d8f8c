// Device-resident volume store (include/xvit.h, "Device-resident volume store"): the batches a captured step draws.
//   xvit_batch_draw     case indices of one batch from (seed, global ordinal): weighted with replacement, a keyed permutation per epoch,
//                       or sequential; the call index may live on the device, so a replay draws the next batch
//   xvit_batch_gather   dst[b] = store[idx[b]] byte for byte, idx read on the device; labels and a per-sample status beside it
// No atomics, no dependence on execution order: both are bit-reproducible (tests/_data_check.py restates them).
#include "xvit_common.h"

namespace xvit {

constexpr uint64_t kBatchTag = 0x5356444154415354ull;   // keeps this stream apart from the other draw streams under one seed

// ------------------------------------------------------------------------------------------
// draw: one block; thread i serves samples i, i + 256, ...  Every thread reads the counter before the barrier, one thread advances it
// behind it.  Sample i has the global ordinal k = (c * world + rank) * B + i and is a function of (seed, k) only.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int batch_weighted(const double* __restrict__ cdf, int n, uint64_t s, uint64_t k) {
  const uint64_t bits = ((uint64_t)draw24(s, 2 * k) << 24) | (uint64_t)draw24(s, 2 * k + 1);
  const double u = (double)bits * (1.0 / 281474976710656.0);        // 2^-48: exact in fp64, in [0, 1)
  int lo = 0, hi = n;                                                // the number of j with cdf[j] <= u, cdf non-decreasing
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (cdf[mid] <= u) lo = mid + 1;
    else hi = mid;
  }
  return lo < n - 1 ? lo : n - 1;
}

// pi_e(q): a balanced 4-round Feistel network on 2 * half bits, cycle-walked into [0, n).  2^(2 half) < 4 n + 4: a few rounds at most.
__device__ __forceinline__ int batch_permute(uint64_t n, int half, uint64_t key, uint64_t q) {
  const uint64_t mask = (1ull << half) - 1;
  uint64_t x = q;
  do {
    uint64_t L = x >> half, R = x & mask;
#pragma unroll
    for (uint64_t r = 0; r < 4; ++r) {
      const uint64_t t = L ^ ((uint64_t)hash32(key, (r << 32) | R) & mask);
      L = R;
      R = t;
    }
    x = (L << half) | R;
  } while (x >= n);
  return (int)x;
}

__global__ void __launch_bounds__(256) batch_draw_kernel(int32_t* __restrict__ idx, const double* __restrict__ cdf, int64_t n_cases, int B, int mode, int rank,
                                                         int world, uint64_t seed, uint64_t call, uint64_t* counter, int advance, int half) {
  const uint64_t c = counter ? *counter : call;
  __syncthreads();
  if (advance && threadIdx.x == 0) *counter = c + 1;
  const uint64_t n = (uint64_t)n_cases, s = seed ^ kBatchTag;
  const uint64_t k0 = (c * (uint64_t)world + (uint64_t)rank) * (uint64_t)B;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const uint64_t k = k0 + (uint64_t)i;
    int out;
    if (mode == XVIT_BATCH_WEIGHTED) {
      out = batch_weighted(cdf, (int)n_cases, s, k);
    } else {
      const uint64_t e = k / n, q = k - e * n;
      out = mode == XVIT_BATCH_SHUFFLE ? batch_permute(n, half, s + e * kSeedStride, q) : (int)q;
    }
    idx[i] = out;
  }
}

// ------------------------------------------------------------------------------------------
// gather.  A 256-thread workgroup owns kBatchItems * 256 consecutive accesses of ONE case (V: 16 bytes where case_bytes % 16 == 0, so
// that every case base of the store and of the batch is 16-byte aligned; 2 bytes otherwise, where the two phases differ per case).  All
// loads of a lane are issued before its first store.  An index outside [0, n_cases) reads nothing: zeros, label -1, status 1.
// ------------------------------------------------------------------------------------------
constexpr int kBatchItems = 8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

template <typename V>
__global__ void __launch_bounds__(256) batch_gather_kernel(const char* __restrict__ store, int64_t case_bytes, int64_t n_cases, const int32_t* __restrict__ idx,
                                                           char* __restrict__ dst, const int64_t* __restrict__ labels_src, int64_t* __restrict__ labels_dst,
                                                           int32_t* __restrict__ status, int chunks) {
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const int i = idx[b];
  const bool ok = i >= 0 && (int64_t)i < n_cases;
  if (chunk == 0 && threadIdx.x == 0) {
    if (labels_src) labels_dst[b] = ok ? labels_src[i] : -1;
    if (status) status[b] = ok ? 0 : 1;
  }
  const int64_t nvec = case_bytes / (int64_t)sizeof(V);
  const int64_t v0 = (int64_t)chunk * (kBatchItems * 256) + threadIdx.x;
  V* __restrict__ to = (V*)(dst + (int64_t)b * case_bytes);
  if (!ok) {                                                         // per workgroup: the store is not read at all
#pragma unroll
    for (int j = 0; j < kBatchItems; ++j) {
      const int64_t v = v0 + j * 256;
      if (v < nvec) to[v] = V{};
    }
    return;
  }
  const V* __restrict__ from = (const V*)(store + (int64_t)i * case_bytes);
  V val[kBatchItems];
#pragma unroll
  for (int j = 0; j < kBatchItems; ++j) {                            // unconditional loads, clamped into the case: no branch, hence no wait, between them
    const int64_t v = v0 + j * 256;
    val[j] = from[v < nvec ? v : nvec - 1];
  }
#pragma unroll
  for (int j = 0; j < kBatchItems; ++j) {
    const int64_t v = v0 + j * 256;
    if (v < nvec) to[v] = val[j];
  }
}

}  // namespace xvit

using namespace xvit;

extern "C" int xvit_batch_draw(int32_t* idx, const double* cdf, int64_t n_cases, int B, int mode, int rank, int world, uint64_t seed, uint64_t call,
                               uint64_t* counter, int advance, xvit_stream_t stream) {
  XVIT_REQUIRE(idx, "xvit_batch_draw: null index buffer");
  XVIT_REQUIRE(((uintptr_t)idx & 3) == 0, "xvit_batch_draw: the index buffer must be 4-byte aligned");
  XVIT_REQUIRE(n_cases > 0 && n_cases <= 0x7FFFFFFFll, "xvit_batch_draw: n_cases=%lld must lie in [1, 2^31 - 1]", (long long)n_cases);
  XVIT_REQUIRE(B > 0, "xvit_batch_draw: B=%d must be positive", B);
  XVIT_REQUIRE(mode == XVIT_BATCH_WEIGHTED || mode == XVIT_BATCH_SHUFFLE || mode == XVIT_BATCH_SEQUENTIAL, "xvit_batch_draw: unknown mode %d", mode);
  XVIT_REQUIRE(world > 0 && rank >= 0 && rank < world, "xvit_batch_draw: rank=%d must lie in [0, world=%d)", rank, world);
  XVIT_REQUIRE_COUNTER("xvit_batch_draw", counter, advance);
  XVIT_REQUIRE(mode != XVIT_BATCH_WEIGHTED || cdf, "xvit_batch_draw: the weighted mode needs a cdf");
  XVIT_REQUIRE(mode != XVIT_BATCH_WEIGHTED || ((uintptr_t)cdf & 7) == 0, "xvit_batch_draw: the cdf must be 8-byte aligned");
  int bits = 0;                                                      // ceil(log2 n_cases)
  while ((1ll << bits) < n_cases) ++bits;
  const int half = bits <= 2 ? 1 : (bits + 1) / 2;                   // max(2, bits) rounded up to even, halved
  hipLaunchKernelGGL(batch_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, idx, cdf, n_cases, B, mode, rank, world, seed, call, counter, advance, half);
  return check_launch("xvit_batch_draw");
}

extern "C" int xvit_batch_gather(const void* store, int64_t case_bytes, int64_t n_cases, const int32_t* idx, int B, void* dst, const int64_t* labels_src,
                                 int64_t* labels_dst, int32_t* status, xvit_stream_t stream) {
  XVIT_REQUIRE(store && idx && dst, "xvit_batch_gather: null store, index or destination");
  XVIT_REQUIRE(!labels_src || labels_dst, "xvit_batch_gather: null label destination (labels_src is given)");
  XVIT_REQUIRE(case_bytes > 0 && case_bytes % 2 == 0, "xvit_batch_gather: case_bytes=%lld must be a positive multiple of 2", (long long)case_bytes);
  XVIT_REQUIRE(n_cases > 0 && B > 0, "xvit_batch_gather: n_cases=%lld and B=%d must be positive", (long long)n_cases, B);
  XVIT_REQUIRE(aligned16({store, dst}), "xvit_batch_gather: store and dst must be 16-byte aligned");
  XVIT_REQUIRE(((uintptr_t)idx & 3) == 0 && ((uintptr_t)status & 3) == 0 && (((uintptr_t)labels_src | (uintptr_t)labels_dst) & 7) == 0,
               "xvit_batch_gather: idx and status must be 4-byte, the labels 8-byte aligned");
  const bool wide = case_bytes % 16 == 0;
  const int64_t per_chunk = (int64_t)kBatchItems * 256 * (wide ? 16 : 2);
  const int64_t chunks = (case_bytes + per_chunk - 1) / per_chunk;
  XVIT_REQUIRE(chunks * B < (1ll << 31), "xvit_batch_gather: too many workgroups for one launch (B x chunks >= 2^31)");
  auto launch = [&](auto v) {
    hipLaunchKernelGGL(batch_gather_kernel<decltype(v)>, dim3((unsigned)(chunks * B)), dim3(256), 0, (hipStream_t)stream, (const char*)store, case_bytes, n_cases, idx,
                       (char*)dst, labels_src, labels_dst, status, (int)chunks);
  };
  if (wide) launch(u32x4{});
  else launch(uint16_t{});
  return check_launch("xvit_batch_gather");
}
