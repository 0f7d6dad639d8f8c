// bf16 wire format of the data-parallel gradient reducer (xvit/ddp.py, comm_dtype=torch.bfloat16).
//
// pack:   dst[seg.dst_offset + i] = bf16(src[i] * scale) for i < seg.n, zeros up to the segment's 64-element slot end;
//         every segment of one launch in ONE kernel, its table passed by value in the kernel arguments (no H2D copy: capturable).
// unpack: dst[i] = float(src_bf16[i]) * scale.
// Both are streaming passes: 16-byte loads and stores, 8 elements per vector, RNE conversion by v_cvt_pk_bf16_f32 (NaN stays NaN).
#include "xvit_common.h"

namespace xvit {
namespace {

constexpr int kSegMax = XVIT_GRAD_PACK_MAX_SEGMENTS;
constexpr int kThreads = 256;
constexpr int kVecPerThread = 4;                                   // 8-element vectors per thread of a pack block
constexpr int64_t kBlockVecs = (int64_t)kThreads * kVecPerThread;  // 8192 elements per pack block

struct PackTable {
  xvit_grad_segment seg[kSegMax];
  int32_t block_start[kSegMax + 1];   // first block of segment s; block_start[n_seg] = grid size
  int32_t n_seg;
};

__host__ __device__ __forceinline__ int64_t slot_of(int64_t n) { return (n + 63) & ~(int64_t)63; }

// One block covers kBlockVecs vectors of ONE segment; which segment is found from the block index by a wave-uniform binary search over
// the table's block starts (kernel-argument loads, no divergence).
__global__ __launch_bounds__(kThreads) void grad_pack_kernel(const PackTable t, bf16* __restrict__ dst, float scale) {
  const int b = blockIdx.x;
  int lo = 0, hi = t.n_seg - 1;       // the last s with block_start[s] <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.block_start[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const int s = uniform(lo);
  const float* __restrict__ src = t.seg[s].src;
  const int64_t n = t.seg[s].n;
  bf16* __restrict__ out = dst + t.seg[s].dst_offset;
  const int64_t nv = slot_of(n) >> 3;
  const int64_t v0 = (int64_t)(b - t.block_start[s]) * kBlockVecs + threadIdx.x;
  f32x4 a[kVecPerThread], c[kVecPerThread];
#pragma unroll
  for (int k = 0; k < kVecPerThread; ++k) {
    const int64_t e = (v0 + (int64_t)k * kThreads) << 3;
    if (e + 8 <= n) {
      a[k] = ((const f32x4*)(src + e))[0];
      c[k] = ((const f32x4*)(src + e))[1];
    } else {                          // the segment's tail and its slot padding: zeros beyond n
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[k][j] = e + j < n ? src[e + j] : 0.0f;
        c[k][j] = e + 4 + j < n ? src[e + 4 + j] : 0.0f;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kVecPerThread; ++k) {
    const int64_t v = v0 + (int64_t)k * kThreads;
    if (v < nv) {
      const f32x4 x = a[k] * scale, y = c[k] * scale;
      ((bf16x8*)out)[v] = to_bf16x8(x, y);
    }
  }
}

__global__ __launch_bounds__(kThreads) void grad_unpack_kernel(const bf16* __restrict__ src, float* __restrict__ dst, int64_t n, float scale) {
  const int64_t nv = n >> 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    const bf16x8 v = ((const bf16x8*)src)[i];
    ((f32x4*)dst)[2 * i] = f32x4{bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])} * scale;
    ((f32x4*)dst)[2 * i + 1] = f32x4{bf2f(v[4]), bf2f(v[5]), bf2f(v[6]), bf2f(v[7])} * scale;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 7)) dst[(nv << 3) + threadIdx.x] = bf2f(src[(nv << 3) + threadIdx.x]) * scale;
}

}  // namespace
}  // namespace xvit

using namespace xvit;

extern "C" int xvit_grad_pack_bf16(const xvit_grad_segment* segments, int n_segments, void* dst_bf16, int64_t dst_n, float scale, xvit_stream_t stream) {
  XVIT_REQUIRE(segments && dst_bf16, "xvit_grad_pack_bf16: null pointer");
  XVIT_REQUIRE(n_segments > 0 && n_segments <= kSegMax, "xvit_grad_pack_bf16: %d segments (1 .. %d per launch)", n_segments, kSegMax);
  XVIT_REQUIRE(dst_n > 0, "xvit_grad_pack_bf16: dst_n must be positive");
  XVIT_REQUIRE((reinterpret_cast<uintptr_t>(dst_bf16) & 15) == 0, "xvit_grad_pack_bf16: dst must be 16-byte aligned");
  PackTable t;
  int64_t blocks = 0;
  for (int s = 0; s < n_segments; ++s) {
    const xvit_grad_segment& g = segments[s];
    XVIT_REQUIRE(g.src, "xvit_grad_pack_bf16: segment %d: null src", s);
    XVIT_REQUIRE((reinterpret_cast<uintptr_t>(g.src) & 15) == 0, "xvit_grad_pack_bf16: segment %d: src must be 16-byte aligned", s);
    XVIT_REQUIRE(g.n > 0, "xvit_grad_pack_bf16: segment %d: n must be positive", s);
    XVIT_REQUIRE(g.dst_offset >= 0 && g.dst_offset % 64 == 0, "xvit_grad_pack_bf16: segment %d: dst_offset must be a non-negative multiple of 64", s);
    XVIT_REQUIRE(g.dst_offset <= dst_n && slot_of(g.n) <= dst_n - g.dst_offset, "xvit_grad_pack_bf16: segment %d: its 64-element slot ends beyond dst_n", s);
    t.seg[s] = g;
    t.block_start[s] = (int32_t)blocks;
    blocks += ((slot_of(g.n) >> 3) + kBlockVecs - 1) / kBlockVecs;
    XVIT_REQUIRE(blocks < (1ll << 31), "xvit_grad_pack_bf16: too many elements in one launch");
  }
  t.block_start[n_segments] = (int32_t)blocks;
  t.n_seg = n_segments;
  for (int s = n_segments; s < kSegMax; ++s) {   // defined bytes in the unused entries
    t.seg[s] = xvit_grad_segment{nullptr, 0, 0};
    t.block_start[s + 1] = (int32_t)blocks;
  }
  hipLaunchKernelGGL(grad_pack_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, t, (bf16*)dst_bf16, scale);
  return check_launch("xvit_grad_pack_bf16");
}

extern "C" int xvit_grad_unpack_bf16(const void* src_bf16, float* dst, int64_t n, float scale, xvit_stream_t stream) {
  XVIT_REQUIRE(src_bf16 && dst && n > 0, "xvit_grad_unpack_bf16: bad arguments");
  XVIT_REQUIRE(((reinterpret_cast<uintptr_t>(src_bf16) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0, "xvit_grad_unpack_bf16: pointers must be 16-byte aligned");
  const int64_t g = (n / 8 + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(grad_unpack_kernel, dim3((unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g))), dim3(kThreads), 0, (hipStream_t)stream,
                     (const bf16*)src_bf16, dst, n, scale);
  return check_launch("xvit_grad_unpack_bf16");
}
