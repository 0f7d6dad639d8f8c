// HBM-bound helpers around the GEMMs: 3-D patchify, CLS/pos rows, column sums (bias grads),
// casts, dropout and the num_classes head (the mean + cross-entropy tail: mix.hip).
#include "token_rows.h"

namespace xvit {

// ------------------------------------------------------------------------------------------
// patchify (reference model_cross.py:193).  Threads walk the INPUT in memory order (8 voxels =
// one 16/32-byte run each), so reads are fully coalesced; a wave then covers 4 H-rows of 8
// patches and its writes land as whole 128-byte lines of 8 different token rows.
// ------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ void patchify_kernel(const T* __restrict__ img, bf16* __restrict__ out, const PatchGeom g, int64_t total_vec) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total_vec; idx += (int64_t)gridDim.x * blockDim.x)
    copy_run<VEC>(out + patch_elem<VEC>(g, idx), img + idx * VEC);
}

// unpatchify: the exact inverse of patchify_kernel (fp32 patch rows -> fp32 / bf16 volume).  Threads walk the OUTPUT in memory
// order, 8 voxels = one 32 / 16-byte run each, so the volume is written fully coalesced; each reads its 32 bytes from one patch row.
template <typename T, int VEC>
__global__ void unpatchify_kernel(const float* __restrict__ in, T* __restrict__ img, const PatchGeom g, int64_t total_vec) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total_vec; idx += (int64_t)gridDim.x * blockDim.x)
    copy_run<VEC>(img + idx * VEC, in + patch_elem<VEC>(g, idx));
}

// zero row 0 of every [rows_per, pd] sample (the CLS slot of the padded patch matrix)
__global__ void zero_rows_kernel(bf16* __restrict__ out, int samples, int64_t sample_stride, int pd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int pv = pd >> 3;
  if (i < (int64_t)samples * pv) {
    const int s = (int)(i / pv), c = (int)(i - (int64_t)s * pv);
    ((bf16x8*)(out + s * sample_stride))[c] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
}

__global__ void cls_row_kernel(const float* __restrict__ cls, const float* __restrict__ pos, float* __restrict__ x, int MB, int64_t row_stride, int d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < MB * d) {
    const int c = i % d, mb = i / d;
    x[(int64_t)mb * row_stride + c] = cls[c] + pos[c];
  }
}

// dpos[n, c] += sum_mb dx[mb, n, c];  dcls[c] += sum_mb dx[mb, 0, c]
__global__ void embed_bwd_kernel(const float* __restrict__ dx, float* __restrict__ dpos, float* __restrict__ dcls, int MB, int N, int d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over N*d/4
  const int dv = d >> 2;
  if (i >= (int64_t)N * dv) return;
  const int n = (int)(i / dv), c = (int)(i - (int64_t)n * dv) * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int mb = 0; mb < MB; ++mb) acc += *(const f32x4*)(dx + ((int64_t)mb * N + n) * d + c);
  f32x4* dp = (f32x4*)(dpos + (int64_t)n * d + c);
  *dp += acc;
  if (n == 0) *(f32x4*)(dcls + c) += acc;
}

__global__ void cast_kernel(const float* __restrict__ src, bf16* __restrict__ dst, int64_t n) {
  const int64_t nv = n >> 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4 a = ((const f32x4*)src)[2 * i], c = ((const f32x4*)src)[2 * i + 1];
    ((bf16x8*)dst)[i] = to_bf16x8(a, c);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 7)) dst[(nv << 3) + threadIdx.x] = f2bf(src[(nv << 3) + threadIdx.x]);
}

// out = a + b (fp32) with a bf16 copy of the sum: the fan-out sum of two gradient tensors (cross_vit._FanOut) handed on in both dtypes,
// one pass instead of an add and a cast (n % 8 == 0: rows of d % 8 == 0 floats)
__global__ void add_cast_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, bf16* __restrict__ outb, int64_t n) {
  const int64_t nv = n >> 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4 s0 = ((const f32x4*)a)[2 * i] + ((const f32x4*)b)[2 * i], s1 = ((const f32x4*)a)[2 * i + 1] + ((const f32x4*)b)[2 * i + 1];
    ((f32x4*)out)[2 * i] = s0;
    ((f32x4*)out)[2 * i + 1] = s1;
    ((bf16x8*)outb)[i] = to_bf16x8(s0, s1);
  }
}

// dst[r, :] (and dst2[r, :]) = a[r, :] + b[r, :] over `rows` rows of d columns; a missing operand is zero; every tensor has its own
// dtype and row stride (the B CLS rows of a [B, N, d] token tensor are rows of stride N d).  One block per row.  The CLS-row
// bookkeeping of the fusions (model_cross.py:140-142: split off / re-attach the CLS token, and the same on the gradients) in ONE launch
// per site instead of 2-4 strided torch copies / adds.  dst may be a or b.
template <typename T>
__device__ __forceinline__ float ld1(const void* p, int64_t i) {
  if constexpr (sizeof(T) == 4) return ((const float*)p)[i];
  else return bf2f(((const bf16*)p)[i]);
}
__device__ __forceinline__ float ld_dt(const void* p, int dt, int64_t i) { return dt == XVIT_F32 ? ld1<float>(p, i) : ld1<bf16>(p, i); }
__device__ __forceinline__ void st_dt(void* p, int dt, int64_t i, float v) {
  if (dt == XVIT_F32) ((float*)p)[i] = v;
  else ((bf16*)p)[i] = f2bf(v);
}
__global__ __launch_bounds__(256) void rows_combine_kernel(void* __restrict__ dst, int dst_dt, int64_t ld_dst, void* __restrict__ dst2, int dst2_dt, int64_t ld_dst2,
                                                           const void* a, int a_dt, int64_t ld_a, const void* b, int b_dt, int64_t ld_b, int d) {
  const int64_t r = blockIdx.x;
  for (int c = threadIdx.x; c < d; c += 256) {
    float v = 0.f;
    if (a) v = ld_dt(a, a_dt, r * ld_a + c);
    if (b) v += ld_dt(b, b_dt, r * ld_b + c);
    if (dst_dt == XVIT_BF16) v = bf2f(f2bf(v));      // what the bf16 destination holds is what a second destination gets too
    st_dt(dst, dst_dt, r * ld_dst + c, v);
    if (dst2) st_dt(dst2, dst2_dt, r * ld_dst2 + c, v);
  }
}

__global__ void zero_f32_kernel(float* __restrict__ p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0.f;
}

// column sums: block = 64 column-quads (256 columns) x 4 row lanes over a contiguous slab of rows;
// 4 independent 16-B loads in flight per thread; one atomic per column per block
template <typename T>
__device__ __forceinline__ f32x4 ld4(const T* p) {
  if constexpr (sizeof(T) == 4) {
    return *(const f32x4*)p;
  } else {
    const bf16x4 v = *(const bf16x4*)p;
    return f32x4{bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])};
  }
}
// `part` != nullptr: deterministic form — each row chunk stores its partial sums to part[chunk][n] (plain stores) and
// colsum_reduce_kernel adds them up in chunk order; otherwise the chunks meet in fp32 atomics on `out`.
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ x, int64_t ldx, float* __restrict__ out, float* __restrict__ part, int rows, int n,
                                                     int rows_per_block) {
  __shared__ f32x4 red[4][64];
  const int cq = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + cq) * 4;
  const int r_begin = blockIdx.y * rows_per_block, r_end = min(rows, r_begin + rows_per_block);
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
  if (col < n) {
    const T* base = x + col;
    int r = r_begin + rl;
    for (; r + 12 < r_end; r += 16) {
      a0 += ld4(base + (int64_t)r * ldx);
      a1 += ld4(base + (int64_t)(r + 4) * ldx);
      a2 += ld4(base + (int64_t)(r + 8) * ldx);
      a3 += ld4(base + (int64_t)(r + 12) * ldx);
    }
    for (; r < r_end; r += 4) a0 += ld4(base + (int64_t)r * ldx);
  }
  red[rl][cq] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (rl == 0 && col < n) {
    const f32x4 acc = red[0][cq] + red[1][cq] + red[2][cq] + red[3][cq];
    if (part) {
      *(f32x4*)(part + (int64_t)blockIdx.y * n + col) = acc;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) unsafeAtomicAdd(out + col + e, acc[e]);
    }
  }
}

// out[c] (+)= sum over chunks of part[chunk][c], in chunk order (bit-reproducible)
__global__ void colsum_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int chunks, int n, int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  float acc = accumulate ? out[c] : 0.f;
  for (int k = 0; k < chunks; ++k) acc += part[(int64_t)k * n + c];
  out[c] = acc;
}

template <typename T>
__global__ void dropout_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n, const Dropout drop_in) {
  const Dropout drop = drop_in.at_run_time();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = drop.keep((uint64_t)i) ? (T)((float)x[i] * drop.inv) : (T)0.0f;
}

// ---- tiny fp32 linear (num_classes head) ---------------------------------------------------
__global__ void small_linear_fwd_kernel(const bf16* __restrict__ x, int64_t ldx, const float* __restrict__ W, const float* __restrict__ b,
                                        float* __restrict__ y, int M, int N, int K) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (wave >= M * N) return;
  const int m = wave / N, n = wave - m * N;
  float acc = 0.f;
  for (int k = lane; k < K; k += 64) acc = fmaf(bf2f(x[(int64_t)m * ldx + k]), W[(int64_t)n * K + k], acc);
  acc = wave_sum(acc);
  if (lane == 0) y[wave] = acc + (b ? b[n] : 0.f);
}

// grid (K / 256, row chunks): a block handles `rows` consecutive samples for 256 columns; the dW / db partial sums of
// the chunks meet in fp32 atomics (the caller zero-fills dW and db).  One thread per column looping over ALL rows
// (the first version) is a chain of M dependent loads: 119 us at M = 126 for 0.8 MB of data.
__global__ void small_linear_bwd_kernel(const float* __restrict__ dy, const bf16* __restrict__ x, int64_t ldx, const float* __restrict__ W,
                                        const bf16* __restrict__ z, int64_t ldz, bf16* __restrict__ dx, int64_t lddx, float* __restrict__ dW,
                                        float* __restrict__ db, int M, int N, int K, int rows) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int m0 = blockIdx.y * rows, m1 = min(M, m0 + rows);
  if (k < K) {
    for (int m = m0; m < m1; ++m) {
      float acc = 0.f;
      for (int n = 0; n < N; ++n) acc = fmaf(dy[m * N + n], W[(int64_t)n * K + k], acc);
      if (z) acc *= dgelu_f(bf2f(z[(int64_t)m * ldz + k]));
      dx[(int64_t)m * lddx + k] = f2bf(acc);
    }
    for (int n = 0; n < N; ++n) {
      float acc = 0.f;
      for (int m = m0; m < m1; ++m) acc = fmaf(dy[m * N + n], bf2f(x[(int64_t)m * ldx + k]), acc);
      unsafeAtomicAdd(dW + (int64_t)n * K + k, acc);
    }
  }
  if (k < N) {   // block column 0 only (K >= N)
    float acc = 0.f;
    for (int m = m0; m < m1; ++m) acc += dy[m * N + k];
    unsafeAtomicAdd(db + k, acc);
  }
}

}  // namespace xvit

using namespace xvit;

extern "C" int xvit_patchify(const void* img, int img_dtype, void* out, int B, int M, int D, int H, int W, int dp, int hp, int wp,
                             int64_t stride_b, int64_t stride_m, int row_off, int zero_rows, int64_t zero_row_stride, xvit_stream_t stream) {
  XVIT_REQUIRE(img && out, "xvit_patchify: null pointer");
  XVIT_REQUIRE_PATCH_GRID("xvit_patchify", dtype_ok(img_dtype));
  XVIT_REQUIRE(stride_b > 0 && stride_m > 0 && row_off >= 0 && zero_rows >= 0, "xvit_patchify: bad output placement");
  XVIT_REQUIRE(zero_rows == 0 || (dp * hp * wp) % 8 == 0, "xvit_patchify: zero rows need patch_dim %% 8 == 0");
  const int64_t total = (int64_t)B * M * D * H * W;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = (wp % 8 == 0) && ((reinterpret_cast<uintptr_t>(img) & 31) == 0);
  bf16* o = (bf16*)out;
  const PatchGeom g = {M, D, H, W, dp, hp, wp, stride_b, stride_m, row_off};
  by_dtype_vec(img_dtype, vec, [&](auto t, auto v) {
    using T = decltype(t);
    const int64_t work = total / decltype(v)::value;
    hipLaunchKernelGGL((patchify_kernel<T, decltype(v)::value>), dim3(grid_for(work, 256)), dim3(256), 0, s, (const T*)img, o, g, work);
  });
  if (zero_rows > 0) {
    const int pd = dp * hp * wp;
    const int64_t work = (int64_t)zero_rows * (pd / 8);
    hipLaunchKernelGGL(zero_rows_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, o, zero_rows, zero_row_stride * pd, pd);
  }
  return check_launch("xvit_patchify");
}

extern "C" int xvit_unpatchify(const float* patches, void* img, int img_dtype, int B, int M, int D, int H, int W, int dp, int hp, int wp, int64_t stride_b,
                               int64_t stride_m, int row_off, xvit_stream_t stream) {
  XVIT_REQUIRE(patches && img, "xvit_unpatchify: null pointer");
  XVIT_REQUIRE_PATCH_GRID("xvit_unpatchify", dtype_ok(img_dtype));
  XVIT_REQUIRE(stride_b > 0 && stride_m > 0 && row_off >= 0, "xvit_unpatchify: bad input placement");
  const int64_t total = (int64_t)B * M * D * H * W;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = (wp % 8 == 0) && ((reinterpret_cast<uintptr_t>(patches) & 31) == 0) && ((reinterpret_cast<uintptr_t>(img) & 31) == 0);
  const PatchGeom g = {M, D, H, W, dp, hp, wp, stride_b, stride_m, row_off};
  by_dtype_vec(img_dtype, vec, [&](auto t, auto v) {
    using T = decltype(t);
    const int64_t work = total / decltype(v)::value;
    hipLaunchKernelGGL((unpatchify_kernel<T, decltype(v)::value>), dim3(grid_for(work, 256)), dim3(256), 0, s, patches, (T*)img, g, work);
  });
  return check_launch("xvit_unpatchify");
}

extern "C" int xvit_cls_row_fwd(const float* cls, const float* pos, float* x, int MB, int N, int d, xvit_stream_t stream) {
  XVIT_REQUIRE(cls && pos && x && MB > 0 && N > 0 && d > 0, "xvit_cls_row_fwd: bad arguments");
  hipLaunchKernelGGL(cls_row_kernel, dim3((MB * d + 255) / 256), dim3(256), 0, (hipStream_t)stream, cls, pos, x, MB, (int64_t)N * d, d);
  return check_launch("xvit_cls_row_fwd");
}

extern "C" int xvit_embed_bwd(const float* dx, float* dpos, float* dcls, int MB, int N, int d, xvit_stream_t stream) {
  XVIT_REQUIRE(dx && dpos && dcls && MB > 0 && N > 0 && d > 0 && d % 4 == 0, "xvit_embed_bwd: bad arguments");
  const int64_t work = (int64_t)N * (d / 4);
  hipLaunchKernelGGL(embed_bwd_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dx, dpos, dcls, MB, N, d);
  return check_launch("xvit_embed_bwd");
}

extern "C" int xvit_cast_f32_bf16(const float* src, void* dst, int64_t n, xvit_stream_t stream) {
  XVIT_REQUIRE(src && dst && n > 0, "xvit_cast_f32_bf16: bad arguments");
  XVIT_REQUIRE(aligned16({src, dst}), "xvit_cast_f32_bf16: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(cast_kernel, dim3(grid_for(n / 8 + 1, 256)), dim3(256), 0, (hipStream_t)stream, src, (bf16*)dst, n);
  return check_launch("xvit_cast_f32_bf16");
}

extern "C" int xvit_add_cast_f32_bf16(const float* a, const float* b, float* out, void* out_bf16, int64_t n, xvit_stream_t stream) {
  XVIT_REQUIRE(a && b && out && out_bf16 && n > 0 && n % 8 == 0, "xvit_add_cast_f32_bf16: bad arguments (n must be a positive multiple of 8)");
  XVIT_REQUIRE(aligned16({a, b, out, out_bf16}), "xvit_add_cast_f32_bf16: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(add_cast_kernel, dim3(grid_for(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, (bf16*)out_bf16, n);
  return check_launch("xvit_add_cast_f32_bf16");
}

extern "C" int xvit_rows_combine(void* dst, int dst_dtype, int64_t ld_dst, void* dst2, int dst2_dtype, int64_t ld_dst2, const void* a, int a_dtype, int64_t ld_a,
                                 const void* b, int b_dtype, int64_t ld_b, int rows, int d, xvit_stream_t stream) {
  XVIT_REQUIRE(dst && rows > 0 && d > 0, "xvit_rows_combine: bad arguments");
  auto ok = [](int dt) { return dt == XVIT_F32 || dt == XVIT_BF16; };
  XVIT_REQUIRE(ok(dst_dtype) && (!dst2 || ok(dst2_dtype)) && (!a || ok(a_dtype)) && (!b || ok(b_dtype)), "xvit_rows_combine: dtypes must be XVIT_F32 or XVIT_BF16");
  XVIT_REQUIRE(ld_dst >= d && (!dst2 || ld_dst2 >= d) && (!a || ld_a >= d) && (!b || ld_b >= d), "xvit_rows_combine: a row stride is smaller than d");
  hipLaunchKernelGGL(rows_combine_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, dst, dst_dtype, ld_dst, dst2, dst2_dtype, ld_dst2, a, a_dtype, ld_a, b, b_dtype, ld_b, d);
  return check_launch("xvit_rows_combine");
}

static int colsum_rows_per_block(int rows, int n) {
  const int gx = (n / 4 + 63) / 64;
  int rpb = 64;                                   // rows per block: >= 64, and at most ~2048 blocks in all
  while ((int64_t)gx * ((rows + rpb - 1) / rpb) > 2048) rpb *= 2;
  return rpb;
}

extern "C" int64_t xvit_colsum_workspace_bytes(int rows, int n) {
  if (rows <= 0 || n <= 0) return 0;
  const int rpb = colsum_rows_per_block(rows, n);
  return (int64_t)((rows + rpb - 1) / rpb) * n * (int64_t)sizeof(float);
}

extern "C" int xvit_colsum(const void* x, int x_dtype, int64_t ldx, float* out, int rows, int n, int accumulate, float* workspace,
                           int64_t workspace_bytes, xvit_stream_t stream) {
  XVIT_REQUIRE(x && out && rows > 0 && n > 0, "xvit_colsum: bad arguments");
  XVIT_REQUIRE(n % 4 == 0 && ldx % 4 == 0, "xvit_colsum: n and ldx must be multiples of 4");
  XVIT_REQUIRE(!workspace || workspace_bytes >= xvit_colsum_workspace_bytes(rows, n), "xvit_colsum: workspace too small (%lld bytes)", (long long)workspace_bytes);
  hipStream_t s = (hipStream_t)stream;
  if (!accumulate && !workspace)   // a kernel, not hipMemsetAsync: the memset node was observed not to replay from a captured HIP graph
    hipLaunchKernelGGL(zero_f32_kernel, dim3((n + 255) / 256), dim3(256), 0, s, out, n);
  const int gx = (n / 4 + 63) / 64;
  const int rpb = colsum_rows_per_block(rows, n);
  const dim3 grid(gx, (rows + rpb - 1) / rpb), block(256);
  by_dtype(x_dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((colsum_kernel<T>), grid, block, 0, s, (const T*)x, ldx, out, workspace, rows, n, rpb);
  });
  if (workspace) hipLaunchKernelGGL(colsum_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, s, workspace, out, (int)grid.y, n, accumulate);
  return check_launch("xvit_colsum");
}

extern "C" int xvit_dropout(const void* x, void* y, int dtype, int64_t n, float p, uint64_t seed, xvit_stream_t stream) {
  XVIT_REQUIRE(x && y && n > 0 && p >= 0.f && p < 1.f, "xvit_dropout: bad arguments");
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((dropout_kernel<T>), dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, n, Dropout(p, seed));
  });
  return check_launch("xvit_dropout");
}

extern "C" int xvit_small_linear_fwd(const void* x, int64_t ldx, const float* W, const float* b, float* y, int M, int N, int K, xvit_stream_t stream) {
  XVIT_REQUIRE(x && W && y && M > 0 && N > 0 && K > 0, "xvit_small_linear_fwd: bad arguments");
  const int waves = M * N;
  hipLaunchKernelGGL(small_linear_fwd_kernel, dim3((waves + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx, W, b, y, M, N, K);
  return check_launch("xvit_small_linear_fwd");
}

extern "C" int xvit_small_linear_bwd(const float* dy, const void* x, int64_t ldx, const float* W, const void* z, int64_t ldz, void* dx, int64_t lddx,
                                     float* dW, float* db, int M, int N, int K, int deterministic, xvit_stream_t stream) {
  XVIT_REQUIRE(dy && x && W && dx && dW && db && M > 0 && N > 0 && K >= N, "xvit_small_linear_bwd: bad arguments");
  const int rows = deterministic ? M : 8;   // one row chunk: every dW / db element receives exactly one add (bit-reproducible, slower)
  hipLaunchKernelGGL(small_linear_bwd_kernel, dim3((K + 255) / 256, (M + rows - 1) / rows), dim3(256), 0, (hipStream_t)stream, dy, (const bf16*)x, ldx, W,
                     (const bf16*)z, ldz, (bf16*)dx, lddx, dW, db, M, N, K, rows);
  return check_launch("xvit_small_linear_bwd");
}

// ------------------------------------------------------------------------------------------
// Fused multi-tensor Adam (reference: torch.optim.Adam(lr, weight_decay) at model_cross.py:277 — L2 decay added
// to the gradient, bias-corrected moments, eps outside the square root).  One launch updates every tensor of a
// parameter group: p, m, v in fp32 and, when given, the bf16 operand copy of p (so no separate cast pass).
// ------------------------------------------------------------------------------------------
namespace xvit {
struct AdamTensor { float* p; const float* g; float* m; float* v; bf16* shadow; int64_t n; };
constexpr int ADAM_CHUNK = 16384;   // elements per block

// The chunk of this block: its tensor's row of the table, with EXTRAS its row of the extras table (zeros otherwise), and the elements
// [begin, end) of that tensor.  Both rows are fetched before either is used: one scalar-load round trip per block, not two.
struct AdamChunk { AdamTensor t; xvit_adamw_extra x; int64_t begin, end; };
template <bool EXTRAS>
__device__ __forceinline__ AdamChunk adam_chunk(const AdamTensor* __restrict__ table, const xvit_adamw_extra* __restrict__ extras,
                                                const int2* __restrict__ chunks) {
  const int2 ch = chunks[blockIdx.x];
  const AdamTensor t = table[ch.x];
  xvit_adamw_extra x = {nullptr, 0.f, 0.f};
  if constexpr (EXTRAS) x = extras[ch.x];
  const int64_t begin = (int64_t)ch.y * ADAM_CHUNK;
  return {t, x, begin, begin + ADAM_CHUNK < t.n ? begin + ADAM_CHUNK : t.n};
}

// 16-byte accesses for every array of the tensor, the average included when there is one (the chunk start is a multiple of 16384
// elements, so the base decides)
__device__ __forceinline__ bool adam_vec_ok(const AdamTensor& t, const float* ema = nullptr) {
  return ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m) | reinterpret_cast<uintptr_t>(t.v) |
           reinterpret_cast<uintptr_t>(ema)) & 15) == 0 && (!t.shadow || (reinterpret_cast<uintptr_t>(t.shadow) & 7) == 0);
}

// The element loops of one chunk.  vec: quad(i) on every whole group of four elements, 16 bytes per array and lane, then scalar(i) on
// the up to three left over; otherwise scalar(i) throughout.
template <class Quad, class Scalar>
__device__ __forceinline__ void adam_walk(const AdamChunk& c, bool vec, Quad quad, Scalar scalar) {
  if (vec) {
    for (int64_t i = c.begin + threadIdx.x * 4; i + 3 < c.end; i += 256 * 4) quad(i);
    const int64_t tail = c.begin + ((c.end - c.begin) & ~(int64_t)3);
    for (int64_t i = tail + threadIdx.x; i < c.end; i += 256) scalar(i);
  } else {
    for (int64_t i = c.begin + threadIdx.x; i < c.end; i += 256) scalar(i);
  }
}

// ADAM_PLAIN (xvit_adam_step / xvit_adam_step_dev): one rate for the launch, group-wide decay `wd` by value, L2 decay added to the
// gradient; no extras table, no average.  The other two (xvit_adamw_step / xvit_adamw_step_dev) read one xvit_adamw_extra row per
// tensor: its own rate scale and decay and, when non-null, a weight average updated in the same pass (the 16-byte path then needs it
// 16-byte aligned too).  ADAM_COUPLED is the plain update with those; ADAM_DECOUPLED does p *= 1 - lr_t wd_t first (torch.optim.AdamW:
// the raw rate, not lr / bc1), then Adam on g * grad_scale.
enum AdamMode { ADAM_PLAIN, ADAM_COUPLED, ADAM_DECOUPLED };

// FROM_RECORD = false: rate, bias corrections, gradient scale and the average's weight arrive by value.  true: they are read from the
// device-resident record the step prologue wrote, so a captured launch follows the step count, the learning rate and the clip
// coefficient of each replay; a step the prologue flagged as skipped returns before touching anything.  The average e += w (p' - e)
// and the bf16 copy are formed from the p' just stored, in the same registers.  The step count the warm-up reads is the one the
// prologue already advanced.
template <bool FROM_RECORD, AdamMode MODE>
__global__ __launch_bounds__(256) void adam_kernel(const AdamTensor* __restrict__ table, const xvit_adamw_extra* __restrict__ extras,
                                                   const int2* __restrict__ chunks, float lr, float lr_over_bc1, float beta1, float beta2, float eps,
                                                   float wd, float inv_sqrt_bc2, float grad_scale, float ema_w, int ema_warmup,
                                                   const xvit_adam_state* __restrict__ st) {
  constexpr bool EXTRAS = MODE != ADAM_PLAIN;
  if constexpr (FROM_RECORD) {
    if (st->skip) return;
    lr_over_bc1 = st->lr_over_bc1;
    inv_sqrt_bc2 = st->inv_sqrt_bc2;
    grad_scale = st->clip_coef;
    if constexpr (EXTRAS) {
      lr = st->lr;
      float d = ema_w;                      // arrives as ema_decay
      if (ema_warmup) {
        const float s = (float)st->step;
        d = fminf(d, (1.0f + s) / (10.0f + s));
      }
      ema_w = 1.0f - d;
    }
  }
  const AdamChunk c = adam_chunk<EXTRAS>(table, extras, chunks);
  const AdamTensor& t = c.t;
  float a = lr_over_bc1, lr_t = lr;
  float* __restrict__ const ema = c.x.ema;
  if constexpr (EXTRAS) {
    a = lr_over_bc1 * c.x.lr_scale; lr_t = lr * c.x.lr_scale; wd = c.x.weight_decay;
  }
  auto upd = [&](float& p, float g, float& m, float& v) {
    if constexpr (MODE == ADAM_DECOUPLED) {
      p *= 1.0f - lr_t * wd;
      g = g * grad_scale;
    } else {
      g = fmaf(g, grad_scale, wd * p);   // g * grad_scale + wd * p with the contraction spelled out: left to the compiler, the 16-byte path of
    }                                    // the folded kernel fused the other product, one rounding apart from what these entry points always gave
    m = beta1 * m + (1.0f - beta1) * g;
    v = beta2 * v + (1.0f - beta2) * g * g;
    p -= a * m / (sqrtf(v) * inv_sqrt_bc2 + eps);
  };
  adam_walk(c, adam_vec_ok(t, ema),
    [&](int64_t i) {
      f32x4 p = *(f32x4*)(t.p + i), m = *(f32x4*)(t.m + i), v = *(f32x4*)(t.v + i), e = {0.f, 0.f, 0.f, 0.f};
      const f32x4 g = *(const f32x4*)(t.g + i);
      if constexpr (EXTRAS) { if (ema) e = *(f32x4*)(ema + i); }
#pragma unroll
      for (int k = 0; k < 4; ++k) {   // vector elements cannot bind to references: go through scalars
        float pe = p[k], me = m[k], ve = v[k];
        upd(pe, g[k], me, ve);
        p[k] = pe; m[k] = me; v[k] = ve;
        if constexpr (EXTRAS) e[k] = e[k] + ema_w * (pe - e[k]);
      }
      *(f32x4*)(t.p + i) = p; *(f32x4*)(t.m + i) = m; *(f32x4*)(t.v + i) = v;
      if constexpr (EXTRAS) { if (ema) *(f32x4*)(ema + i) = e; }
      if (t.shadow) *(bf16x4*)(t.shadow + i) = to_bf16x4(p);
    },
    [&](int64_t i) {
      upd(t.p[i], t.g[i], t.m[i], t.v[i]);
      const float p = t.p[i];
      if constexpr (EXTRAS) { if (ema) { const float e = ema[i]; ema[i] = e + ema_w * (p - e); } }
      if (t.shadow) t.shadow[i] = f2bf(p);
    });
}

// Exchanges p and the average element by element and writes bf16 of the new p: copies only, so twice is the identity.
__global__ __launch_bounds__(256) void ema_swap_kernel(const AdamTensor* __restrict__ table, const xvit_adamw_extra* __restrict__ extras,
                                                       const int2* __restrict__ chunks) {
  const AdamChunk c = adam_chunk<true>(table, extras, chunks);
  const AdamTensor& t = c.t;
  float* const ema = c.x.ema;
  if (!ema) return;
  adam_walk(c, adam_vec_ok(t, ema),
    [&](int64_t i) {
      const f32x4 p = *(f32x4*)(t.p + i), e = *(f32x4*)(ema + i);
      *(f32x4*)(t.p + i) = e; *(f32x4*)(ema + i) = p;
      if (t.shadow) *(bf16x4*)(t.shadow + i) = to_bf16x4(e);
    },
    [&](int64_t i) {
      const float p = t.p[i], e = ema[i];
      t.p[i] = e; ema[i] = p;
      if (t.shadow) t.shadow[i] = f2bf(e);
    });
}

// Sum of g*g over one 16384-element chunk per block, written with ONE plain store to partials[blockIdx.x]: no float atomics, so the
// norm is bit-identical from run to run.  Summation order per chunk (all fp32, the products fused into the adds): 16-byte path: four
// accumulators per thread, 16 sequential adds each (one more for a tail element), 2 levels to join them; scalar path: 64 sequential
// adds; then 6 levels across the wave and 3 adds across the four waves, 2 of them on any path.  With non-negative terms the relative
// error is at most the roundings on the longest path: (64 + 6 + 2) * 2^-24 = 4.3e-6 (scalar), (17 + 2 + 6 + 2) * 2^-24 = 1.6e-6 (16-byte).
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const AdamTensor* __restrict__ table, const int2* __restrict__ chunks, float* __restrict__ partials) {
  __shared__ float wave_part[4];
  const AdamChunk c = adam_chunk<false>(table, nullptr, chunks);
  const AdamTensor& t = c.t;
  const int64_t begin = c.begin, end = c.end;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (adam_vec_ok(t)) {
#pragma unroll 4
    for (int64_t i = begin + threadIdx.x * 4; i + 3 < end; i += 256 * 4) {
      const f32x4 g = *(const f32x4*)(t.g + i);
      a0 = fmaf(g[0], g[0], a0); a1 = fmaf(g[1], g[1], a1); a2 = fmaf(g[2], g[2], a2); a3 = fmaf(g[3], g[3], a3);
    }
    const int64_t tail = begin + ((end - begin) & ~(int64_t)3);
    for (int64_t i = tail + threadIdx.x; i < end; i += 256) a0 = fmaf(t.g[i], t.g[i], a0);
  } else {
#pragma unroll 4
    for (int64_t i = begin + threadIdx.x; i < end; i += 256) a0 = fmaf(t.g[i], t.g[i], a0);
  }
  const float w = wave_sum((a0 + a1) + (a2 + a3));   // every lane of every wave gets here: the DPP steps need the full wave
  if (lane_id() == 0) wave_part[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

// One block.  Sums the chunk partials in a fixed order in double (thread i takes i, i + 256, ...; then a fixed tree), and thread 0
// writes the record the Adam kernel reads: norm, clip coefficient, the advanced step count and its bias corrections.
__global__ __launch_bounds__(256) void adam_prologue_kernel(const float* __restrict__ partials, int n_partials, xvit_adam_state* __restrict__ st, float max_norm,
                                                            float beta1, float beta2, int skip_nonfinite) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += 256) s += (double)partials[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(part[0]);
  float coef = 1.0f;
  if (max_norm < INFINITY) {            // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1), a NaN stays a NaN
    const float c = max_norm / (norm + 1e-6f);
    coef = (c < 1.0f || c != c) ? c : 1.0f;
  }
  st->grad_norm = norm;
  st->clip_coef = coef;
  if (skip_nonfinite && !(fabsf(norm) < INFINITY)) {   // inf or NaN: the step did not happen
    st->skip = 1;
    st->skipped += 1;
    return;
  }
  const int64_t step = st->step + 1;
  st->step = step;
  st->skip = 0;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);   // as xvit_adam_step does on the host
  st->lr_over_bc1 = (float)((double)st->lr / bc1);
  st->inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
}

// adam_kernel's by-value arguments, in its order.  With a record (st) the kernel reads lr, lr_over_bc1, inv_sqrt_bc2 and grad_scale from it
// and takes ema_w as the average's DECAY; ADAM_PLAIN uses neither lr, ema_w nor ema_warmup, the other modes take wd from the extras.
struct AdamScalars { float lr, lr_over_bc1, beta1, beta2, eps, wd, inv_sqrt_bc2, grad_scale, ema_w; int ema_warmup; };

static void adam_launch(AdamMode mode, const void* table, const xvit_adamw_extra* extras, const void* chunks, int n_chunks, const AdamScalars& a,
                        const xvit_adam_state* st, xvit_stream_t stream) {
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const AdamTensor*)table, extras, (const int2*)chunks, a.lr, a.lr_over_bc1,
                       a.beta1, a.beta2, a.eps, a.wd, a.inv_sqrt_bc2, a.grad_scale, a.ema_w, a.ema_warmup, st);
  };
  switch (mode) {
    case ADAM_PLAIN:     st ? go(adam_kernel<true, ADAM_PLAIN>)     : go(adam_kernel<false, ADAM_PLAIN>);     break;
    case ADAM_COUPLED:   st ? go(adam_kernel<true, ADAM_COUPLED>)   : go(adam_kernel<false, ADAM_COUPLED>);   break;
    case ADAM_DECOUPLED: st ? go(adam_kernel<true, ADAM_DECOUPLED>) : go(adam_kernel<false, ADAM_DECOUPLED>); break;
  }
}
}  // namespace xvit

extern "C" int xvit_adam_step(const void* table_dev, const void* chunks_dev, int n_chunks, float lr, float beta1, float beta2, float eps,
                              float weight_decay, int step, float grad_scale, xvit_stream_t stream) {
  XVIT_REQUIRE(table_dev && chunks_dev && n_chunks > 0 && step >= 1, "xvit_adam_step: bad arguments");
  XVIT_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "xvit_adam_step: bad hyper-parameters");
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  xvit::adam_launch(xvit::ADAM_PLAIN, table_dev, nullptr, chunks_dev, n_chunks,
                    {0.f, (float)(lr / bc1), beta1, beta2, eps, weight_decay, (float)(1.0 / sqrt(bc2)), grad_scale, 0.f, 0}, nullptr, stream);
  return xvit::check_launch("xvit_adam_step");
}

extern "C" int xvit_grad_sqnorm_partials(const void* table_dev, const void* chunks_dev, int n_chunks, float* partials_dev, xvit_stream_t stream) {
  XVIT_REQUIRE(table_dev && chunks_dev && partials_dev, "xvit_grad_sqnorm_partials: null table, chunk list or partials");
  XVIT_REQUIRE(n_chunks > 0, "xvit_grad_sqnorm_partials: n_chunks=%d must be positive", n_chunks);
  hipLaunchKernelGGL(xvit::grad_sqnorm_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const xvit::AdamTensor*)table_dev, (const int2*)chunks_dev, partials_dev);
  return xvit::check_launch("xvit_grad_sqnorm_partials");
}

extern "C" int xvit_adam_prologue(const float* partials_dev, int n_partials, xvit_adam_state* state_dev, float max_norm, float beta1, float beta2,
                                  int skip_nonfinite, xvit_stream_t stream) {
  XVIT_REQUIRE(state_dev, "xvit_adam_prologue: null state record");
  XVIT_REQUIRE((partials_dev && n_partials > 0) || (!partials_dev && n_partials == 0),
               "xvit_adam_prologue: partials and n_partials=%d must be given together (n_partials > 0) or both left out", n_partials);
  XVIT_REQUIRE(max_norm > 0.f, "xvit_adam_prologue: max_norm must be positive (INFINITY switches clipping off)");
  XVIT_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "xvit_adam_prologue: betas must lie in [0, 1)");
  hipLaunchKernelGGL(xvit::adam_prologue_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials_dev, n_partials, state_dev, max_norm, beta1, beta2, skip_nonfinite);
  return xvit::check_launch("xvit_adam_prologue");
}

extern "C" int xvit_adam_step_dev(const void* table_dev, const void* chunks_dev, int n_chunks, const xvit_adam_state* state_dev, float beta1, float beta2,
                                  float eps, float weight_decay, xvit_stream_t stream) {
  XVIT_REQUIRE(table_dev && chunks_dev && state_dev, "xvit_adam_step_dev: null table, chunk list or state record");
  XVIT_REQUIRE(n_chunks > 0, "xvit_adam_step_dev: n_chunks=%d must be positive", n_chunks);
  XVIT_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "xvit_adam_step_dev: bad hyper-parameters");
  xvit::adam_launch(xvit::ADAM_PLAIN, table_dev, nullptr, chunks_dev, n_chunks, {0.f, 0.f, beta1, beta2, eps, weight_decay, 0.f, 0.f, 0.f, 0}, state_dev, stream);
  return xvit::check_launch("xvit_adam_step_dev");
}

extern "C" int xvit_adamw_step(const void* table_dev, const xvit_adamw_extra* extras_dev, const void* chunks_dev, int n_chunks, float lr, float beta1,
                               float beta2, float eps, int step, float grad_scale, int decoupled, float ema_weight, xvit_stream_t stream) {
  XVIT_REQUIRE(table_dev && extras_dev && chunks_dev, "xvit_adamw_step: null table, extras or chunk list");
  XVIT_REQUIRE(n_chunks > 0 && step >= 1, "xvit_adamw_step: n_chunks=%d must be positive and step=%d at least 1", n_chunks, step);
  XVIT_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "xvit_adamw_step: bad hyper-parameters");
  XVIT_REQUIRE(ema_weight >= 0.f && ema_weight <= 1.f, "xvit_adamw_step: ema_weight=%g must lie in [0, 1]", (double)ema_weight);
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  xvit::adam_launch(decoupled ? xvit::ADAM_DECOUPLED : xvit::ADAM_COUPLED, table_dev, extras_dev, chunks_dev, n_chunks,
                    {lr, (float)(lr / bc1), beta1, beta2, eps, 0.f, (float)(1.0 / sqrt(bc2)), grad_scale, ema_weight, 0}, nullptr, stream);
  return xvit::check_launch("xvit_adamw_step");
}

extern "C" int xvit_adamw_step_dev(const void* table_dev, const xvit_adamw_extra* extras_dev, const void* chunks_dev, int n_chunks,
                                   const xvit_adam_state* state_dev, float beta1, float beta2, float eps, int decoupled, float ema_decay, int ema_warmup,
                                   xvit_stream_t stream) {
  XVIT_REQUIRE(table_dev && extras_dev && chunks_dev && state_dev, "xvit_adamw_step_dev: null table, extras, chunk list or state record");
  XVIT_REQUIRE(n_chunks > 0, "xvit_adamw_step_dev: n_chunks=%d must be positive", n_chunks);
  XVIT_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "xvit_adamw_step_dev: bad hyper-parameters");
  XVIT_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, "xvit_adamw_step_dev: ema_decay=%g must lie in [0, 1)", (double)ema_decay);
  xvit::adam_launch(decoupled ? xvit::ADAM_DECOUPLED : xvit::ADAM_COUPLED, table_dev, extras_dev, chunks_dev, n_chunks,
                    {0.f, 0.f, beta1, beta2, eps, 0.f, 0.f, 0.f, ema_decay, ema_warmup}, state_dev, stream);
  return xvit::check_launch("xvit_adamw_step_dev");
}

extern "C" int xvit_ema_swap(const void* table_dev, const xvit_adamw_extra* extras_dev, const void* chunks_dev, int n_chunks, xvit_stream_t stream) {
  XVIT_REQUIRE(table_dev && extras_dev && chunks_dev, "xvit_ema_swap: null table, extras or chunk list");
  XVIT_REQUIRE(n_chunks > 0, "xvit_ema_swap: n_chunks=%d must be positive", n_chunks);
  hipLaunchKernelGGL(xvit::ema_swap_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const xvit::AdamTensor*)table_dev, extras_dev, (const int2*)chunks_dev);
  return xvit::check_launch("xvit_ema_swap");
}

// ------------------------------------------------------------------------------------------
// Input stage (reference dataset_ucsf.py:84-88,152-158): MONAI ResizeWithPadOrCropd(spatial_size, constant_values=-1)
// = symmetric pad (before = deficit/2, after = the rest) then centre crop (start = size/2 - target/2), then .float().
// Here: int16 NIfTI payload [nvol, Ds, Hs, Ws] on the device -> bf16 [nvol, D, H, W], one pass, no fp32 volume.
// ------------------------------------------------------------------------------------------
namespace xvit {
__global__ void resize_pad_crop_i16_kernel(const int16_t* __restrict__ src, bf16* __restrict__ dst, int Ds, int Hs, int Ws, int D, int H, int W,
                                           int od, int oh, int ow, float pad_value, int64_t total) {
  // (od, oh, ow): source index = destination index + offset; negative offsets are padding
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int w = (int)(i % W);
    int64_t r = i / W;
    const int h = (int)(r % H); r /= H;
    const int d = (int)(r % D);
    const int64_t vol = r / D;
    const int sd = d + od, sh = h + oh, sw = w + ow;
    const bool in = sd >= 0 && sd < Ds && sh >= 0 && sh < Hs && sw >= 0 && sw < Ws;
    dst[i] = f2bf(in ? (float)src[((vol * Ds + sd) * Hs + sh) * (int64_t)Ws + sw] : pad_value);
  }
}
}  // namespace xvit

extern "C" int xvit_resize_pad_crop_i16(const void* src_i16, void* dst_bf16, int nvol, int Ds, int Hs, int Ws, int D, int H, int W,
                                        float pad_value, xvit_stream_t stream) {
  XVIT_REQUIRE(src_i16 && dst_bf16 && nvol > 0 && Ds > 0 && Hs > 0 && Ws > 0 && D > 0 && H > 0 && W > 0, "xvit_resize_pad_crop_i16: bad arguments");
  // per dimension: size < target -> pad, before = (target - size) / 2; size > target -> crop, start = size / 2 - target / 2
  auto offset = [](int size, int target) { return size >= target ? size / 2 - target / 2 : -((target - size) / 2); };
  const int64_t total = (int64_t)nvol * D * H * W;
  hipLaunchKernelGGL(xvit::resize_pad_crop_i16_kernel, dim3(xvit::grid_for(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const int16_t*)src_i16, (xvit::bf16*)dst_bf16,
                     Ds, Hs, Ws, D, H, W, offset(Ds, D), offset(Hs, H), offset(Ws, W), pad_value, total);
  return xvit::check_launch("xvit_resize_pad_crop_i16");
}

// ------------------------------------------------------------------------------------------
// Placement trace: where does the dispatcher put the workgroups of a stream?  Each block records its XCC
// (XCD) id and HW_ID, then lingers ~`linger_us` so that the launch spreads over every CU the stream may
// use.  Used to map hipExtStreamCreateWithCUMask bits to XCDs and to check the blockIdx -> XCD round-robin
// the GEMM tile remap assumes.
// ------------------------------------------------------------------------------------------
namespace xvit {
__global__ void cu_trace_kernel(uint32_t* __restrict__ out, int linger_us) {
  if (threadIdx.x == 0) {
    uint32_t xcc, hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    out[2 * blockIdx.x] = xcc;
    out[2 * blockIdx.x + 1] = hw;
  }
  const uint64_t t0 = wall_clock64();   // 100 MHz
  while (wall_clock64() - t0 < (uint64_t)linger_us * 100) __builtin_amdgcn_s_sleep(32);
}
}  // namespace xvit

extern "C" int xvit_cu_trace(uint32_t* out, int nblocks, int linger_us, xvit_stream_t stream) {
  XVIT_REQUIRE(out && nblocks > 0 && linger_us >= 0 && linger_us <= 10000, "xvit_cu_trace: bad arguments");
  hipLaunchKernelGGL(xvit::cu_trace_kernel, dim3((unsigned)nblocks), dim3(64), 0, (hipStream_t)stream, out, linger_us);
  return xvit::check_launch("xvit_cu_trace");
}
