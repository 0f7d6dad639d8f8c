// Typed element access of the input-stage kernels (augment_apply.h, contrast.hip) and the token-path kernels (token_rows.h): volumes are
// int16, bf16 or fp32 on the way in, bf16 or fp32 on the way out, and every value passes through fp32 in between (copy_run8 excepted).
#pragma once
#include "xvit_common.h"

namespace xvit {

__device__ __forceinline__ float src_f(int16_t v) { return (float)v; }
__device__ __forceinline__ float src_f(bf16 v) { return bf2f(v); }
__device__ __forceinline__ float src_f(float v) { return v; }
__device__ __forceinline__ void store_one(bf16* p, float v) { *p = f2bf(v); }
__device__ __forceinline__ void store_one(float* p, float v) { *p = v; }

// 8 consecutive source elements at any element-aligned address (a crop offset decides the alignment, not the kernel)
template <typename S>
__device__ __forceinline__ void load_run8(const S* p, float (&v)[8]) {
  struct Run { S e[8]; } r;
  __builtin_memcpy(&r, __builtin_assume_aligned(p, sizeof(S)), sizeof(r));
  for (int i = 0; i < 8; ++i) v[i] = src_f(r.e[i]);
}
// ... from a 16-byte aligned address
__device__ __forceinline__ void load_run8_aligned(const bf16* p, float (&v)[8]) {
  const bf16x8 r = *(const bf16x8*)p;
  for (int i = 0; i < 8; ++i) v[i] = bf2f(r[i]);
}
__device__ __forceinline__ void load_run8_aligned(const float* p, float (&v)[8]) {
  const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
  for (int i = 0; i < 4; ++i) v[i] = a[i], v[4 + i] = b[i];
}

// 8 consecutive elements to a 16-byte aligned address; 4 to an address aligned to the run's own size
__device__ __forceinline__ void store_run8(bf16* p, const float (&v)[8]) {
  bf16x8 o;
  for (int i = 0; i < 8; ++i) o[i] = f2bf(v[i]);
  *(bf16x8*)p = o;
}
__device__ __forceinline__ void store_run8(float* p, const float (&v)[8]) {
  *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
  *(f32x4*)(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
}
__device__ __forceinline__ void store_run4(bf16* p, const f32x4& v) { *(bf16x4*)p = to_bf16x4(v); }
__device__ __forceinline__ void store_run4(float* p, const f32x4& v) { *(f32x4*)p = v; }

// 8 consecutive elements from one 16-byte aligned address to another.  The same type on both sides moves the bits (16 or 2 x 16 bytes,
// no conversion: a signalling NaN keeps its payload); any other pair goes through fp32.
template <typename D, typename S>
__device__ __forceinline__ void copy_run8(D* dst, const S* src) {
  float v[8];
  load_run8_aligned(src, v);
  store_run8(dst, v);
}
__device__ __forceinline__ void copy_run8(bf16* dst, const bf16* src) { *(bf16x8*)dst = *(const bf16x8*)src; }
__device__ __forceinline__ void copy_run8(float* dst, const float* src) {
  const f32x4 a = *(const f32x4*)src, b = *(const f32x4*)(src + 4);
  *(f32x4*)dst = a;
  *(f32x4*)(dst + 4) = b;
}

}  // namespace xvit
