// What the kernels that take foreground boxes share (volume_bbox.hip, volume_components.hip): the box of a set of voxels and its
// merges, the foreground mask of a 16-byte run, the chunk rule of the partial boxes, and the launch of the finish kernel that turns
// partial boxes into boxes, the sample crop and the fold.
#pragma once
#include "volume_io.h"

namespace xvit {

constexpr int kBoxThreads = 256;
constexpr int kBoxWaves = kBoxThreads / kWave;

// volume_bbox.hip: the chunk rule of the header, parts per volume and voxels per part
int bbox_parts(int nvol, int64_t nvox, int64_t* chunk_out);

struct Box {
  int z0, z1, y0, y1, x0, x1, n;   // inclusive; empty: lo = size, hi = -1
  __device__ __forceinline__ void add(int z, int y, int xa, int xb) {
    z0 = min(z0, z), z1 = max(z1, z), y0 = min(y0, y), y1 = max(y1, y), x0 = min(x0, xa), x1 = max(x1, xb);
  }
  __device__ __forceinline__ void merge(const Box& o) {
    z0 = min(z0, o.z0), z1 = max(z1, o.z1), y0 = min(y0, o.y0), y1 = max(y1, o.y1), x0 = min(x0, o.x0), x1 = max(x1, o.x1), n += o.n;
  }
};
__device__ __forceinline__ Box empty_box(int Ds, int Hs, int Ws) { return Box{Ds, -1, Hs, -1, Ws, -1, 0}; }

// bit e of the result: element e of the 16-byte run is foreground (NaN compares false)
template <class S>
__device__ __forceinline__ uint32_t fg_mask(const uint4& r, float fg) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (sizeof(S) == 4) {
      m |= (uint32_t)(__builtin_bit_cast(float, w[i]) > fg) << i;
    } else if constexpr (std::is_same<S, bf16>::value) {
      m |= (uint32_t)(__builtin_bit_cast(float, w[i] << 16) > fg) << (2 * i);
      m |= (uint32_t)(__builtin_bit_cast(float, w[i] & 0xFFFF0000u) > fg) << (2 * i + 1);
    } else {
      m |= (uint32_t)((float)(int16_t)(w[i] & 0xFFFFu) > fg) << (2 * i);
      m |= (uint32_t)((float)(int16_t)(w[i] >> 16) > fg) << (2 * i + 1);
    }
  }
  return m;
}

// E consecutive voxels from flat index `flat` of the volume, foreground where `mask` is set.  The two divisions are paid by runs that hold
// foreground only; a run that crosses a row end walks its elements.
template <int E>
__device__ __forceinline__ void add_run(Box& b, uint32_t mask, uint32_t flat, int Hs, int Ws) {
  if (mask == 0) return;
  const uint32_t row = flat / (uint32_t)Ws, z = row / (uint32_t)Hs;
  int x = (int)(flat - row * (uint32_t)Ws), y = (int)(row - z * (uint32_t)Hs), zi = (int)z;
  b.n += __popc(mask);
  if (E == 1 || x + E <= Ws) {
    b.add(zi, y, x + (__ffs(mask) - 1), x + (31 - __clz(mask)));
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if ((mask >> e) & 1u) b.add(zi, y, x, x);
      if (++x == Ws) {
        x = 0;
        if (++y == Hs) y = 0, ++zi;
      }
    }
  }
}

__device__ __forceinline__ Box wave_merge(Box b) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    Box o;
    o.z0 = __shfl_xor(b.z0, d), o.z1 = __shfl_xor(b.z1, d), o.y0 = __shfl_xor(b.y0, d), o.y1 = __shfl_xor(b.y1, d);
    o.x0 = __shfl_xor(b.x0, d), o.x1 = __shfl_xor(b.x1, d), o.n = __shfl_xor(b.n, d);
    b.merge(o);
  }
  return b;
}
// every thread gets the workgroup's box; the leading barrier lets consecutive calls share `red`
__device__ __forceinline__ Box block_merge(Box b, int4* red) {
  b = wave_merge(b);
  __syncthreads();
  if (lane_id() == 0) {
    red[2 * (threadIdx.x >> 6)] = int4{b.z0, b.z1, b.y0, b.y1};
    red[2 * (threadIdx.x >> 6) + 1] = int4{b.x0, b.x1, b.n, 0};
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kBoxWaves; ++w) {
    const int4 p = red[2 * w], q = red[2 * w + 1];
    const Box o{p.x, p.y, p.z, p.w, q.x, q.y, q.z};
    if (w == 0) b = o;
    else b.merge(o);
  }
  return b;
}

// volume_bbox.hip, (b): one workgroup per sample reduces its M x per_vol partial boxes, writes boxes and crop and folds the crop into params
void launch_volume_bbox_finish(const int4* partial, int nvol, int M, int per_vol, int Ds, int Hs, int Ws, int D, int H, int W, const xvit_crop_config& cfg,
                               int4* boxes, int4* crop, float* params, hipStream_t s);

}  // namespace xvit
