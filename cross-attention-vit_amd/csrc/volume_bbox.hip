// Foreground bounding box and crop (include/xvit.h, "Foreground bounding box and crop"): the index range of the foreground voxels of every
// volume, the union per sample widened by a margin, and the crop folded into the sample's augmentation records.  Two launches: per-chunk
// partial boxes, then one workgroup per sample.  Integer minima, maxima and counts only, and one thread per record in the fold: the
// result does not depend on the execution order.
#include <math.h>

#include "volume_box.h"

namespace xvit {

constexpr int64_t kBoxMinChunk = 8192;   // voxels: one round of four 16-byte loads per lane of a 16-bit source
constexpr int kBoxMaxGroups = 2048;      // about eight 256-thread workgroups per CU

// The chunk rule of the header: parts per volume and voxels per part.
int bbox_parts(int nvol, int64_t nvox, int64_t* chunk_out) {
  const int64_t cap = nvol >= kBoxMaxGroups ? 1 : kBoxMaxGroups / nvol;
  int64_t parts = min(cap, (nvox + kBoxMinChunk - 1) / kBoxMinChunk);
  const int64_t chunk = ((nvox + parts - 1) / parts + 7) & ~(int64_t)7;
  parts = (nvox + chunk - 1) / chunk;   // no empty workgroup
  if (chunk_out) *chunk_out = chunk;
  return (int)parts;
}

// ------------------------------------------------------------------------------------------
// (a) partial boxes.  A workgroup owns `chunk` consecutive voxels of one volume and writes one 8-int record.
// ------------------------------------------------------------------------------------------
template <class S>
__global__ void __launch_bounds__(kBoxThreads) volume_bbox_kernel(const S* __restrict__ src, int4* __restrict__ partial, int64_t nvox, int per_vol, int64_t chunk,
                                                                  int Ds, int Hs, int Ws, float fg) {
  constexpr int E = 16 / (int)sizeof(S);   // voxels per 16-byte run
  __shared__ int4 red[2 * kBoxWaves];
  const int tid = threadIdx.x;
  const int vol = blockIdx.x / per_vol, part = blockIdx.x - vol * per_vol;
  const int64_t beg = (int64_t)part * chunk;
  const int64_t len = max((int64_t)0, min(nvox, beg + chunk) - beg);
  const S* __restrict__ p = src + (int64_t)vol * nvox + beg;
  Box b = empty_box(Ds, Hs, Ws);

  // a volume's base is only element-aligned when nvox is odd: scalar head up to the first 16-byte boundary, 16-byte runs, scalar tail
  const int head = (int)min(len, (int64_t)(((0 - (uintptr_t)p) & 15) / sizeof(S)));
  if (tid < head) add_run<1>(b, (uint32_t)(src_f(p[tid]) > fg), (uint32_t)(beg + tid), Hs, Ws);
  const uint4* __restrict__ pv = (const uint4*)(p + head);
  const int64_t nvec = (len - head) / E;
  const uint32_t flat0 = (uint32_t)(beg + head);   // a volume has fewer than 2^31 voxels
  int64_t i = tid;
  for (; i + 3 * kBoxThreads < nvec; i += 4 * kBoxThreads) {   // four loads in flight per lane
    const uint4 r0 = pv[i], r1 = pv[i + kBoxThreads], r2 = pv[i + 2 * kBoxThreads], r3 = pv[i + 3 * kBoxThreads];
    add_run<E>(b, fg_mask<S>(r0, fg), flat0 + (uint32_t)i * E, Hs, Ws);
    add_run<E>(b, fg_mask<S>(r1, fg), flat0 + (uint32_t)(i + kBoxThreads) * E, Hs, Ws);
    add_run<E>(b, fg_mask<S>(r2, fg), flat0 + (uint32_t)(i + 2 * kBoxThreads) * E, Hs, Ws);
    add_run<E>(b, fg_mask<S>(r3, fg), flat0 + (uint32_t)(i + 3 * kBoxThreads) * E, Hs, Ws);
  }
  for (; i < nvec; i += kBoxThreads) add_run<E>(b, fg_mask<S>(pv[i], fg), flat0 + (uint32_t)i * E, Hs, Ws);
  const int64_t done = head + nvec * E;
  if (tid < (int)(len - done)) add_run<1>(b, (uint32_t)(src_f(p[done + tid]) > fg), (uint32_t)(beg + done + tid), Hs, Ws);

  b = block_merge(b, red);
  if (tid == 0) {
    partial[2 * (int64_t)blockIdx.x] = int4{b.z0, b.z1, b.y0, b.y1};
    partial[2 * (int64_t)blockIdx.x + 1] = int4{b.x0, b.x1, b.n, 0};
  }
}

// ------------------------------------------------------------------------------------------
// (b) finish.  One workgroup per sample: its M volumes' boxes, their union -> crop, and the fold, record m by thread m.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int pad_crop_offset(int size, int target) { return size >= target ? size / 2 - target / 2 : -((target - size) / 2); }

__global__ void __launch_bounds__(kBoxThreads) volume_bbox_finish_kernel(const int4* __restrict__ partial, int M, int per_vol, int Ds, int Hs, int Ws, int D,
                                                                         int H, int W, xvit_crop_config cfg, int4* __restrict__ boxes,
                                                                         int4* __restrict__ crop, float* __restrict__ params) {
  __shared__ int4 red[2 * kBoxWaves];
  const int tid = threadIdx.x, b = blockIdx.x;
  Box u = empty_box(Ds, Hs, Ws);   // the union: an empty volume's box (lo = size, hi = -1) leaves it as it is
  for (int m = 0; m < M; ++m) {
    const int64_t vol = (int64_t)b * M + m;
    Box v = empty_box(Ds, Hs, Ws);
    for (int i = tid; i < per_vol; i += kBoxThreads) {
      const int4 p = partial[2 * (vol * per_vol + i)], q = partial[2 * (vol * per_vol + i) + 1];
      v.merge(Box{p.x, p.y, p.z, p.w, q.x, q.y, q.z});
    }
    v = block_merge(v, red);
    if (tid == 0) {
      boxes[2 * vol] = int4{v.z0, v.z1, v.y0, v.y1};
      boxes[2 * vol + 1] = int4{v.x0, v.x1, v.n, 0};
    }
    u.merge(v);
  }

  const bool any = u.n > 0;
  const int size[3] = {Ds, Hs, Ws}, n[3] = {D, H, W};
  int lo[3] = {u.z0, u.y0, u.x0}, hi[3] = {u.z1, u.y1, u.x1};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = any ? (int)max((long long)lo[a] - cfg.margin[a], 0ll) : 0;
    hi[a] = any ? (int)min((long long)hi[a] + cfg.margin[a], (long long)size[a] - 1) : size[a] - 1;
  }
  if (tid == 0) {
    crop[2 * (int64_t)b] = int4{lo[0], hi[0], lo[1], hi[1]};
    crop[2 * (int64_t)b + 1] = int4{lo[2], hi[2], any ? 1 : 0, 0};
  }
  if (!params || cfg.mode == XVIT_CROP_BOXES_ONLY || !any) return;

  double k = 1.0;
  if (cfg.mode == XVIT_CROP_FIT) {
    k = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) k = fmax(k, (double)(hi[a] - lo[a] + 1) / (double)n[a]);
    if (!cfg.allow_upscale) k = fmax(k, 1.0);
  }
  const float kf = (float)k;
  for (int m = tid; m < M; m += kBoxThreads) {   // every slot of a record by one thread, in double, rounded once
    float* __restrict__ P = params + ((int64_t)b * M + m) * XVIT_AUG_NPARAM;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int o = pad_crop_offset(size[a], n[a]);
      float* t = P + XVIT_AUG_MATRIX + 4 * a + 3;
      if (kf == 1.f) {
        *t = (float)((double)*t + (double)(lo[a] + pad_crop_offset(hi[a] - lo[a] + 1, n[a]) - o));
      } else {
        const double c = 0.5 * (double)(n[a] - 1), cb = 0.5 * ((double)lo[a] + (double)hi[a]);
        for (int j = 0; j < 3; ++j) P[XVIT_AUG_MATRIX + 4 * a + j] = (float)((double)kf * (double)P[XVIT_AUG_MATRIX + 4 * a + j]);
        *t = (float)((double)kf * ((double)*t - c - (double)o) + cb);
      }
    }
    if (kf != 1.f) P[XVIT_AUG_FLAGS] = (float)((int)P[XVIT_AUG_FLAGS] & ~XVIT_AUG_FLAG_EXACT);
    P[XVIT_AUG_CROP_SCALE] = kf;
  }
}

void launch_volume_bbox_finish(const int4* partial, int nvol, int M, int per_vol, int Ds, int Hs, int Ws, int D, int H, int W, const xvit_crop_config& cfg,
                               int4* boxes, int4* crop, float* params, hipStream_t s) {
  hipLaunchKernelGGL(volume_bbox_finish_kernel, dim3((unsigned)(nvol / M)), dim3(kBoxThreads), 0, s, partial, M, per_vol, Ds, Hs, Ws, D, H, W, cfg, boxes, crop,
                     params);
}

}  // namespace xvit

extern "C" int64_t xvit_volume_bbox_workspace_bytes(int nvol, int64_t nvox) {
  if (nvol <= 0 || nvox <= 0) return 0;
  return (int64_t)nvol * xvit::bbox_parts(nvol, nvox, nullptr) * XVIT_BBOX_NREC * (int64_t)sizeof(int32_t);
}

extern "C" int xvit_volume_bbox(const void* src, int src_dtype, int nvol, int M, int Ds, int Hs, int Ws, int D, int H, int W, const xvit_crop_config* cfg,
                                int32_t* boxes, int32_t* crop, float* params, void* workspace, int64_t workspace_bytes, xvit_stream_t stream) {
  XVIT_REQUIRE(src && cfg && boxes && crop && workspace, "xvit_volume_bbox: null source, config, boxes, crop or workspace");
  XVIT_REQUIRE(src_dtype == XVIT_I16 || src_dtype == XVIT_BF16 || src_dtype == XVIT_F32, "xvit_volume_bbox: unknown source dtype %d", src_dtype);
  XVIT_REQUIRE(cfg->mode == XVIT_CROP_BOXES_ONLY || cfg->mode == XVIT_CROP_CENTER || cfg->mode == XVIT_CROP_FIT, "xvit_volume_bbox: unknown mode %d", cfg->mode);
  XVIT_REQUIRE(nvol > 0 && M > 0 && nvol % M == 0, "xvit_volume_bbox: nvol=%d must be a positive multiple of M=%d > 0", nvol, M);
  XVIT_REQUIRE(Ds > 0 && Hs > 0 && Ws > 0 && D > 0 && H > 0 && W > 0, "xvit_volume_bbox: sizes (%d, %d, %d) -> (%d, %d, %d) must be positive", Ds, Hs, Ws, D, H, W);
  const int64_t nvox = (int64_t)Ds * Hs * Ws;
  XVIT_REQUIRE(nvox < (1ll << 31), "xvit_volume_bbox: a volume must have fewer than 2^31 voxels, got %lld", (long long)nvox);
  XVIT_REQUIRE(cfg->margin[0] >= 0 && cfg->margin[1] >= 0 && cfg->margin[2] >= 0, "xvit_volume_bbox: margin (%d, %d, %d) must be >= 0", cfg->margin[0],
               cfg->margin[1], cfg->margin[2]);
  XVIT_REQUIRE(!isnan(cfg->foreground_above), "xvit_volume_bbox: foreground_above is NaN");
  XVIT_REQUIRE(((uintptr_t)src & (src_dtype == XVIT_F32 ? 3 : 1)) == 0, "xvit_volume_bbox: the source is not aligned to its element size");
  XVIT_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)crop & 15) == 0, "xvit_volume_bbox: boxes and crop must be 16-byte aligned");
  XVIT_REQUIRE(((uintptr_t)params & 15) == 0, "xvit_volume_bbox: the parameter table must be 16-byte aligned");
  XVIT_REQUIRE(((uintptr_t)workspace & 15) == 0, "xvit_volume_bbox: the workspace must be 16-byte aligned");
  XVIT_REQUIRE(workspace_bytes >= xvit_volume_bbox_workspace_bytes(nvol, nvox), "xvit_volume_bbox: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)xvit_volume_bbox_workspace_bytes(nvol, nvox));
  int64_t chunk;
  const int per_vol = xvit::bbox_parts(nvol, nvox, &chunk);
  const hipStream_t s = (hipStream_t)stream;
  xvit::by_src_dtype(src_dtype, [&](auto t) {
    using S = decltype(t);
    hipLaunchKernelGGL(xvit::volume_bbox_kernel<S>, dim3((unsigned)((int64_t)nvol * per_vol)), dim3(xvit::kBoxThreads), 0, s, (const S*)src, (int4*)workspace, nvox,
                       per_vol, chunk, Ds, Hs, Ws, cfg->foreground_above);
  });
  xvit::launch_volume_bbox_finish((const int4*)workspace, nvol, M, per_vol, Ds, Hs, Ws, D, H, W, *cfg, (int4*)boxes, (int4*)crop, params, s);
  return xvit::check_launch("xvit_volume_bbox");
}
