// Per-patch foreground occupancy (include/xvit.h, "Foreground-ranked token selection"): occ[s, t] = the number of voxels of patch t of
// sequence s whose fp32 value is > above.  One pass over the volumes, every voxel read once, every count written once by one thread.
//
// A workgroup owns a row band: the dp * hp rows of W voxels that make the Wn patches (d, h, *) of one volume.  The dp pieces of hp * W
// voxels of a band are each contiguous in memory and the bands follow each other in memory order.  A thread keeps ONE column (a run of
// VEC voxels) of the band and walks down its rows, so all its voxels belong to one patch and the count stays in a register: popcounts
// per run, one LDS add per thread and band, no global atomics and no workspace.  Integer sums: the order does not matter.
#include <math.h>

#include "token_rows.h"

namespace xvit {

constexpr int kOccThreads = 256;
constexpr int kOccPatches = 1024;     // patches of a band counted at once (the LDS counters); a wider band is walked in column chunks
constexpr int kOccMaxGroups = 2048;   // about eight 256-thread workgroups per CU; more bands than that are walked with a grid stride

// tw_log2: log2 of the threads along a row (a power of two <= the columns of a chunk); the other 256 / TW walk the rows.
template <typename T, int VEC>
__global__ __launch_bounds__(kOccThreads) void patch_occupancy_kernel(const T* __restrict__ img, int* __restrict__ occ, const PatchGeom g, int tw_log2, int64_t units,
                                                                      float above) {
  __shared__ int cnt[kOccPatches];
  const int tid = threadIdx.x;
  const int Dn = g.D / g.dp, Hn = g.H / g.hp, Wn = g.W / g.wp;
  const int chunks = (Wn + kOccPatches - 1) / kOccPatches;
  const int lp = g.wp / VEC;                        // columns (runs of VEC voxels) per patch
  const int pd = g.dp * g.hp * g.wp, rows = g.dp * g.hp;
  const int TW = 1 << tw_log2, TY = kOccThreads >> tw_log2;
  const int tx = tid & (TW - 1), ty = tid >> tw_log2;
  const int step1 = TY / g.hp, step2 = TY - step1 * g.hp;   // a step of TY rows as (planes, rows of the plane)
  for (int i = tid; i < kOccPatches; i += kOccThreads) cnt[i] = 0;
  __syncthreads();

  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int chunk = (int)(u % chunks);
    int64_t r = u / chunks;
    const int h = (int)(r % Hn); r /= Hn;
    const int d = (int)(r % Dn);
    const int64_t vol = r / Dn;   // b M + m
    const int w0 = chunk * kOccPatches, nw = min(kOccPatches, Wn - w0);
    const int cols = nw * lp;
    const int64_t first = ((vol * g.D + (int64_t)d * g.dp) * g.H + (int64_t)h * g.hp) * g.W + (int64_t)w0 * g.wp;   // the band's first voxel
    for (int col = tx; col < cols; col += TW) {
      const T* __restrict__ p = img + first + (int64_t)col * VEC;
      int n = 0, p1 = ty / g.hp, p2 = ty - p1 * g.hp;   // row j of the band is row p2 of plane p1
#pragma unroll 4
      for (int j = ty; j < rows; j += TY) {
        float v[VEC];
        load_run<VEC>(p + ((int64_t)p1 * g.H + p2) * g.W, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) n += v[e] > above ? 1 : 0;   // NaN compares false
        p1 += step1, p2 += step2;
        if (p2 >= g.hp) p2 -= g.hp, ++p1;
      }
      if (n) atomicAdd(&cnt[col / lp], n);
    }
    __syncthreads();
    for (int t = tid; t < nw; t += kOccThreads) {
      occ[patch_elem<1>(g, first + (int64_t)t * g.wp) / pd] = cnt[t];   // row s P + t of a [S P, pd] patch matrix (token_rows.h)
      cnt[t] = 0;
    }
    __syncthreads();
  }
}

}  // namespace xvit

using namespace xvit;

extern "C" int xvit_patch_occupancy(const void* img, int img_dtype, int32_t* occ, int B, int M, int D, int H, int W, int dp, int hp, int wp, float above,
                                    xvit_stream_t stream) {
  XVIT_REQUIRE(img && occ, "xvit_patch_occupancy: null pointer");
  XVIT_REQUIRE_PATCH_GRID("xvit_patch_occupancy", dtype_ok(img_dtype));
  XVIT_REQUIRE(isfinite(above), "xvit_patch_occupancy: the threshold must be finite");
  const int Dn = D / dp, Hn = H / hp, Wn = W / wp;
  const int64_t P = (int64_t)Dn * Hn * Wn, pd = (int64_t)dp * hp * wp;
  XVIT_REQUIRE(P < (1ll << 31) && pd < (1ll << 31) && (int64_t)M * B < (1ll << 31), "xvit_patch_occupancy: geometry too large");
  // 8-voxel runs are 16-byte accesses (two of them for fp32): a 16-byte aligned volume, else one voxel per lane (xvit_patchify_select's switch)
  const bool vec = (wp % 8 == 0) && aligned16({img});
  const int cols = min(Wn, kOccPatches) * (wp / (vec ? 8 : 1));   // of a full chunk; <= W
  int tw_log2 = 0;
  while ((2 << tw_log2) <= min(cols, kOccThreads)) ++tw_log2;
  const int64_t units = (int64_t)M * B * Dn * Hn * ((Wn + kOccPatches - 1) / kOccPatches);
  const PatchGeom g = {M, D, H, W, dp, hp, wp, P, (int64_t)B * P, 0};   // row (b, m, t) of the patch matrix = (m B + b) P + t
  by_dtype_vec(img_dtype, vec, [&](auto t, auto v) {
    using T = decltype(t);
    constexpr int VEC = decltype(v)::value;
    hipLaunchKernelGGL((patch_occupancy_kernel<T, VEC>), dim3((unsigned)min(units, (int64_t)kOccMaxGroups)), dim3(kOccThreads), 0, (hipStream_t)stream, (const T*)img, occ,
                       g, tw_log2, units, above);
  });
  return check_launch("xvit_patch_occupancy");
}
