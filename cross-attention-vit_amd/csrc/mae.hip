// Masked-volume pretraining (MAE, He et al. 2022) on top of patch dropout (token_select.hip): the encoder sees the K kept patches, a light
// decoder sees the full grid again, and the prediction of the P - K dropped patches is scored against the volume.
//   xvit_token_select_complement   the dropped patches of every sequence, ascending, and the inverse map
//   xvit_mae_unshuffle_fwd / _bwd  encoder tokens back on the full grid, a mask token in the dropped places, + decoder pos / modality
//   xvit_token_rows_gather/scatter the dropped rows of the decoder output (only they reach the prediction head), and the backward
//   xvit_mae_loss_fwd / _bwd       mean squared error against the (per-patch normalised) voxels, read straight from the volume
// No atomics: every sum below has one fixed order, stated in include/xvit.h.
#include "token_rows.h"

namespace xvit {

constexpr int kComplBlock = 1024;
constexpr int kLossBlock = 256;

// One workgroup per sequence, 1024 patches per compaction round, on "dropped" where the draw compacts "kept".  Positions past Rm (a slot
// row with fewer than K kept entries) are not written and read as kept in mslot; a row with more than K kept entries leaves the tail of
// drop_idx at -1.
__global__ __launch_bounds__(kComplBlock) void token_select_complement_kernel(const int* __restrict__ slot, int* __restrict__ drop_idx, int* __restrict__ mslot,
                                                                              int P, int Rm) {
  __shared__ int wave_tot[kComplBlock / kWave];
  const int s = blockIdx.x, tid = threadIdx.x;
  int base = 0;   // dropped patches in the rounds before this one (the same in every thread)
  for (int p0 = 0; p0 < P; p0 += kComplBlock) {     // uniform over the workgroup
    const int p = p0 + tid;
    const bool dropped = p < P && slot[(int64_t)s * P + p] < 0;
    const int pos = compact_round<kComplBlock>(dropped, wave_tot, base);
    if (p < P) {
      const bool place = dropped && pos < Rm;
      mslot[(int64_t)s * P + p] = place ? pos : -1;
      if (place) drop_idx[(int64_t)s * Rm + pos] = p;
    }
  }
  for (int j = base + tid; j < Rm; j += kComplBlock) drop_idx[(int64_t)s * Rm + j] = -1;   // fewer dropped patches than Rm: no stale index
}

// y[s, 0] = (xe[s, 0] + dpos[0]) + dmod[m];  y[s, 1 + p] = ((kept ? xe[s, 1 + slot[s][p]] : mask_token) + dpos[1 + p]) + dmod[m]
__global__ void mae_unshuffle_fwd_kernel(const float* __restrict__ xe, const float* __restrict__ mask_token, const float* __restrict__ dpos,
                                         const float* __restrict__ dmod, const int* __restrict__ slot, float* __restrict__ y, int B, int P, int K, int dd,
                                         int64_t total) {
  const int dv = dd >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const auto [row, c] = row_col(i, dv);
    const int n = (int)(row % (P + 1));
    const int64_t s = row / (P + 1);
    const int m = (int)(s / B);
    const int j = n == 0 ? 0 : 1 + slot[s * P + (n - 1)];      // 0 on a patch row: dropped
    const bool from_xe = n == 0 || (j > 0 && j <= K);
    const f32x4 src = from_xe ? *(const f32x4*)(xe + (s * (K + 1) + j) * dd + c) : *(const f32x4*)(mask_token + c);
    *(f32x4*)(y + row * dd + c) = (src + *(const f32x4*)(dpos + (int64_t)n * dd + c)) + *(const f32x4*)(dmod + (int64_t)m * dd + c);
  }
}

// The maps of the three row movers (move_rows_kernel): output row -> input row, or -1 for a zero row.
// dxe[s, 0] = dy[s, 0];  dxe[s, 1 + j] = dy[s, 1 + keep_idx[s][j]]  (an index outside the grid gives a zero row)
struct UnshuffleDxeMap {
  const int* __restrict__ keep_idx; int P, K;
  __device__ __forceinline__ int64_t operator()(int64_t row) const {
    const int j = (int)(row % (K + 1));
    const int64_t s = row / (K + 1);
    const int n = j == 0 ? 0 : 1 + keep_idx[s * K + (j - 1)];
    return (unsigned)n <= (unsigned)P ? s * (P + 1) + n : -1;
  }
};
// g[s Rm + j] = x[s, 1 + drop_idx[s][j]]  (an index outside the grid gives a zero row)
struct RowsGatherMap {
  const int* __restrict__ drop_idx; int P, Rm;
  __device__ __forceinline__ int64_t operator()(int64_t row) const {
    const int t = drop_idx[row];
    return (unsigned)t < (unsigned)P ? (row / Rm) * (P + 1) + 1 + t : -1;
  }
};
// dx[s, 0] = 0;  dx[s, 1 + p] = mslot[s][p] >= 0 ? dg[s Rm + mslot[s][p]] : 0
struct RowsScatterMap {
  const int* __restrict__ mslot; int P, Rm;
  __device__ __forceinline__ int64_t operator()(int64_t row) const {
    const int n = (int)(row % (P + 1));
    const int64_t s = row / (P + 1);
    const int j = n == 0 ? -1 : mslot[s * P + (n - 1)];
    return (unsigned)j < (unsigned)Rm ? s * Rm + j : -1;
  }
};

// ddpos_m[m, n] = sum over b ascending of dy[(m, b), n]: one thread per (m, n, 4 features), its sequences in order
__global__ void mae_unshuffle_dpos_kernel(const float* __restrict__ dy, float* __restrict__ ddpos_m, int B, int P, int dd, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over M (P + 1) dd / 4
  if (i >= total) return;
  const auto [row, c] = row_col(i, dd >> 2);
  const int n = (int)(row % (P + 1));
  const int64_t m = row / (P + 1);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < B; ++b) acc += *(const f32x4*)(dy + ((m * B + b) * (P + 1) + n) * dd + c);
  *(f32x4*)(ddpos_m + row * dd + c) = acc;
}

// part[s] = sum over p ascending of dy[s, 1 + p] where slot[s][p] < 0: one thread per (s, 4 features)
__global__ void mae_unshuffle_dmask_part_kernel(const float* __restrict__ dy, const int* __restrict__ slot, float* __restrict__ part, int P, int dd, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over S dd / 4
  if (i >= total) return;
  const auto [s, c] = row_col(i, dd >> 2);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < P; ++p)
    if (slot[s * P + p] < 0) acc += *(const f32x4*)(dy + (s * (P + 1) + 1 + p) * dd + c);
  *(f32x4*)(part + s * dd + c) = acc;
}

// dmask_token = sum over s ascending of part[s]: one thread per 4 features
__global__ void mae_unshuffle_dmask_kernel(const float* __restrict__ part, float* __restrict__ dmask_token, int S, int dd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (dd >> 2)) return;
  const int c = i * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < S; ++s) acc += *(const f32x4*)(part + (int64_t)s * dd + c);
  *(f32x4*)(dmask_token + c) = acc;
}

// ---- the loss ------------------------------------------------------------------------------------------------------------------------

// One workgroup per predicted row.  The patch's voxels go to LDS once (the volume is read once); the mean, then the centred squares, then
// the squared error against pred are each a block-wide sum in a fixed order (thread-strided partial sums, wave_reduce, the waves in order).
template <typename TV, typename TP, int VEC>
__global__ __launch_bounds__(kLossBlock) void mae_loss_fwd_kernel(const TP* __restrict__ pred, const int* __restrict__ drop_idx, const TV* __restrict__ img,
                                                                  int norm_pix, float* __restrict__ stats, float* __restrict__ row_loss, const TokenGeom g) {
  extern __shared__ float vox[];              // pd floats
  __shared__ float red[kLossBlock / kWave];
  const int pd = g.dp * g.hp * g.wp;
  const int P = patch_count(g);
  const int r = blockIdx.x, s = r / g.n, tid = threadIdx.x;
  const int t = drop_idx[r];
  if ((unsigned)t >= (unsigned)P) {           // no such patch (uniform over the workgroup): the row scores nothing
    if (tid == 0) stats[2 * (int64_t)r] = 0.f, stats[2 * (int64_t)r + 1] = 1.f, row_loss[r] = 0.f;
    return;
  }
  float part = 0.f;
  for (int f = tid * VEC; f < pd; f += kLossBlock * VEC) {
    float v[VEC];
    load_run<VEC>(img + voxel_index(g, s, t, f), v);
#pragma unroll
    for (int i = 0; i < VEC; ++i) vox[f + i] = v[i], part += v[i];
  }
  float mean = 0.f, rstd = 1.f;
  if (norm_pix) {
    mean = block_reduce<kLossBlock / kWave>(part, SumOp{}, red) / (float)pd;
    float sq = 0.f;
    for (int f = tid * VEC; f < pd; f += kLossBlock * VEC) {     // each thread re-reads what it wrote
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float c = vox[f + i] - mean;
        sq += c * c;
      }
    }
    const float var = block_reduce<kLossBlock / kWave>(sq, SumOp{}, red) / (float)(pd - 1);
    rstd = 1.0f / sqrtf(var + 1e-6f);
  }
  float err = 0.f;
  const TP* prow = pred + (int64_t)r * pd;
  for (int f = tid * VEC; f < pd; f += kLossBlock * VEC) {
    float p[VEC];
    load_run<VEC>(prow + f, p);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float e = p[i] - (vox[f + i] - mean) * rstd;
      err += e * e;
    }
  }
  err = block_reduce<kLossBlock / kWave>(err, SumOp{}, red);
  if (tid == 0) {
    stats[2 * (int64_t)r] = mean;
    stats[2 * (int64_t)r + 1] = rstd;
    row_loss[r] = err / (float)pd;
  }
}

// One workgroup: loss_seq[s] = (row_loss[s Rm] + ... + row_loss[s Rm + Rm - 1], ascending) / Rm, one thread per sequence; then
// loss = (loss_seq[0] + ... + loss_seq[S - 1], ascending) / S.
__global__ __launch_bounds__(kLossBlock) void mae_loss_finish_kernel(const float* __restrict__ row_loss, float* __restrict__ loss_seq, float* __restrict__ loss, int S, int Rm) {
  for (int s = threadIdx.x; s < S; s += kLossBlock) {
    float acc = 0.f;
    for (int j = 0; j < Rm; ++j) acc += row_loss[(int64_t)s * Rm + j];
    loss_seq[s] = acc / (float)Rm;
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += ((volatile const float*)loss_seq)[s];
    loss[0] = acc / (float)S;
  }
}

// dpred[r, f] = coef (pred[r, f] - target[r, f]),  coef = g 2 / (pd rows), the target recomputed from the volume and stats
template <typename TV, typename TP, int VEC>
__global__ void mae_loss_bwd_kernel(const TP* __restrict__ pred, const int* __restrict__ drop_idx, const TV* __restrict__ img, const float* __restrict__ stats,
                                    const float* __restrict__ gup, TP* __restrict__ dpred, const TokenGeom g, int64_t rows, int64_t total_vec) {
  const int pd = g.dp * g.hp * g.wp, pv = pd / VEC;
  const int P = patch_count(g);
  const float coef = gup[0] * (2.0f / ((float)pd * (float)rows));
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total_vec; idx += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(idx % pv) * VEC;
    const int64_t r = idx / pv;
    const int t = drop_idx[r];
    float o[VEC];
    if ((unsigned)t >= (unsigned)P) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) o[i] = 0.f;
    } else {
      const float mean = stats[2 * r], rstd = stats[2 * r + 1];
      float v[VEC], p[VEC];
      load_run<VEC>(img + voxel_index(g, (int)(r / g.n), t, f), v);
      load_run<VEC>(pred + r * pd + f, p);
#pragma unroll
      for (int i = 0; i < VEC; ++i) o[i] = coef * (p[i] - (v[i] - mean) * rstd);
    }
    store_run<VEC>(dpred + r * pd + f, o);
  }
}

}  // namespace xvit

using namespace xvit;

extern "C" int xvit_token_select_complement(const int32_t* slot, int32_t* drop_idx, int32_t* mslot, int S, int P, int K, xvit_stream_t stream) {
  XVIT_REQUIRE(slot && drop_idx && mslot, "xvit_token_select_complement: null pointer");
  XVIT_REQUIRE(S > 0 && P > 0, "xvit_token_select_complement: bad sizes (S=%d P=%d)", S, P);
  XVIT_REQUIRE(K >= 1 && K < P, "xvit_token_select_complement: K=%d outside 1 .. P - 1 = %d (at least one patch kept and one dropped)", K, P - 1);
  XVIT_REQUIRE(P <= XVIT_TOKEN_SELECT_MAX_P, "xvit_token_select_complement: P=%d too long (P <= %d, as in xvit_token_select_draw)", P, XVIT_TOKEN_SELECT_MAX_P);
  hipLaunchKernelGGL(token_select_complement_kernel, dim3(S), dim3(kComplBlock), 0, (hipStream_t)stream, slot, drop_idx, mslot, P, P - K);
  return check_launch("xvit_token_select_complement");
}

#define XVIT_MAE_GRID_ARGS(name)                                                                                                                  \
  XVIT_REQUIRE(S > 0 && B > 0 && S % B == 0 && P > 0 && K >= 1 && K < P && dd > 0 && dd % 4 == 0,                                                \
               name ": bad sizes (S=%d B=%d P=%d K=%d dd=%d; S %% B == 0, 1 <= K < P, dd %% 4 == 0)", S, B, P, K, dd);                           \
  XVIT_REQUIRE((int64_t)S * (P + 1) * dd < (1ll << 40), name ": token tensor too large")

extern "C" int xvit_mae_unshuffle_fwd(const float* xe, const float* mask_token, const float* dpos, const float* dmod, const int32_t* slot, float* y, int S, int B,
                                      int P, int K, int dd, xvit_stream_t stream) {
  XVIT_REQUIRE(xe && mask_token && dpos && dmod && slot && y, "xvit_mae_unshuffle_fwd: null pointer");
  XVIT_MAE_GRID_ARGS("xvit_mae_unshuffle_fwd");
  XVIT_REQUIRE(aligned16({xe, mask_token, dpos, dmod, y}), "xvit_mae_unshuffle_fwd: xe, mask_token, dpos, dmod and y must be 16-byte aligned");
  const int64_t total = (int64_t)S * (P + 1) * (dd / 4);
  hipLaunchKernelGGL(mae_unshuffle_fwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, xe, mask_token, dpos, dmod, slot, y, B, P, K, dd, total);
  return check_launch("xvit_mae_unshuffle_fwd");
}

extern "C" int xvit_mae_unshuffle_bwd(const float* dy, const int32_t* keep_idx, const int32_t* slot, float* dxe, float* dmask_token, float* ddpos_m,
                                      float* dmask_part, int S, int B, int P, int K, int dd, xvit_stream_t stream) {
  XVIT_REQUIRE(dy && keep_idx && slot && dxe && dmask_token && ddpos_m && dmask_part, "xvit_mae_unshuffle_bwd: null pointer");
  XVIT_MAE_GRID_ARGS("xvit_mae_unshuffle_bwd");
  XVIT_REQUIRE(aligned16({dy, dxe, dmask_token, ddpos_m, dmask_part}), "xvit_mae_unshuffle_bwd: dy, dxe, dmask_token, ddpos_m and dmask_part must be 16-byte aligned");
  const int dv = dd / 4, M = S / B;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t t_xe = (int64_t)S * (K + 1) * dv, t_pos = (int64_t)M * (P + 1) * dv, t_part = (int64_t)S * dv;
  hipLaunchKernelGGL(move_rows_kernel<UnshuffleDxeMap>, dim3(grid_for(t_xe, 256)), dim3(256), 0, st, dy, dxe, UnshuffleDxeMap{keep_idx, P, K}, dd, t_xe);
  hipLaunchKernelGGL(mae_unshuffle_dpos_kernel, dim3((unsigned)((t_pos + 255) / 256)), dim3(256), 0, st, dy, ddpos_m, B, P, dd, t_pos);
  hipLaunchKernelGGL(mae_unshuffle_dmask_part_kernel, dim3((unsigned)((t_part + 63) / 64)), dim3(64), 0, st, dy, slot, dmask_part, P, dd, t_part);
  hipLaunchKernelGGL(mae_unshuffle_dmask_kernel, dim3((unsigned)((dv + 63) / 64)), dim3(64), 0, st, (const float*)dmask_part, dmask_token, S, dd);
  return check_launch("xvit_mae_unshuffle_bwd");
}

#define XVIT_MAE_ROWS_ARGS(name)                                                                                                        \
  XVIT_REQUIRE(S > 0 && P > 0 && Rm >= 1 && Rm < P && dd > 0 && dd % 4 == 0,                                                           \
               name ": bad sizes (S=%d P=%d Rm=%d dd=%d; 1 <= Rm < P, dd %% 4 == 0)", S, P, Rm, dd);                                   \
  XVIT_REQUIRE((int64_t)S * (P + 1) * dd < (1ll << 40), name ": token tensor too large")

extern "C" int xvit_token_rows_gather(const float* x, const int32_t* drop_idx, float* g, int S, int P, int Rm, int dd, xvit_stream_t stream) {
  XVIT_REQUIRE(x && drop_idx && g, "xvit_token_rows_gather: null pointer");
  XVIT_MAE_ROWS_ARGS("xvit_token_rows_gather");
  XVIT_REQUIRE(aligned16({x, g}), "xvit_token_rows_gather: x and g must be 16-byte aligned");
  const int64_t total = (int64_t)S * Rm * (dd / 4);
  hipLaunchKernelGGL(move_rows_kernel<RowsGatherMap>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, x, g, RowsGatherMap{drop_idx, P, Rm}, dd, total);
  return check_launch("xvit_token_rows_gather");
}

extern "C" int xvit_token_rows_scatter(const float* dg, const int32_t* mslot, float* dx, int S, int P, int Rm, int dd, xvit_stream_t stream) {
  XVIT_REQUIRE(dg && mslot && dx, "xvit_token_rows_scatter: null pointer");
  XVIT_MAE_ROWS_ARGS("xvit_token_rows_scatter");
  XVIT_REQUIRE(aligned16({dg, dx}), "xvit_token_rows_scatter: dg and dx must be 16-byte aligned");
  const int64_t total = (int64_t)S * (P + 1) * (dd / 4);
  hipLaunchKernelGGL(move_rows_kernel<RowsScatterMap>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, dg, dx, RowsScatterMap{mslot, P, Rm}, dd, total);
  return check_launch("xvit_token_rows_scatter");
}

// Shared argument checks of the two loss entry points -> 0, or an error already set.
static int mae_loss_args(const char* name, const void* pred, int pred_dtype, const void* img, int img_dtype, const void* dpred, int B, int M, int D, int H, int W, int dp, int hp, int wp, int Rm, int norm_pix) {
  XVIT_REQUIRE_PATCH_GRID(name, dtype_ok(pred_dtype) && dtype_ok(img_dtype));
  const uintptr_t pa = pred_dtype == XVIT_F32 ? 3 : 1, ia = img_dtype == XVIT_F32 ? 3 : 1;
  XVIT_REQUIRE(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(dpred)) & pa) == 0 && (reinterpret_cast<uintptr_t>(img) & ia) == 0,
               "%s: the volume and the prediction must be aligned to their element size", name);
  const int64_t P = (int64_t)(D / dp) * (H / hp) * (W / wp), pd = (int64_t)dp * hp * wp;
  XVIT_REQUIRE(Rm >= 1 && Rm < P, "%s: Rm=%d outside 1 .. P - 1 = %lld", name, Rm, (long long)(P - 1));
  XVIT_REQUIRE(pd <= XVIT_MAE_MAX_PD, "%s: patch of %lld voxels too large (a patch sits in LDS: dp*hp*wp <= %d)", name, (long long)pd, XVIT_MAE_MAX_PD);
  XVIT_REQUIRE(!norm_pix || pd >= 2, "%s: norm_pix needs at least 2 voxels per patch (unbiased variance)", name);
  XVIT_REQUIRE(P < (1ll << 31) && (int64_t)M * B * Rm < (1ll << 31), "%s: geometry too large", name);
  return 0;
}

extern "C" int xvit_mae_loss_fwd(const void* pred, int pred_dtype, const int32_t* drop_idx, const void* img, int img_dtype, int norm_pix, float* stats,
                                 float* row_loss, float* loss_seq, float* loss, int B, int M, int D, int H, int W, int dp, int hp, int wp, int Rm,
                                 xvit_stream_t stream) {
  XVIT_REQUIRE(pred && drop_idx && img && stats && row_loss && loss_seq && loss, "xvit_mae_loss_fwd: null pointer");
  XVIT_REQUIRE(((reinterpret_cast<uintptr_t>(stats) | reinterpret_cast<uintptr_t>(row_loss) | reinterpret_cast<uintptr_t>(loss_seq) | reinterpret_cast<uintptr_t>(loss)) & 3) == 0,
               "xvit_mae_loss_fwd: stats, row_loss, loss_seq and loss must be 4-byte aligned");
  if (int rc = mae_loss_args("xvit_mae_loss_fwd", pred, pred_dtype, img, img_dtype, nullptr, B, M, D, H, W, dp, hp, wp, Rm, norm_pix)) return rc;
  const int pd = dp * hp * wp, S = M * B;
  // 8-voxel runs are 16-byte accesses (two of them for fp32): 16-byte aligned volume and prediction, else one voxel per access
  const bool vec = (wp % 8 == 0) && aligned16({img, pred});
  const TokenGeom g = {B, M, D, H, W, dp, hp, wp, Rm};
  by_dtype(img_dtype, [&](auto tv) { by_dtype_vec(pred_dtype, vec, [&](auto tp, auto v) {
    using TV = decltype(tv);
    using TP = decltype(tp);
    hipLaunchKernelGGL((mae_loss_fwd_kernel<TV, TP, decltype(v)::value>), dim3(S * Rm), dim3(kLossBlock), (size_t)pd * sizeof(float), (hipStream_t)stream,
                       (const TP*)pred, drop_idx, (const TV*)img, norm_pix ? 1 : 0, stats, row_loss, g);
  }); });
  hipLaunchKernelGGL(mae_loss_finish_kernel, dim3(1), dim3(kLossBlock), 0, (hipStream_t)stream, (const float*)row_loss, loss_seq, loss, S, Rm);
  return check_launch("xvit_mae_loss_fwd");
}

extern "C" int xvit_mae_loss_bwd(const void* pred, int pred_dtype, const int32_t* drop_idx, const void* img, int img_dtype, const float* stats, const float* g_up,
                                 void* dpred, int B, int M, int D, int H, int W, int dp, int hp, int wp, int Rm, xvit_stream_t stream) {
  XVIT_REQUIRE(pred && drop_idx && img && stats && g_up && dpred, "xvit_mae_loss_bwd: null pointer");
  if (int rc = mae_loss_args("xvit_mae_loss_bwd", pred, pred_dtype, img, img_dtype, dpred, B, M, D, H, W, dp, hp, wp, Rm, 0)) return rc;
  const int pd = dp * hp * wp;
  const int64_t rows = (int64_t)M * B * Rm, total = rows * pd;
  const bool vec = (wp % 8 == 0) && aligned16({img, pred, dpred});
  const TokenGeom g = {B, M, D, H, W, dp, hp, wp, Rm};
  by_dtype(img_dtype, [&](auto tv) { by_dtype_vec(pred_dtype, vec, [&](auto tp, auto v) {
    using TV = decltype(tv);
    using TP = decltype(tp);
    constexpr int VEC = decltype(v)::value;
    hipLaunchKernelGGL((mae_loss_bwd_kernel<TV, TP, VEC>), dim3(grid_for(total / VEC, 256)), dim3(256), 0, (hipStream_t)stream, (const TP*)pred, drop_idx,
                       (const TV*)img, stats, g_up, (TP*)dpred, g, rows, total / VEC);
  }); });
  return check_launch("xvit_mae_loss_bwd");
}
