// Patch dropout (PatchDropout, Liu et al. 2023): train on a random subset of K of the P patch tokens of every sequence, plus CLS.
//   xvit_token_select_draw   which patches each sequence keeps (counter hash, capturable, no host read-back)
//   xvit_token_select_ranked the same, ranked by per-patch foreground counts (token_occupancy.hip): tissue first, or the most occupied
//   xvit_patchify_select     the stored patch matrix of the kept rows only
//   xvit_embed_select_fwd    + pos of the KEPT patch, and the CLS row
//   xvit_embed_select_bwd    dpos / dcls through the selection, in a fixed order
// The GEMMs in between are the ordinary NT / TN ones on the shorter matrix (xvit_gemm).
#include "token_rows.h"

namespace xvit {

constexpr int kDrawBlock = 1024;
static_assert(XVIT_TOKEN_SELECT_MAX_P == 8 * kDrawBlock, "the draw kernel is instantiated for up to 8 patches per thread");

// How a sequence's patches are ordered: by the counter hash alone (xvit_token_select_draw), or by occupancy (xvit_token_select_ranked):
// foreground before background and the hash inside each class, or the most occupied first.
enum { kRankHash = -1, kRankRandom = XVIT_TOKEN_RANK_RANDOM, kRankTop = XVIT_TOKEN_RANK_TOP };

// One workgroup per sequence.  The keys of the sequence sit in LDS; thread t owns the patches t, t + 1024, ... and ranks them in ONE
// sweep over the LDS array (every lane reads the same address: a broadcast) by counting the (key, p) pairs below its own.  The pairs are
// distinct, so the ranks are a permutation and "kept" is rank < K.  The ascending position of a kept patch is the number of kept patches
// in front of it: a ballot prefix inside each wave, the waves' totals through LDS, 1024 patches per round.  PER: patches a thread
// ranks (P <= PER * 1024).  RANK: the key is the hash, or ~count for kRankTop (a larger count ranks first, ties to the smaller p);
// kRankRandom puts one class bit per patch (1: background) from a bit mask in LDS above the hash.  The count of a patch is occ[s, p],
// or with `shared` the sum over the S / B modalities of its sample, saturated at 2^32 - 1.
template <int PER, int RANK>
__global__ __launch_bounds__(kDrawBlock) void token_select_kernel(const int* __restrict__ occ, int* __restrict__ keep_idx, int* __restrict__ slot, int* __restrict__ n_fg,
                                                                   int S, int B, int P, int K, int shared, int min_count, uint64_t seed,
                                                                   const uint64_t* __restrict__ epoch) {
  __shared__ uint32_t keys[PER * kDrawBlock];
  __shared__ uint64_t background[RANK == kRankRandom ? PER * kDrawBlock / kWave : 1];   // bit p % 64 of word p / 64
  __shared__ int wave_tot[kDrawBlock / kWave];
  const int s = blockIdx.x, tid = threadIdx.x;
  const uint64_t u = shared ? (uint64_t)(s % B) : (uint64_t)s;
  if constexpr (RANK != kRankTop) {
    const uint64_t sd = drop_seed_at(seed, epoch);
    for (int p = tid; p < P; p += kDrawBlock) keys[p] = hash32(sd, u * (uint64_t)P + (uint64_t)p);
  }
  if constexpr (RANK != kRankHash) {
    const int first = shared ? s % B : s, last = shared ? S : s + 1;   // the sequences whose counts add up, B apart
    int total_fg = 0;
    for (int p0 = 0; p0 < P; p0 += kDrawBlock) {     // whole waves: the ballot below needs every lane
      const int p = p0 + tid;
      uint64_t c = 0;
      if (p < P)
        for (int q = first; q < last; q += B) c += (uint32_t)occ[(int64_t)q * P + p];
      const bool fg = p < P && c >= (uint64_t)min_count;
      if constexpr (RANK == kRankTop) {
        if (p < P) keys[p] = ~(c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c);
      } else {
        const uint64_t vote = __ballot(!fg);
        if ((tid & (kWave - 1)) == 0) background[p / kWave] = vote;
      }
      if (n_fg) compact_round<kDrawBlock>(fg, wave_tot, total_fg);   // uniform: n_fg is an argument
    }
    if (n_fg && tid == 0) n_fg[s] = total_fg;
  }
  __syncthreads();

  // (key, p) as one integer: ties on the key go to the smaller p
  auto pair = [&](int p) -> uint64_t {
    if constexpr (RANK == kRankRandom) return ((background[p / kWave] >> (p % kWave)) & 1ull) << 63 | (uint64_t)keys[p] << 31 | (uint32_t)p;
    else return ((uint64_t)keys[p] << 32) | (uint32_t)p;
  };
  uint64_t mine[PER];
  int below[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int p = tid + i * kDrawBlock;
    mine[i] = p < P ? pair(p) : 0;   // 0: nothing is below
    below[i] = 0;
  }
  for (int q = 0; q < P; ++q) {
    const uint64_t other = pair(q);
#pragma unroll
    for (int i = 0; i < PER; ++i)
      below[i] += other < mine[i] ? 1 : 0;
  }

  int base = 0;   // kept patches in the rounds before this one (the same in every thread)
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    if (i * kDrawBlock >= P) break;     // uniform over the workgroup
    const int p = tid + i * kDrawBlock;
    const bool kept = p < P && below[i] < K;
    const int pos = compact_round<kDrawBlock>(kept, wave_tot, base);
    if (p < P) {
      slot[(int64_t)s * P + p] = kept ? pos : -1;
      if (kept) keep_idx[(int64_t)s * K + pos] = p;
    }
  }
}

// Threads walk the OUTPUT [M, B (K + 1), pd] (VEC features each), so only the voxels of kept patches are read: row 0 of a sequence is
// zero, row 1 + j gathers patch keep_idx[s][j].
template <typename T, int VEC>
__global__ void patchify_select_kernel(const T* __restrict__ img, bf16* __restrict__ out, const int* __restrict__ keep_idx, const TokenGeom g, int64_t total_vec) {
  const int pd = g.dp * g.hp * g.wp, pv = pd / VEC, K = g.n;
  const int P = patch_count(g);
  const float zero[VEC] = {};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total_vec; idx += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(idx % pv) * VEC;
    const int64_t row = idx / pv;
    const int j = (int)(row % (K + 1)), s = (int)(row / (K + 1));   // s = m B + b
    bf16* dst = out + row * pd + f;
    const int t = j > 0 ? keep_idx[(int64_t)s * K + (j - 1)] : -1;
    if ((unsigned)t >= (unsigned)P) store_run<VEC>(dst, zero);     // the CLS slot (an index outside the grid reads nothing either)
    else copy_run<VEC>(dst, img + voxel_index(g, s, t, f));
  }
}

// x[s, 0, :] = cls + pos[0];  x[s, 1 + j, :] += pos[1 + keep_idx[s][j], :]   (x fp32 [S (K + 1), d], 4 features per thread)
__global__ void embed_select_fwd_kernel(float* __restrict__ x, const float* __restrict__ cls, const float* __restrict__ pos, const int* __restrict__ keep_idx,
                                        int K, int d, int64_t total) {
  const int dv = d >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const auto [row, c] = row_col(i, dv);
    const int j = (int)(row % (K + 1));
    const int64_t s = row / (K + 1);
    f32x4* xp = (f32x4*)(x + row * d + c);
    if (j == 0) {
      *xp = *(const f32x4*)(cls + c) + *(const f32x4*)(pos + c);
    } else {
      const int t = keep_idx[s * K + (j - 1)];
      *xp += *(const f32x4*)(pos + (int64_t)(1 + t) * d + c);
    }
  }
}

// dpos[1 + p, :] += sum over s (ascending) of dx[s, 1 + slot[s][p], :] where slot >= 0;  dpos[0, :] and dcls += sum over s of dx[s, 0, :].
// One thread per (pos row, 4 features), the sequences in order: no atomics, the same bits at every run.  The row of a patch that no
// sequence kept is not written.
__global__ void embed_select_bwd_kernel(const float* __restrict__ dx, const int* __restrict__ slot, float* __restrict__ dpos, float* __restrict__ dcls,
                                        int S, int P, int K, int d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over (P + 1) * d / 4
  const int dv = d >> 2;
  if (i >= (int64_t)(P + 1) * dv) return;
  const int n = (int)(i / dv), c = (int)(i - (int64_t)n * dv) * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  bool any = false;
  for (int s = 0; s < S; ++s) {
    const int j = n == 0 ? 0 : 1 + slot[(int64_t)s * P + (n - 1)];   // 0: dropped in this sequence
    if (n == 0 || (j > 0 && j <= K)) {
      acc += *(const f32x4*)(dx + ((int64_t)s * (K + 1) + j) * d + c);
      any = true;
    }
  }
  if (!any) return;
  *(f32x4*)(dpos + (int64_t)n * d + c) += acc;
  if (n == 0) *(f32x4*)(dcls + c) += acc;
}

}  // namespace xvit

using namespace xvit;

// Both draws: what they refuse alike, under the caller's name, and the launch of the instantiation for P and the ranking.
static int token_select(const char* who, int rank, const int32_t* occ, int32_t* keep_idx, int32_t* slot, int32_t* n_fg, int S, int B, int P, int K, int shared,
                        int min_count, uint64_t seed, xvit_stream_t stream) {
  XVIT_REQUIRE(S > 0 && B > 0 && P > 0, "%s: bad sizes (S=%d B=%d P=%d)", who, S, B, P);
  XVIT_REQUIRE(K >= 1, "%s: K=%d, at least one patch must be kept", who, K);
  XVIT_REQUIRE(K <= P, "%s: K=%d exceeds the P=%d patches of a sequence", who, K, P);
  XVIT_REQUIRE(P <= XVIT_TOKEN_SELECT_MAX_P, "%s: P=%d too long (the keys of a sequence sit in LDS: P <= %d)", who, P, XVIT_TOKEN_SELECT_MAX_P);
  XVIT_REQUIRE(keep_idx && slot, "%s: null pointer", who);
  auto launch = [&](auto per, auto r) {
    hipLaunchKernelGGL((token_select_kernel<decltype(per)::value, decltype(r)::value>), dim3(S), dim3(kDrawBlock), 0, (hipStream_t)stream, occ, keep_idx, slot, n_fg, S, B, P,
                       K, shared ? 1 : 0, min_count, seed, drop_epoch_ptr());
  };
  auto by_length = [&](auto r) {
    if (P <= kDrawBlock) launch(Int<1>{}, r);
    else if (P <= 2 * kDrawBlock) launch(Int<2>{}, r);
    else if (P <= 4 * kDrawBlock) launch(Int<4>{}, r);
    else launch(Int<8>{}, r);
  };
  if (rank == kRankHash) by_length(Int<kRankHash>{});
  else if (rank == kRankRandom) by_length(Int<kRankRandom>{});
  else by_length(Int<kRankTop>{});
  return check_launch(who);
}

extern "C" int xvit_token_select_draw(int32_t* keep_idx, int32_t* slot, int S, int B, int P, int K, int shared, uint64_t seed, xvit_stream_t stream) {
  return token_select("xvit_token_select_draw", kRankHash, nullptr, keep_idx, slot, nullptr, S, B, P, K, shared, 0, seed, stream);
}

extern "C" int xvit_token_select_ranked(const int32_t* occ, int32_t* keep_idx, int32_t* slot, int32_t* n_fg, int S, int B, int P, int K, int shared, int mode,
                                        int min_count, uint64_t seed, xvit_stream_t stream) {
  XVIT_REQUIRE(occ, "xvit_token_select_ranked: null occupancy");
  XVIT_REQUIRE(mode == XVIT_TOKEN_RANK_RANDOM || mode == XVIT_TOKEN_RANK_TOP, "xvit_token_select_ranked: unknown mode %d", mode);
  XVIT_REQUIRE(min_count >= 0, "xvit_token_select_ranked: min_count=%d must be >= 0", min_count);
  XVIT_REQUIRE(!shared || (B > 0 && S % B == 0), "xvit_token_select_ranked: with shared, S=%d must be a multiple of B=%d", S, B);
  return token_select("xvit_token_select_ranked", mode, occ, keep_idx, slot, n_fg, S, B, P, K, shared, min_count, seed, stream);
}

extern "C" int xvit_patchify_select(const void* img, int img_dtype, void* out_bf16, const int32_t* keep_idx, int B, int M, int D, int H, int W, int dp, int hp,
                                    int wp, int K, xvit_stream_t stream) {
  XVIT_REQUIRE(img && out_bf16 && keep_idx, "xvit_patchify_select: null pointer");
  XVIT_REQUIRE_PATCH_GRID("xvit_patchify_select", dtype_ok(img_dtype));
  const int64_t P = (int64_t)(D / dp) * (H / hp) * (W / wp), pd = (int64_t)dp * hp * wp;
  XVIT_REQUIRE(K >= 1 && K <= P, "xvit_patchify_select: K=%d outside 1 .. P=%lld", K, (long long)P);
  XVIT_REQUIRE(P < (1ll << 31) && pd < (1ll << 31) && (int64_t)M * B < (1ll << 31), "xvit_patchify_select: geometry too large");
  const int64_t total = (int64_t)M * B * (K + 1) * pd;
  // 8-voxel runs are 16-byte accesses (two of them for fp32): 16-byte aligned volume and destination, else one voxel per thread
  const bool vec = (wp % 8 == 0) && aligned16({img, out_bf16});
  const TokenGeom g = {B, M, D, H, W, dp, hp, wp, K};
  by_dtype_vec(img_dtype, vec, [&](auto t, auto v) {
    using T = decltype(t);
    constexpr int VEC = decltype(v)::value;
    hipLaunchKernelGGL((patchify_select_kernel<T, VEC>), dim3(grid_for(total / VEC, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)img, (bf16*)out_bf16, keep_idx, g,
                       total / VEC);
  });
  return check_launch("xvit_patchify_select");
}

extern "C" int xvit_embed_select_fwd(float* x, const float* cls, const float* pos, const int32_t* keep_idx, int S, int K, int d, xvit_stream_t stream) {
  XVIT_REQUIRE(x && cls && pos && keep_idx, "xvit_embed_select_fwd: null pointer");
  XVIT_REQUIRE(S > 0 && K >= 1 && d > 0 && d % 4 == 0, "xvit_embed_select_fwd: bad sizes (S=%d K=%d d=%d; d %% 4 == 0)", S, K, d);
  XVIT_REQUIRE(aligned16({x, cls, pos}), "xvit_embed_select_fwd: x, cls and pos must be 16-byte aligned");
  const int64_t total = (int64_t)S * (K + 1) * (d / 4);
  hipLaunchKernelGGL(embed_select_fwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, x, cls, pos, keep_idx, K, d, total);
  return check_launch("xvit_embed_select_fwd");
}

extern "C" int xvit_embed_select_bwd(const float* dx, const int32_t* slot, float* dpos, float* dcls, int S, int P, int K, int d, xvit_stream_t stream) {
  XVIT_REQUIRE(dx && slot && dpos && dcls, "xvit_embed_select_bwd: null pointer");
  XVIT_REQUIRE(S > 0 && P > 0 && K >= 1 && K <= P && d > 0 && d % 4 == 0, "xvit_embed_select_bwd: bad sizes (S=%d P=%d K=%d d=%d; d %% 4 == 0)", S, P, K, d);
  XVIT_REQUIRE(aligned16({dx, dpos, dcls}), "xvit_embed_select_bwd: dx, dpos and dcls must be 16-byte aligned");
  const int64_t work = (int64_t)(P + 1) * (d / 4);
  hipLaunchKernelGGL(embed_select_bwd_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dx, slot, dpos, dcls, S, P, K, d);
  return check_launch("xvit_embed_select_bwd");
}
