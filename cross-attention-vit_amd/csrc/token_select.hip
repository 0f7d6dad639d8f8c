// Patch dropout (PatchDropout, Liu et al. 2023): train on a random subset of K of the P patch tokens of every sequence, plus CLS.
//   xvit_token_select_draw   which patches each sequence keeps (counter hash, capturable, no host read-back)
//   xvit_patchify_select     the stored patch matrix of the kept rows only
//   xvit_embed_select_fwd    + pos of the KEPT patch, and the CLS row
//   xvit_embed_select_bwd    dpos / dcls through the selection, in a fixed order
// The GEMMs in between are the ordinary NT / TN ones on the shorter matrix (xvit_gemm).
#include "xvit_common.h"

namespace xvit {

constexpr int kDrawBlock = 1024;
static_assert(XVIT_TOKEN_SELECT_MAX_P == 8 * kDrawBlock, "the draw kernel is instantiated for up to 8 patches per thread");

// One workgroup per sequence.  The keys of the sequence sit in LDS; thread t owns the patches t, t + 1024, ... and ranks them in ONE
// sweep over the LDS array (every lane reads the same address: a broadcast) by counting the (key, p) pairs below its own.  The pairs are
// distinct, so the ranks are a permutation and "kept" is rank < K.  The ascending position of a kept patch is the number of kept patches
// in front of it: a ballot prefix inside each wave, the waves' totals through LDS, 1024 patches per round.  PER: patches a thread
// ranks (P <= PER * 1024).
template <int PER>
__global__ __launch_bounds__(kDrawBlock) void token_select_draw_kernel(int* __restrict__ keep_idx, int* __restrict__ slot, int B, int P, int K, int shared,
                                                                        uint64_t seed, const uint64_t* __restrict__ epoch) {
  __shared__ uint32_t keys[PER * kDrawBlock];
  __shared__ int wave_tot[kDrawBlock / kWave];
  const int s = blockIdx.x, tid = threadIdx.x;
  const uint64_t sd = drop_seed_at(seed, epoch);
  const uint64_t u = shared ? (uint64_t)(s % B) : (uint64_t)s;
  for (int p = tid; p < P; p += kDrawBlock) keys[p] = hash32(sd, u * (uint64_t)P + (uint64_t)p);
  __syncthreads();

  uint64_t mine[PER];
  int below[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int p = tid + i * kDrawBlock;
    mine[i] = p < P ? ((uint64_t)keys[p] << 32) | (uint32_t)p : 0;   // (key, p) as one integer: ties on the key go to the smaller p; 0: nothing is below
    below[i] = 0;
  }
  for (int q = 0; q < P; ++q) {
    const uint64_t other = ((uint64_t)keys[q] << 32) | (uint32_t)q;
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
    const uint64_t vote = __ballot(kept);
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    const int in_wave = __popcll(vote & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = __popcll(vote);
    __syncthreads();
    int before = 0, round = 0;
    for (int w = 0; w < kDrawBlock / kWave; ++w) {
      const int t = wave_tot[w];
      before += w < wave ? t : 0;
      round += t;
    }
    if (p < P) {
      const int pos = base + before + in_wave;
      slot[(int64_t)s * P + p] = kept ? pos : -1;
      if (kept) keep_idx[(int64_t)s * K + pos] = p;
    }
    base += round;
    __syncthreads();                    // wave_tot is rewritten in the next round
  }
}

// Threads walk the OUTPUT [M, B (K + 1), pd] (VEC features each), so only the voxels of kept patches are read: row 0 of a sequence is
// zero, row 1 + j gathers patch keep_idx[s][j] with the token / feature order of patchify_kernel (t = (h Wn + w) Dn + d,
// f = (p1 hp + p2) wp + p3).  A run of VEC features stays inside one W-run of the volume (VEC divides wp).
struct SelectGeom { int B, M, D, H, W, dp, hp, wp, K; };
template <typename T, int VEC>
__global__ void patchify_select_kernel(const T* __restrict__ img, bf16* __restrict__ out, const int* __restrict__ keep_idx, const SelectGeom g, int64_t total_vec) {
  const int pd = g.dp * g.hp * g.wp, pv = pd / VEC;
  const int Dn = g.D / g.dp, Hn = g.H / g.hp, Wn = g.W / g.wp;
  const int P = Dn * Hn * Wn;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total_vec; idx += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(idx % pv) * VEC;
    const int64_t row = idx / pv;
    const int j = (int)(row % (g.K + 1)), s = (int)(row / (g.K + 1));   // s = m B + b
    bf16* dst = out + row * pd + f;
    const int t = j > 0 ? keep_idx[(int64_t)s * g.K + (j - 1)] : -1;
    if ((unsigned)t >= (unsigned)P) {     // the CLS slot (an index outside the grid reads nothing either)
      if constexpr (VEC == 8) *(bf16x8*)dst = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      else *dst = f2bf(0.f);
      continue;
    }
    const int m = s / g.B, b = s - m * g.B;
    const int d = t % Dn, hw = t / Dn, w = hw % Wn, h = hw / Wn;
    const int p3 = f % g.wp, p12 = f / g.wp, p2 = p12 % g.hp, p1 = p12 / g.hp;
    const T* src = img + ((((int64_t)b * g.M + m) * g.D + (d * g.dp + p1)) * g.H + (h * g.hp + p2)) * g.W + (w * g.wp + p3);
    if constexpr (VEC == 8) {
      bf16x8 o;
      if constexpr (sizeof(T) == 4) {
        const f32x4 a = ((const f32x4*)src)[0], c = ((const f32x4*)src)[1];
        o = to_bf16x8(a, c);
      } else {
        o = *(const bf16x8*)src;
      }
      *(bf16x8*)dst = o;
    } else {
      *dst = f2bf((float)*src);
    }
  }
}

// x[s, 0, :] = cls + pos[0];  x[s, 1 + j, :] += pos[1 + keep_idx[s][j], :]   (x fp32 [S (K + 1), d], 4 features per thread)
__global__ void embed_select_fwd_kernel(float* __restrict__ x, const float* __restrict__ cls, const float* __restrict__ pos, const int* __restrict__ keep_idx,
                                        int K, int d, int64_t total) {
  const int dv = d >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % dv) * 4;
    const int64_t row = i / dv;
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

extern "C" int xvit_token_select_draw(int32_t* keep_idx, int32_t* slot, int S, int B, int P, int K, int shared, uint64_t seed, xvit_stream_t stream) {
  XVIT_REQUIRE(S > 0 && B > 0 && P > 0, "xvit_token_select_draw: bad sizes (S=%d B=%d P=%d)", S, B, P);
  XVIT_REQUIRE(K >= 1, "xvit_token_select_draw: K=%d, at least one patch must be kept", K);
  XVIT_REQUIRE(K <= P, "xvit_token_select_draw: K=%d exceeds the P=%d patches of a sequence", K, P);
  XVIT_REQUIRE(P <= XVIT_TOKEN_SELECT_MAX_P, "xvit_token_select_draw: P=%d too long (the keys of a sequence sit in LDS: P <= %d)", P, XVIT_TOKEN_SELECT_MAX_P);
  XVIT_REQUIRE(keep_idx && slot, "xvit_token_select_draw: null pointer");
  auto launch = [&](auto per) {
    hipLaunchKernelGGL((token_select_draw_kernel<decltype(per)::value>), dim3(S), dim3(kDrawBlock), 0, (hipStream_t)stream, keep_idx, slot, B, P, K, shared ? 1 : 0, seed,
                       drop_epoch_ptr());
  };
  if (P <= kDrawBlock) launch(Int<1>{});
  else if (P <= 2 * kDrawBlock) launch(Int<2>{});
  else if (P <= 4 * kDrawBlock) launch(Int<4>{});
  else launch(Int<8>{});
  return check_launch("xvit_token_select_draw");
}

extern "C" int xvit_patchify_select(const void* img, int img_dtype, void* out_bf16, const int32_t* keep_idx, int B, int M, int D, int H, int W, int dp, int hp,
                                    int wp, int K, xvit_stream_t stream) {
  XVIT_REQUIRE(img && out_bf16 && keep_idx, "xvit_patchify_select: null pointer");
  XVIT_REQUIRE(B > 0 && M > 0 && D > 0 && H > 0 && W > 0 && dp > 0 && hp > 0 && wp > 0, "xvit_patchify_select: bad sizes");
  XVIT_REQUIRE(D % dp == 0 && H % hp == 0 && W % wp == 0, "xvit_patchify_select: image dimensions must be divisible by the patch size");
  XVIT_REQUIRE(img_dtype == XVIT_F32 || img_dtype == XVIT_BF16, "xvit_patchify_select: bad dtype");
  const int64_t P = (int64_t)(D / dp) * (H / hp) * (W / wp), pd = (int64_t)dp * hp * wp;
  XVIT_REQUIRE(K >= 1 && K <= P, "xvit_patchify_select: K=%d outside 1 .. P=%lld", K, (long long)P);
  XVIT_REQUIRE(P < (1ll << 31) && pd < (1ll << 31) && (int64_t)M * B < (1ll << 31), "xvit_patchify_select: geometry too large");
  const int64_t total = (int64_t)M * B * (K + 1) * pd;
  // 8-voxel runs are 16-byte accesses (two of them for fp32): 16-byte aligned volume and destination, else one voxel per thread
  const bool vec = (wp % 8 == 0) && (((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(out_bf16)) & 15) == 0);
  const SelectGeom g = {B, M, D, H, W, dp, hp, wp, K};
  by_dtype(img_dtype, [&](auto t) {
    using T = decltype(t);
    if (vec)
      hipLaunchKernelGGL((patchify_select_kernel<T, 8>), dim3(grid_for(total / 8, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)img, (bf16*)out_bf16, keep_idx, g, total / 8);
    else
      hipLaunchKernelGGL((patchify_select_kernel<T, 1>), dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)img, (bf16*)out_bf16, keep_idx, g, total);
  });
  return check_launch("xvit_patchify_select");
}

extern "C" int xvit_embed_select_fwd(float* x, const float* cls, const float* pos, const int32_t* keep_idx, int S, int K, int d, xvit_stream_t stream) {
  XVIT_REQUIRE(x && cls && pos && keep_idx, "xvit_embed_select_fwd: null pointer");
  XVIT_REQUIRE(S > 0 && K >= 1 && d > 0 && d % 4 == 0, "xvit_embed_select_fwd: bad sizes (S=%d K=%d d=%d; d %% 4 == 0)", S, K, d);
  XVIT_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(cls) | reinterpret_cast<uintptr_t>(pos)) & 15) == 0,
               "xvit_embed_select_fwd: x, cls and pos must be 16-byte aligned");
  const int64_t total = (int64_t)S * (K + 1) * (d / 4);
  hipLaunchKernelGGL(embed_select_fwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, x, cls, pos, keep_idx, K, d, total);
  return check_launch("xvit_embed_select_fwd");
}

extern "C" int xvit_embed_select_bwd(const float* dx, const int32_t* slot, float* dpos, float* dcls, int S, int P, int K, int d, xvit_stream_t stream) {
  XVIT_REQUIRE(dx && slot && dpos && dcls, "xvit_embed_select_bwd: null pointer");
  XVIT_REQUIRE(S > 0 && P > 0 && K >= 1 && K <= P && d > 0 && d % 4 == 0, "xvit_embed_select_bwd: bad sizes (S=%d P=%d K=%d d=%d; d %% 4 == 0)", S, P, K, d);
  XVIT_REQUIRE(((reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dpos) | reinterpret_cast<uintptr_t>(dcls)) & 15) == 0,
               "xvit_embed_select_bwd: dx, dpos and dcls must be 16-byte aligned");
  const int64_t work = (int64_t)(P + 1) * (d / 4);
  hipLaunchKernelGGL(embed_select_bwd_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dx, slot, dpos, dcls, S, P, K, d);
  return check_launch("xvit_embed_select_bwd");
}
