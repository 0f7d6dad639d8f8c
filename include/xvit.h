/* xvit.h — C ABI of libxvit_hip.so: the MI355X (gfx950) hot path of the cross-attention 3-D ViT.
 *
 * The reference (vsahni3/cross-attention-ViT) has no FFI; its hot path sits behind plain
 * torch.nn.Module calls.  Each entry point below stands in for the eager-PyTorch op sequence
 * of the reference lines it cites (paths relative to the reference repo).  The Python host
 * side (cross-attention-vit_amd/xvit/) binds these with ctypes and re-exposes the reference's
 * own nn.Module signatures; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions (SURVEY.md §8(b), C-ABI face)
 *   - extern "C", raw device pointers + explicit sizes/strides (in ELEMENTS) + a HIP stream
 *     handle passed as void*.  No torch types cross this boundary.
 *   - The caller allocates every output and workspace; the library never allocates, frees or
 *     keeps a pointer after the call returns.  Every launch is enqueued on `stream`; there is
 *     no internal synchronisation, so all entry points are HIP-graph capturable.
 *   - Return: 0 = OK; <0 = argument/shape/unsupported error (nothing launched; text via
 *     xvit_last_error_string()); >0 = hipError_t reported by the launch.
 *   - Activations are bf16 (fp32 accumulate); the residual stream, LayerNorm statistics,
 *     parameter gradients and the loss are fp32.
 */
#ifndef XVIT_H
#define XVIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XVIT_VERSION 322 /* 0.3.22: xvit_volume_components, xvit_volume_bbox_components, xvit_volume_components_workspace_bytes, xvit_component_config, the XVIT_CC_* record and keep modes (connected foreground components: the crop follows the largest component or those of a minimum size); 0.3.21: the 256x256 GEMM epilogue adds the right residual row for res_row_mod 1 to 3 (xvit_patch_embed_fwd with 1 or 2 tokens per sample, xvit_gemm), no new entry point; 0.3.20: xvit_batch_draw, xvit_batch_gather and XVIT_BATCH_WEIGHTED / XVIT_BATCH_SHUFFLE / XVIT_BATCH_SEQUENTIAL (a device-resident volume store whose batches a captured step draws); 0.3.19: xvit_patch_occupancy, xvit_token_select_ranked and XVIT_TOKEN_RANK_RANDOM / XVIT_TOKEN_RANK_TOP (foreground-ranked token selection for training and eval()); 0.3.18:xvit_volume_bbox, xvit_volume_bbox_workspace_bytes, xvit_crop_config, the XVIT_BBOX_* record and XVIT_AUG_CROP_SCALE (record slot 31): foreground bounding box and crop folded into the augmenting input stage's table; 0.3.17: xvit_elastic_draw, xvit_augment_apply_elastic, xvit_elastic_config and the XVIT_ELASTIC_* record (cubic B-spline elastic deformation composed into the augmenting input stage's resample); 0.3.16: xvit_contrast_draw, xvit_contrast_apply, xvit_contrast_config and the XVIT_CON_* record (Gaussian blur, bias field and gamma behind the augmenting input stage); 0.3.15: xvit_epoch_metrics_update, xvit_epoch_rank_stats, xvit_epoch_rank_stats_max_n and the XVIT_EPOCH_* state head (pooled multi-class epoch metrics, exact one-vs-rest AUROC / AP and bootstrap replicates); 0.3.14: xvit_adamw_step, xvit_adamw_step_dev, xvit_ema_swap and the xvit_adamw_extra table: AdamW, per-tensor rates, fused weight EMA; 0.3.13: xvit_mix_draw, xvit_mix_apply, xvit_mean_ce_mix, xvit_mix_config and the XVIT_MIX_* record (Mixup / CutMix with a soft-target loss); 0.3.12: xvit_token_select_complement, xvit_mae_unshuffle_fwd, xvit_mae_unshuffle_bwd, xvit_token_rows_gather, xvit_token_rows_scatter, xvit_mae_loss_fwd, xvit_mae_loss_bwd and XVIT_MAE_MAX_PD (masked-volume pretraining); 0.3.11: xvit_token_select_draw, xvit_patchify_select, xvit_embed_select_fwd, xvit_embed_select_bwd and XVIT_TOKEN_SELECT_MAX_P (patch dropout: training on a random subset of the patch tokens); 0.3.10: xvit_volume_stats, xvit_volume_stats_workspace_bytes, xvit_norm_config, the clamp of xvit_augment_apply (record slots 29, 30, flag bit 1): per-volume intensity normalisation on the device; 0.3.9: xvit_augment_draw, xvit_augment_apply, their parameter record and XVIT_I16 (device-side volume augmentation); 0.3.8: xvit_grad_sqnorm_partials, xvit_adam_prologue, xvit_adam_step_dev and their state record: capturable Adam with fused global-norm clipping; 0.3.7: xvit_patch_embed_dgrad, xvit_patch_embed_dgrad_supported, xvit_unpatchify (input-volume gradient); 0.3.6: xvit_attn_relevance_step (gradient-weighted relevance through a self-attention block); 0.3.5: xvit_attn_rollout_step (attention rollout through a self-attention block); 0.3.4: xvit_grad_pack_bf16, xvit_grad_unpack_bf16 (bf16 gradient communication); 0.3.3: xvit_add_cast_f32_bf16, xvit_rows_combine; 0.3.2: probability dropout in the low-rank fusion (xvit_cls_softmax_*, xvit_head_cols bias_scale, xvit_head_bias_grad), xvit_xattn_kv_wgrad removed; 0.3.1: xvit_set_dropout_epoch; 0.3.0: workspaces in xvit_attn_fwd/bwd (CLS peel), xvit_linear_f32_batched; 0.2.0: ld_alt in xvit_layernorm_fwd/bwd, dropout in xvit_attn_*, xvit_patch_embed_*, xvit_attn_fwd_fp8, xvit_linear_f32, workspaces */

enum { XVIT_OK = 0, XVIT_ERR_ARG = -1, XVIT_ERR_UNSUPPORTED = -2 };
enum { XVIT_BF16 = 0, XVIT_F32 = 1, XVIT_I16 = 2 /* source volumes of xvit_augment_apply, xvit_volume_stats and xvit_volume_bbox only */ };

typedef void* xvit_stream_t; /* hipStream_t */

int xvit_version(void);
const char* xvit_last_error_string(void);
/* Process-wide tuning knobs (diagnostics / A-B measurements; results never depend on them):
 *   "gemm_tile"      0 = automatic tile choice, 1 = always the 128x128 kernel, 2 = the 256x256 kernel whenever M, N >= 256
 *   "gemm_group"     0 = automatic, n > 0 = column tiles per super-column of the 256x256 kernel's tile walk
 *   "gemm_epilogue"  0 = automatic, 1 = always the 8-byte-per-lane epilogue (bf16 outputs normally use 16 bytes per lane)
 *   "gemm_res_prefetch"  0 = the 256x256 kernel's plain bias + residual epilogue loads its fp32 residual one 16-row region ahead of
 *                    the stores, 1 = inside the epilogue body, like every other epilogue
 *   "gemm_persistent"  the 256x256 kernel's tile loop (NT / NN, no split-K or batch, 16-byte-per-lane bf16 epilogue): 0 = automatic
 *                    (one workgroup per CU walks the tiles where that was measured faster), 1 = always one workgroup per tile,
 *                    n >= 2 = the loop wherever it exists, on at most n workgroups */
int xvit_set_option(const char* name, int value);
/* Dropout under HIP-graph capture.  The reference seeds its dropout masks from the host RNG at every call (nn.Dropout,
 * model_cross.py:27,47,95,101,170; it trains with p = 0.1 .. 0.25, main_mist.py:71-77); a captured step would freeze the seeds passed
 * below and replay the same masks.  With a device counter registered here (process-wide; NULL = off, the default) every dropout-carrying
 * launch hands its address to the kernel, which uses seed + counter * odd constant, read at run time: a graph that increments the counter
 * at its head draws fresh masks at every replay, identical in its forward and backward.  Results with NULL are unchanged. */
int xvit_set_dropout_epoch(const uint64_t* device_counter);

/* ------------------------------------------------------------------------------------------
 * GEMM with fused epilogue.  Replaces every nn.Linear on the path and its autograd backward:
 *   model_cross.py:23,26 (FeedForward), :43,46 (to_qkv / to_out), :81-85 (wq/wk/wv/proj),
 *   :168 (patch_to_embedding), :177-181 (mlp_head); model.py:110-111,133-137.
 * C[M,N] = op(A) * op(B), bf16 operands, fp32 accumulate (v_mfma_f32_16x16x32_bf16).
 *   layout NT: A[M,K] (k contiguous), B[N,K] (k contiguous)       y = x W^T      (forward)
 *   layout NN: A[M,K] (k contiguous), B[K,N] (n contiguous)       dx = dy W      (dgrad)
 *   layout TN: A stored [K,M] (m contiguous), B[K,N] (n contig.)  dW = dy^T x    (wgrad)
 * Epilogue, in this order: +bias[n]; act; dropout; +residual; row remap; store / accumulate.
 * ---------------------------------------------------------------------------------------- */
enum { XVIT_GEMM_NT = 0, XVIT_GEMM_NN = 1, XVIT_GEMM_TN = 2 };
enum { XVIT_ACT_NONE = 0,
       XVIT_ACT_GELU = 1,  /* aux (bf16, optional) receives the pre-activation z; C = gelu(z), erf form */
       XVIT_ACT_DGELU = 2  /* aux (bf16) supplies z; C = acc * gelu'(z) */ };
enum { XVIT_ACC_STORE = 0, XVIT_ACC_ADD = 1 /* fp32 C only: C += result */ };

typedef struct xvit_gemm_args {
  int32_t layout, M, N, K, batch;
  int32_t c_dtype;    /* XVIT_BF16 | XVIT_F32 */
  int32_t act;        /* XVIT_ACT_* */
  int32_t accumulate; /* XVIT_ACC_* */
  int32_t split_k;    /* >=1.  >1: the contraction is cut into split_k ranges whose fp32 partial tiles go to the
                         workspace (xvit_gemm_workspace_bytes(args) bytes); a second kernel sums them in a fixed
                         order and applies the epilogue (deterministic, no atomics) */
  /* residual row = res_row_off + (row % res_row_mod) when res_row_mod > 0 (broadcast, e.g. pos_embedding) */
  int32_t res_row_mod, res_row_off;
  /* output row = row + (row / out_seg_rows) * out_seg_skip + out_row_off when out_seg_rows > 0
     (patch rows -> token rows that leave room for the CLS row, model_cross.py:195-196) */
  int32_t out_seg_rows, out_seg_skip, out_row_off;
  int32_t aux_mode;   /* 0: aux = the pre-activation z (ACT_GELU writes it, ACT_DGELU reads it and evaluates gelu');
                         1: aux = gelu'(z): ACT_GELU writes the derivative (one more fma next to the shared exponential) and
                            ACT_DGELU only multiplies by it — the backward epilogue loses its erf / exp evaluation */
  const void* A; const void* B; void* C;
  const float* bias;     /* [N] fp32 or NULL */
  const float* residual; /* fp32 [*, N] or NULL */
  void* aux;             /* bf16 [M, N] or NULL (see act) */
  int64_t lda, ldb, ldc, ldr, ldaux;                                  /* leading dims, elements; lda, ldb: multiples of 8, >= the row
                                                                         length.  TN with an odd M: the kernel reads one element
                                                                         past a[k][M - 1] of every k-row (inside the row, as lda > M),
                                                                         so the LAST row must be readable up to an even count too */
  int64_t stride_a, stride_b, stride_c, stride_bias, stride_r, stride_aux; /* per-batch strides */
  void* workspace;         /* caller-owned scratch for split_k > 1 (fp32 partial tiles), else NULL */
  int64_t workspace_bytes;
  float* colsum;           /* optional fp32 [N]: colsum[n] += sum over rows of the stored C before its rounding to c_dtype
                              (bias gradient of the producing Linear; atomic adds, so the caller zeroes it first);
                              per-batch stride = stride_bias */
  /* nn.Dropout fused after the activation: element (row, col) is kept iff hash(seed, row*N + col) >= p * 2^24
     (the mask xvit_dropout applies to a contiguous [M, N] tensor with the same seed), scaled by 1/(1-p) */
  float dropout_p; int32_t reserved2;
  uint64_t dropout_seed;
} xvit_gemm_args;

int xvit_gemm(const xvit_gemm_args* args, xvit_stream_t stream);
/* scratch needed by xvit_gemm for these args (0 when none); no launch, no allocation */
int64_t xvit_gemm_workspace_bytes(const xvit_gemm_args* args);

/* fp32 Linear for the single-token CLS path (model_cross.py:91 wq, :100 proj, :112-113 the FFN on the one fused token,
 * :177-181 the heads): y[M,N] = x[M,K] W[N,K]^T (+bias) (GELU) (dropout) (+residual), ALL fp32 (W is the master weight
 * itself), on the f32-input MFMA; K-chunks are summed in a fixed order through the caller's workspace (deterministic).
 * M = batch rows; K % 16 == 0.  Optional bf16 copies for the backward chain: z_bf16 = pre-activation (act = GELU),
 * y_bf16 = the stored y.  Epilogue order as xvit_gemm.  workspace: xvit_linear_f32_workspace_bytes(M, N, K) bytes. */
int64_t xvit_linear_f32_workspace_bytes(int M, int N, int K);
int xvit_linear_f32(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, float* y, int64_t ldy, int M, int N, int K,
                    int act, void* z_bf16, int64_t ldz, const float* residual, int64_t ldr, void* y_bf16, int64_t ldyb, float dropout_p,
                    uint64_t dropout_seed, void* workspace, int64_t workspace_bytes, xvit_stream_t stream);

/* Tiny fp32 linear for shapes the MFMA tile cannot address (the num_classes=2 head,
 * model_cross.py:181).  y[M,N] = x[M,K] W[N,K]^T + b.  x is bf16, W/b/y fp32.  */
int xvit_small_linear_fwd(const void* x_bf16, int64_t ldx, const float* W, const float* b, float* y, int M, int N, int K, xvit_stream_t stream);
/* dx[M,K] (bf16) = (dy W) * (z ? gelu'(z) : 1);  dW[N,K] += dy^T x;  db[N] += colsum(dy).  dy fp32.
 * z (bf16 [M,K], optional) is the pre-activation of the GELU that produced x (model_cross.py:178). */
int xvit_small_linear_bwd(const float* dy, const void* x_bf16, int64_t ldx, const float* W, const void* z_bf16, int64_t ldz,
                          void* dx_bf16, int64_t lddx, float* dW, float* db, int M, int N, int K, int deterministic, xvit_stream_t stream);
/* deterministic != 0: one row chunk instead of 8-row chunks meeting in fp32 atomics (bit-reproducible, slower) */

/* ------------------------------------------------------------------------------------------
 * LayerNorm (model_cross.py:11-17 PreNorm, :174/:203 final norm; model.py:186-187,207 eps=1e-6).
 * x is the fp32 residual stream [rows, d] (row stride ldx).  If x_alt != NULL, row k * seq_len (the first row of
 * sequence k) is read from x_alt + k * ld_alt instead: the "cls of i + patches of j" concatenation of model_cross.py:140
 * without materialising it (ld_alt = seq_len * ldx when x_alt is the other modality's token tensor, = d for a packed
 * [sequences, d] copy of its CLS rows).
 * Outputs: y_bf16 (the GEMM operand) and / or y_f32 (the fp32 copy the single-token CLS path feeds to xvit_linear_f32);
 * either may be NULL, not both.
 * ---------------------------------------------------------------------------------------- */
int xvit_layernorm_fwd(const float* x, const float* x_alt, int64_t ldx, int seq_len, int64_t ld_alt, const float* gamma, const float* beta,
                       float eps, void* y_bf16, int64_t ldy, float* y_f32, int64_t ldyf, float* mean, float* rstd, int rows, int d,
                       xvit_stream_t stream);
/* dx = (dres ? dres : 0) + LN'(dy); also emits a bf16 copy of dx (the next GEMMs' operand) when
 * dx_bf16 != NULL; dgamma/dbeta are ADDED (fp32 atomics).  Optional dxsum[d] += column sums of dx and
 * dressum[d] += column sums of dres: the bias gradients of the Linears on either side of the norm
 * (dx is the dy of the Linear that produced x; dres the dy of the Linear whose output joined x), for free. */
int xvit_layernorm_bwd(const void* dy_bf16, int64_t lddy, const float* x, const float* x_alt, int64_t ldx, int seq_len, int64_t ld_alt,
                       const float* mean, const float* rstd, const float* gamma, const float* dres, int64_t lddres,
                       float* dx, int64_t lddx, void* dx_bf16, int64_t lddxb, float* dgamma, float* dbeta, float* dxsum,
                       float* dressum, int rows, int d, float* workspace, int64_t workspace_bytes, xvit_stream_t stream);
/* workspace (optional, xvit_layernorm_bwd_workspace_bytes(rows, d) bytes): the deterministic form — per-block partial sums
 * are stored there and added to dgamma / dbeta / dxsum / dressum in block order by a second small kernel instead of by fp32
 * atomics (bit-reproducible run to run; SURVEY.md 8(b) "Determinism"). */
int64_t xvit_layernorm_bwd_workspace_bytes(int rows, int d);

/* ------------------------------------------------------------------------------------------
 * Fused self-attention (model_cross.py:53-60; model.py:165-172): softmax(q k^T * scale) v
 * without materialising the [B,H,N,N] scores.  Element (b, n, h, :) of q/k/v lives at
 * ptr + b*stride_b + n*stride_n + h*dh (q, k, v normally point into one [B,N,3d] tensor).
 * dh must be 64.  lse[B,H,N] = log-sum-exp of the scaled scores (saved for backward).
 * dropout_p > 0 (model.py:169 attn_dropout on the probabilities): element (b, h, q, k) is kept iff
 * hash(seed, ((b*H + h)*N + q)*N + k) >= p * 2^24 (the mask xvit_dropout applies to a contiguous [B, H, N, N] tensor with that
 * seed), scaled by 1/(1-p), applied after the softmax normalisation; the backward regenerates it from the same (p, seed).
 * ---------------------------------------------------------------------------------------- */
int xvit_attn_fwd(const void* q, const void* k, const void* v, int64_t stride_b, int64_t stride_n, void* o, int64_t o_stride_b,
                  int64_t o_stride_n, float* lse, int B, int H, int N, int dh, float scale, float dropout_p, uint64_t dropout_seed,
                  float* workspace, int64_t workspace_bytes, xvit_stream_t stream);
/* workspace: xvit_attn_bwd_workspace_bytes(B, H, N) bytes of fp32, 16-byte aligned (rowsum(do*o), -lse*log2e, CLS-peel partials).
 * dq/dk/dv use the q/k/v strides. */
int xvit_attn_bwd(const void* q, const void* k, const void* v, int64_t stride_b, int64_t stride_n, const void* o, const void* d_o,
                  int64_t o_stride_b, int64_t o_stride_n, const float* lse, float* workspace, int64_t workspace_bytes, void* dq, void* dk,
                  void* dv, int B, int H, int N, int dh, float scale, float dropout_p, uint64_t dropout_seed, xvit_stream_t stream);
/* CLS peel.  The reference's sequences are cls + P patch tokens (model_cross.py:195-196): N = 64 m + 1 at every BASELINE config with
 * cubic power-of-two volumes (513, 1025, 4097).  On a tile grid token 0 costs one more 128-query block per (b, head) and one more
 * 64-key tile per block.  With a workspace (xvit_attn_fwd_workspace_bytes > 0 <=> the shape qualifies: N % 64 == 1, no probability
 * dropout, and under the default xvit_set_option("attn_peel", 1) a grid of >= 768 workgroups; 2 = any grid, 0 = never) the kernels tile the patch tokens only; token 0 enters as the initial
 * online-softmax state / initial gradient accumulators (as a key) and as one extra MFMA block per wave with partial results merged
 * in a fixed order (as a query).  Same outputs (o, lse, dq, dk, dv for all N tokens), bit-reproducible; workspace == NULL keeps
 * token 0 on the tile grid. */
int64_t xvit_attn_fwd_workspace_bytes(int B, int H, int N);
int64_t xvit_attn_bwd_workspace_bytes(int B, int H, int N);
/* One step of attention rollout (Abnar & Zuidema 2020) through one self-attention block, for a row vector r_in [B, N] (fp32,
 * contiguous) over the block's tokens:
 *   r_out[b, n] = r_in[b, n] / 2 + 1 / (2 H) sum_h sum_m r_in[b, m] P_h[b, m, n],   P_h[b, m, n] = exp(scale q[b, m, h] . k[b, n, h] - lse[b, h, m])
 * q / k: the addressing of xvit_attn_fwd (ptr + b stride_b + n stride_n + 64 h, bf16: pointers into the block's qkv); lse: the [B, H, N]
 * tensor xvit_attn_fwd wrote (either form).  P is recomputed and never stored; the r-weighted sum runs in fp32 in a fixed order
 * (no atomics: bit-reproducible).  r_in and r_out must not overlap.  dh = 64 only. */
int xvit_attn_rollout_step(const void* q, const void* k, int64_t stride_b, int64_t stride_n, const float* lse, const float* r_in, float* r_out,
                           int B, int H, int N, int dh, float scale, xvit_stream_t stream);
/* One step of class-specific relevance (Chefer, Gur & Wolf 2021) through one self-attention block, for a row vector r_in [B, N] (fp32,
 * contiguous):
 *   r_out[b, n] = r_in[b, n] + 1 / H sum_h sum_m r_in[b, m] max(0, P_h[b, m, n] dP_h[b, m, n]),   dP_h[b, m, n] = dO[b, m, h] . v[b, n, h]
 * P_h as in xvit_attn_rollout_step; q / k / v: the addressing of xvit_attn_fwd (pointers into the block's qkv); d_o: the gradient of
 * the block's attention output, bf16 (ptr + b stride_b_do + n stride_n_do + 64 h).  P and dP are recomputed and never stored; the sum
 * runs in fp32 in a fixed order (no atomics: bit-reproducible) and 1 / H times it is added to r_in last (r_in >= 0: r_out >= r_in
 * exactly; dO = 0: r_out == r_in).  r_in and r_out must not overlap.  dh = 64 only. */
int xvit_attn_relevance_step(const void* q, const void* k, const void* v, int64_t stride_b, int64_t stride_n, const float* lse, const void* d_o,
                             int64_t stride_b_do, int64_t stride_n_do, const float* r_in, float* r_out, int B, int H, int N, int dh, float scale,
                             xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CLS-query cross-attention (model_cross.py:91-99): one query row per (b, h) against N keys.
 * q [B, d] bf16 (row stride ldq); k/v as above; o [B, d] bf16; p [B,H,N] fp32 probabilities
 * (saved for backward).  HBM-bound GEMV-style kernel.  q_f32 [B, d] (optional, row stride ldqf) replaces q as the query and
 * o_f32 (optional) receives an fp32 copy of o: the single-token CLS path keeps its operands in fp32 (xvit_linear_f32).
 * ---------------------------------------------------------------------------------------- */
int xvit_cls_xattn_fwd(const void* q, int64_t ldq, const float* q_f32, int64_t ldqf, const void* k, const void* v, int64_t stride_b,
                       int64_t stride_n, void* o, int64_t ldo, float* o_f32, int64_t ldof, float* p, int B, int H, int N, int dh, float scale,
                       float dropout_p, uint64_t dropout_seed, xvit_stream_t stream);
/* dropout_p / dropout_seed: attn_drop on the probabilities (model_cross.py:97); p[] holds the pre-dropout values */
int xvit_cls_xattn_bwd(const void* q, int64_t ldq, const void* k, const void* v, int64_t stride_b, int64_t stride_n, const float* p,
                       const void* d_o, int64_t lddo, float* dq, int64_t lddq, void* dk, void* dv, float* coef, int B, int H, int N, int dh,
                       float scale, float dropout_p, uint64_t dropout_seed, xvit_stream_t stream);
/* dk / dv (bf16, laid out like k / v; both or neither) and / or coef (fp32 [B, N, 2 H]).  dK and dV of one (b, head) are rank one:
 * dk[n] = coef[b][n][head] * q_head (the softmax scale included), dv[n] = coef[b][n][H + head] * dO_head.
 *   xvit_xattn_kv_dgrad (the low-rank fusion's token gradient): dhn[b, n, :] (bf16) = dk[b, n, :] Wk + dv[b, n, :] Wv
 *     = sum_j coef[b, n, j] R[j, b, :], with R (fp32 [2 H, B, d]): R[h, b, :] = q[b, h, :] Wk[64 h .. 64 h + 63, :],
 *     R[H + h, b, :] = dO[b, h, :] Wv[64 h .., :] (xvit_head_rows).  d = 64 H, 2 H <= 32. */
int xvit_xattn_kv_dgrad(const float* coef, const float* R, void* dhn_bf16, int64_t lddh, int B, int H, int N, int d, xvit_stream_t stream);

/* The fusion's key / value path in its low-rank form (model_cross.py:88-99): with one query row per (sample, head),
 *   scores[b, n, h] = hn[b, n, :] . U[b, h, :] (+ a constant over n),  U[b, h, :] = q[b, h, :] Wk[64 h .. 64 h + 63, :]          (xvit_head_rows)
 *   out[b, 64 h + e] = rz[b, h] sum_c Wv[64 h + e, c] S[b, h, c] + bv[64 h + e],  S[b, h, :] = sum_n e[b, n, h] hn[b, n, :]       (xvit_head_cols)
 * so wk and wv are never applied to the N tokens: the two passes over hn are batched xvit_gemm calls ([N, d] x [d, 16] and
 * [16, N] x [N, d] per sample) and the softmax over n sits between them (xvit_cls_softmax_fwd: bf16 weights e = exp(scale (s - max)),
 * rz = 1 / sum e).  Backward: dp = hn . Y (Y = dO_h Wv_h, xvit_head_rows), xvit_cls_softmax_bwd -> coef (the input of
 * xvit_xattn_kv_dgrad) and bf16 ds, T = sum_n ds hn (xvit_gemm), dq = Wk_h T (xvit_head_cols), dWk_h = q_h^T T, dWv_h = dO_h^T (rz S)
 * (xvit_head_wgrad).  All per-head products are fp32 on the f32-input MFMA against the fp32 master weights; d = 64 H, H <= 16.
 *   xvit_head_rows : out[b, h, c] (fp32, element strides out_sb / out_sh; optional bf16 copy with its own strides) = sum_e x[b, 64 h + e] W[64 h + e, c]
 *   xvit_head_cols : out[b, 64 h + e] (fp32, row stride ldo; optional bf16 copy) = row_scale[b, h] * sum_c t[b, h, c] W[64 h + e, c]
 *                    + bias_scale[b, h] * bias[64 h + e]   (row_scale, bias, bias_scale optional: 1, 0, 1)
 *   xvit_head_wgrad: dW[64 h + e, c] = sum_b x[b, 64 h + e] row_scale[b, h] t[b, h, c]
 *   xvit_head_bias_grad: out[j] = sum_b x[b, j] w[b, j / 64] (the gradient of bv under dropout; samples summed in order)
 * Dropout on the probabilities (attn_drop, model_cross.py:97; the reference trains with 0.1 .. 0.25): p'[n] = m[n] p[n] / (1 - rate) with
 * the mask xvit_cls_xattn_fwd uses (xvit_dropout on a contiguous [B, H, N] tensor).  xvit_cls_softmax_fwd then also writes the KEPT weights
 * e_masked (the operand of the row-sum GEMM: S = sum_n e_masked hn) and rz becomes a [3][B][H] block: rz, rz / (1 - rate) (the row scale
 * of xvit_head_cols and of dWv) and rz / (1 - rate) * sum_n e_masked (bias_scale: the weight in front of bv, which no longer is one);
 * xvit_cls_softmax_bwd regenerates the mask: dp~ = m dp / (1 - rate) replaces dp and the second half of coef is p'.                    */
int xvit_head_rows(const float* x, int64_t ldx, const float* W, int64_t ldw, float* out, int64_t out_sb, int64_t out_sh, void* out_bf16, int64_t ob_sb,
                   int64_t ob_sh, int ob_heads, int B, int H, int d, xvit_stream_t stream);   /* head rows H .. ob_heads - 1 of the bf16 copy are zeroed */
int xvit_head_cols(const float* t, int64_t t_sb, int64_t t_sh, const float* W, int64_t ldw, const float* row_scale, int64_t rs_ld, const float* bias,
                   const float* bias_scale, int64_t bsc_ld, float* out, int64_t ldo, void* out_bf16, int64_t ldob, int B, int H, int d, xvit_stream_t stream);
int xvit_head_bias_grad(const float* x, int64_t ldx, const float* w, int64_t ldw, float* out, int B, int H, int d, xvit_stream_t stream);
int xvit_head_wgrad(const float* x, int64_t ldx, const float* t, int64_t t_sb, int64_t t_sh, const float* row_scale, int64_t rs_ld, float* dW, int64_t lddw,
                    int B, int H, int d, xvit_stream_t stream);
/* s [B, N, lds] fp32 -> e [B, N, lde] bf16 (columns >= H zeroed; lde <= 16), rz [B, H]; dropout_p > 0: also e_masked (like e) and rz is [3][B][H] */
int xvit_cls_softmax_fwd(const float* s, int64_t lds, void* e_bf16, int64_t lde, float* rz, int B, int H, int N, float scale, void* e_masked_bf16,
                         float dropout_p, uint64_t dropout_seed, xvit_stream_t stream);
/* p = e rz; ds = scale p (dp~ - sum_n p dp~) -> coef [B, N, 2 H] fp32 = (ds | p'), ds_bf16 [B, N, ldb] (columns >= H zeroed) */
int xvit_cls_softmax_bwd(const void* e_bf16, int64_t lde, const float* rz, const float* dp, int64_t ldp, float* coef, void* ds_bf16, int64_t ldb, int B, int H,
                         int N, float scale, float dropout_p, uint64_t dropout_seed, xvit_stream_t stream);

/* MX-fp8 forward attention (BASELINE.json configs[4] "fp8 MFMA QK^T/AV path"; reference ops model_cross.py:55-59):
 * same arguments and outputs as xvit_attn_fwd without dropout, but q, k, v are first quantised to OCP e4m3 with one e8m0
 * scale per 32 contraction elements (q, k along d_h; v transposed, along the keys) into the caller's workspace, and both
 * products run on v_mfma_scale_f32_32x32x64_f8f6f4 (2x the bf16 MFMA rate).  Accuracy is that of 3-bit mantissas (stated in
 * tests/test_attn_fp8_gpu.py); lse / o feed the bf16 backward unchanged.  Opt-in: nothing selects it by default. */
int64_t xvit_attn_fp8_workspace_bytes(int B, int H, int N, int dh);
int xvit_attn_fwd_fp8(const void* q, const void* k, const void* v, int64_t stride_b, int64_t stride_n, void* o, int64_t o_stride_b, int64_t o_stride_n,
                      float* lse, int B, int H, int N, int dh, float scale, void* workspace, int64_t workspace_bytes, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 3-D patchify (model_cross.py:193, modelv3.py:129): img [B, M, 1, D, H, W] (fp32 or bf16, contiguous) ->
 * rows of a bf16 patch matrix [*, pd]; token t = (h*Wn + w)*Dn + d, feature f = (p1*hp + p2)*wp + p3.
 * Patch (b, m, t) goes to row  b*stride_b + m*stride_m + t + row_off,  so the same kernel lays the rows out
 *   per modality with a CLS slot  (ModelCross: stride_b = P+1, stride_m = B*(P+1), row_off = 1) or
 *   concatenated per sample       (ModelVIT:   stride_b = M*P+1, stride_m = P,     row_off = 1).
 * zero_rows rows (0, zero_row_stride, 2*zero_row_stride, ...) are zero-filled: the CLS slots, so the patch
 * matrix lines up row-for-row with the token tensor (model_cross.py:195-196).
 * ---------------------------------------------------------------------------------------- */
int xvit_patchify(const void* img, int img_dtype, void* patches_bf16, int B, int M, int D, int H, int W, int dp, int hp, int wp,
                  int64_t stride_b, int64_t stride_m, int row_off, int zero_rows, int64_t zero_row_stride, xvit_stream_t stream);
/* The exact inverse of xvit_patchify, for gradients: patches fp32 [*, pd] -> img [B, M, 1, D, H, W] (fp32 or bf16 by img_dtype, contiguous,
 * rounded once to nearest even).  Voxel (b, m, z, y, x) is read from row  b*stride_b + m*stride_m + t + row_off, column f  (token and
 * feature order of xvit_patchify), so the same placements apply (ModelCross: stride_b = P+1, stride_m = B*(P+1), row_off = 1; ModelVIT:
 * stride_b = M*P+1, stride_m = P, row_off = 1) and the CLS rows are never read.  Every voxel of img is written. */
int xvit_unpatchify(const float* patches, void* img, int img_dtype, int B, int M, int D, int H, int W, int dp, int hp, int wp, int64_t stride_b,
                    int64_t stride_m, int row_off, xvit_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Patch embedding straight from the volume (model_cross.py:193-197: rearrange -> patch_to_embedding -> + pos_embedding):
 *   x[(m*B + b)*(cls_rows + P) + cls_rows + t, :] = patch(b, m, t) W^T + bias + pos[cls_rows + t, :]
 * with the token / feature order of xvit_patchify, WITHOUT writing the [rows, dp*hp*wp] patch matrix: the GEMM's LDS-DMA
 * loaders gather the patch rows from img [B, M, 1, D, H, W] (bf16, contiguous).  CLS rows (cls_rows = 1) come out as
 * bias + pos[0] and are overwritten by xvit_cls_row_fwd, exactly as with a zero CLS row in a stored patch matrix.
 * xvit_patch_embed_wgrad: dW[d, pd] = sum over patch rows of dx[row, :]^T patch(row) (CLS rows of dx are skipped), fp32,
 * split over the contraction into the caller's workspace and summed in a fixed order (deterministic).
 * xvit_patch_embed_supported: 1 when the geometry fits the fused kernels (wp in {8,16,32,64}, hp*wp % 64 == 0, pd and d multiples of
 * 256, >= 2048 rows, volume < 2 GiB); otherwise use xvit_patchify + xvit_gemm.  ANY patch grid qualifies: where 64 consecutive tokens
 * are whole d-columns of one h-row (64 % (D/dp) == 0 and (D/dp)*(W/wp) % 64 == 0: 128^3 volumes) the weight gradient's K-step offsets
 * are wave-uniform; elsewhere (15 patches per axis at the 240^3 UCSF-PDGM shape, dataset_ucsf.py:84-88) every lane places its k-rows
 * per K-step from the running token count (three multiply-high divisions), K-steps may straddle samples.
 * ---------------------------------------------------------------------------------------- */
typedef struct xvit_patch_geom {
  int32_t B, M;          /* img [B, M, 1, D, H, W] */
  int32_t D, H, W;
  int32_t dp, hp, wp;    /* patch_size (model_cross.py:151) */
  int32_t cls_rows;      /* 1: every sample's rows start with one CLS row (ModelCross); 0: patch rows only */
} xvit_patch_geom;
int xvit_patch_embed_supported(const xvit_patch_geom* g, int d);
int xvit_patch_embed_fwd(const void* img_bf16, const xvit_patch_geom* g, const void* W_bf16, int64_t ldw, const float* bias, const float* pos, int64_t ldpos,
                         float* x, int64_t ldx, int d, xvit_stream_t stream);
int64_t xvit_patch_embed_wgrad_workspace_bytes(const xvit_patch_geom* g, int d);
int xvit_patch_embed_wgrad(const void* img_bf16, const xvit_patch_geom* g, const void* dx_bf16, int64_t lddx, float* dW, int64_t lddw, int d, void* workspace,
                           int64_t workspace_bytes, xvit_stream_t stream);
/* Input gradient of the patch embedding, the patch-gradient matrix never stored:
 *   dimg[b, m, 0, z, y, x] = sum_c dx[(m*B + b)*(cls_rows + P) + cls_rows + t, c] W[c, f]
 * for the voxel at feature f of patch t (the token / feature order of xvit_patchify).  The 256x256 NN GEMM with dx (bf16, CLS rows
 * included, row stride lddx) as A and W (bf16 [d, pd], row stride ldw) as B; its epilogue maps each (row, column) to its voxel and stores
 * whole 16-byte runs.  CLS rows are computed but never stored.  dimg [B, M, 1, D, H, W] contiguous, fp32 or bf16 by dimg_dtype (bf16:
 * rounded once from the fp32 accumulator), independent of the forward volume's dtype; every voxel is written exactly once (patches do
 * not overlap), no atomics, no split-K: bit-reproducible.
 * xvit_patch_embed_dgrad_supported: 1 when the geometry fits (wp % 8 == 0, d % 64 == 0, >= 2048 token rows, < 2^30 voxels); a superset of
 * xvit_patch_embed_supported.  Otherwise: xvit_gemm (NN, fp32 C) into a patch matrix, then xvit_unpatchify. */
int xvit_patch_embed_dgrad_supported(const xvit_patch_geom* g, int d);
int xvit_patch_embed_dgrad(const void* dx_bf16, int64_t lddx, const void* W_bf16, int64_t ldw, const xvit_patch_geom* g, int d, void* dimg, int dimg_dtype,
                           xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Input stage (dataset_ucsf.py:84-88, 152-158): MONAI `ResizeWithPadOrCropd(spatial_size, constant_values=pad_value)`
 * followed by `.to(torch.float)`, on the raw int16 NIfTI voxels already on the device:
 * src int16 [nvol, Ds, Hs, Ws] -> dst bf16 [nvol, D, H, W].  Per dimension: symmetric pad with before = deficit/2
 * when the source is smaller, centre crop with start = size/2 - target/2 when it is larger (MONAI SpatialPad
 * "symmetric" + CenterSpatialCrop).  MONAI is not installed here: PARITY UNPINNED (restated from its documented rule).
 * ---------------------------------------------------------------------------------------- */
int xvit_resize_pad_crop_i16(const void* src_i16, void* dst_bf16, int nvol, int Ds, int Hs, int Ws, int D, int H, int W,
                             float pad_value, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Augmenting input stage (stands where dataset_ucsf.py:94-113 runs MONAI's random transforms on five CPU loader workers): pad / crop to
 * img_size, one random affine resample and one random intensity transform, straight from the raw volume on the device into the
 * [B, M, 1, D, H, W] tensor xvit_patch_embed_fwd reads.  The source is read once and the destination written once.  The transform set and
 * its ranges are this project's own; parity with MONAI's random stream is NOT claimed (the position dropout takes).
 *
 * Two kernels with a table between them.  xvit_augment_draw turns (config, seed) into params[B, M, XVIT_AUG_NPARAM] (fp32, one record
 * per volume) that can be read back; xvit_augment_apply is a pure function of (src, params).
 *
 * Record (fp32 slots):
 *    0..11  A | t, row-major 3 x 4: source voxel index p = A (z, y, x) + t for the destination voxel index (z, y, x)
 *    12, 13 intensity: v = a v + b                       14  noise sigma (0: no noise)
 *    15     noise seed, a uint32 bit pattern             16  flags (integer-valued): bit 0 = exact path: A is a diagonal of +-1 and t is integral;
 *                                                            bit 1 = clamp: the resampled value is clamped to [slot 29, slot 30] before a v + b
 *    17..19 flips (1 = the axis is reversed)             20..22 rotation angles, radians (0 when not drawn)
 *    23..25 zooms (1 when not drawn)                     26..28 translation in voxels (0 when not drawn)
 *    29, 30 clamp window lo, hi in SOURCE units (zero as drawn; xvit_volume_stats writes them)
 *    31     the crop scale k folded by xvit_volume_bbox (zero as drawn: no crop folded)
 * Slots 17..28 record what was drawn; xvit_augment_apply reads slots 0..16 and, only when flag bit 1 is set, slots 29 and 30.
 *
 * xvit_augment_draw.  Uniform numbers are u(i) = (hash32(seed', i) & 0xFFFFFF) / 2^24 with the dropout hash (xvit_dropout), seed' = seed +
 * *counter * 0xD1B54A32D192ED03 when a device counter is given (read at run time; advance != 0: one thread stores counter + 1 after every
 * thread has read it, so a replayed graph draws anew at every replay), else seed.  Spatial draws of sample b use i = 64 b + k: k = 0..2
 * flip z, y, x (u < flip_prob); 3 rotate (u < rotate_prob), 4..6 the angles about z, y, x, uniform in [-rotate_range, rotate_range];
 * 7 zoom, 8..10 the zooms, uniform in zoom_range; 11 translate, 12..14 the translation, uniform in [-translate_range, translate_range].
 * They never depend on the modality: the M volumes of a sample are co-registered scans and move together.  Intensity draws of volume
 * (b, m) use i = 64 (b M + m) + 32 + k: 0 scale?, 1 the factor s in scale_range, 2 shift?, 3 the shift h in shift_range, 4 noise?,
 * 5 sigma = noise_std (1 + draw) / 2^24 (never 0), 6 the noise seed (all 32 bits of the hash).  a = s intensity_scale,
 * b = s intensity_shift + h: the fixed affine (normalisation) comes first.
 * Matrix, composed in double and rounded once: with c = ((D, H, W) - 1) / 2 the destination centre and o the per-axis offset of
 * xvit_resize_pad_crop_i16 (source index = destination index + o),
 *    L = F Rz Ry Rx diag(1 / zoom),   F = diag(+-1),   Rz = [[1, 0, 0], [0, cz, -sz], [0, sz, cz]] (turns the y-x plane about z),
 *    Ry = [[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]],   Rx = [[cx, -sx, 0], [sx, cx, 0], [0, 0, 1]]   (axes in index order z, y, x),
 *    A = L,   t = c + o + translation - L c.
 * All probabilities 0: A = I, t = o, exact.  config is a HOST struct, read during the call.  params 16-byte, counter 8-byte aligned.
 *
 * xvit_augment_apply.  src [nvol, Ds, Hs, Ws] int16 / bf16 / fp32 -> dst [nvol, D, H, W] bf16 / fp32, both contiguous; a volume has fewer than
 * 2^31 voxels on either side.  General path: trilinear interpolation at p (fp32), source voxels outside the volume counting as pad_value
 * (borders blend with it); exact path (flag bit 0): the source voxel at the integer index is copied (a flip is a reversed run).  With
 * flag bit 1 (XVIT_AUG_FLAG_CLAMP) the value, pad_value included, is then clamped in source units, v = fminf(fmaxf(v, lo), hi) with lo, hi
 * of slots 29, 30 (a NaN becomes lo); with the bit clear nothing of this happens and the slots are not read.  Then
 * v = a v + b; sigma > 0: v += sigma n with n = sqrt(-2 ln u1) cos(2 pi u2), u1 = ((hash32(noise_seed, 2 i) & 0xFFFFFF) + 1) / 2^24,
 * u2 = (hash32(noise_seed, 2 i + 1) & 0xFFFFFF) / 2^24 for voxel i = (z H + y) W + x of its volume; one rounding to the destination dtype.
 * With a = 1, b = 0, sigma = 0, int16 -> bf16 the exact path reproduces xvit_resize_pad_crop_i16 bit for bit.  A workgroup owns one
 * destination brick, every lane 8 consecutive voxels along W (16-byte stores where the address allows, any W); no atomics: bit-reproducible.
 * ---------------------------------------------------------------------------------------- */
#define XVIT_AUG_NPARAM 32
enum { XVIT_AUG_MATRIX = 0, XVIT_AUG_SCALE = 12, XVIT_AUG_SHIFT = 13, XVIT_AUG_SIGMA = 14, XVIT_AUG_NOISE_SEED = 15, XVIT_AUG_FLAGS = 16,
       XVIT_AUG_FLIPS = 17, XVIT_AUG_ANGLES = 20, XVIT_AUG_ZOOMS = 23, XVIT_AUG_TRANSLATION = 26, XVIT_AUG_CLAMP_LO = 29, XVIT_AUG_CLAMP_HI = 30 };
enum { XVIT_AUG_FLAG_EXACT = 1, XVIT_AUG_FLAG_CLAMP = 2 };
typedef struct xvit_augment_config {
  float flip_prob[3];                          /* per axis z, y, x */
  float rotate_prob, rotate_range[3];          /* radians, about z, y, x */
  float zoom_prob, zoom_range[2];              /* lo <= hi, lo > 0; one draw per axis */
  float translate_prob, translate_range[3];    /* voxels, >= 0 */
  float scale_prob, scale_range[2];            /* multiplicative factor, lo <= hi */
  float shift_prob, shift_range[2];            /* lo <= hi */
  float noise_prob, noise_std;                 /* noise_std >= 0 */
  float intensity_scale, intensity_shift;      /* the fixed affine folded into a, b */
} xvit_augment_config;
int xvit_augment_draw(const xvit_augment_config* config, float* params, int B, int M, int Ds, int Hs, int Ws, int D, int H, int W, uint64_t seed,
                      uint64_t* counter, int advance, xvit_stream_t stream);
int xvit_augment_apply(const void* src, int src_dtype, void* dst, int dst_dtype, const float* params, int nvol, int Ds, int Hs, int Ws, int D, int H,
                       int W, float pad_value, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Elastic deformation (csrc/elastic.hip): random non-rigid deformation composed into the ONE resample of the augmenting input stage, so
 * that a volume is never interpolated twice.  The rule is this project's own: a cubic B-spline free-form deformation on a coarse control
 * grid, as TorchIO's RandomElasticDeformation / SimpleITK's BSplineTransform build it; parity with their random streams is NOT claimed.
 *
 * Control grid, per SAMPLE (the M modalities of a sample are co-registered and move together): field [B, 3, Gz, Gy, Gx] fp32, contiguous,
 * 16-byte aligned, component order (z, y, x), units DESTINATION voxels, 4 <= G_axis <= XVIT_ELASTIC_MAX_GRID.
 * Record erec [B, XVIT_ELASTIC_NREC] fp32: slot 0 flag (1 = the sample is deformed), 1 the uniform draw behind the decision, 2..4
 * max |phi| per component as drawn, 5..7 zero.
 *
 * Displacement at destination voxel index i along an axis of length n with G control points: s = (G - 3) / (n - 1) (0 when n = 1; fp32,
 * rounded once), g = i s, c = min(floor(g), G - 4), tau = g - c in [0, 1]: the last voxel has c = G - 4, tau = 1 and nothing is read at
 * c + 4.  Weights B0 = (1 - tau)^3 / 6, B1 = (3 tau^3 - 6 tau^2 + 4) / 6, B2 = (-3 tau^3 + 3 tau^2 + 3 tau + 1) / 6, B3 = tau^3 / 6;
 *    u_k(q) = sum over a, b, c = 0..3 of B_a(tau_z) B_b(tau_y) B_c(tau_x) phi_k[c_z + a, c_y + b, c_x + c],   k = z, y, x.
 * Composition: the deformation acts on the destination grid first, then the record's affine, p = A (q + u(q)) + t, computed as
 * p_affine + A u with p_affine formed exactly as xvit_augment_apply forms it, so a zero field is bit-identical to xvit_augment_apply's
 * general path.  Everything behind p is that path unchanged: the [-2, size + 1] clamp, trilinear taps with pad_value outside, the optional
 * clamp window, a v + b, noise, one rounding.
 *
 * xvit_elastic_draw.  u(i) = (hash32(seed', i) & 0xFFFFFF) / 2^24, seed' = (seed + *counter * 0xD1B54A32D192ED03) ^ 0x00454C4153544943
 * ("ELASTIC": apart from the augment and contrast streams under one seed); the counter is optional, read at run time, and advanced by one
 * behind the draw when advance != 0, as in xvit_augment_draw.  Sample b uses i = 16384 b + k: k = 0 the decision (u < prob); the control
 * point (component a, gz, gy, gx) uses k = 16 + ((a Gz + gz) Gy + gy) Gx + gx (< 16384 for G <= 16).  A free control point is
 * fminf(fmaxf(fmaf(u, 2 m, -m), -m), m), m = max_displacement[a]; a locked one (an index < L or >= G - L along any axis, L =
 * locked_borders) is 0: with L = 2 the displacement and its first derivative vanish at the volume faces (TorchIO's default).  A sample
 * whose decision is false gets an all-zero field and flag 0.  config is a HOST struct, read during the call.
 *
 * xvit_augment_apply_elastic.  A pure function of (src, params, field, erec) with the dtypes, layouts and refusals of xvit_augment_apply;
 * nvol is a multiple of M and volume v takes the field and record of sample v / M.  A sample whose flag is 0 is processed exactly as
 * xvit_augment_apply processes it (exact path included) and its field is NOT read; a sample whose flag is 1 takes the general path even
 * when its record carries XVIT_AUG_FLAG_EXACT.  Brick layout and order of xvit_augment_apply; no atomics: bit-reproducible.
 * ---------------------------------------------------------------------------------------- */
#define XVIT_ELASTIC_MAX_GRID 16
#define XVIT_ELASTIC_NREC 8
enum { XVIT_ELASTIC_FLAG = 0, XVIT_ELASTIC_U = 1, XVIT_ELASTIC_MAX_ABS = 2 };
typedef struct xvit_elastic_config {
  float prob;                                  /* of deforming a sample */
  float max_displacement[3];                   /* destination voxels, z, y, x: finite, >= 0 */
  int locked_borders;                          /* 0..3 outer control layers held at zero */
} xvit_elastic_config;
int xvit_elastic_draw(const xvit_elastic_config* config, float* field, float* erec, int B, int Gz, int Gy, int Gx, uint64_t seed, uint64_t* counter,
                      int advance, xvit_stream_t stream);
int xvit_augment_apply_elastic(const void* src, int src_dtype, void* dst, int dst_dtype, const float* params, const float* field, const float* erec, int nvol,
                               int M, int Gz, int Gy, int Gx, int Ds, int Hs, int Ws, int D, int H, int W, float pad_value, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-volume intensity statistics and normalisation (stands where a loader runs MONAI's NormalizeIntensity(nonzero=True) or
 * ScaleIntensityRangePercentiles on the CPU: MRI intensities carry no unit, so every volume is normalised by its own statistics).  The
 * rule is this project's own; parity with MONAI's numerics is NOT claimed.
 *
 * A 16-bit source has at most 65 536 distinct values, so a per-volume histogram holds everything needed, exactly, and integer atomics make
 * it independent of the execution order: the result is bit-reproducible with no switch.  Sources: int16, keyed by v + 32768; bf16, keyed
 * by a monotone key of the bit pattern (all bits of negative patterns flipped, the sign bit of the others set), so that key order is value
 * order (-0.0 sorts directly below +0.0).  fp32 sources are refused: there is no 2^32-bin path.
 *
 * Definitions, per volume and over the whole source volume (src [nvol, nvox], contiguous), not the crop:
 *    Foreground  F = { v : v > foreground_above }.  NaN compares false and is never foreground.  n = |F|.
 *    With percentiles (q_lo, q_hi), 0 <= q_lo <= q_hi <= 1:  k = max(1, ceil(q n)), computed in double from the fp32 q (nearest rank);
 *    lo is the k_lo-th smallest value of F and hi the k_hi-th smallest.  Without percentiles (q_lo < 0): lo = min F, hi = max F.
 *    W = { v in F : lo <= v <= hi },  n_w = |W|.
 *    mu is the mean of W;  sigma = sqrt(mean((v - mu)^2)) over W, the population standard deviation.
 * sigma is taken in two passes over the HISTOGRAM: mu first, then sum h (v - mu)^2 in double (no sum v^2 - (sum v)^2 / n cancellation).
 * For int16, sum h v is an exact int64 sum and mu = (double)S / n_w is rounded once; for bf16 the sum is a double sum in a fixed order.
 *
 * stats [nvol, XVIT_STATS_NSTAT] (fp64, 8-byte aligned):  n, n_w, mu, sigma, lo, hi, min F, max F.   n = 0 gives a record of zeros.
 *
 * Folding (params != NULL and mode != XVIT_NORM_STATS_ONLY): params is the table of xvit_augment_draw, [nvol, XVIT_AUG_NPARAM].  With
 * (a, b) the record's slots 12 / 13 as the draw wrote them,
 *    XVIT_NORM_ZSCORE:  a_n = 1 / sigma', b_n = -mu / sigma',  sigma' = sigma if sigma > 0, else 1;
 *    XVIT_NORM_WINDOW:  r = hi - lo if positive, else 1;  a_n = 1 / r, b_n = -lo / r;
 *    n = 0:  a_n = 1, b_n = 0, no clamp (the record is left as it is);
 *    SCALE <- fl32(a a_n),  SHIFT <- fl32(a b_n + b), both computed in double: the normalisation comes first and the drawn scale / shift
 *    act on normalised values.  With clip != 0: slot 29 <- lo, slot 30 <- hi (exact in fp32 for either source type) and
 *    FLAGS |= XVIT_AUG_FLAG_CLAMP, so that xvit_augment_apply clamps the resampled source-unit value to [lo, hi] before a v + b (padding
 *    included: the background lands on the window floor).  No other slot is written.
 *
 * Two launches.  (a) The histogram counts foreground voxels only (the background bin would otherwise take more than half of a brain
 * volume's voxels in one address), in 32-bit counters: keys in [XVIT_STATS_WINDOW_LO, XVIT_STATS_WINDOW_LO + XVIT_STATS_WINDOW_BINS), the
 * non-negative half of either key space, are counted in LDS and flushed with global integer atomics, the others go straight to global
 * memory.  The window is a performance choice; no result depends on it.  16-byte loads with a scalar head and tail per workgroup (a volume's
 * base is only 2-byte aligned when nvox is odd).  (b) One workgroup per volume scans its 65 536 bins: prefix counts -> lo, hi, n_w, mu, then
 * sigma; it writes the record, folds, and leaves the histogram zeroed.  The workspace (xvit_volume_stats_workspace_bytes(nvol), 16-byte
 * aligned, caller-owned) must therefore be zero-filled ONCE by the caller and is zero again after every call: no memset, and the pair can
 * be captured in a graph.  One workspace serves one stream at a time.
 * Argument errors, raised before any launch: null pointers, an fp32 or unknown source dtype, nvol <= 0, nvox <= 0 or >= 2^31, an unknown
 * mode, a NaN foreground_above, percentiles out of order or above 1, misaligned stats / params / workspace, a workspace that is too small.
 * cfg is a HOST struct, read during the call.
 * ---------------------------------------------------------------------------------------- */
#define XVIT_STATS_NSTAT 8
enum { XVIT_STATS_WINDOW_LO = 32768, XVIT_STATS_WINDOW_BINS = 32768 };
enum { XVIT_NORM_STATS_ONLY = 0, XVIT_NORM_ZSCORE = 1, XVIT_NORM_WINDOW = 2 };
typedef struct xvit_norm_config {
  int mode;                /* 0 stats only, 1 zscore, 2 window */
  int clip;                /* != 0: write the clamp window and set XVIT_AUG_FLAG_CLAMP */
  float foreground_above;  /* F = { v > foreground_above }; -inf: every voxel that is not NaN */
  float q_lo, q_hi;        /* q_lo < 0: no percentiles */
} xvit_norm_config;
int64_t xvit_volume_stats_workspace_bytes(int nvol);
int xvit_volume_stats(const void* src, int src_dtype, int nvol, int64_t nvox, const xvit_norm_config* cfg, double* stats, float* params /* NULL: no fold */,
                      void* workspace, int64_t workspace_bytes, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Foreground bounding box and crop (csrc/volume_bbox.hip; stands where a loader runs MONAI's CropForegroundd followed by a resize or
 * ResizeWithPadOrCropd on the CPU).  xvit_augment_draw windows the source around the centre of the VOLUME; this moves the window to the
 * foreground.  It is not a second resample: the box is folded into the record's A | t between the draw and the apply, as
 * xvit_volume_stats folds the normalisation into SCALE / SHIFT, and the voxels are still interpolated once.  The rule is this project's
 * own; parity with MONAI's numerics is NOT claimed.
 *
 * Boxes.  src [nvol, Ds, Hs, Ws] int16 / bf16 / fp32 (only a comparison is needed, so fp32 is supported here), contiguous, aligned to its
 * element size; a volume has fewer than 2^31 voxels.  F = { (z, y, x) : src[v, z, y, x] > foreground_above }; NaN compares false and is
 * never foreground, -0.0 is not above 0.  boxes [nvol, XVIT_BBOX_NREC] (int32): slots 0..5 the inclusive index range of F along z, y, x
 * (XVIT_BBOX_Z0 .. XVIT_BBOX_X1), slot 6 |F|, slot 7 zero.  A volume without foreground gets lo = size, hi = -1, count 0.  This box
 * follows every voxel of F: one isolated bright background voxel widens it to itself ("Connected foreground components" filters that).
 *
 * Sample crop.  The M modalities of a sample (volumes b M .. b M + M - 1; nvol is a multiple of M) are co-registered and share one
 * spatial transform, so they share one box.  crop [nvol / M, XVIT_BBOX_NREC] (int32): the union of the sample's non-empty volume boxes,
 * widened by margin[axis] on both sides, then clipped to [0, size - 1]; slot 6 is 1 when the sample has any foreground, else 0; slot 7
 * zero.  For a sample without foreground the six box slots are 0, size - 1 per axis and nothing is folded into its records.
 *
 * Fold (params != NULL, mode != XVIT_CROP_BOXES_ONLY, the sample has foreground), into each of the sample's M records of params
 * [nvol, XVIT_AUG_NPARAM], in double from the fp32 slots, every written slot rounded once.  Per axis i with [lo, hi] of crop:
 * s = hi - lo + 1, n the destination size, o the draw's offset (that of xvit_resize_pad_crop_i16 for (source size, n)), c = (n - 1) / 2.
 *    k = 1 for XVIT_CROP_CENTER;  XVIT_CROP_FIT: k = max_i (s_i / n_i), raised to 1 unless allow_upscale.  kf = fl32(k) is what is
 *    applied, and what slot XVIT_AUG_CROP_SCALE receives.
 *    kf == 1:  o'_i = lo_i + offset(s_i, n_i), the centre pad / crop rule applied to the box instead of the volume;
 *              t_i <- fl32(t_i + (o'_i - o_i)).  A and FLAGS are untouched: an exact record stays exact and the apply is still the copy.
 *    kf != 1:  cb_i = (lo_i + hi_i) / 2;  A_ij <- fl32(kf A_ij) (the product of two fp32 values is exact in double: one rounding);
 *              t_i <- fl32(kf (t_i - c_i - o_i) + cb_i);  FLAGS &= ~XVIT_AUG_FLAG_EXACT.  The destination centre lands on the box centre
 *              plus kf times the drawn translation; rotation, zoom and the elastic displacement (p = A (q + u) + t with the new A, t) stay
 *              in destination voxels.
 * No other slot is written.  The statistics fold (slots 12, 13, 16, 29, 30) and this one commute; both read-modify-write slot 16, in
 * stream order.  The box moves the window; it masks nothing: voxels outside the box but inside the volume are the source's own, and
 * pad_value appears only outside the VOLUME.
 *
 * Two launches, no host read-back, no atomics, no pre-initialised workspace: the pair can be captured in a graph.  (a) A 256-thread
 * workgroup owns `chunk` consecutive voxels of one volume, read with 16-byte loads (scalar head and tail: a volume's base is only
 * element-aligned when nvox is odd; rows are not aligned, (z, y, x) comes from the flat index, by two divisions per 16-byte run that
 * holds foreground), and writes one 8-int partial box with plain stores.  Chunk rule, with nvox = Ds Hs Ws:
 *    parts = min(max(1, 2048 / nvol), ceil(nvox / 8192));  chunk = ceil(nvox / parts) rounded up to a multiple of 8;
 *    parts = ceil(nvox / chunk);  part j of a volume owns the flat voxel indices [j chunk, min(nvox, (j + 1) chunk)).
 * xvit_volume_bbox_workspace_bytes(nvol, nvox) = nvol parts 32 (16-byte aligned, caller-owned, contents irrelevant on entry).
 * (b) One workgroup per sample reduces its M x parts partials, writes boxes and crop, and thread m folds record m.  Every result is an
 * integer or computed by one thread in a fixed order: the pair is bit-reproducible.
 * Argument errors, raised before any launch: null pointers (params may be NULL; boxes and crop may not), an unknown dtype or mode,
 * nvol <= 0, M <= 0 or nvol not a multiple of M, non-positive sizes or nvox >= 2^31, a negative margin, a NaN foreground_above, boxes /
 * crop / params / workspace not 16-byte aligned, a workspace that is too small.  cfg is a HOST struct, read during the call.
 * ---------------------------------------------------------------------------------------- */
#define XVIT_BBOX_NREC 8
enum { XVIT_BBOX_Z0 = 0, XVIT_BBOX_Z1 = 1, XVIT_BBOX_Y0 = 2, XVIT_BBOX_Y1 = 3, XVIT_BBOX_X0 = 4, XVIT_BBOX_X1 = 5, XVIT_BBOX_COUNT = 6 };
enum { XVIT_CROP_BOXES_ONLY = 0, XVIT_CROP_CENTER = 1, XVIT_CROP_FIT = 2 };
#define XVIT_AUG_CROP_SCALE 31          /* slot 31 of an augment record: the crop scale k that was folded, 0 = no crop folded */
typedef struct xvit_crop_config {
  int mode;                 /* 0 boxes only, 1 center, 2 fit */
  int margin[3];            /* voxels added on both sides, z, y, x; >= 0 */
  int allow_upscale;        /* fit: k may fall below 1 */
  float foreground_above;   /* F = { v > foreground_above }; NaN is never foreground */
} xvit_crop_config;
int64_t xvit_volume_bbox_workspace_bytes(int nvol, int64_t nvox);
int xvit_volume_bbox(const void* src, int src_dtype, int nvol, int M, int Ds, int Hs, int Ws, int D, int H, int W, const xvit_crop_config* cfg,
                     int32_t* boxes /* [nvol, 8] */, int32_t* crop /* [nvol / M, 8] */, float* params /* [nvol, 32]; NULL: no fold */, void* workspace,
                     int64_t workspace_bytes, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Connected foreground components (csrc/volume_components.hip; stands where a loader runs MONAI's KeepLargestConnectedComponent or
 * RemoveSmallObjects in front of CropForegroundd).  The box of xvit_volume_bbox follows every voxel above the threshold; this takes the
 * box over the voxels of the kept connected components only, so that a speck of noise, a residue of skull-stripping or a fiducial marker
 * no longer widens it.  It changes where the window goes and masks nothing: a dropped component that falls inside the window stays in
 * the image.  The rule is this project's own; parity with MONAI's numerics is NOT claimed.
 *
 * Foreground.  The predicate of xvit_volume_bbox: F = { (z, y, x) : src[v, z, y, x] > foreground_above }, strict; NaN is never
 * foreground; -0.0 is not above 0.  src [nvol, Ds, Hs, Ws] int16 / bf16 / fp32, contiguous, aligned to its element size, nvox = Ds Hs Ws
 * < 2^31.
 *
 * Labels.  labels [nvol, nvox] (int32).  A foreground voxel holds the smallest flat index (z Hs + y) Ws + x of its component; a
 * background voxel holds -1.  Two foreground voxels are neighbours when they differ by at most one along every axis and, for
 * connectivity 6, along exactly one axis (faces); for connectivity 26 along one, two or three (faces, edges, corners).  18 is refused.
 * The smallest index of a component does not depend on the execution order: the labels are bit-reproducible.
 *
 * Kept set, per volume.  The size of a component is its number of voxels, an exact integer.
 *    XVIT_CC_LARGEST      keeps the component of greatest size; a tie goes to the smaller root index.
 *    XVIT_CC_MIN_VOXELS   keeps every component with at least min_voxels voxels; if none qualifies it keeps the largest (as above), so a
 *                         volume with foreground never becomes empty.
 * comps [nvol, XVIT_CC_NREC] (int32): slot 0 the number of components, 1 the largest component's root (-1 without foreground), 2 its
 * size, 3 the number of kept components, 4 the number of kept voxels, 5 the status (0 = fine; any other value is a defect of the
 * kernels: a union-find loop reached its step cap, bit 0 in a tile, bit 1 in the merge, bit 2 in the flatten, and the other outputs are
 * not to be used), 6 and 7 zero.
 *
 * Boxes (xvit_volume_bbox_components).  boxes [nvol, XVIT_BBOX_NREC] in xvit_volume_bbox's layout, over the kept voxels only; slot 6 is
 * the kept-voxel count; a volume without foreground gets lo = size, hi = -1, count 0.  The per-sample union, margin, clip, crop and the
 * fold into params are those of xvit_volume_bbox, by the same kernel.  cfg->foreground_above must equal comp->foreground_above.
 *
 * Launches: zero, tile (an 8 x 8 x 32 tile labelled by union-find in LDS, 16-byte source loads where a run lies inside its row and is
 * aligned), merge (voxels on tile faces, device-scope atomicMin on the labels), flatten, count (sizes aggregated per wave and workgroup
 * before one global add per (workgroup, root)), pick (64-bit atomicMax of (size << 32) | (0x7fffffff - root) per workgroup), table;
 * xvit_volume_bbox_components adds the partial boxes over the labels and xvit_volume_bbox's finish.  A fixed number of launches, no host
 * read-back, no host loop, no spinning; every device loop has a step cap that reports through the status.  The workspace is zeroed
 * inside the call, so the sequence can be captured in a graph and replayed.
 * Memory: labels cost 4 bytes per source voxel (571 MB at 16 volumes of 240 x 240 x 155).  xvit_volume_components_workspace_bytes(nvol,
 * nvox) = 32 nvol + (4 nvol nvox rounded up to 16) + xvit_volume_bbox_workspace_bytes(nvol, nvox): the accumulators, one int32 size per
 * voxel (as much again as the labels) and the partial boxes; 16-byte aligned, caller-owned, contents irrelevant on entry.
 * Argument errors, raised before any launch: null pointers (params may be NULL), an unknown dtype, connectivity other than 6 or 26, an
 * unknown keep mode, min_voxels < 1 (in either mode), non-positive sizes or nvox >= 2^31, a NaN foreground_above, labels / comps / boxes /
 * crop / params / workspace not 16-byte aligned, a workspace that is too small, and for xvit_volume_bbox_components what xvit_volume_bbox
 * refuses.  Both configs are HOST structs, read during the call.
 * ---------------------------------------------------------------------------------------- */
#define XVIT_CC_NREC 8
enum { XVIT_CC_COUNT = 0, XVIT_CC_LARGEST_ROOT = 1, XVIT_CC_LARGEST_SIZE = 2, XVIT_CC_KEPT = 3, XVIT_CC_KEPT_VOXELS = 4, XVIT_CC_STATUS = 5 };
enum { XVIT_CC_LARGEST = 0, XVIT_CC_MIN_VOXELS = 1 };
typedef struct xvit_component_config {
  int connectivity;         /* 6 or 26 */
  int keep;                 /* XVIT_CC_LARGEST or XVIT_CC_MIN_VOXELS */
  int min_voxels;           /* >= 1; read by XVIT_CC_MIN_VOXELS */
  float foreground_above;   /* F = { v > foreground_above }; NaN is never foreground */
} xvit_component_config;
int64_t xvit_volume_components_workspace_bytes(int nvol, int64_t nvox);
int xvit_volume_components(const void* src, int src_dtype, int nvol, int Ds, int Hs, int Ws, const xvit_component_config* cfg, int32_t* labels /* [nvol, nvox] */,
                           int32_t* comps /* [nvol, 8] */, void* workspace, int64_t workspace_bytes, xvit_stream_t stream);
int xvit_volume_bbox_components(const void* src, int src_dtype, int nvol, int M, int Ds, int Hs, int Ws, int D, int H, int W, const xvit_crop_config* cfg,
                                const xvit_component_config* comp, int32_t* boxes /* [nvol, 8] */, int32_t* crop /* [nvol / M, 8] */,
                                float* params /* [nvol, 32]; NULL: no fold */, int32_t* labels /* [nvol, nvox] */, int32_t* comps /* [nvol, 8] */, void* workspace,
                                int64_t workspace_bytes, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Contrast augmentations (csrc/contrast.hip): Gaussian blur, a smooth multiplicative bias field and gamma, as a second, independent
 * stage behind the augmenting input stage (what MONAI RandGaussianSmooth / RandBiasField / RandAdjustContrast, nnU-Net's blur + gamma and
 * TorchIO's RandomBlur / RandomBiasField / RandomGamma do in kind).  The transform set and its ranges are this project's own; parity
 * with the random streams of MONAI or TorchIO is NOT claimed.  Two kernels with a table between them, like the stage in front:
 * xvit_contrast_draw turns (config, seed) into params[nvol, XVIT_CON_NPARAM] (fp32, one record per volume, i.e. per (sample, modality));
 * xvit_contrast_apply is a pure, out-of-place function of (src, params) that reads every volume once and writes it once.
 *
 * Record (fp32 slots):
 *    0      flags (integer-valued): bit 0 blur, bit 1 bias, bit 2 gamma       1..3   sigma in voxels along z, y, x (0: axis not blurred)
 *    4..6   radius along z, y, x = min(ceil(3 sigma), 6), integral (0 where sigma is 0)
 *    7      gamma g = (float)exp((double)beta) (1 when not drawn)              8, 9   gamma window lo, hi
 *    10..18 bias coefficients of the monomials z, y, x, z^2, y^2, x^2, zy, zx, yx, in this order (0 when not drawn)
 *    19..21 the uniform draws behind the blur, bias and gamma decisions        22     beta = log gamma as drawn (0 when not drawn)
 *    23..31 zero
 * xvit_contrast_apply reads slots 0..18 only.
 *
 * xvit_contrast_draw.  Uniform numbers are u(i) = (hash32(seed', i) & 0xFFFFFF) / 2^24 with the dropout hash, where
 * seed' = (seed + *counter * 0xD1B54A32D192ED03) ^ 0x434F4E5452415354 (the counter as in xvit_augment_draw: optional, read at run time,
 * advance != 0: one thread stores counter + 1 after every thread has read it; the xor keeps this stream apart from xvit_augment_draw's
 * when both stages are given one seed).  Volume v uses i = 64 v + k, and a value "uniform in [lo, hi]" is
 * fminf(fmaxf(fmaf(u, hi - lo, lo), lo), hi) in fp32:
 *    k = 0        blur?  (u < blur_prob)        1, 2, 3   sigma along z, y, x, uniform in blur_sigma_range (blur_isotropic: draw 1 on all axes)
 *    k = 4        bias?  (u < bias_prob)        5 .. 13   the nine coefficients in record order, each uniform in [-bias_coeff, bias_coeff]
 *    k = 14       gamma? (u < gamma_prob)       15        beta, uniform in log_gamma_range
 * Draws behind a decision that came out false are not taken (their slots stay 0, gamma 1).  The window is copied from the config into
 * every record.  config is a HOST struct, read during the call.  params 16-byte, counter 8-byte aligned.  Refused before the launch:
 * null pointers, nvol <= 0, a probability outside [0, 1], blur_sigma_range with lo <= 0, lo > hi or hi > 2.0 (the radius cap),
 * bias_coeff < 0 or not finite, a reversed or non-finite log_gamma_range, a gamma_window with hi <= lo or not finite.
 *
 * xvit_contrast_apply.  src, dst [nvol, D, H, W] contiguous, bf16 or fp32 each (all four combinations), fewer than 2^31 voxels per volume,
 * src != dst.  Per voxel, in fp32, with ONE rounding at the end:
 *  1. Blur, only with flag bit 0: separable, along x, then y, then z.  Along an axis with radius R and sigma s the weights are
 *     w_k = exp(-k^2 / (2 s^2)) for |k| <= R, divided by their sum; a tap outside the volume takes the nearest edge voxel (index clamp), so
 *     a constant volume stays constant and every D, H, W >= 1 is legal, sizes below R included.  An axis with R = 0 (or a sigma that is
 *     not positive) is skipped.  The kernel clamps every record's radius into [0, XVIT_CON_MAX_RADIUS] before use: no table content makes
 *     it read outside its own volume.
 *  2. Bias, only with flag bit 1: v *= exp(c . m(u)) with u_axis = 2 i / (n - 1) - 1 (0 when n = 1) for index i of an axis of length n,
 *     m(u) the nine monomials above and c slots 10..18.
 *  3. Gamma, only with flag bit 2: t = (v - lo) / (hi - lo); if 0 <= t <= 1 then v = lo + (hi - lo) t^g, otherwise v is unchanged: the
 *     map is continuous and monotone and a NaN passes through.  Gamma and bias are meant for window-normalised volumes (the default
 *     window is [0, 1]).
 *  4. One rounding to the destination dtype (nearest even).
 * A record with flags 0 is a copy, bit for bit (bf16 -> fp32: the exact widening; fp32 -> bf16: one rounding).  A 256-thread workgroup
 * owns a 64 x 16 (x, y) tile of a blur record and marches along z: each source plane goes through LDS once (blurred along x, then y) into
 * a ring of 2 R_z + 1 planes from which the z-sum, bias, gamma and the store are taken; long columns of a small grid are cut into
 * z-segments that re-read 2 R_z planes each.  Records without blur take a pointwise path over the flat volume, 16 bytes per lane; the
 * branch is per volume.  No atomics and no dependence on execution order: two runs are bit-identical.
 * Refused before the launch: null pointers, unknown dtype codes, nvol, D, H or W <= 0, 2^31 voxels or more per volume, src, dst or params
 * not 16-byte aligned, src == dst.
 * ---------------------------------------------------------------------------------------- */
#define XVIT_CON_NPARAM 32
#define XVIT_CON_MAX_RADIUS 6
enum { XVIT_CON_FLAGS = 0, XVIT_CON_SIGMA = 1, XVIT_CON_RADIUS = 4, XVIT_CON_GAMMA = 7, XVIT_CON_WINDOW_LO = 8, XVIT_CON_WINDOW_HI = 9, XVIT_CON_BIAS = 10,
       XVIT_CON_U_BLUR = 19, XVIT_CON_U_BIAS = 20, XVIT_CON_U_GAMMA = 21, XVIT_CON_BETA = 22 };
enum { XVIT_CON_FLAG_BLUR = 1, XVIT_CON_FLAG_BIAS = 2, XVIT_CON_FLAG_GAMMA = 4 };
typedef struct xvit_contrast_config {
  float blur_prob, blur_sigma_range[2];        /* sigma in voxels, 0 < lo <= hi <= 2.0 */
  int blur_isotropic;                          /* != 0: one sigma for the three axes */
  float bias_prob, bias_coeff;                 /* nine coefficients, each uniform in [-bias_coeff, bias_coeff] */
  float gamma_prob, log_gamma_range[2];        /* g = exp(beta), beta uniform in the range */
  float gamma_window[2];                       /* lo < hi: the curve acts inside the window only */
} xvit_contrast_config;
int xvit_contrast_draw(const xvit_contrast_config* config, float* params, int nvol, uint64_t seed, uint64_t* counter, int advance, xvit_stream_t stream);
int xvit_contrast_apply(const void* src, void* dst, int src_dtype, int dst_dtype, const float* params, int nvol, int D, int H, int W, xvit_stream_t stream);

/* x[m, b, 0, :] = cls + pos[0]  (model_cross.py:195-197, the CLS row); x fp32 [M*B, N, d] */
int xvit_cls_row_fwd(const float* cls, const float* pos, float* x, int MB, int N, int d, xvit_stream_t stream);
/* dpos[n,:] += sum_{mb} dx[mb,n,:];  dcls += sum_{mb} dx[mb,0,:] */
int xvit_embed_bwd(const float* dx, float* dpos, float* dcls, int MB, int N, int d, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Patch dropout (csrc/token_select.hip): in training, every sequence keeps a random subset of K of its P patch tokens, plus CLS.
 * S = M * B sequences, sequence s = m * B + b; a patch index is the token t of xvit_patchify, (h * Wn + w) * Dn + d.
 *
 * xvit_token_select_draw: patch p of sequence s gets the key hash32(seed', u * P + p), where seed' is the seed mixed with the dropout epoch
 * (xvit_set_dropout_epoch, read at run time: a captured step draws a new subset at every replay) and u = s, or s mod B with `shared` so
 * that every modality of a sample keeps the same patches.  Kept are the K patches with the smallest (key, p): equal 32-bit keys go to the
 * smaller p.  keep_idx [S, K]: the kept patch indices in ascending order; slot [S, P]: the position 0 .. K - 1 of a kept patch in
 * keep_idx, -1 for a dropped one.  One workgroup per sequence with the keys in LDS, hence P <= XVIT_TOKEN_SELECT_MAX_P; K < 1, K > P and
 * a longer P are refused.  No host read-back.
 *
 * xvit_patchify_select: out [M, B * (K + 1), dp*hp*wp] bf16, the rows of the zero-padded patch matrix of xvit_patchify (one zero row in
 * front of every sequence) that keep_idx names: row 0 of a sequence is zero, row 1 + j is patch keep_idx[s][j].  Only kept voxels are
 * read; img [B, M, 1, D, H, W] fp32 or bf16, converted as by xvit_patchify.  8 voxels per thread where wp % 8 == 0 and img and out are
 * 16-byte aligned; any other patch width or alignment takes the one-voxel-per-thread kernel (same result, slower).
 *
 * xvit_embed_select_fwd: x fp32 [S * (K + 1), d] holds patches W^T + b;  x[s, 1 + j, :] += pos[1 + keep_idx[s][j], :] and
 * x[s, 0, :] = cls + pos[0, :].  pos is the full [P + 1, d] table.  d % 4 == 0.
 *
 * xvit_embed_select_bwd: for every pos row 1 + p, acc = 0, then acc += dx[s, 1 + slot[s][p], :] for s = 0 .. S - 1 in this order wherever
 * slot[s][p] >= 0, then dpos[1 + p, :] += acc (a row no sequence kept is left alone); dpos[0, :] and dcls both += the sum of the CLS rows
 * dx[s, 0, :] in the same order.  No atomics: bit-reproducible.  dx fp32 [S * (K + 1), d], dpos [P + 1, d], dcls [d]; d % 4 == 0. */
#define XVIT_TOKEN_SELECT_MAX_P 8192
int xvit_token_select_draw(int32_t* keep_idx, int32_t* slot, int S, int B, int P, int K, int shared, uint64_t seed, xvit_stream_t stream);
int xvit_patchify_select(const void* img, int img_dtype, void* out_bf16, const int32_t* keep_idx, int B, int M, int D, int H, int W, int dp, int hp, int wp,
                         int K, xvit_stream_t stream);
int xvit_embed_select_fwd(float* x, const float* cls, const float* pos, const int32_t* keep_idx, int S, int K, int d, xvit_stream_t stream);
int xvit_embed_select_bwd(const float* dx, const int32_t* slot, float* dpos, float* dcls, int S, int P, int K, int d, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Foreground-ranked token selection (csrc/token_occupancy.hip, csrc/token_select.hip): the draw of patch dropout ranked by how much
 * foreground a patch holds, so that tissue is kept before air; without randomness it also serves eval().  Integer work throughout: the
 * results are the same bits at every run.  Nothing is read back to the host.
 *
 * xvit_patch_occupancy: img [B, M, 1, D, H, W] contiguous, bf16 or fp32 -> occ int32 [M * B, P]: occ[s, t] is the number of voxels of
 * patch t of sequence s = m * B + b whose fp32 value v satisfies v > above.  The compare is strict and is xvit_volume_bbox's
 * foreground_above rule: NaN is never counted, +inf is, -0.0 > 0.0 is false.  Patch order as above, t = (h * Wn + w) * Dn + d.  One pass
 * in memory order, every voxel read once: 16 bytes per lane where wp % 8 == 0 and img is 16-byte aligned (xvit_patchify_select's
 * switch), else one voxel per lane, with the same integers.  No global atomics and no workspace; every element of occ is written exactly
 * once.  Refused: null pointers, an unknown dtype, sizes that the patch does not divide, a non-finite `above`, and P, dp*hp*wp or M * B
 * at or beyond 2^31.
 *
 * xvit_token_select_ranked: occ int32 [S, P] -> keep_idx [S, K] and slot [S, P] as xvit_token_select_draw writes them.  The count of
 * patch p of sequence s is c[p] = occ[s, p]; with `shared` (S = M * B) it is the sum of occ[m * B + b, p] over the M = S / B modalities
 * of sample b = s mod B, saturated at 2^32 - 1, so that all modalities of a sample get the same result.  A patch is foreground when
 * c[p] >= min_count; n_fg [S] (NULL: not wanted) receives the number of foreground patches of every sequence.
 *   XVIT_TOKEN_RANK_RANDOM  keeps the K smallest of (not foreground, hash32(seed', u * P + p), p), with the hash, seed' and u of
 *                           xvit_token_select_draw: foreground patches first, and inside each class the order of that draw.  Where all
 *                           patches of a sequence fall in one class the result is xvit_token_select_draw's, bit for bit.
 *   XVIT_TOKEN_RANK_TOP     keeps the K smallest of (-c[p], p): the most occupied patches, ties to the smaller index.  Reads neither the
 *                           seed nor the dropout epoch.
 * Refused: what xvit_token_select_draw refuses, a null occ, an unknown mode, min_count < 0, and `shared` with S not a multiple of B. */
#define XVIT_TOKEN_RANK_RANDOM 0
#define XVIT_TOKEN_RANK_TOP    1
int xvit_patch_occupancy(const void* img, int img_dtype, int32_t* occ, int B, int M, int D, int H, int W, int dp, int hp, int wp, float above,
                         xvit_stream_t stream);
int xvit_token_select_ranked(const int32_t* occ, int32_t* keep_idx, int32_t* slot, int32_t* n_fg /* NULL: not wanted */, int S, int B, int P, int K, int shared,
                             int mode, int min_count, uint64_t seed, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Masked-volume pretraining (csrc/mae.hip; MAE, He et al. 2022) on top of patch dropout: the encoder runs on the K kept patches of every
 * sequence, a decoder on the full grid with a mask token in the P - K = Rm dropped places, and the prediction of the dropped patches is
 * scored against the volume.  S = M * B sequences, s = m * B + b, patch indices as above.  No entry point uses atomics; every sum has the
 * one order written here, so results are the same bits at every run.  Nothing is read back to the host.
 *
 * xvit_token_select_complement: from slot [S, P] (xvit_token_select_draw) -> drop_idx int32 [S, Rm], the dropped patch indices of every
 * sequence in ascending order, and mslot int32 [S, P], the position of a dropped patch inside drop_idx, -1 for a kept one.  One workgroup
 * per sequence (ballot prefix per wave, wave totals through LDS), P <= XVIT_TOKEN_SELECT_MAX_P, 1 <= K < P.  A slot row that does not have
 * exactly K kept entries is the caller's error; nothing outside drop_idx and mslot is written then: with more dropped entries than Rm the
 * first Rm (ascending) are listed and the others read -1 (kept) in mslot, with fewer the tail of drop_idx is -1.  The kernels below read a
 * row index outside its range as "no row" (zeros, or the mask token), never out of bounds.
 *
 * xvit_mae_unshuffle_fwd: xe fp32 [S, K + 1, dd] (CLS row first, then the kept tokens in keep_idx order), mask_token [dd], dpos [P + 1, dd],
 * dmod [M, dd] -> y fp32 [S, P + 1, dd]:
 *     y[s, 0]     = (xe[s, 0] + dpos[0]) + dmod[m]
 *     y[s, 1 + p] = ((slot[s][p] >= 0 ? xe[s, 1 + slot[s][p]] : mask_token) + dpos[1 + p]) + dmod[m]
 * with exactly this association: two fp32 additions per element.  16-byte accesses: dd % 4 == 0, 16-byte aligned pointers.
 *
 * xvit_mae_unshuffle_bwd: from dy fp32 [S, P + 1, dd]
 *     dxe [S, K + 1, dd]      dxe[s, 0] = dy[s, 0], dxe[s, 1 + j] = dy[s, 1 + keep_idx[s][j]]: every row written exactly once
 *     ddpos_m [M, P + 1, dd]  ddpos_m[m, n] = dy[(m, 0), n] + dy[(m, 1), n] + ... (b ascending, from 0)
 *     dmask_part [S, dd]      dmask_part[s] = the sum of dy[s, 1 + p] over the dropped p, ascending, from 0   (caller-owned scratch)
 *     dmask_token [dd]        dmask_part[0] + dmask_part[1] + ... (s ascending, from 0): s ascending, inside a sequence p ascending
 * One thread per (row, 4 features) walks its sequences in order.  The host finishes ddpos = sum over m ascending of ddpos_m[m] and
 * ddmod[m] = xvit_colsum(ddpos_m[m]).
 *
 * xvit_token_rows_gather: g[s * Rm + j, :] = x[s, 1 + drop_idx[s][j], :]; x fp32 [S, P + 1, dd], g fp32 [S * Rm, dd].
 * xvit_token_rows_scatter (its backward): dx[s, 1 + p, :] = mslot[s][p] >= 0 ? dg[s * Rm + mslot[s][p], :] : 0 and dx[s, 0, :] = 0; every
 * row of dx is written once: no memset, no accumulation.  dd % 4 == 0, 16-byte aligned pointers, 1 <= Rm < P.
 *
 * xvit_mae_loss_fwd: pred [S * Rm, pd] (bf16 | fp32), pd = dp * hp * wp; row r = s * Rm + j predicts patch drop_idx[s][j] of volume (b, m) of
 * img [B, M, 1, D, H, W] (bf16 | fp32), in the token and feature order of xvit_patchify (t = (h Wn + w) Dn + d, f = (p1 hp + p2) wp + p3).
 * The target is never stored: one workgroup per row holds the patch's voxels in LDS (pd <= XVIT_MAE_MAX_PD).  With norm_pix the target is
 * (v - mean) * rstd, mean = sum v / pd, rstd = 1 / sqrt(var + 1e-6), var = sum (v - mean)^2 / (pd - 1) (unbiased, two passes: mean first,
 * then the centred squares); without, the target is v and stats = (0, 1).  Outputs: stats fp32 [S * Rm, 2] = (mean, rstd);
 * row_loss fp32 [S * Rm] = sum_f (pred - target)^2 / pd; then one workgroup forms loss_seq [S], loss_seq[s] = (row_loss[s Rm] + ... +
 * row_loss[s Rm + Rm - 1], ascending from 0) / Rm, and loss [1] = (loss_seq[0] + ... + loss_seq[S - 1], ascending from 0) / S, the mean
 * over all S * Rm rows.  Sums inside a row: thread-strided partial sums, then the lanes and waves in a fixed order.  8 voxels per access
 * where wp % 8 == 0 and img and pred are 16-byte aligned, else one voxel per access (same switch as xvit_patchify_select).
 * A drop_idx entry outside the grid scores 0 with stats (0, 1).
 *
 * xvit_mae_loss_bwd: dpred[r, f] = g * 2 (pred[r, f] - target[r, f]) / (pd * S * Rm) in pred's dtype; g is the upstream scalar, read from
 * DEVICE memory; the target is recomputed from the volume and stats.
 * Argument errors (nothing launched): null or misaligned pointers, bad sizes or dtypes, Rm outside 1 .. P - 1, pd > XVIT_MAE_MAX_PD,
 * norm_pix with pd < 2. */
#define XVIT_MAE_MAX_PD 8192
int xvit_token_select_complement(const int32_t* slot, int32_t* drop_idx, int32_t* mslot, int S, int P, int K, xvit_stream_t stream);
int xvit_mae_unshuffle_fwd(const float* xe, const float* mask_token, const float* dpos, const float* dmod, const int32_t* slot, float* y, int S, int B, int P,
                           int K, int dd, xvit_stream_t stream);
int xvit_mae_unshuffle_bwd(const float* dy, const int32_t* keep_idx, const int32_t* slot, float* dxe, float* dmask_token, float* ddpos_m, float* dmask_part,
                           int S, int B, int P, int K, int dd, xvit_stream_t stream);
int xvit_token_rows_gather(const float* x, const int32_t* drop_idx, float* g, int S, int P, int Rm, int dd, xvit_stream_t stream);
int xvit_token_rows_scatter(const float* dg, const int32_t* mslot, float* dx, int S, int P, int Rm, int dd, xvit_stream_t stream);
int xvit_mae_loss_fwd(const void* pred, int pred_dtype, const int32_t* drop_idx, const void* img, int img_dtype, int norm_pix, float* stats, float* row_loss,
                      float* loss_seq, float* loss, int B, int M, int D, int H, int W, int dp, int hp, int wp, int Rm, xvit_stream_t stream);
int xvit_mae_loss_bwd(const void* pred, int pred_dtype, const int32_t* drop_idx, const void* img, int img_dtype, const float* stats, const float* g,
                      void* dpred, int B, int M, int D, int H, int W, int dp, int hp, int wp, int Rm, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mixup / CutMix (csrc/mix.hip; Zhang et al. 2018, Yun et al. 2019): the label regulariser of ViT fine-tuning.  Every sample b of a batch
 * is mixed with a partner sample, voxels and labels alike.  Two kernels with a table between them, as in the augmenting input stage: the
 * draw turns (config, seed) into table[B, XVIT_MIX_NPARAM] (fp32, one readable record per sample), the apply kernel and the loss are pure
 * functions of their inputs and that table.  A table may be written by hand.  The record:
 *     [XVIT_MIX_MODE]        0 none, XVIT_MIX_MODE_MIXUP (1), XVIT_MIX_MODE_CUTMIX (2)
 *     [XVIT_MIX_PARTNER]     index of the other sample, an integer stored as a float
 *     [XVIT_MIX_LAM]         weight of the sample's own label and, for mixup, of its own voxels
 *     [XVIT_MIX_OML]         1 - lam (fp32 subtraction of the stored lam)
 *     [XVIT_MIX_BOX .. + 5]  d0, d1, h0, h1, w0, w1: the half-open CutMix box, integers stored exactly as floats (read clamped to the volume)
 *     [XVIT_MIX_LAM0]        the raw Beta draw (for the reader only)
 *     [11 .. 15]             zero
 * A record is a plain copy of the sample's own volume with the sample's own label as the target, and its partner is never read, when its
 * mode is neither 1 nor 2, when its partner is not an integer in [0, B), or when lam == 1.
 *
 * xvit_mix_draw: one thread per record, in fp64, nothing read back.  seed' = the seed mixed with the dropout epoch (xvit_set_dropout_epoch,
 * read at run time: a captured step draws a new table at every replay).  Uniform i of decision block r is
 * (hash32(seed', r * XVIT_MIX_DRAW_STRIDE + i) + 0.5) / 2^32; block b decides for sample b under per_sample, block 0 for the whole batch
 * otherwise.  In a block: i = 0 mixes if u < prob; i = 1 picks CutMix if u < switch_prob (only when both alphas are positive, else the
 * positive one decides); i = 2, 3, 4 the box centre floor(u * size) along D, H, W; i = 8 + g the U^(1 / alpha) boost of gamma draw g (alpha <
 * 1: Gamma(alpha) = Gamma(alpha + 1) U^(1 / alpha)); i = 16 + 64 g + 4 k + (0, 1, 2): round k < 16 of gamma draw g, two uniforms for the
 * Box-Muller normal x = sqrt(-2 ln u) cos(2 pi u') and one for the acceptance ln u'' < x^2 / 2 + d - d v + d ln v, v = (1 + x / sqrt(9 d))^3 > 0,
 * d = alpha - 1 / 3 (Marsaglia-Tsang).  lam0 = G0 / (G0 + G1), or 0.5 if a gamma draw accepted none of its rounds.  Block B, i = 0: the shift
 * s = 1 + floor(u * (B - 1)) of the batch; partner[b] = (b + s) mod B, so nobody is paired with themself; B = 1 gives mode 0.  Mixup:
 * lam = lam0.  CutMix: extents floor(size * r), r = cbrt(1 - lam0); the box starts at centre - extent / 2 (integer division), is `extent`
 * long and is then clipped to the volume; lam = 1 - box voxels / (D H W).  One box and one lam per sample, for all its modalities.
 * Refused: null pointers, a table not 16-byte aligned, B outside 1 .. 2^24 - 1, a volume of 2^31 voxels or more, a negative or non-finite
 * alpha, a probability outside [0, 1].
 *
 * xvit_mix_apply: dst [B, M, D H W] contiguous = src mixed through the table; src element (b, m, v) at b * stride_b + m * stride_m + v
 * (strides in elements, each volume contiguous); dtype XVIT_BF16 or XVIT_F32 for both.  Mixup: fmaf(lam, own, oml * partner) in fp32,
 * rounded once to dtype.  CutMix: the partner's voxel inside the box, the own voxel outside, copied bit for bit, every voxel read from
 * exactly one of the two.  Out of place: a dst that overlaps the source range is refused.  16 bytes per lane where W and both strides
 * are multiples of 16 bytes of elements and src and dst are 16-byte aligned, else one voxel per lane (same result, slower).  No atomics.
 *
 * xvit_mean_ce_mix: xvit_mean_ce with the target lam * smooth(y_b) + oml * smooth(y_partner[b]), smooth(y) = (1 - eps) onehot(y) + eps / C,
 * lam, oml and partner read from the table on the device; a copy record (see above) has the own label's target.  Same operations in the
 * same order as xvit_mean_ce: a table whose records all have lam = 1 gives its logits, loss and dlogits_m bit for bit.  A NULL table is
 * refused.
 * ---------------------------------------------------------------------------------------- */
#define XVIT_MIX_NPARAM 16
#define XVIT_MIX_MODE 0
#define XVIT_MIX_PARTNER 1
#define XVIT_MIX_LAM 2
#define XVIT_MIX_OML 3
#define XVIT_MIX_BOX 4
#define XVIT_MIX_LAM0 10
#define XVIT_MIX_MODE_MIXUP 1
#define XVIT_MIX_MODE_CUTMIX 2
#define XVIT_MIX_DRAW_STRIDE 256
typedef struct xvit_mix_config {
  float mixup_alpha;  /* Beta(alpha, alpha) of mixup; 0: no mixup */
  float cutmix_alpha; /* Beta(alpha, alpha) of CutMix; 0: no CutMix */
  float prob;         /* a batch (a sample under per_sample) is mixed with this probability */
  float switch_prob;  /* with both alphas positive: CutMix with this probability, else mixup */
  int32_t per_sample; /* 0: one mode, lam0 and box for the batch; 1: drawn per sample */
} xvit_mix_config;
int xvit_mix_draw(const xvit_mix_config* config, float* table, int B, int D, int H, int W, uint64_t seed, xvit_stream_t stream);
int xvit_mix_apply(const void* src, void* dst, int dtype, const float* table, int B, int M, int D, int H, int W, int64_t stride_b, int64_t stride_m,
                   xvit_stream_t stream);
int xvit_mean_ce_mix(const float* logits_m, const int64_t* labels, const float* table, float label_smoothing, float* logits, float* loss, float* dlogits_m,
                     int M, int B, int C, xvit_stream_t stream);

/* ---- elementwise / reductions --------------------------------------------------------- */
int xvit_cast_f32_bf16(const float* src, void* dst_bf16, int64_t n, xvit_stream_t stream);
/* out = a + b (fp32) and its bf16 copy in one pass: the sum of a branch output's two gradients (one per reader: its own fusion and the
 * partner's, model_cross.py:140-142) handed to the block before it in both dtypes.  n % 8 == 0; out may be a or b. */
int xvit_add_cast_f32_bf16(const float* a, const float* b, float* out, void* out_bf16, int64_t n, xvit_stream_t stream);
/* dst[r, :] (and dst2[r, :], optional) = a[r, :] + b[r, :] for r < rows, d columns; a NULL operand is zero; each tensor has its own dtype
 * (XVIT_F32 / XVIT_BF16) and row stride in elements.  The CLS-row bookkeeping of the fusions — take the B CLS rows out of a [B, N, d] token
 * tensor (row stride N d), write the fused token back, add / zero / copy the same rows of the gradients (model_cross.py:140-142 and its
 * backward) — one launch per site.  dst may alias a or b. */
int xvit_rows_combine(void* dst, int dst_dtype, int64_t ld_dst, void* dst2, int dst2_dtype, int64_t ld_dst2, const void* a, int a_dtype, int64_t ld_a,
                      const void* b, int b_dtype, int64_t ld_b, int rows, int d, xvit_stream_t stream);
/* out[n] (+)= sum_r x[r, n];  x bf16 or fp32.  workspace (optional, xvit_colsum_workspace_bytes(rows, n) bytes): the row chunks'
 * partial sums are stored there and added in chunk order (bit-reproducible) instead of meeting in fp32 atomics on out. */
int xvit_colsum(const void* x, int x_dtype, int64_t ldx, float* out, int rows, int n, int accumulate, float* workspace, int64_t workspace_bytes,
                xvit_stream_t stream);
int64_t xvit_colsum_workspace_bytes(int rows, int n);
/* dropout with a counter-based mask (same (seed, element index) -> same mask in fwd and bwd):
 * y = x * keep / (1-p).  In-place allowed.  dtype XVIT_BF16 | XVIT_F32. */
int xvit_dropout(const void* x, void* y, int dtype, int64_t n, float p, uint64_t seed, xvit_stream_t stream);

/* Per-step classification statistics kept on the device (replaces log_stats -> compute_metrics, model_cross.py:243-255 /
   utils.py:18-62: six torchmetrics objects, six .item() host syncs and an AUROC per step).  logits fp32 [B, C = 2] (row stride
   ld), labels int64 [B].  pred = argmax; the step's accuracy, precision, recall, specificity, F1, NPV (0 for an empty
   denominator) and exact AUROC of softmax(logits)[:, 1] (0 if a class is absent) are folded into
   state[XVIT_METRIC_STATE] (fp64, caller-zeroed at the start of an epoch):
     [0..3] pooled tn, fp, fn, tp   [4] samples   [5] steps   [6..12] sum of batch_size * {acc, prec, rec, spec, f1, npv, auroc}
   so state[6+k] / state[4] is the batch-size-weighted epoch mean Lightning logs for on_epoch=True.  B <= 8192. */
#define XVIT_METRIC_STATE 16
int xvit_binary_metrics_step(const float* logits, int64_t ld, const int64_t* labels, int B, int C, double* state, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Pooled epoch metrics for any number of classes (csrc/epoch_metrics.hip).  The entry point above keeps batch-size-weighted means of
 * per-step values, as the reference logs them; the pair below keeps the epoch's scores on the device and yields the POOLED values a
 * paper reports (confusion-matrix metrics, one-vs-rest AUROC and average precision over the whole fold) with percentile-bootstrap
 * replicates, all from integer rank statistics.
 *
 * xvit_epoch_metrics_update: one single-workgroup launch per step, no host read, capturable (the cursor lives on the device: every
 * replay of a captured launch appends).  logits fp32 [B, C] (row stride ld >= C), labels int64 [B]; 2 <= C <= XVIT_EPOCH_MAX_C,
 * 1 <= B <= XVIT_EPOCH_MAX_B, 1 <= cap < 2^31.  Caller-owned epoch buffers: scores fp32 [cap, C], labels32 int32 [cap], preds int32 [cap],
 * state int64 [XVIT_EPOCH_STATE_HEAD + C*C] (8-byte aligned, zeroed by the caller at the start of an epoch):
 *    state[XVIT_EPOCH_STORED]     rows stored so far = the cursor        state[XVIT_EPOCH_SEEN]      rows handed in (sum of B)
 *    state[XVIT_EPOCH_STEPS]      launches                               state[XVIT_EPOCH_IGNORED]   rows whose label is outside [0, C)
 *    state[XVIT_EPOCH_NONFINITE]  rows with a NaN or infinite logit      state[XVIT_EPOCH_OVERFLOW]  kept rows that did not fit under cap
 *    state[XVIT_EPOCH_STATE_HEAD + label*C + pred]                       the confusion counts of the kept rows
 * Per row, in this order: a label outside [0, C) counts in IGNORED only; otherwise a non-finite logit counts in NONFINITE only; otherwise
 * the row is KEPT: pred = argmax (first maximum on ties), confusion[label][pred] += 1, and the row is appended at the cursor, in row
 * order, while the cursor is below cap: scores[c] = expf(l_c - max) / sum_k expf(l_k - max) with the sum taken in class order (for C = 2
 * the expression of xvit_binary_metrics_step, so saturated probabilities tie as there), labels32 = label, preds = pred.  A kept row past
 * cap counts in the confusion and in OVERFLOW and is not stored.  Integer counters and a row-order compaction: the buffers after two
 * updates equal those after one update of the concatenated batch.  All stores are plain vector stores by the one workgroup.
 *
 * xvit_epoch_rank_stats: epoch end; grid (R + 1 replicates) x (C classes), one workgroup each.  n = min(*n_dev, n_max) is read on the
 * device (n_dev: the address of state[XVIT_EPOCH_STORED] or of any int64 count); n_max, the host's bound, sizes the LDS.  perm int64
 * [C, ldp]: row c lists the samples 0 .. n - 1 in descending order of scores[:, c] (any order among equal scores: the results do not
 * depend on it; an index outside [0, n) carries no weight and is never dereferenced).
 *    Replicate 0 weighs every sample once (the point estimate).  Replicate r >= 1 draws n samples with replacement: draw k = 0 .. n - 1
 *    lands on sample (uint64(hash32(seed + r * 0x9E3779B97F4A7C15, k)) * n) >> 32, hash32 being the dropout hash of xvit_dropout; the seed
 *    sum wraps at 2^64.  The multiplicities w_r[i] are indexed by sample, so all classes of a replicate share one resample.  They are
 *    16-bit LDS counters: with R > 0, n_max <= XVIT_EPOCH_RANK_MAX_N = 65 535, which both fits the 160 KiB of LDS and keeps a counter from
 *    overflowing (a sample can be drawn at most n times); xvit_epoch_rank_stats_max_n returns the limit.  R = 0 has no limit but 2^31 - 1.
 *    Per (r, c), with "positive" = label c, over the tie groups of the sorted order (gp / gn: the group's positive / negative weight;
 *    cp / cn: cumulative down to and including the group):
 *      ranks[r, c, XVIT_EPOCH_RANK_U2]   = sum_groups gp (2 (wneg - cn) + gn)       exact;  AUROC = 0.5 u2 / (wpos wneg)
 *      ranks[r, c, XVIT_EPOCH_RANK_WPOS], [.., XVIT_EPOCH_RANK_WNEG]                 total positive / negative weight
 *      ap[r, c]   = (sum_{groups, gp > 0} (double)(gp cp) / (double)(cp + cn)) / wpos   fp64, summed in a fixed order (the same bits at
 *                   every run and for every order among equal scores); 0 when wpos = 0
 *      conf[r, c, p] = sum_i w_r[i] [label_i = c] [pred_i = p]                       the replicate's confusion row
 *    The walk takes XVIT_EPOCH_RANK_PASS sorted elements per pass.  n_max = 0 launches nothing and zeroes the outputs.
 * Argument errors, raised before any launch: null pointers, C outside 2..64, B outside 1..8192, ld < C, cap < 1 or >= 2^31, R outside 0..65534, n_max < 0 or >= 2^31,
 * n_max > XVIT_EPOCH_RANK_MAX_N with R > 0, ldp < n_max, misaligned state or outputs.
 * ---------------------------------------------------------------------------------------- */
#define XVIT_EPOCH_MAX_C 64
#define XVIT_EPOCH_MAX_B 8192
#define XVIT_EPOCH_STATE_HEAD 8
enum { XVIT_EPOCH_STORED = 0, XVIT_EPOCH_SEEN = 1, XVIT_EPOCH_STEPS = 2, XVIT_EPOCH_IGNORED = 3, XVIT_EPOCH_NONFINITE = 4, XVIT_EPOCH_OVERFLOW = 5 };
#define XVIT_EPOCH_RANK_PASS 1024
#define XVIT_EPOCH_RANK_MAX_N 65535
#define XVIT_EPOCH_RANK_NSTAT 3
enum { XVIT_EPOCH_RANK_U2 = 0, XVIT_EPOCH_RANK_WPOS = 1, XVIT_EPOCH_RANK_WNEG = 2 };
int xvit_epoch_metrics_update(const float* logits, int64_t ld, const int64_t* labels, int B, int C, float* scores, int32_t* labels32, int32_t* preds,
                              int64_t cap, int64_t* state, xvit_stream_t stream);
int64_t xvit_epoch_rank_stats_max_n(void);
int xvit_epoch_rank_stats(const float* scores, const int32_t* labels32, const int32_t* preds, const int64_t* perm, int64_t ldp, const int64_t* n_dev,
                          int64_t n_max, int C, int R, uint64_t seed, int64_t* ranks, double* ap, int64_t* conf, xvit_stream_t stream);

/* Diagnostic (no reference counterpart): out[2*b] = XCC (XCD) id and out[2*b+1] = HW_ID register of the CU
   that ran workgroup b of an `nblocks`-block launch on `stream`; every block lingers `linger_us` so the
   launch spreads over all CUs the stream may use.  Maps CU-mask bits of a masked stream to XCDs. */
int xvit_cu_trace(uint32_t* out, int nblocks, int linger_us, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused multi-tensor Adam step with torch.optim.Adam semantics (model_cross.py:276-278: L2 weight decay added to
 * the gradient, bias correction with `step`, eps outside the square root).  table_dev: device array of
 *   struct { float* p; const float* g; float* m; float* v; void* shadow_bf16 (or NULL); int64_t n; }
 * chunks_dev: device array of int32 pairs (tensor index, chunk index), one block per 16384-element chunk.
 * When shadow_bf16 is given it receives bf16(p) — the GEMM operand copy, so no cast pass follows the step.
 * grad_scale multiplies every gradient first (1 for plain training).
 * ---------------------------------------------------------------------------------------- */
#define XVIT_ADAM_CHUNK 16384
int xvit_adam_step(const void* table_dev, const void* chunks_dev, int n_chunks, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step, float grad_scale, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same step with every per-step number on the device, so that its three launches can be captured into a graph and replayed:
 * gradient norm -> prologue -> Adam.  Same table_dev / chunks_dev as above; nothing here allocates, copies or synchronises.
 *
 * xvit_grad_sqnorm_partials: partials_dev[i] = sum of g*g over chunk i (fp32, fixed summation order, one plain store per block, no
 *   atomics: bit-identical from run to run).  partials_dev holds n_chunks floats.  Several tables may fill disjoint ranges of one
 *   partials array; the prologue then sees the norm over all of them.
 * xvit_adam_prologue (one block): sums partials_dev[0 .. n_partials) in index order in double and updates *state_dev:
 *   grad_norm = sqrt(sum);  clip_coef = min(1, max_norm / (grad_norm + 1e-6)) (torch.nn.utils.clip_grad_norm_; exactly 1 under the limit,
 *   and with max_norm = INFINITY, which switches clipping off);  step += 1;  lr_over_bc1 = lr / (1 - beta1^step) and
 *   inv_sqrt_bc2 = 1 / sqrt(1 - beta2^step) in double from the record's own `lr`, which the host writes whenever the learning rate changes.
 *   skip_nonfinite != 0: an inf / NaN norm leaves `step` alone, sets `skip` and increments `skipped`; a finite one clears `skip`.
 *   partials_dev = NULL with n_partials = 0: no norm was taken (grad_norm = 0, clip_coef = 1).
 * xvit_adam_step_dev: the update of the by-value entry point with lr / bias corrections / gradient scale (= clip_coef) read from *state_dev;
 *   returns without writing anything when `skip` is set.  The gradients are scaled in registers: g in memory stays unclipped.
 * A caller zero-fills the record, sets `lr`, and keeps one record per parameter group (one step count per group).
 * ---------------------------------------------------------------------------------------- */
typedef struct xvit_adam_state {
  int64_t step;       /* steps taken so far */
  int64_t skipped;    /* steps skipped because the gradient norm was not finite */
  float lr;           /* written by the host */
  float grad_norm;    /* total L2 norm of the gradients of this step, before clipping */
  float clip_coef;
  float lr_over_bc1;
  float inv_sqrt_bc2;
  int32_t skip;       /* this step is skipped */
  int32_t reserved[2];
} xvit_adam_state;    /* 48 bytes */
int xvit_grad_sqnorm_partials(const void* table_dev, const void* chunks_dev, int n_chunks, float* partials_dev, xvit_stream_t stream);
int xvit_adam_prologue(const float* partials_dev, int n_partials, xvit_adam_state* state_dev, float max_norm, float beta1, float beta2,
                       int skip_nonfinite, xvit_stream_t stream);
int xvit_adam_step_dev(const void* table_dev, const void* chunks_dev, int n_chunks, const xvit_adam_state* state_dev, float beta1, float beta2,
                       float eps, float weight_decay, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * AdamW with a rate and a decay per tensor and a fused exponential moving average of the weights.  table_dev / chunks_dev are the tables
 * of xvit_adam_step (so xvit_grad_sqnorm_partials and xvit_adam_prologue run unchanged on them); extras_dev is a device array with one
 * xvit_adamw_extra per row of table_dev:
 *   lr_scale      the tensor's rate is lr * lr_scale (layer-wise learning-rate decay);  a = (lr / bc1) * lr_scale, lr_t = lr * lr_scale in fp32
 *   weight_decay  the tensor's decay wd_t
 *   ema           fp32 average of p (n elements), or NULL: this tensor keeps none
 * Update order per element, all fp32:
 *   decoupled != 0 (torch.optim.AdamW):  p *= 1 - lr_t * wd_t  (first, with the raw rate, not lr / bc1);  g^ = g * grad_scale
 *   decoupled == 0 (torch.optim.Adam):   g^ = g * grad_scale + wd_t * p
 *   m = beta1 m + (1 - beta1) g^;  v = beta2 v + (1 - beta2) g^ g^;  p -= a * m / (sqrt(v) * inv_sqrt_bc2 + eps)
 *   ema += w * (p - ema) with the p just stored;  shadow_bf16 = bf16(p)
 * xvit_adamw_step: w = ema_weight, in [0, 1].  xvit_adamw_step_dev reads lr, the bias corrections, clip_coef (the gradient scale) and
 *   `skip` from *state_dev as xvit_adam_step_dev does (a skipped step writes nothing, the average included), and forms
 *   w = 1 - ema_decay, or with ema_warmup != 0  w = 1 - min(ema_decay, (1 + t) / (10 + t)),  t = (float)state->step, the count the
 *   prologue already advanced (1 at the first step).  ema_decay in [0, 1).
 * xvit_ema_swap: exchanges p and ema element by element for every tensor that has an average and writes shadow_bf16 = bf16(new p);
 *   copies only, so a second call restores every bit.  Tensors with ema = NULL and chunks the list does not name are left alone.
 * ---------------------------------------------------------------------------------------- */
typedef struct xvit_adamw_extra {
  float* ema;          /* or NULL */
  float lr_scale;
  float weight_decay;
} xvit_adamw_extra;    /* 16 bytes */
int xvit_adamw_step(const void* table_dev, const xvit_adamw_extra* extras_dev, const void* chunks_dev, int n_chunks, float lr, float beta1,
                    float beta2, float eps, int step, float grad_scale, int decoupled, float ema_weight, xvit_stream_t stream);
int xvit_adamw_step_dev(const void* table_dev, const xvit_adamw_extra* extras_dev, const void* chunks_dev, int n_chunks,
                        const xvit_adam_state* state_dev, float beta1, float beta2, float eps, int decoupled, float ema_decay, int ema_warmup,
                        xvit_stream_t stream);
int xvit_ema_swap(const void* table_dev, const xvit_adamw_extra* extras_dev, const void* chunks_dev, int n_chunks, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * bf16 wire format of the data-parallel gradient reducer (xvit/ddp.py, comm_dtype=torch.bfloat16; the counterpart of DDP's
 * bf16_compress_hook).  A bucket is a flat fp32 buffer of 64-element slots, one per parameter; its bf16 communication buffer has
 * the same slot layout.
 *
 * pack: for each segment, dst_bf16[dst_offset + i] = bf16(src[i] * scale) for i < n (round to nearest even, bit-identical to
 * (x * scale).to(torch.bfloat16); NaN stays NaN) and 0 for n <= i < round_up(n, 64), the slot padding.  `segments` is a HOST
 * array, read during the call and passed to the kernel by value in its arguments: no device table, nothing to copy, so the launch
 * can be captured into a graph.  At most XVIT_GRAD_PACK_MAX_SEGMENTS segments per call (a larger bucket takes several calls).
 * src 16-byte aligned, dst_offset a multiple of 64, every slot inside [0, dst_n), dst_bf16 16-byte aligned.
 * unpack: dst[i] = float(src_bf16[i]) * scale, i < n; both pointers 16-byte aligned.
 * ---------------------------------------------------------------------------------------- */
#define XVIT_GRAD_PACK_MAX_SEGMENTS 32
typedef struct xvit_grad_segment {
  const float* src;
  int64_t dst_offset; /* elements */
  int64_t n;
} xvit_grad_segment;
int xvit_grad_pack_bf16(const xvit_grad_segment* segments, int n_segments, void* dst_bf16, int64_t dst_n, float scale, xvit_stream_t stream);
int xvit_grad_unpack_bf16(const void* src_bf16, float* dst, int64_t n, float scale, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Device-resident volume store (csrc/batch_store.hip; xvit/data.py).  The reference draws its batches on the host
 * (main_mist.py:194-207: WeightedRandomSampler over the case table, five loader workers); here the raw volumes of every case live in one
 * device allocation, the sampler is drawn on the device and the batch is gathered through an index tensor that never leaves it, so a
 * captured step replays draw -> gather -> augment -> forward -> backward -> optimizer with no host data work.
 *
 * xvit_batch_draw writes idx[B] (int32), the case index of every sample of one batch.  With c = counter ? *counter : call, sample i has the
 * global ordinal k = (c * world + rank) * B + i (uint64, modulo 2^64), and its index is a function of (seed, k) alone: the sample stream
 * does not depend on how it is cut into ranks and calls.  s = seed ^ 0x5356444154415354 keeps the stream apart from the other draw streams
 * under one seed; hash32 is the dropout hash (xvit_dropout), draw24 its low 24 bits.
 *    XVIT_BATCH_WEIGHTED    with replacement (WeightedRandomSampler(replacement=True) in kind; parity with torch's stream is NOT claimed):
 *                           u = (draw24(s, 2k) * 2^24 + draw24(s, 2k + 1)) * 2^-48, exact in fp64; idx = the number of j with cdf[j] <= u,
 *                           clamped to n_cases - 1.  cdf[n_cases] is the inclusive fp64 prefix of the normalised weights, built on the
 *                           host, non-decreasing, with every entry from the last positive weight on exactly 1: a zero-weight case is never
 *                           drawn.  cdf is required in this mode and ignored in the others.
 *    XVIT_BATCH_SHUFFLE     without replacement within an epoch: q = k mod n, e = k div n, idx = pi_e(q).  pi_e is a keyed bijection on
 *                           [0, n): a balanced 4-round Feistel network on w bits, w = max(2, ceil(log2 n)) rounded up to even, with cycle
 *                           walking.  L = x >> w/2, R = x & mask; each round r = 0..3: (L, R) <- (R, L ^ (hash32(key, r << 32 | R) & mask)),
 *                           key = s + e * 0xD1B54A32D192ED03; x = L << w/2 | R; repeat while x >= n.  Any n consecutive ordinals from a
 *                           multiple of n see every case exactly once, so the ranks of an epoch are disjoint; a batch may straddle two
 *                           epochs.  A bijection; uniformity over all permutations is not claimed.
 *    XVIT_BATCH_SEQUENTIAL  idx = k mod n.
 * The counter as in xvit_augment_draw: optional, 8-byte aligned, read at run time; advance != 0: one thread stores counter + 1 after every
 * thread has read it.  One workgroup loops over B.  Refused before the launch: null idx, n_cases <= 0 or > 2^31 - 1, B <= 0, an unknown
 * mode, rank outside [0, world), a misaligned counter, idx or cdf, advance without a counter, the weighted mode without a cdf.
 *
 * xvit_batch_gather: dst[b] = store[idx[b]] byte for byte (case_bytes bytes each, any dtype) and, with labels_src != NULL,
 * labels_dst[b] = labels_src[idx[b]]; status (optional) receives 0 per sample.  idx is read on the device: the next replay of a captured
 * launch gathers another batch.  An index outside [0, n_cases) gives a zero-filled case, label -1 and status[b] = 1; the kernel never
 * reads outside the store whatever idx holds.  store [n_cases, case_bytes] and dst [B, case_bytes] are contiguous and 16-byte aligned,
 * case_bytes a positive multiple of 2.  With case_bytes % 16 == 0 (every real volume shape) every case base is aligned: 16 bytes per
 * lane, eight loads of a lane in flight before its first store, each 256-thread workgroup owns a 32 KiB chunk of one case.  Otherwise
 * the phases of source and destination differ per case and a 2-byte-per-lane path runs (4 KiB chunks).  Refused before the launch: null
 * store, idx or dst, labels_src without labels_dst, sizes <= 0, an odd case_bytes, misalignment, B x chunks >= 2^31.
 * ---------------------------------------------------------------------------------------- */
enum { XVIT_BATCH_WEIGHTED = 0, XVIT_BATCH_SHUFFLE = 1, XVIT_BATCH_SEQUENTIAL = 2 };
int xvit_batch_draw(int32_t* idx, const double* cdf, int64_t n_cases, int B, int mode, int rank, int world, uint64_t seed, uint64_t call,
                    uint64_t* counter, int advance, xvit_stream_t stream);
int xvit_batch_gather(const void* store, int64_t case_bytes, int64_t n_cases, const int32_t* idx, int B, void* dst, const int64_t* labels_src,
                      int64_t* labels_dst, int32_t* status, xvit_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Head tail (model_cross.py:205-211): logits = mean_m logits_m;  loss = CE(logits, labels,
 * label_smoothing), mean over the batch.  Also writes dlogits_m[M,B,C] = d loss / d logits_m.
 * ---------------------------------------------------------------------------------------- */
int xvit_mean_ce(const float* logits_m, const int64_t* labels, float label_smoothing, float* logits, float* loss, float* dlogits_m,
                 int M, int B, int C, xvit_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* XVIT_H */
