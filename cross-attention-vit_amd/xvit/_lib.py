"""ctypes binding of libxvit_hip.so (the C ABI declared in include/xvit.h).

There is NO fallback: if the library is missing or a call fails, this raises."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("XVIT_LIB") or os.path.join(_HERE, "libxvit_hip.so")   # XVIT_LIB: A/B-test another build of the same ABI

i32, i64, f32, u64, vp = C.c_int32, C.c_int64, C.c_float, C.c_uint64, C.c_void_p


class GemmArgs(C.Structure):
    """struct xvit_gemm_args (include/xvit.h)."""
    _fields_ = [(n, i32) for n in (
        "layout", "M", "N", "K", "batch", "c_dtype", "act", "accumulate", "split_k",
        "res_row_mod", "res_row_off", "out_seg_rows", "out_seg_skip", "out_row_off", "aux_mode")] + [
        (n, vp) for n in ("A", "B", "C", "bias", "residual", "aux")] + [
        (n, i64) for n in ("lda", "ldb", "ldc", "ldr", "ldaux",
                           "stride_a", "stride_b", "stride_c", "stride_bias", "stride_r", "stride_aux")] + [
        ("workspace", vp), ("workspace_bytes", i64), ("colsum", vp), ("dropout_p", f32), ("reserved2", i32), ("dropout_seed", u64)]


class PatchGeom(C.Structure):
    """struct xvit_patch_geom (include/xvit.h)."""
    _fields_ = [(n, i32) for n in ("B", "M", "D", "H", "W", "dp", "hp", "wp", "cls_rows")]


class GradSegment(C.Structure):
    """struct xvit_grad_segment (include/xvit.h)."""
    _fields_ = [("src", vp), ("dst_offset", i64), ("n", i64)]


GRAD_PACK_MAX_SEGMENTS = 32   # XVIT_GRAD_PACK_MAX_SEGMENTS


class AugmentConfig(C.Structure):
    """struct xvit_augment_config (include/xvit.h)."""
    _fields_ = [("flip_prob", f32 * 3), ("rotate_prob", f32), ("rotate_range", f32 * 3), ("zoom_prob", f32), ("zoom_range", f32 * 2),
                ("translate_prob", f32), ("translate_range", f32 * 3), ("scale_prob", f32), ("scale_range", f32 * 2),
                ("shift_prob", f32), ("shift_range", f32 * 2), ("noise_prob", f32), ("noise_std", f32),
                ("intensity_scale", f32), ("intensity_shift", f32)]


AUG_NPARAM = 32   # XVIT_AUG_NPARAM


class ElasticConfig(C.Structure):
    """struct xvit_elastic_config (include/xvit.h)."""
    _fields_ = [("prob", f32), ("max_displacement", f32 * 3), ("locked_borders", i32)]


ELASTIC_MAX_GRID, ELASTIC_NREC = 16, 8   # XVIT_ELASTIC_MAX_GRID, XVIT_ELASTIC_NREC


class ContrastConfig(C.Structure):
    """struct xvit_contrast_config (include/xvit.h)."""
    _fields_ = [("blur_prob", f32), ("blur_sigma_range", f32 * 2), ("blur_isotropic", i32), ("bias_prob", f32), ("bias_coeff", f32),
                ("gamma_prob", f32), ("log_gamma_range", f32 * 2), ("gamma_window", f32 * 2)]


CON_NPARAM, CON_MAX_RADIUS = 32, 6   # XVIT_CON_NPARAM, XVIT_CON_MAX_RADIUS


class NormConfig(C.Structure):
    """struct xvit_norm_config (include/xvit.h)."""
    _fields_ = [("mode", i32), ("clip", i32), ("foreground_above", f32), ("q_lo", f32), ("q_hi", f32)]


STATS_NSTAT = 8                                        # XVIT_STATS_NSTAT
STATS_WINDOW_LO, STATS_WINDOW_BINS = 32768, 32768      # XVIT_STATS_WINDOW_*: the keys the histogram kernel counts in LDS
NORM_STATS_ONLY, NORM_ZSCORE, NORM_WINDOW = 0, 1, 2    # XVIT_NORM_*


class CropConfig(C.Structure):
    """struct xvit_crop_config (include/xvit.h)."""
    _fields_ = [("mode", i32), ("margin", i32 * 3), ("allow_upscale", i32), ("foreground_above", f32)]


BBOX_NREC = 8                                          # XVIT_BBOX_NREC
BBOX_Z0, BBOX_Z1, BBOX_Y0, BBOX_Y1, BBOX_X0, BBOX_X1, BBOX_COUNT = 0, 1, 2, 3, 4, 5, 6   # XVIT_BBOX_*
CROP_BOXES_ONLY, CROP_CENTER, CROP_FIT = 0, 1, 2       # XVIT_CROP_*
AUG_CROP_SCALE = 31                                    # XVIT_AUG_CROP_SCALE


class ComponentConfig(C.Structure):
    """struct xvit_component_config (include/xvit.h)."""
    _fields_ = [("connectivity", i32), ("keep", i32), ("min_voxels", i32), ("foreground_above", f32)]


CC_NREC = 8                                            # XVIT_CC_NREC
CC_COUNT, CC_LARGEST_ROOT, CC_LARGEST_SIZE, CC_KEPT, CC_KEPT_VOXELS, CC_STATUS = 0, 1, 2, 3, 4, 5   # XVIT_CC_*: the slots of a comps record
CC_LARGEST, CC_MIN_VOXELS = 0, 1                       # XVIT_CC_LARGEST, XVIT_CC_MIN_VOXELS: the keep modes
MAE_MAX_PD = 8192                                      # XVIT_MAE_MAX_PD: the largest patch (voxels) xvit_mae_loss_fwd holds in LDS
TOKEN_SELECT_MAX_P = 8192                              # XVIT_TOKEN_SELECT_MAX_P: the longest sequence xvit_token_select_draw ranks in LDS
TOKEN_RANK_RANDOM, TOKEN_RANK_TOP = 0, 1               # XVIT_TOKEN_RANK_*: the modes of xvit_token_select_ranked
EPOCH_MAX_C, EPOCH_MAX_B = 64, 8192                   # XVIT_EPOCH_MAX_C, XVIT_EPOCH_MAX_B: the limits of xvit_epoch_metrics_update
EPOCH_STATE_HEAD = 8                                   # XVIT_EPOCH_STATE_HEAD: int64 counters in front of the C x C confusion
EPOCH_STORED, EPOCH_SEEN, EPOCH_STEPS, EPOCH_IGNORED, EPOCH_NONFINITE, EPOCH_OVERFLOW = 0, 1, 2, 3, 4, 5   # XVIT_EPOCH_*: the counters
EPOCH_RANK_PASS = 1024                                 # XVIT_EPOCH_RANK_PASS: sorted elements per pass of xvit_epoch_rank_stats' walk
EPOCH_RANK_MAX_N = 65535                               # XVIT_EPOCH_RANK_MAX_N: the largest epoch with bootstrap replicates
EPOCH_RANK_NSTAT = 3                                   # XVIT_EPOCH_RANK_NSTAT
EPOCH_RANK_U2, EPOCH_RANK_WPOS, EPOCH_RANK_WNEG = 0, 1, 2   # XVIT_EPOCH_RANK_*


class MixConfig(C.Structure):
    """struct xvit_mix_config (include/xvit.h)."""
    _fields_ = [("mixup_alpha", f32), ("cutmix_alpha", f32), ("prob", f32), ("switch_prob", f32), ("per_sample", i32)]


MIX_NPARAM = 16                                        # XVIT_MIX_NPARAM: floats per record of the Mixup / CutMix table
MIX_MODE, MIX_PARTNER, MIX_LAM, MIX_OML, MIX_BOX, MIX_LAM0 = 0, 1, 2, 3, 4, 10    # XVIT_MIX_*: the record's fields
MIX_MODE_MIXUP, MIX_MODE_CUTMIX = 1, 2                 # XVIT_MIX_MODE_*
MIX_DRAW_STRIDE = 256                                  # XVIT_MIX_DRAW_STRIDE: hash indices per decision block of xvit_mix_draw
BATCH_WEIGHTED, BATCH_SHUFFLE, BATCH_SEQUENTIAL = 0, 1, 2   # XVIT_BATCH_*: the modes of xvit_batch_draw


# name -> argtypes; every function returns int except the two noted below
SIGNATURES = {
    "xvit_gemm": [C.POINTER(GemmArgs), vp],
    "xvit_small_linear_fwd": [vp, i64, vp, vp, vp, i32, i32, i32, vp],
    "xvit_small_linear_bwd": [vp, vp, i64, vp, vp, i64, vp, i64, vp, vp, i32, i32, i32, i32, vp],
    "xvit_layernorm_fwd": [vp, vp, i64, i32, i64, vp, vp, f32, vp, i64, vp, i64, vp, vp, i32, i32, vp],
    "xvit_linear_f32": [vp, i64, vp, i64, vp, vp, i64, i32, i32, i32, i32, vp, i64, vp, i64, vp, i64, f32, u64, vp, i64, vp],
    "xvit_layernorm_bwd": [vp, i64, vp, vp, i64, i32, i64, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, i32, i32, vp, i64, vp],
    "xvit_attn_fwd": [vp, vp, vp, i64, i64, vp, i64, i64, vp, i32, i32, i32, i32, f32, f32, u64, vp, i64, vp],
    "xvit_attn_bwd": [vp, vp, vp, i64, i64, vp, vp, i64, i64, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, f32, f32, u64, vp],
    "xvit_attn_rollout_step": [vp, vp, i64, i64, vp, vp, vp, i32, i32, i32, i32, f32, vp],
    "xvit_attn_relevance_step": [vp, vp, vp, i64, i64, vp, vp, i64, i64, vp, vp, i32, i32, i32, i32, f32, vp],
    "xvit_attn_fwd_fp8": [vp, vp, vp, i64, i64, vp, i64, i64, vp, i32, i32, i32, i32, f32, vp, i64, vp],
    "xvit_cls_xattn_fwd": [vp, i64, vp, i64, vp, vp, i64, i64, vp, i64, vp, i64, vp, i32, i32, i32, i32, f32, f32, u64, vp],
    "xvit_cls_xattn_bwd": [vp, i64, vp, vp, i64, i64, vp, vp, i64, vp, i64, vp, vp, vp, i32, i32, i32, i32, f32, f32, u64, vp],
    "xvit_head_rows": [vp, i64, vp, i64, vp, i64, i64, vp, i64, i64, i32, i32, i32, i32, vp],
    "xvit_head_cols": [vp, i64, i64, vp, i64, vp, i64, vp, vp, i64, vp, i64, vp, i64, i32, i32, i32, vp],
    "xvit_head_bias_grad": [vp, i64, vp, i64, vp, i32, i32, i32, vp],
    "xvit_head_wgrad": [vp, i64, vp, i64, i64, vp, i64, vp, i64, i32, i32, i32, vp],
    "xvit_cls_softmax_fwd": [vp, i64, vp, i64, vp, i32, i32, i32, f32, vp, f32, u64, vp],
    "xvit_cls_softmax_bwd": [vp, i64, vp, vp, i64, vp, vp, i64, i32, i32, i32, f32, f32, u64, vp],
    "xvit_xattn_kv_dgrad": [vp, vp, vp, i64, i32, i32, i32, i32, vp],
    "xvit_patchify": [vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, i64, i64, i32, i32, i64, vp],
    "xvit_patch_embed_supported": [C.POINTER(PatchGeom), i32],
    "xvit_patch_embed_fwd": [vp, C.POINTER(PatchGeom), vp, i64, vp, vp, i64, vp, i64, i32, vp],
    "xvit_patch_embed_wgrad": [vp, C.POINTER(PatchGeom), vp, i64, vp, i64, i32, vp, i64, vp],
    "xvit_patch_embed_dgrad_supported": [C.POINTER(PatchGeom), i32],
    "xvit_patch_embed_dgrad": [vp, i64, vp, i64, C.POINTER(PatchGeom), i32, vp, i32, vp],
    "xvit_unpatchify": [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i64, i64, i32, vp],
    "xvit_cls_row_fwd": [vp, vp, vp, i32, i32, i32, vp],
    "xvit_embed_bwd": [vp, vp, vp, i32, i32, i32, vp],
    "xvit_token_select_draw": [vp, vp, i32, i32, i32, i32, i32, u64, vp],
    "xvit_patchify_select": [vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "xvit_embed_select_fwd": [vp, vp, vp, vp, i32, i32, i32, vp],
    "xvit_embed_select_bwd": [vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "xvit_token_select_complement": [vp, vp, vp, i32, i32, i32, vp],
    "xvit_patch_occupancy": [vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp],
    "xvit_token_select_ranked": [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, u64, vp],
    "xvit_mae_unshuffle_fwd": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "xvit_mae_unshuffle_bwd": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "xvit_token_rows_gather": [vp, vp, vp, i32, i32, i32, i32, vp],
    "xvit_token_rows_scatter": [vp, vp, vp, i32, i32, i32, i32, vp],
    "xvit_mae_loss_fwd": [vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "xvit_mae_loss_bwd": [vp, i32, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "xvit_cast_f32_bf16": [vp, vp, i64, vp],
    "xvit_add_cast_f32_bf16": [vp, vp, vp, vp, i64, vp],
    "xvit_rows_combine": [vp, i32, i64, vp, i32, i64, vp, i32, i64, vp, i32, i64, i32, i32, vp],
    "xvit_colsum": [vp, i32, i64, vp, i32, i32, i32, vp, i64, vp],
    "xvit_dropout": [vp, vp, i32, i64, f32, u64, vp],
    "xvit_cu_trace": [vp, i32, i32, vp],
    "xvit_binary_metrics_step": [vp, i64, vp, i32, i32, vp, vp],
    "xvit_epoch_metrics_update": [vp, i64, vp, i32, i32, vp, vp, vp, i64, vp, vp],
    "xvit_epoch_rank_stats": [vp, vp, vp, vp, i64, vp, i64, i32, i32, u64, vp, vp, vp, vp],
    "xvit_mean_ce": [vp, vp, f32, vp, vp, vp, i32, i32, i32, vp],
    "xvit_mix_draw": [C.POINTER(MixConfig), vp, i32, i32, i32, i32, u64, vp],
    "xvit_mix_apply": [vp, vp, i32, vp, i32, i32, i32, i32, i32, i64, i64, vp],
    "xvit_mean_ce_mix": [vp, vp, vp, f32, vp, vp, vp, i32, i32, i32, vp],
    "xvit_batch_draw": [vp, vp, i64, i32, i32, i32, i32, u64, u64, vp, i32, vp],
    "xvit_batch_gather": [vp, i64, i64, vp, i32, vp, vp, vp, vp, vp],
    "xvit_resize_pad_crop_i16": [vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp],
    "xvit_augment_draw": [C.POINTER(AugmentConfig), vp, i32, i32, i32, i32, i32, i32, i32, i32, u64, vp, i32, vp],
    "xvit_augment_apply": [vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp],
    "xvit_elastic_draw": [C.POINTER(ElasticConfig), vp, vp, i32, i32, i32, i32, u64, vp, i32, vp],
    "xvit_augment_apply_elastic": [vp, i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp],
    "xvit_contrast_draw": [C.POINTER(ContrastConfig), vp, i32, u64, vp, i32, vp],
    "xvit_contrast_apply": [vp, vp, i32, i32, vp, i32, i32, i32, i32, vp],
    "xvit_volume_stats": [vp, i32, i32, i64, C.POINTER(NormConfig), vp, vp, vp, i64, vp],
    "xvit_volume_bbox": [vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(CropConfig), vp, vp, vp, vp, i64, vp],
    "xvit_volume_components": [vp, i32, i32, i32, i32, i32, C.POINTER(ComponentConfig), vp, vp, vp, i64, vp],
    "xvit_volume_bbox_components": [vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(CropConfig), C.POINTER(ComponentConfig), vp, vp, vp, vp, vp, vp, i64, vp],
    "xvit_set_option": [C.c_char_p, i32],
    "xvit_set_dropout_epoch": [C.c_void_p],
    "xvit_adam_step": [vp, vp, i32, f32, f32, f32, f32, f32, i32, f32, vp],
    "xvit_grad_sqnorm_partials": [vp, vp, i32, vp, vp],
    "xvit_adam_prologue": [vp, i32, vp, f32, f32, f32, i32, vp],
    "xvit_adam_step_dev": [vp, vp, i32, vp, f32, f32, f32, f32, vp],
    "xvit_adamw_step": [vp, vp, vp, i32, f32, f32, f32, f32, i32, f32, i32, f32, vp],
    "xvit_adamw_step_dev": [vp, vp, vp, i32, vp, f32, f32, f32, i32, f32, i32, vp],
    "xvit_ema_swap": [vp, vp, vp, i32, vp],
    "xvit_grad_pack_bf16": [C.POINTER(GradSegment), i32, vp, i64, f32, vp],
    "xvit_grad_unpack_bf16": [vp, vp, i64, f32, vp],
}
EXPORTS = sorted(list(SIGNATURES) + ["xvit_version", "xvit_last_error_string", "xvit_gemm_workspace_bytes", "xvit_linear_f32_workspace_bytes",
                                    "xvit_colsum_workspace_bytes", "xvit_layernorm_bwd_workspace_bytes", "xvit_patch_embed_wgrad_workspace_bytes", "xvit_attn_fp8_workspace_bytes",
                                    "xvit_attn_fwd_workspace_bytes", "xvit_attn_bwd_workspace_bytes", "xvit_volume_stats_workspace_bytes", "xvit_volume_bbox_workspace_bytes", "xvit_volume_components_workspace_bytes", "xvit_epoch_rank_stats_max_n"])

_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"xvit: {LIB_PATH} is missing. Build it with `python cross-attention-vit_amd/build.py` "
                "(hipcc, gfx950). There is no CPU or PyTorch fallback for this path.")
        lib = C.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = C.c_int
        lib.xvit_gemm_workspace_bytes.argtypes = [C.POINTER(GemmArgs)]
        lib.xvit_gemm_workspace_bytes.restype = C.c_int64
        lib.xvit_linear_f32_workspace_bytes.argtypes = [i32, i32, i32]
        lib.xvit_linear_f32_workspace_bytes.restype = C.c_int64
        for name in ("xvit_colsum_workspace_bytes", "xvit_layernorm_bwd_workspace_bytes"):
            getattr(lib, name).argtypes = [i32, i32]
            getattr(lib, name).restype = C.c_int64
        lib.xvit_attn_fp8_workspace_bytes.argtypes = [i32, i32, i32, i32]
        lib.xvit_attn_fp8_workspace_bytes.restype = C.c_int64
        for name in ("xvit_attn_fwd_workspace_bytes", "xvit_attn_bwd_workspace_bytes"):
            getattr(lib, name).argtypes = [i32, i32, i32]
            getattr(lib, name).restype = C.c_int64
        lib.xvit_patch_embed_wgrad_workspace_bytes.argtypes = [C.POINTER(PatchGeom), i32]
        lib.xvit_patch_embed_wgrad_workspace_bytes.restype = C.c_int64
        lib.xvit_volume_stats_workspace_bytes.argtypes = [i32]
        lib.xvit_volume_stats_workspace_bytes.restype = C.c_int64
        for name in ("xvit_volume_bbox_workspace_bytes", "xvit_volume_components_workspace_bytes"):
            getattr(lib, name).argtypes = [i32, i64]
            getattr(lib, name).restype = C.c_int64
        lib.xvit_epoch_rank_stats_max_n.argtypes = []
        lib.xvit_epoch_rank_stats_max_n.restype = C.c_int64
        lib.xvit_version.restype = C.c_int
        lib.xvit_last_error_string.restype = C.c_char_p
        _lib = lib
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().xvit_last_error_string().decode(errors="replace")
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")
