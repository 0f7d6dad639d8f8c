"""NumPy restatement of foreground-ranked token selection (include/xvit.h, csrc/token_occupancy.hip, csrc/token_select.hip), shared by the
tokfg tests.

  occupancy            xvit_patch_occupancy: per patch, the voxels whose fp32 value is > above (strict; NaN never counts)
  counts               the count a sequence is ranked by: its own row, or the sum over the modalities of its sample (saturated)
  ranked               xvit_token_select_ranked: the K smallest of (not foreground, key, p) or of (-count, p), ascending, and the inverse map
  min_count            the rule ModelCross derives the foreground threshold from

Everything the kernels compute is integer work, so every comparison against these functions is bit-exact."""
import math

import numpy as np
import torch

import _tokdrop_check as T

RANDOM, TOP = 0, 1       # XVIT_TOKEN_RANK_*


def as_f32(img):
    """A torch volume tensor (fp32 | bf16) -> float32 NumPy array of the same values: bf16 is read as the bits torch gives it."""
    img = img.detach().cpu()
    if img.dtype == torch.bfloat16:
        return (img.contiguous().view(torch.int16).numpy().astype(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)
    return img.numpy().astype(np.float32)


def occupancy(img, patch, above):
    """img [B, M, 1, D, H, W] (torch fp32 | bf16, or a float NumPy array) -> int32 [M * B, P]; s = m B + b, t = (h Wn + w) Dn + d."""
    v = as_f32(img) if isinstance(img, torch.Tensor) else np.asarray(img, dtype=np.float32)
    B, M, _, D, H, W = v.shape
    dp, hp, wp = patch
    Dn, Hn, Wn = D // dp, H // hp, W // wp
    with np.errstate(invalid="ignore"):
        fg = v[:, :, 0] > np.float32(above)                                             # NaN > x is False
    c = fg.reshape(B, M, Dn, dp, Hn, hp, Wn, wp).sum(axis=(3, 5, 7), dtype=np.int64)    # [B, M, Dn, Hn, Wn]
    return c.transpose(1, 0, 3, 4, 2).reshape(M * B, Hn * Wn * Dn).astype(np.int32)     # [M, B, Hn, Wn, Dn]


def counts(occ, B, shared):
    """[S, P] int64: what each sequence is ranked by."""
    occ = np.asarray(occ).astype(np.int64)
    S, P = occ.shape
    if not shared:
        return occ
    c = np.minimum(occ.reshape(S // B, B, P).sum(axis=0), 0xFFFFFFFF)
    return np.tile(c, (S // B, 1))


def ranked(occ, B, K, shared, mode, min_count, seed=0, epoch=None):
    """-> keep_idx int32 [S, K] (ascending), slot int32 [S, P], n_fg int32 [S]."""
    S, P = np.asarray(occ).shape
    c = counts(occ, B, shared)
    fg = c >= min_count
    p = np.broadcast_to(np.arange(P), (S, P))
    if mode == RANDOM:
        order = np.lexsort((p, T.keys(S, B, P, shared, seed, epoch), ~fg), axis=1)     # the last key is the primary one
    else:
        order = np.lexsort((p, -c), axis=1)
    keep_idx = np.sort(order[:, :K], axis=1).astype(np.int32)
    return keep_idx, T.slot_of(keep_idx, P), fg.sum(axis=1).astype(np.int32)


def min_count(pd, fraction, modalities=1):
    """max(1, ceil(fraction pd modalities)), the product taken exactly (fractions are decimal)."""
    from fractions import Fraction
    return max(1, math.ceil(Fraction(str(fraction)) * pd * modalities))
