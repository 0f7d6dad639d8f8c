"""NumPy / float64 restatement of Mixup / CutMix (include/xvit.h "Mixup / CutMix", csrc/mix.hip) and the gates of the mix tests.

  draw          xvit_mix_draw: the same hash stream and the same algorithm in float64 -> (table fp32 [B, 16], margin [B]).  Everything
                between the hash and the table is IEEE arithmetic that the device repeats bit for bit (products, floors, the integer box)
                EXCEPT what depends on log, cos, pow and cbrt, whose last bits differ between the device's library and NumPy's.  margin[b]
                is the smallest distance from its threshold of any decision of record b that such a function feeds: v > 0 and
                ln u < x^2 / 2 + d - d v + d ln v of every Marsaglia-Tsang round that was reached, and the distance of size * cbrt(1 - lam0)
                from the nearest integer for the three CutMix extents.  A record with a margin under MARGIN may legitimately come out
                otherwise on the device; `check_draw` leaves those out and caps their share at 1 %.
  apply         xvit_mix_apply in float64 -> (ref, bound, exact): `exact` marks the voxels that are copies (every CutMix and copy record)
                and must match bit for bit; a mixup voxel r = lam a + oml b must lie within 2^-23 (|lam a| + |oml b|) of it (the product
                oml b and the fused multiply-add: two fp32 roundings of at most 2^-24 relative each) and, for bf16, 2^-8 |r| more (one
                rounding to 8 significant bits: half an ulp is at most 2^-8 relative).
  loss          xvit_mean_ce_mix in float64 with the magnitudes of _cls_check.ce_ref; gate: _cls_check.ce_check, the bound of xvit_mean_ce.
  fault=...     the planted faults of tests/test_mix_gate_cpu.py."""
import math

import numpy as np
import torch

import _cls_check as X
from _tokdrop_check import EPOCH_STRIDE, hash32, seed_at  # noqa: F401

NPARAM, MODE, PARTNER, LAM, OML, BOX, LAM0 = 16, 0, 1, 2, 3, 4, 10     # XVIT_MIX_*
MIXUP, CUTMIX = 1, 2
STRIDE = 256                                                          # XVIT_MIX_DRAW_STRIDE
ATTEMPTS = 16
U_MIX, U_SWITCH, U_CENTRE, U_BOOST, U_GAMMA = 0, 1, 2, 8, 16
MARGIN = 1e-9
MAX_SKIPPED = 0.01


# ---------------------------------------------------------------------------------------------------------------- draw
def uniform(sd, idx):
    return (hash32(sd, idx).astype(np.float64) + 0.5) * (1.0 / 4294967296.0)


def _gamma(sd, base, g, alpha):
    """-> (value, accepted, margin) per record; base uint64 [n]."""
    n = base.shape[0]
    a = alpha + 1.0 if alpha < 1.0 else alpha
    d = a - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    val, done, margin = np.zeros(n), np.zeros(n, dtype=bool), np.full(n, np.inf)
    for k in range(ATTEMPTS):
        i = base + np.uint64(U_GAMMA + 64 * g + 4 * k)
        x = np.sqrt(-2.0 * np.log(uniform(sd, i))) * np.cos(6.283185307179586 * uniform(sd, i + np.uint64(1)))
        t = 1.0 + c * x
        v = t * t * t
        live = ~done
        margin = np.where(live, np.minimum(margin, np.abs(v)), margin)
        pos = live & (v > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            lhs, rhs = np.log(uniform(sd, i + np.uint64(2))), 0.5 * x * x + d - d * v + d * np.log(np.where(v > 0.0, v, 1.0))
        margin = np.where(pos, np.minimum(margin, np.abs(lhs - rhs)), margin)
        acc = pos & (lhs < rhs)
        val = np.where(acc, d * v, val)
        done |= acc
    if alpha < 1.0:
        val = val * np.power(uniform(sd, base + np.uint64(U_BOOST + g)), 1.0 / alpha)
    return val, done, margin


def draw(cfg, B, D, H, W, seed, epoch=None):
    """cfg: dict(mixup_alpha, cutmix_alpha, prob, switch_prob, per_sample) -> (table float32 [B, 16], margin float64 [B])."""
    f32 = lambda v: float(np.float32(v))   # noqa: E731   the config crosses the C ABI as floats
    ma, ca, prob, sw = f32(cfg["mixup_alpha"]), f32(cfg["cutmix_alpha"]), f32(cfg["prob"]), f32(cfg["switch_prob"])
    sd = seed_at(seed, epoch)
    b = np.arange(B, dtype=np.uint64)
    base = (b if cfg["per_sample"] else np.zeros(B, dtype=np.uint64)) * np.uint64(STRIDE)
    table = np.zeros((B, NPARAM), dtype=np.float32)
    table[:, PARTNER], table[:, LAM], table[:, LAM0] = np.arange(B), 1.0, 1.0
    margin = np.full(B, np.inf)
    if B > 1 and (ma > 0 or ca > 0):
        mixed = uniform(sd, base + np.uint64(U_MIX)) < prob
        cut = (uniform(sd, base + np.uint64(U_SWITCH)) < sw) if (ma > 0 and ca > 0) else np.full(B, ca > 0)
        lam0 = np.full(B, 0.5)
        ok = np.ones(B, dtype=bool)
        for is_cut, alpha in ((False, ma), (True, ca)):
            sel = mixed & (cut == is_cut)
            if alpha <= 0 or not sel.any():
                continue
            g0, a0, m0 = _gamma(sd, base[sel], 0, alpha)
            g1, a1, m1 = _gamma(sd, base[sel], 1, alpha)
            good = a0 & a1 & (g0 + g1 > 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                lam0[sel] = np.where(good, g0 / (g0 + g1), 0.5)
            margin[sel] = np.where(a0, np.minimum(m0, m1), m0)         # the second draw is not reached when the first accepted nothing
            ok[sel] = good
        shift = 1 + int(math.floor(float(uniform(sd, np.uint64(B * STRIDE))) * (B - 1)))
        lam = lam0.copy()
        box = np.zeros((B, 6))
        r = np.cbrt(1.0 - lam0)
        vox = np.ones(B)
        for k, size in enumerate((D, H, W)):
            e = size * r
            ext = np.floor(e)
            frac = np.minimum(e - ext, ext + 1.0 - e)
            margin = np.where(mixed & cut, np.minimum(margin, frac), margin)
            ctr = np.floor(uniform(sd, base + np.uint64(U_CENTRE + k)) * size)
            lo = ctr - np.floor(ext / 2.0)
            hi = lo + ext
            lo, hi = np.maximum(lo, 0.0), np.minimum(hi, float(size))
            box[:, 2 * k], box[:, 2 * k + 1] = lo, hi
            vox = vox * (hi - lo)
        lam = np.where(cut, 1.0 - vox / (float(D) * float(H) * float(W)), lam0)
        table[mixed, MODE] = np.where(cut[mixed], CUTMIX, MIXUP)
        table[mixed, PARTNER] = ((np.arange(B) + shift) % B)[mixed]
        table[mixed, LAM] = lam[mixed].astype(np.float32)
        table[mixed, LAM0] = lam0[mixed].astype(np.float32)
        m2 = mixed & cut
        table[m2, BOX:BOX + 6] = box[m2].astype(np.float32)
        margin = np.where(mixed, margin, np.inf)
    table[:, OML] = np.float32(1.0) - table[:, LAM]
    return table, margin


def check_draw(name, got, ref, margin):
    """got: the device's table (CPU, float32 [B, 16]) against the restatement, record by record.  -> the share of records left out."""
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, f"{name}: table {got.shape} != {ref.shape}"
    use = margin >= MARGIN
    skipped = 1.0 - float(use.mean())
    assert skipped <= MAX_SKIPPED, f"{name}: {skipped:.2%} of the records have a decision margin under {MARGIN:g} (cap {MAX_SKIPPED:.0%})"
    exact = [MODE, PARTNER] + list(range(BOX, BOX + 6)) + list(range(LAM0 + 1, NPARAM))
    for b in np.nonzero(use)[0]:
        for k in exact:
            assert got[b, k] == ref[b, k], f"{name}: record {b} field {k}: {got[b, k]!r} != {ref[b, k]!r}\n got {got[b]}\n ref {ref[b]}"
        for k in (LAM, OML, LAM0):
            g, r = float(got[b, k]), float(ref[b, k])
            assert abs(g - r) <= 1e-9 * abs(r), f"{name}: record {b} field {k}: {g!r} != {r!r} (1e-9 relative)\n got {got[b]}\n ref {ref[b]}"
    return skipped


# the draw cases of tests/test_mix_kernels_gpu.py: (config, B, (D, H, W), seed).  tests/test_mix_gate_cpu.py checks on the CPU that the
# restatement alone leaves at most MAX_SKIPPED of each case's records under MARGIN (at B < 100 that means none).
DRAW_ALPHAS = (0.4, 0.8, 1.0, 2.0)
DRAW_CASES = [(dict(mixup_alpha=a, cutmix_alpha=a, prob=0.9, switch_prob=0.5, per_sample=ps), B, (6, 10, 12), 100 + 37 * i + 5 * B + int(ps))
              for i, a in enumerate(DRAW_ALPHAS) for B in (1, 2, 7, 64) for ps in (False, True)]
DRAW_CASES += [(dict(mixup_alpha=0.8, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, per_sample=True), 64, (5, 7, 9), 901),
               (dict(mixup_alpha=0.0, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, per_sample=True), 64, (16, 16, 32), 902),
               (dict(mixup_alpha=1.0, cutmix_alpha=1.0, prob=0.0, switch_prob=0.5, per_sample=True), 7, (8, 8, 16), 903),
               (dict(mixup_alpha=0.4, cutmix_alpha=2.0, prob=0.5, switch_prob=0.25, per_sample=True), 600, (128, 128, 128), 904)]


def draw_case_id(case):
    cfg, B, vol, seed = case
    return f"mixup{cfg['mixup_alpha']:g}-cutmix{cfg['cutmix_alpha']:g}-prob{cfg['prob']:g}-B{B}-{'sample' if cfg['per_sample'] else 'batch'}-seed{seed}"


# ---------------------------------------------------------------------------------------------------------------- records by hand
def record(mode=0, partner=0, lam=1.0, box=(0, 0, 0, 0, 0, 0), oml=None, lam0=0.0):
    r = np.zeros(NPARAM, dtype=np.float32)
    r[MODE], r[PARTNER], r[LAM], r[LAM0] = mode, partner, lam, lam0
    r[OML] = np.float32(1.0) - r[LAM] if oml is None else oml
    r[BOX:BOX + 6] = box
    return r


def is_mixed(rec, B):
    """The rule of include/xvit.h: mixed only for mode 1 / 2, an integral partner in [0, B) and lam != 1."""
    p = float(rec[PARTNER])
    return float(rec[MODE]) in (1.0, 2.0) and 0.0 <= p < B and p == math.floor(p) and float(rec[LAM]) != 1.0


def box_of(rec, D, H, W):
    e = [int(min(max(float(v), 0.0), s)) if not math.isnan(float(v)) else 0 for v, s in zip(rec[BOX:BOX + 6], (D, D, H, H, W, W))]
    return e


# ---------------------------------------------------------------------------------------------------------------- apply
def apply(src, table, bf16, fault=None):
    """src float64-representable array [B, M, D, H, W] (the values of the bf16 / fp32 tensor), table float32 [B, 16] ->
    (ref float64, bound float64, exact bool), each [B, M, D, H, W].  NaN in src propagates only through what a record reads."""
    src = np.asarray(src, dtype=np.float64)
    B, M, D, H, W = src.shape
    ref, bound, exact = src.copy(), np.zeros_like(src), np.ones(src.shape, dtype=bool)
    for b in range(B):
        rec = table[b]
        if not is_mixed(rec, B):
            continue
        p = int(rec[PARTNER])
        lam, oml = float(rec[LAM]), float(rec[OML])
        if fault == "partner_off_by_one":
            p = (p + 1) % B
        if fault == "swapped_lam_oml":
            lam, oml = oml, lam
        if int(rec[MODE]) == MIXUP:
            ta, tb = lam * src[b], oml * src[p]
            ref[b] = ta + tb
            bound[b] = 2.0 ** -23 * (np.abs(ta) + np.abs(tb)) + (2.0 ** -8 * np.abs(ref[b]) if bf16 else 0.0)
            exact[b] = False
        else:
            d0, d1, h0, h1, w0, w1 = box_of(rec, D, H, W)
            if fault == "box_shifted":
                d0, d1, h0, h1, w0, w1 = d0 + 1, d1 + 1, h0 + 1, h1 + 1, w0 + 1, w1 + 1
            inside = np.zeros((D, H, W), dtype=bool)
            inside[d0:d1, h0:h1, w0:w1] = True
            if fault == "both_sources":                       # arithmetic on both voxels: right on finite data, poisoned by a NaN it must not read
                ref[b] = inside * src[p] + (~inside) * src[b]
            else:
                ref[b] = np.where(inside, src[p], src[b])
    return ref, bound, exact


def to_dtype(ref, bf16):
    """What a correct kernel stores for a float64 value (one rounding) -> torch tensor."""
    t = torch.from_numpy(np.asarray(ref, dtype=np.float64)).to(torch.float32)
    return t.to(torch.bfloat16) if bf16 else t


def check_apply(name, got, ref, bound, exact):
    """got: torch tensor [B, M, D, H, W] (bf16 or fp32, CPU).  Copied voxels bit for bit against ref in got's dtype (NaN is a failure
    wherever ref is finite), mixup voxels within their bound."""
    bf16 = got.dtype == torch.bfloat16
    want = to_dtype(ref, bf16)
    ex, ref_t = torch.from_numpy(exact), torch.from_numpy(ref)
    nan = torch.isnan(ref_t)                                  # a NaN the record reads on purpose (the tests' poison in its own volume) stays a NaN
    wrong = nan != torch.isnan(got.float())
    if bool(wrong.any()):
        i = tuple(int(v) for v in wrong.nonzero()[0])
        raise AssertionError(f"{name}: {int(wrong.sum())} voxels are NaN on one side only (a NaN where the reference is finite: a voxel was read that the "
                             f"record must not read); first at (b, m, z, y, x) = {i}: got {float(got[i])!r}, reference {float(ref[i])!r}")
    bad = (X._bits(got) != X._bits(want)) & ex & ~nan
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} copied voxels differ; first at (b, m, z, y, x) = {i}: {float(got[i])!r} != {float(want[i])!r}")
    err = (got.double() - ref_t).abs()
    over = ~(err <= torch.from_numpy(bound)) & ~ex & ~nan
    if bool(over.any()):
        i = tuple(int(v) for v in over.nonzero()[0])
        raise AssertionError(f"{name}: {int(over.sum())} mixup voxels out of bound; first at (b, m, z, y, x) = {i}: got {float(got[i])!r}, float64 "
                             f"{float(ref[i])!r}, bound {float(bound[i]):.3g}")


# ---------------------------------------------------------------------------------------------------------------- loss
def ce_ref(lm, labels, table, eps, fault=None):
    """_cls_check.ce_ref with the two-label target: float64 on the fp32 inputs -> dict of values and magnitudes."""
    M, B, Cn = lm.shape
    smooth = lambda y, e: torch.nn.functional.one_hot(y, Cn).double() * (1.0 - e) + e / Cn   # noqa: E731
    tgt = smooth(labels, eps)
    for b in range(B):
        rec = table[b]
        if not is_mixed(rec, B):
            continue
        p, lam, oml = int(rec[PARTNER]), float(rec[LAM]), float(rec[OML])
        if fault == "partner_off_by_one":
            p = (p + 1) % B
        if fault == "swapped_lam_oml":
            lam, oml = oml, lam
        tgt[b] = lam * smooth(labels[b:b + 1], eps)[0] + oml * smooth(labels[p:p + 1], 0.0 if fault == "partner_unsmoothed" else eps)[0]
    l64 = lm.double()
    logits = l64.mean(0)
    lz = torch.logsumexp(logits, -1, keepdim=True)
    logp = logits - lz
    loss = -(tgt * logp).sum(-1).mean()
    p = torch.exp(logp)
    dl = ((p - tgt) / (B * M)).expand(M, B, Cn)
    mag = logits.abs() + lz.abs()
    return {"logits": logits, "S_logits": l64.abs().mean(0), "loss": loss, "S_loss": (tgt * mag).sum(-1).mean(), "dl": dl,
            "S_dl": ((p * (1 + mag) + tgt) / (B * M)).expand(M, B, Cn)}


def ce_written(ref, M, B, Cn):
    """The windows a kernel that computed `ref` exactly (rounded once to fp32) would leave: input of X.ce_check in the gate tests."""
    w = X.ce_windows(M, B, Cn)
    w["logits"][0, :B * Cn] = ref["logits"].float().reshape(-1)
    w["loss"][0, 0] = ref["loss"].float()
    w["dl"][0, :M * B * Cn] = ref["dl"].float().reshape(-1)
    return w


def ce_launch(lm, labels, table, eps):
    from xvit import _lib
    lib, dev = _lib.load(), X._dev()
    M, B, Cn = lm.shape
    lmd, lab, tab = lm.to(dev), labels.to(dev), torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    wd = {k: t.to(dev) for k, t in X.ce_windows(M, B, Cn).items()}
    rc = lib.xvit_mean_ce_mix(lmd.data_ptr(), lab.data_ptr(), tab.data_ptr(), eps, wd["logits"].data_ptr(), wd["loss"].data_ptr(), wd["dl"].data_ptr(), M, B, Cn,
                              X._stream())
    torch.cuda.synchronize()
    return rc, {k: t.cpu() for k, t in wd.items()}
