"""The element-wise GEMM check shared by the production-site test (256x256 kernel), the small-kernel test (128x128 kernel and the
split-K reduce) and the CPU gate on the check itself.

Operands are small integers times a power of two (_util.exact_operands), bias / residual / accumulate prefill are integers on the
product's grid (unit 2^-(sa+sb)): every partial sum stays below 2^24 units, the fp32 result is exact in ANY summation order, and each
output element is compared on its own -- equal to the CPU reference (rounded to nearest-even for bf16 outputs), or within the stated
tolerance where the epilogue evaluates GELU / GELU' (ACT_ABS) or sums columns (COLSUM_REL).

Three steps, so that the comparison can be exercised without a GPU (tests/test_gemm_gate_cpu.py):
  reference(spec, mask)   CPU: operands, epilogue inputs and the expected C / aux / column sums
  launch(spec, ref)       GPU: destinations prefilled with NaN (to be written) and a sentinel (remap gaps, padding rows and the
                          columns >= N of an ldc > N / ldaux > N view), one ops.gemm call per pass, everything copied back
  compare(spec, ref, out) CPU: every written element, and every element that must not have been written, bit for bit
check_site = the three in a row, with the dropout mask ops.dropout draws for the same seed.
"""
import math
from contextlib import contextmanager
from dataclasses import dataclass

import torch

from _util import assert_exact, bf16_ulp, dev, exact_grid, exact_operands, note

DROP_P, DROP_SEED = 0.5, 987654321   # p = 0.5: the kept values are scaled by exactly 2
# |error| allowed on top of one bf16 ulp where the epilogue evaluates GELU / GELU' (csrc/xvit_common.h gelu_parts): the
# erf approximation is good to 1.5e-7 absolute, which for |z| < 3 stays below 2^-21 in both gelu = z cdf and gelu' = cdf + z pdf
ACT_ABS = 2.0 ** -21
# column sums: the epilogue adds the fp32 values it is about to round and store, in fp32, along a chain of ~600 additions per
# column at M = 64638 (32 rows per lane, 2 shuffles, one atomic per 128-row wave tile): 600 * 2^-24 of the column's sum of |values|
COLSUM_REL = 4e-5
COLSUM_START = 0.25                  # the epilogue accumulates onto what is there
SENTINEL = -1232.0                   # exact in bf16; what remap gaps, padding rows and padding columns hold before and after
PAD_ROWS = 2                         # untouched rows behind the last output row of every destination

# (K, split): k_per_split = ceil(ceil(K / 64) / split) K-steps; a split starting at or beyond K gets nk = 0 or (C division) < 0
TN_EDGES = [(65, 1), (127, 1), (769, 1), (831, 1),      # K = 64 n + 1 and 64 n + 63
            (320, 4),                                    # splits of 2, 2, 1, 0 K-steps
            (257, 4),                                    # 2, 2, 1 (one row), then k_begin = 384 > K: nk = -1
            (769, 6),                                    # 3, 3, 3, 3, 1, then k_begin = 960: nk = -2
            (641, 3),                                    # 4, 4, 3 (the last one ragged)
            (4104, 7)]                                   # 6 x 10, then 5 (ragged)


def _ops():
    from xvit import ops
    return ops


@dataclass(frozen=True)
class Spec:
    name: str
    layout: str            # "NT" (forward Linear), "NN" (dgrad), "TN" (weight gradient)
    M: int
    N: int
    K: int
    f32: bool = False      # fp32 output (else bf16)
    bias: bool = False
    res: bool = False      # fp32 residual added after the activation / dropout
    act: str = "none"      # "none" | "gelu" (forward, aux written) | "dgelu" (dgrad, aux read)
    aux_mode: int = 0      # 1: aux holds gelu'(z) instead of z
    colsum: bool = False   # += column sums of the output (bias gradient)
    drop: bool = False     # dropout after the activation
    split: int = 1         # split-K factor
    batch: int = 0         # > 0: 3-D operands, per-batch bias / residual / aux (and column sums, which take the bias stride)
    res_mod: int = 0       # > 0: residual row = res_off + row % res_mod (the position table of the patch embedding)
    res_off: int = 0
    seg: tuple = (0, 0, 0)  # (rows, skip, off): output row = row + (row // rows) * skip + off
    ldc_pad: int = 0       # C is the first N columns of a [rows, N + ldc_pad] tensor
    ldaux_pad: int = 0
    lda_slice: bool = False  # A is the middle third of the columns of a three times wider tensor
    accumulate: str = ""   # "again": a second pass with accumulate on known values; "first": the only pass accumulates on them
    tile: int = 256        # the kernel the case runs on: names the coordinates of a failure (256: gemm_big_kernel, 128: gemm_kernel)
    force: bool = False    # set gemm_tile = 1 for the call (cases the automatic choice would send to the 256x256 kernel)
    s: int = 4             # operands in {-3..3} 2^-s: unit 2^-2s (s = 4, K = 768: the pre-activation has std 0.43, inside the erf's accurate range)
    seed: int = 11

    @property
    def bt(self):
        return (self.batch,) if self.batch else ()

    @property
    def tag(self):
        return f"{self.name} {self.layout} {'%dx' % self.batch if self.batch else ''}{self.M}x{self.N}x{self.K} split {self.split}"

    def out_rows(self):
        """Destination row of every GEMM row (out_seg)."""
        r = torch.arange(self.M)
        rows, skip, off = self.seg
        return r + (r // rows) * skip + off if rows > 0 else r


def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def _dgelu(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _rowwise(fn, x, rows=8192):
    """fn of fp64 x, chunk by chunk (the outputs here reach 2e8 elements)."""
    out = torch.empty(x.shape, dtype=torch.float64)
    for r in range(0, x.shape[0], rows):
        out[r:r + rows] = fn(x[r:r + rows].double())
    return out


def _mask(shape, p, seed):
    """The dropout epilogue's mask as ops.dropout draws it for the same (seed, element index): values 0 or 1 / (1 - p)."""
    ops = _ops()
    return ops.dropout(torch.ones(*shape, device=dev()), p, seed).cpu()


def _operands(layout, M, N, K, seed, sa, sb, batch=()):
    shp_a = {"NT": (M, K), "NN": (M, K), "TN": (K, M)}[layout]
    shp_b = {"NT": (N, K), "NN": (K, N), "TN": (K, N)}[layout]
    a, b = exact_operands(batch + shp_a, seed, sa), exact_operands(batch + shp_b, seed + 1, sb)
    eq = {"NT": "...mk,...nk->...mn", "NN": "...mk,...kn->...mn", "TN": "...km,...kn->...mn"}[layout]
    return a, b, torch.einsum(eq, a, b)


def _check_colsum(cs, start, pre, what, tile=256):
    """cs = start + column sums of `pre`, the epilogue's values before their bf16 rounding (fp64 sum of the reference)."""
    v = pre.double()
    assert_exact(cs, start + v.sum(-2), what, tol=COLSUM_REL * v.abs().sum(-2) + 1e-6, tile=tile)


@contextmanager
def _options(**opts):
    ops = _ops()
    try:
        for k, v in opts.items():
            ops.set_option(k, v)
        yield ops
    finally:
        for k in opts:
            ops.set_option(k, 0)


# ---- the CPU reference ---------------------------------------------------------------------------------------------------
def reference(spec, mask=None):
    """Operands, epilogue inputs and expected outputs of one case (all on the CPU).  mask: the dropout mask (0 or 2) of shape
    [batch,] M, N when spec.drop."""
    s, M, N, K, bt = spec, spec.M, spec.N, spec.K, spec.bt
    assert not (s.accumulate and (not s.f32 or s.act != "none")), "accumulate: fp32 C, exact epilogues only"
    assert (mask is not None) == s.drop
    unit = 2.0 ** -(2 * s.s)
    R = dict(unit=unit, mask=mask)
    R["a"], R["b"], acc = _operands(s.layout, M, N, K, s.seed, s.s, s.s, bt)
    R["acc"] = acc
    z = acc
    if s.bias:
        R["bias"] = exact_grid(bt + (N,), s.seed + 10, unit, 32)
        z = acc + R["bias"].unsqueeze(-2)
    rres = None
    if s.res:
        R["res"] = exact_grid(bt + ((s.res_off + s.res_mod) if s.res_mod else M, N), s.seed + 11, unit, 256)
        rres = R["res"][..., s.res_off + torch.arange(M) % s.res_mod, :] if s.res_mod else R["res"]
    mk = mask if mask is not None else 1.0
    R["tol"] = None                                 # None: the stored C is the rounded reference, bit for bit
    if s.act == "gelu":             # aux: gelu'(z) (aux_mode 1) or z itself; C: gelu(z) [* mask]
        R["aux_out"] = _rowwise(_dgelu, z) if s.aux_mode else z
        v = _rowwise(_gelu, z)
        if mask is not None:
            v *= mask
        R["what"] = "gelu"
        R["tol"] = lambda ref: (ref.abs() * 2.0 ** -24 if s.f32 else bf16_ulp(ref)) + ACT_ABS * mk
    elif s.act == "dgelu":          # C = acc * gelu'(z) [* mask]: exact when the derivative is the saved bf16 operand
        zin = exact_grid(bt + (M, N), s.seed + 12, 2.0 ** -5, 96)                     # a pre-activation in [-3, 3]
        R["aux_in"] = _rowwise(_dgelu, zin).to(torch.bfloat16) if s.aux_mode else zin.to(torch.bfloat16)
        if s.aux_mode:
            v = acc * R["aux_in"].float()          # <= 21 significant bits: exact in fp32
            R["what"] = "dgrad x saved gelu'"
        else:
            v = acc.double() * _rowwise(_dgelu, R["aux_in"].float())
            R["what"] = "dgrad x gelu'(z)"
            R["tol"] = lambda ref: (ref.abs() * 2.0 ** -24 if s.f32 else bf16_ulp(ref)) + ACT_ABS * acc.abs().double() * mk
        if mask is not None:
            v *= mask
    else:                              # exact: (acc + bias) [* mask] [+ residual]
        v = z if mask is None else z * mask
        R["what"] = ""
    if rres is not None:
        v = v + rres
    R["v"] = v
    if s.accumulate:
        R["P"] = exact_grid(bt + (M, N), s.seed + 13, unit, 1024)
    return R


def stored(spec, R):
    """What the (first) pass leaves in C, before rounding to C's dtype."""
    return R["P"] + R["v"] if spec.accumulate == "first" else R["v"]


def colsum_pre(spec, R):
    """The values whose column sums the epilogue adds to COLSUM_START: the stored ones before their rounding; one row of sums per
    batch when the bias is per batch (the column sums take the bias stride), else all batches meet in one row."""
    v = stored(spec, R)
    return v.reshape(-1, spec.N) if spec.batch and not spec.bias else v


# ---- destinations -------------------------------------------------------------------------------------------------------
def _dest(spec, dtype, rows_of, pad, fill):
    """[batch,] (last output row + 1 + PAD_ROWS) x (N + pad) of SENTINEL, with `fill` (a value or a tensor [.., M, N]) in the
    elements the kernel may write."""
    t = torch.full(spec.bt + (int(rows_of.max()) + 1 + PAD_ROWS, spec.N + pad), SENTINEL, dtype=dtype)
    t[..., rows_of, :spec.N] = fill.to(dtype) if torch.is_tensor(fill) else fill
    return t


def buffers(spec, R):
    """CPU images of the destinations as they are before the (first) pass."""
    B = {}
    nan = float("nan")
    B["C"] = _dest(spec, torch.float32 if spec.f32 else torch.bfloat16, spec.out_rows(), spec.ldc_pad, R["P"] if spec.accumulate == "first" else nan)
    if spec.act == "gelu":
        B["aux"] = _dest(spec, torch.bfloat16, torch.arange(spec.M), spec.ldaux_pad, nan)
    elif spec.act == "dgelu":
        B["aux"] = _dest(spec, torch.bfloat16, torch.arange(spec.M), spec.ldaux_pad, R["aux_in"])
    if spec.colsum:
        B["cs"] = torch.full((spec.batch, spec.N) if spec.batch and spec.bias else (spec.N,), COLSUM_START)
    return B


def ideal(spec, R):
    """The destinations as a faultless kernel leaves them (the CPU gate plants its faults into these)."""
    out = buffers(spec, R)
    out["C"][..., spec.out_rows(), :spec.N] = stored(spec, R).to(out["C"].dtype)
    if spec.act == "gelu":
        out["aux"][..., :spec.M, :spec.N] = R["aux_out"].to(torch.bfloat16)
    if spec.colsum:
        out["cs"] = (COLSUM_START + colsum_pre(spec, R).double().sum(-2)).float()
    if spec.accumulate == "again":
        out["C2"] = out["C"].clone()
        out["C2"][..., spec.out_rows(), :spec.N] = (R["P"] + R["v"]).to(out["C"].dtype)
    return out


# ---- the GPU side -------------------------------------------------------------------------------------------------------
def _ld8(t):
    """t (CPU fp32 [.., rows, cols]) as a bf16 GPU view whose leading dimension is a multiple of 8 elements (xvit_gemm's rule); the
    padding columns hold operand-like values, not zeros: a loader that reads past a row's end must not get away with it."""
    cols = t.shape[-1]
    ld = (cols + 7) // 8 * 8
    if ld == cols:
        return t.to(dev(), torch.bfloat16)
    full = exact_operands(t.shape[:-1] + (ld,), 99, 0)
    full[..., :cols] = t
    return full.to(dev(), torch.bfloat16)[..., :cols]


def launch(spec, R):
    """Run the case (under the caller's options) and return the destinations as CPU tensors."""
    ops = _ops()
    s = spec
    lay = {"NT": ops.NT, "NN": ops.NN, "TN": ops.TN}[s.layout]
    if s.lda_slice:                 # e.g. the q / k / v columns of a [rows, 3 d] tensor
        assert not s.batch
        w = R["a"].shape[1]
        wide = exact_operands((R["a"].shape[0], 3 * w), 98, s.s)
        wide[:, w:2 * w] = R["a"]
        ad = wide.to(dev(), torch.bfloat16)[:, w:2 * w]
    else:
        ad = _ld8(R["a"])
    bd = _ld8(R["b"])
    B = {k: v.to(dev()) for k, v in buffers(s, R).items()}
    kw = dict(split_k=s.split)
    if s.bias:
        kw["bias"] = R["bias"].to(dev())
    if s.res:
        kw["residual"] = R["res"].to(dev())
    if s.res_mod:
        kw.update(res_row_mod=s.res_mod, res_row_off=s.res_off)
    if s.seg[0]:
        kw["out_seg"] = s.seg
    if s.drop:
        kw["dropout"] = (DROP_P, DROP_SEED)
    if s.act != "none":
        kw.update(act=ops.ACT_GELU if s.act == "gelu" else ops.ACT_DGELU, aux=B["aux"][..., :s.M, :s.N], aux_mode=s.aux_mode)
    if s.colsum:
        kw["colsum"] = B["cs"]
    Cv = B["C"][..., :s.N]
    if s.split > 1:     # the partial tiles go to a NaN-filled workspace (of the size the library asks for): one that no split writes shows up as NaN
        need = ops.gemm_workspace_bytes(lay, s.M, s.N, s.K, s.split, max(s.batch, 1))
        kw["workspace"] = torch.full((need // 4,), float("nan"), device=dev())
    ops.gemm(lay, ad, bd, Cv, accumulate=s.accumulate == "first", **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in B.items()}
    if s.accumulate == "again":     # once more on top of known values (beta = 1)
        kw.pop("colsum", None)
        if s.split > 1:
            kw["workspace"].fill_(float("nan"))
        B["C"][..., s.out_rows().to(dev()), :s.N] = R["P"].to(dev())
        ops.gemm(lay, ad, bd, Cv, accumulate=True, **kw)
        torch.cuda.synchronize()
        out["C2"] = B["C"].cpu()
    return out


# ---- the comparison -----------------------------------------------------------------------------------------------------
def _untouched(t, rows_of, N, what):
    """Every element of destination t outside (rows_of x columns < N) still holds SENTINEL, bit for bit."""
    bits = t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    want = int(torch.tensor(SENTINEL, dtype=t.dtype).view(bits.dtype))
    keep = torch.ones(t.shape[-2], dtype=torch.bool)
    keep[rows_of] = False
    for part, name, rows in ((bits[..., N:], "columns >= N", None), (bits[..., keep, :N], "a row outside the output's row map", keep.nonzero()[:, 0])):
        bad = part != want
        if int(bad.sum()):
            idx = bad.nonzero()[0].tolist()
            r = idx[-2] if rows is None else int(rows[idx[-2]])
            c = idx[-1] + (N if rows is None else 0)
            raise AssertionError(f"{what}: {int(bad.sum())} elements outside the output were overwritten ({name}); first at "
                                 f"{'batch %d, ' % idx[0] if t.dim() == 3 else ''}destination (row {r}, col {c})")


def _written(t, spec, rows_of):
    """The [.., M, N] elements of destination t the kernel writes (a view where the row map is the identity)."""
    return t[..., rows_of, :spec.N] if spec.seg[0] else t[..., :spec.M, :spec.N]


def _measure(spec, cls, got, ref, tol):
    """XVIT_MEASURE_LOG: the largest |out - ref| of one tolerance class against the unrounded reference, and the largest share of its
    tolerance an element used (column sums: the largest |out - ref| as a fraction of the column's sum of |values|, bound COLSUM_REL)."""
    d = (got.double() - ref.double()).abs()
    note(f"gemm:{spec.tile}:{spec.name}:{cls}:max_abs_err", float(d.max()))
    note(f"gemm:{spec.tile}:{spec.name}:{cls}:max_err_over_bound", float(torch.where(d == 0, torch.zeros_like(d), d / tol).max()))


def compare(spec, R, out):
    s, tag, tile = spec, spec.tag, spec.tile
    rows_of = s.out_rows()
    C = _written(out["C"], s, rows_of)
    f = "f32" if s.f32 else "bf16"
    if s.act == "gelu":
        aux = out["aux"][..., :s.M, :s.N]
        if s.aux_mode:
            assert_exact(aux, R["aux_out"], f"{tag}: saved gelu'", tol=bf16_ulp(R["aux_out"]) + ACT_ABS, tile=tile)
            _measure(s, "gelu_bf16_aux", aux, R["aux_out"], bf16_ulp(R["aux_out"]) + ACT_ABS)
        else:
            assert_exact(aux, R["aux_out"], f"{tag}: saved pre-activation", tile=tile)
    ref = stored(s, R)
    what = f"{tag}: {R['what']}" if R["what"] else tag
    tol = R["tol"](ref) if R["tol"] else None
    wrong = assert_exact(C, ref, what, tol=tol, tile=tile)
    if R["tol"]:
        _measure(s, f"gelu_{f}" if s.act == "gelu" else f"acc_dgelu_{f}", C, ref, tol)
    else:
        note(f"gemm:{tile}:{s.name}:exact_{f}_wrong", float(wrong))      # the count assert_exact found (it raises on any other than 0)
    _untouched(out["C"], rows_of, s.N, f"{tag}: C")
    if "aux" in out:
        if s.act == "dgelu":
            assert torch.equal(out["aux"][..., :s.M, :s.N].view(torch.int16), R["aux_in"].view(torch.int16)), f"{tag}: the aux operand of GELU' was modified"
        _untouched(out["aux"], torch.arange(s.M), s.N, f"{tag}: aux")
    if s.colsum:
        pre = colsum_pre(s, R).double()
        _check_colsum(out["cs"], COLSUM_START, pre, f"{tag}: colsum", tile=tile)
        _measure(s, "colsum", out["cs"], COLSUM_START + pre.sum(-2), COLSUM_REL * pre.abs().sum(-2) + 1e-6)
        note(f"gemm:{tile}:{s.name}:colsum:max_err_over_sum_abs",
             float(((out["cs"].double() - COLSUM_START - pre.sum(-2)).abs() / pre.abs().sum(-2).clamp_min(1e-30)).max()))
    if s.accumulate == "again":
        assert_exact(_written(out["C2"], s, rows_of), R["P"] + R["v"], f"{tag}: accumulate", tile=tile)
        _untouched(out["C2"], rows_of, s.N, f"{tag}: C (accumulate)")


def check_site(spec, repeat=False):
    """One GEMM, every output element (and every element around the output) checked; repeat: run it twice, the results must be equal bit for bit."""
    mask = _mask(spec.bt + (spec.M, spec.N), DROP_P, DROP_SEED) if spec.drop else None
    R = reference(spec, mask)
    with _options(**({"gemm_tile": 1} if spec.force else {})):
        out = launch(spec, R)
        again = launch(spec, R) if repeat else None
    compare(spec, R, out)
    if again is not None:
        for k in out:
            assert torch.equal(out[k].view(torch.uint8), again[k].view(torch.uint8)), f"{spec.tag}: {k} differs between two runs"
