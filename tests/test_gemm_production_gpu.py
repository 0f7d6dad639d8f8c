"""The 256x256 GEMM (gemm_big_kernel) at the model's own GEMM sites and at its edges, against a bit-exact oracle.

Operands are small integers times a power of two (_util.exact_operands): the fp32 product is exact in any summation order, so
every output element is compared on its own — equal to the CPU reference (rounded to nearest-even for bf16 outputs), or within
one bf16 ulp plus the erf approximation's error (ACT_ABS) where the epilogue evaluates GELU / GELU'.  A single wrong 16x16 fragment fails, and the message names its
256x256 tile, 128x64 wave sub-tile and fragment.

SITES mirrors the GEMMs of functional.block_forward / block_backward and of the dense K/V fusion, with the flags those functions
pass and the split their rules pick; test_sites_cover_every_big_kernel_launch (no GPU needed) checks that each gemm_big_kernel
launch of xvit_gemm is reached by at least one site, so a new instantiation without a test fails before any GPU run.
"""
import math
import os
import re
from contextlib import contextmanager
from dataclasses import dataclass

import pytest
import torch

import xvit.functional as XF
from _util import assert_exact, bf16_ulp, dev, exact_grid, exact_operands

GEMM_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cross-attention-vit_amd", "csrc", "gemm.hip")

D, F = 768, 3072                 # configs[1]: width, FFN width
TOK = 513                        # tokens per sample (512 patches + CLS)
B126, B8 = 126 * TOK, 8 * TOK    # rows at the bench batch (64638) and at the reference's batch (4104)
DROP_P, DROP_SEED = 0.5, 987654321   # p = 0.5: the kept values are scaled by exactly 2
# |error| allowed on top of one bf16 ulp where the epilogue evaluates GELU / GELU' (csrc/xvit_common.h gelu_parts): the
# erf approximation is good to 1.5e-7 absolute, which for |z| < 3 stays below 2^-21 in both gelu = z cdf and gelu' = cdf + z pdf
ACT_ABS = 2.0 ** -21
# column sums: the epilogue adds the fp32 values it is about to round and store, in fp32, along a chain of ~600 additions per
# column at M = 64638 (32 rows per lane, 2 shuffles, one atomic per 128-row wave tile): 600 * 2^-24 of the column's sum of |values|
COLSUM_REL = 4e-5


def _ops():
    from xvit import ops
    return ops


@dataclass(frozen=True)
class Site:
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

    @property
    def split(self):
        """The split-K factor the production caller picks (_wgrad for TN, _linear / _dgrad otherwise)."""
        if self.layout == "TN":
            return XF._wgrad_split(self.M, self.N, self.K)
        return XF._skinny_split(self.M, self.N, self.K)


SITES = [
    # block_forward / the dense K/V fusion: _linear
    Site("qkv", "NT", B126, 3 * D, D),
    Site("kv-dense", "NT", B126, 2 * D, D, bias=True),
    Site("out-proj", "NT", B126, D, D, f32=True, bias=True, res=True),
    Site("out-proj-drop", "NT", B126, D, D, f32=True, bias=True, res=True, drop=True),
    Site("ffn1", "NT", B126, F, D, bias=True, act="gelu", aux_mode=1),
    Site("ffn1-aux0", "NT", B126, F, D, bias=True, act="gelu", aux_mode=0),
    Site("ffn1-drop", "NT", B126, F, D, bias=True, act="gelu", aux_mode=1, drop=True),
    Site("ffn2", "NT", B126, D, F, f32=True, bias=True, res=True),
    # block_backward: _dgrad
    Site("ffn2-dgrad", "NN", B126, F, D, act="dgelu", aux_mode=1, colsum=True),
    Site("ffn2-dgrad-aux0", "NN", B126, F, D, act="dgelu", aux_mode=0, colsum=True),
    Site("ffn2-dgrad-drop", "NN", B126, F, D, act="dgelu", aux_mode=1, colsum=True, drop=True),
    Site("ffn1-dgrad", "NN", B126, D, F),
    Site("out-proj-dgrad", "NN", B126, D, D),
    Site("qkv-dgrad", "NN", B126, D, 3 * D),
    # block_backward: _wgrad, dW[out, in] = dy^T x over the tokens (K = 64638 = 1009 * 64 + 62: a ragged last K-step)
    Site("w1-wgrad", "TN", F, D, B126, f32=True),
    Site("w2-wgrad", "TN", D, F, B126, f32=True),
    Site("wo-wgrad", "TN", D, D, B126, f32=True),
    Site("wqkv-wgrad", "TN", 3 * D, D, B126, f32=True),
    Site("wo-wgrad-b56", "TN", D, D, 56 * TOK, f32=True),     # 449 K-steps in 28 splits of 17: the last split starts beyond K
    # the reference's batch 8: the sites whose grid is still large enough for the 256x256 kernel
    Site("qkv-b8", "NT", B8, 3 * D, D),
    Site("ffn1-b8", "NT", B8, F, D, bias=True, act="gelu", aux_mode=1),
    Site("ffn2-dgrad-b8", "NN", B8, F, D, act="dgelu", aux_mode=1, colsum=True),
    Site("w1-wgrad-b8", "TN", F, D, B8, f32=True),
    Site("w2-wgrad-b8", "TN", D, F, B8, f32=True),
]


# ---- which kernels a site launches: a mirror of use_big_tile() and of the `wide` predicate + launch chain of xvit_gemm()
# in csrc/gemm.hip (automatic tile choice, default epilogue, plain row layout: ldc = ldaux = N) --------------------------
def _uses_big_tile(s):
    blocks = ((s.M + 255) // 256) * ((s.N + 255) // 256) * max(s.split, 1)
    return s.M >= 256 and s.N >= 256 and blocks > 128


def _launches(s):
    if not _uses_big_tile(s):
        return {"gemm_kernel"}
    slab = s.split > 1
    wide = (not s.f32 and not slab and not s.res and not s.drop and s.layout != "TN" and s.N % 8 == 0 and
            (s.act != "dgelu" if s.layout == "NT" else s.act != "gelu"))
    nt = s.layout == "NT"
    if wide and nt and s.act == "none": t = "false, false, XVIT_ACT_NONE"
    elif wide and nt and s.aux_mode: t = "false, false, ACT_GELU_D"
    elif wide and nt: t = "false, false, XVIT_ACT_GELU"
    elif wide and s.act == "none": t = "false, true, XVIT_ACT_NONE"
    elif wide and s.aux_mode: t = "false, true, ACT_MULAUX"
    elif wide: t = "false, true, XVIT_ACT_DGELU"
    elif nt: t = "false, false, -1"
    elif s.layout == "NN": t = "false, true, -1"
    else: t = "true, true, -1"
    return {f"gemm_big_kernel<{t}>"} | ({"splitk_epilogue_kernel"} if slab else set())


def _launched_in_xvit_gemm():
    src = open(GEMM_HIP).read()
    body = src[src.index('extern "C" int xvit_gemm('):]
    body = body[:body.index('return check_launch("xvit_gemm")')]
    found = {"gemm_big_kernel<%s>" % ", ".join(a.strip() for a in m.split(","))
             for m in re.findall(r"\blaunch_big<([^>]*)>\(", body)}
    if re.search(r"\blaunch_splitk_reduce\(", body):
        found.add("splitk_epilogue_kernel")
    return found


def test_sites_cover_every_big_kernel_launch():
    """Every gemm_big_kernel instantiation xvit_gemm launches (and the split-K slab pass behind it) is reached by a SITES entry,
    every entry runs on the 256x256 kernel, and the mirror above names nothing gemm.hip does not launch."""
    launched = _launched_in_xvit_gemm()
    assert "splitk_epilogue_kernel" in launched and len(launched) > 2, f"could not parse the launches of xvit_gemm: {launched}"
    small = [s.name for s in SITES if not _uses_big_tile(s)]
    assert not small, f"sites that would not run on the 256x256 kernel: {small}"
    claimed = set().union(*(_launches(s) for s in SITES))
    assert not launched - claimed, f"launched by xvit_gemm but reached by no production-site test: {sorted(launched - claimed)}"
    assert not claimed - launched, f"the mirror of xvit_gemm's dispatch is out of date: {sorted(claimed - launched)}"


# ---- the GPU side -------------------------------------------------------------------------------------------------------
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


def _check_colsum(cs, start, pre, what):
    """cs = start + column sums of `pre`, the epilogue's values before their bf16 rounding (fp64 sum of the reference)."""
    v = pre.double()
    assert_exact(cs, start + v.sum(0), what, tol=COLSUM_REL * v.abs().sum(0) + 1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("site", SITES, ids=[s.name for s in SITES])
def test_production_site(site):
    """One production GEMM under the automatic tile choice (the 256x256 kernel), every output checked element by element."""
    ops = _ops()
    lay = {"NT": ops.NT, "NN": ops.NN, "TN": ops.TN}[site.layout]
    M, N, K = site.M, site.N, site.K
    sa = sb = 4                    # unit 2^-8: at K = 768 the pre-activation has std 0.43, inside the erf's accurate range
    unit = 2.0 ** -(sa + sb)
    a, b, acc = _operands(site.layout, M, N, K, 11, sa, sb)
    ad, bd = a.to(dev(), torch.bfloat16), b.to(dev(), torch.bfloat16)
    out_dt = torch.float32 if site.f32 else torch.bfloat16
    C = torch.full((M, N), float("nan"), dtype=out_dt, device=dev())
    kw = dict(split_k=site.split)
    z = acc
    if site.bias:
        bias = exact_grid((N,), 21, unit, 32)
        kw["bias"] = bias.to(dev())
        z = acc + bias
    if site.res:
        res = exact_grid((M, N), 22, unit, 256)
        kw["residual"] = res.to(dev())
    if site.drop:
        kw["dropout"] = (DROP_P, DROP_SEED)
    aux = None
    if site.act == "gelu":
        aux = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
        kw.update(act=ops.ACT_GELU, aux=aux, aux_mode=site.aux_mode)
    elif site.act == "dgelu":
        zin = exact_grid((M, N), 23, 2.0 ** -5, 96)                     # a pre-activation in [-3, 3]
        aux_cpu = _rowwise(_dgelu, zin).to(torch.bfloat16) if site.aux_mode else zin.to(torch.bfloat16)
        aux = aux_cpu.to(dev())
        kw.update(act=ops.ACT_DGELU, aux=aux, aux_mode=site.aux_mode)
    cs = None
    if site.colsum:
        cs = torch.full((N,), 0.25, device=dev())                       # the epilogue accumulates onto what is there
        kw["colsum"] = cs
    ops.gemm(lay, ad, bd, C, **kw)
    torch.cuda.synchronize()
    mask = _mask((M, N), DROP_P, DROP_SEED) if site.drop else None
    tag = f"{site.name} {site.layout} {M}x{N}x{K} split {site.split}"

    if site.act == "gelu":             # aux: gelu'(z) (aux_mode 1) or z itself; C: gelu(z) [* mask]
        if site.aux_mode:
            d = _rowwise(_dgelu, z)
            assert_exact(aux, d, f"{tag}: saved gelu'", tol=bf16_ulp(d) + ACT_ABS)
        else:
            assert_exact(aux, z, f"{tag}: saved pre-activation")
        g = _rowwise(_gelu, z)
        if mask is not None:
            g *= mask
        assert_exact(C, g, f"{tag}: gelu", tol=bf16_ulp(g) + ACT_ABS * (mask if mask is not None else 1.0))
    elif site.act == "dgelu":          # C = acc * gelu'(z) [* mask]: exact when the derivative is the saved bf16 operand
        if site.aux_mode:
            v = acc * aux_cpu.float()          # <= 21 significant bits: exact in fp32
            if mask is not None:
                v *= mask
            assert_exact(C, v, f"{tag}: dgrad x saved gelu'")
        else:
            v = acc.double() * _rowwise(_dgelu, aux_cpu.float())
            if mask is not None:
                v *= mask
            assert_exact(C, v, f"{tag}: dgrad x gelu'(z)", tol=bf16_ulp(v) + ACT_ABS * acc.abs().double() * (mask if mask is not None else 1.0))
    else:                              # exact: (acc + bias) [* mask] [+ residual]
        v = z if mask is None else z * mask
        if site.res:
            v = v + res
        assert_exact(C, v, tag)
    if cs is not None:
        _check_colsum(cs, 0.25, v, f"{tag}: colsum")
    if site.layout == "TN":            # once more on top of known values (beta = 1)
        P = exact_grid((M, N), 24, unit, 1024)
        C.copy_(P.to(dev()))
        ops.gemm(lay, ad, bd, C, accumulate=True, **kw)
        assert_exact(C, P + acc, f"{tag}: accumulate")


# ---- edges at moderate size, forced onto the 256x256 kernel ------------------------------------------------------------
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


def _exact_case(layout, M, N, K, *, f32=False, split=1, batch=(), bias=False, res=False, group=0, what=""):
    """One GEMM on the 256x256 kernel with exact operands; TN (fp32) also once more with accumulate on known values."""
    sa = sb = 2
    unit = 2.0 ** -(sa + sb)
    a, b, ref = _operands(layout, M, N, K, 5, sa, sb, batch)
    kw = dict(split_k=split)
    if bias:
        bv = exact_grid(batch + (N,), 6, unit, 32)
        kw["bias"] = bv.to(dev())
        ref = ref + bv.unsqueeze(-2)
    if res:
        rv = exact_grid(batch + (M, N), 7, unit, 256)
        kw["residual"] = rv.to(dev())
        ref = ref + rv
    with _options(gemm_tile=2, gemm_group=group) as ops:
        lay = {"NT": ops.NT, "NN": ops.NN, "TN": ops.TN}[layout]
        ad, bd = a.to(dev(), torch.bfloat16), b.to(dev(), torch.bfloat16)
        C = torch.full(batch + (M, N), float("nan"), dtype=torch.float32 if f32 else torch.bfloat16, device=dev())
        ops.gemm(lay, ad, bd, C, **kw)
        assert_exact(C, ref, what)
        if f32:
            P = exact_grid(batch + (M, N), 8, unit, 1024)
            C.copy_(P.to(dev()))
            ops.gemm(lay, ad, bd, C, accumulate=True, **kw)
            assert_exact(C, P + ref, f"{what} accumulate")


@pytest.mark.gpu
@pytest.mark.parametrize("nk", [1, 2, 3, 4, 5, 13])
@pytest.mark.parametrize("layout,f32", [("NT", False), ("NT", True), ("NN", False), ("NN", True), ("TN", True)])
def test_ring_prologue_and_drain(layout, f32, nk):
    """nk K-steps through the two-stage LDS ring: prologue only, one steady step, ... (ragged last row and column tile)."""
    M, N, K = 296, 520, 64 * nk
    _exact_case(layout, M, N, K, f32=f32, what=f"{layout} {M}x{N}x{K} ({nk} K-steps)")


# (K, split): k_per_split = ceil(ceil(K / 64) / split) K-steps; a split starting at or beyond K gets nk = 0 or (C division) < 0
TN_EDGES = [(65, 1), (127, 1), (769, 1), (831, 1),      # K = 64 n + 1 and 64 n + 63
            (320, 4),                                    # splits of 2, 2, 1, 0 K-steps
            (257, 4),                                    # 2, 2, 1 (one row), then k_begin = 384 > K: nk = -1
            (769, 6),                                    # 3, 3, 3, 3, 1, then k_begin = 960: nk = -2
            (641, 3),                                    # 4, 4, 3 (the last one ragged)
            (4104, 7)]                                   # 6 x 10, then 5 (ragged)


@pytest.mark.gpu
@pytest.mark.parametrize("K,split", TN_EDGES)
def test_tn_contraction_edges(K, split):
    M, N = 296, 520
    _exact_case("TN", M, N, K, f32=True, split=split, what=f"TN {M}x{N}x{K} split {split}")


@pytest.mark.gpu
@pytest.mark.parametrize("group", [1, 2, 4, 5, 7])
@pytest.mark.parametrize("N", [1784, 3072])         # 7 column tiles (the last one ragged), 12
@pytest.mark.parametrize("layout", ["NT", "TN"])
def test_super_column_tile_walk(layout, N, group):
    """gemm_group: super-columns of `group` column tiles, a ragged last super-column, a ragged last row tile (M = 696)."""
    M, K = 696, 128
    f32, split = layout == "TN", 2 if layout == "TN" else 1
    _exact_case(layout, M, N, K, f32=f32, split=split, group=group, what=f"{layout} {M}x{N}x{K} gemm_group {group}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout,batch,split,f32,bias,res", [
    ("NT", 3, 1, False, True, False),     # 6 tiles x 3 = 18 workgroups
    ("NN", 5, 1, True, False, True),      # 6 x 5 = 30
    ("TN", 3, 3, True, False, False),     # 6 x 3 x 3 = 54
    ("NT", 7, 1, True, True, True),       # 6 x 7 = 42
])
def test_batched_grids(layout, batch, split, f32, bias, res):
    """Batched operands with batch x split x tiles not a multiple of 8: the XCD remap of gemm_big_kernel must stay a bijection."""
    M, N, K = 296, 520, 192
    _exact_case(layout, M, N, K, f32=f32, split=split, batch=(batch,), bias=bias, res=res,
                what=f"batched {layout} {batch}x{M}x{N}x{K} split {split}")
