"""The 256x256 GEMM (gemm_big_kernel) at the model's own GEMM sites and at its edges, against a bit-exact oracle.

Operands are small integers times a power of two (_util.exact_operands): the fp32 product is exact in any summation order, so
every output element is compared on its own — equal to the CPU reference (rounded to nearest-even for bf16 outputs), or within
one bf16 ulp plus the erf approximation's error (ACT_ABS) where the epilogue evaluates GELU / GELU'.  A single wrong 16x16 fragment fails, and the message names its
256x256 tile, 128x64 wave sub-tile and fragment.

SITES mirrors the GEMMs of functional.block_forward / block_backward and of the dense K/V fusion, with the flags those functions
pass and the split their rules pick; test_sites_cover_every_big_kernel_launch (no GPU needed) checks that each gemm_big_kernel
launch of xvit_gemm is reached by at least one site, so a new instantiation without a test fails before any GPU run.
"""
import os
import re
from dataclasses import asdict, dataclass

import pytest
import torch

import xvit.functional as XF
from _gemm_check import TN_EDGES, Spec, _operands, _options, check_site, compare, launch, reference
from _util import assert_exact, dev, exact_grid

GEMM_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cross-attention-vit_amd", "csrc", "gemm.hip")

D, F = 768, 3072                 # configs[1]: width, FFN width
TOK = 513                        # tokens per sample (512 patches + CLS)
B126, B8 = 126 * TOK, 8 * TOK    # rows at the bench batch (64638) and at the reference's batch (4104)


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


# ---- the GPU side: tests/_gemm_check.py builds the reference, runs the call and compares -------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("site", SITES, ids=[s.name for s in SITES])
def test_production_site(site):
    """One production GEMM under the automatic tile choice (the 256x256 kernel), every output checked element by element
    (TN, fp32: once more with accumulate on known values)."""
    check_site(Spec(**asdict(site), split=site.split, accumulate="again" if site.layout == "TN" else ""))


# ---- edges at moderate size, forced onto the 256x256 kernel ------------------------------------------------------------
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


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("period", [1, 2, 3, 4, 5, 7])
def test_short_residual_and_segment_periods(period, f32):
    """A residual table of `period` rows (res_row_mod) and output segments of `period` rows with a one-row gap (out_seg): the narrow
    epilogue steps 4 rows per body, so periods up to 4 wrap more than once per step, or on every step (the patch embedding of a
    volume of 1 or 2 tokens per sample, fused or as patchify + GEMM).  Once with both maps, once each alone; ragged last tiles."""
    M, N, K = 296, 520, 128
    for res_mod, seg in ((period, (period, 1, 1)), (period, (0, 0, 0)), (0, (period, 1, 1))):
        spec = Spec(f"period-{period}-res{res_mod}-seg{seg[0]}", "NT", M, N, K, f32=f32, bias=True, res=res_mod > 0, res_mod=res_mod, res_off=1 if res_mod else 0,
                    seg=seg, s=2)
        R = reference(spec)
        with _options(gemm_tile=2):
            out = launch(spec, R)
        compare(spec, R, out)
