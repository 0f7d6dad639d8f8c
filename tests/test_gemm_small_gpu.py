"""The 128x128 GEMM (gemm_kernel<A_KS, B_KS>) and the split-K reduce (splitk_epilogue_kernel) against a bit-exact oracle: at the
model's own GEMM sites that land on this kernel, at every tile edge, through the LDS ring, at the contraction edges, on grids
whose workgroup count is not a multiple of 8, and through strided views.

tests/_gemm_check.py does the work (exact operands, every output element compared on its own, every element around the output
compared with the sentinel it held); a failure names the 128x128 tile, the 64x64 sub-tile of the wave and the 16x16 fragment.
Tolerances are the project's own (ACT_ABS where GELU / GELU' is evaluated, COLSUM_REL for column sums); everything else is
equality.  tests/test_gemm_gate_cpu.py shows on the CPU that this check catches the faults the rel-L2 gate of test_gemm_gpu.py
lets through.

The two tests without the gpu mark hold the file to its claim: every launch_small<...> instantiation of xvit_gemm and the
split-K reduce behind it are reached by a case here, and no case is routed to the 256x256 kernel.
"""
import os
import re

import pytest

import xvit.functional as XF
from _gemm_check import TN_EDGES, Spec, check_site

GEMM_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cross-attention-vit_amd", "csrc", "gemm.hip")

D, F = 768, 3072                 # configs[1]: width, FFN width
TOK = 513                        # tokens per sample (512 patches + CLS)
B1, B2, B8 = TOK, 2 * TOK, 8 * TOK


def _site(name, layout, M, N, K, **kw):
    """A call of functional._linear / _dgrad / _wgrad: the split is the one their rules pick, the tile choice the automatic one."""
    split = XF._wgrad_split(M, N, K) if layout == "TN" else XF._skinny_split(M, N, K)
    return Spec(name, layout, M, N, K, split=split, tile=128, **kw)


def _ffn_sites():
    out = []
    for M, combos in ((B1, [(1, False), (0, False), (1, True), (0, True)]), (B2, [(1, False), (0, False), (1, True), (0, True)])):
        b = M // TOK
        out.append(_site(f"qkv-b{b}", "NT", M, 3 * D, D))
        for aux_mode, drop in combos:
            sfx = f"-aux{aux_mode}{'-drop' if drop else ''}-b{b}"
            out.append(_site("ffn1" + sfx, "NT", M, F, D, bias=True, act="gelu", aux_mode=aux_mode, drop=drop))
            out.append(_site("ffn2-dgrad" + sfx, "NN", M, F, D, act="dgelu", aux_mode=aux_mode, colsum=True, drop=drop))
    return out


def _lowrank_sites():
    """The batched thin products of the low-rank fusion (functional.cross_forward / cross_backward): scores and dp are
    [N_tok, d] x [16, d]^T per sample, S and T are [N_tok, 16]^T x [N_tok, d] (K = N_tok, never a multiple of 64)."""
    out = []
    for B, H, N in ((5, 12, 513), (2, 3, 17), (3, 16, 130)):
        d = 64 * H
        out += [Spec(f"lowrank-scores-{B}x{H}x{N}", "NT", N, 16, d, f32=True, batch=B, tile=128, seed=31),
                Spec(f"lowrank-S-{B}x{H}x{N}", "TN", 16, d, N, f32=True, batch=B, tile=128, seed=41),
                Spec(f"lowrank-dp-{B}x{H}x{N}", "NT", N, 16, d, f32=True, batch=B, tile=128, seed=51),
                Spec(f"lowrank-T-{B}x{H}x{N}", "TN", 16, d, N, f32=True, batch=B, tile=128, seed=61)]
    return out


def _patch_sites():
    """The unfused patch embedding (PatchEmbedFn.forward): bias + the position table by row modulo; with a zero CLS row in the
    operand (res_row_mod = 1 + P, as functional.py calls it) and with the row remap that leaves the CLS row of the output free."""
    out = []
    for P in (16, 512):
        Bm = 3
        out.append(Spec(f"patch-embed-cls-row-P{P}", "NT", Bm * (P + 1), D, 512, f32=True, bias=True, res=True, res_mod=P + 1, tile=128))
        out.append(Spec(f"patch-embed-remap-P{P}", "NT", Bm * P, D, 512, f32=True, bias=True, res=True, res_mod=P, res_off=1, seg=(P, 1, 1), tile=128))
    return out


SITES = [
    # the reference's batch 8: 17 x 3 tiles of 256x256 for a d-wide product
    _site("out-proj-b8", "NT", B8, D, D, f32=True, bias=True, res=True),
    _site("out-proj-drop-b8", "NT", B8, D, D, f32=True, bias=True, res=True, drop=True),
    _site("ffn2-b8", "NT", B8, D, F, f32=True, bias=True, res=True),
    _site("ffn1-dgrad-b8", "NN", B8, D, F),
    _site("out-proj-dgrad-b8", "NN", B8, D, D),
    _site("qkv-dgrad-b8", "NN", B8, D, 3 * D),
    # the weight gradients _wgrad_split leaves on at most 128 big tiles
    _site("wo-wgrad-b8", "TN", D, D, B8, f32=True, accumulate="again"),
    _site("wqkv-wgrad-b8", "TN", 3 * D, D, B8, f32=True, accumulate="again"),
    _site("w1-wgrad-b2", "TN", F, D, B2, f32=True, accumulate="again"),
    _site("w2-wgrad-b1", "TN", D, F, B1, f32=True, accumulate="again"),
] + _ffn_sites() + _lowrank_sites() + _patch_sites()

# ---- (b) tile edges: K = 128 keeps the ring out of it ---------------------------------------------------------------------
EDGE_M = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257]
EDGE_N = [4, 8, 12, 16, 60, 64, 68, 124, 128, 132, 252, 260]
LAYOUT_DTYPES = [("NT", False), ("NT", True), ("NN", False), ("NN", True), ("TN", False), ("TN", True)]
EDGES = [Spec(f"edge-{lay}-{'f32' if f32 else 'bf16'}-{M}x{N}", lay, M, N, 128, f32=f32, tile=128, force=True, s=2)
         for lay, f32 in LAYOUT_DTYPES for M in EDGE_M for N in EDGE_N]

# ---- (c) nk K-steps through the two-stage LDS ring: prologue only, one steady step, ... at a ragged shape ----------------------
RING = [Spec(f"ring-{lay}-{'f32' if f32 else 'bf16'}-nk{nk}", lay, 200, 136, 64 * nk, f32=f32, tile=128, force=True, s=2)
        for lay, f32 in LAYOUT_DTYPES for nk in (1, 2, 3, 4, 5, 13)]

# ---- (d) contraction edges and split-K with the whole epilogue in the reduce kernel ---------------------------------------------
TN_K = [Spec(f"tn-K{K}-split{split}", "TN", 200, 136, K, f32=True, split=split, accumulate="again", tile=128, force=True, s=2)
        for K, split in TN_EDGES]


def _splitk_cases():
    out = []
    for M in (32, 130, 300):
        for split in (2, 3, 6, 8):        # K = 768: 12 K-steps; 8 splits of 2 steps leave the last two with none
            c = dict(M=M, N=192, K=768, split=split, tile=128, force=True)
            n = f"-M{M}-split{split}"
            out += [Spec("splitk-gelu-aux0-bf16" + n, "NT", bias=True, act="gelu", aux_mode=0, **c),
                    Spec("splitk-gelu-aux1-bf16" + n, "NT", bias=True, act="gelu", aux_mode=1, **c),
                    Spec("splitk-gelu-aux1-f32" + n, "NT", bias=True, act="gelu", aux_mode=1, f32=True, **c),
                    Spec("splitk-gelu-aux0-f32-drop" + n, "NN", bias=True, act="gelu", aux_mode=0, f32=True, drop=True, **c),
                    Spec("splitk-res-mod-f32" + n, "NT", f32=True, bias=True, res=True, res_mod=13, res_off=2, **c),
                    Spec("splitk-res-mod-bf16" + n, "NN", bias=True, res=True, res_mod=32, **c),
                    Spec("splitk-drop-bf16" + n, "NT", bias=True, drop=True, **c),
                    Spec("splitk-drop-res-f32" + n, "NN", f32=True, bias=True, res=True, drop=True, **c),
                    Spec("splitk-dgelu-colsum-aux0" + n, "NN", act="dgelu", aux_mode=0, colsum=True, **c),
                    Spec("splitk-dgelu-colsum-aux1-drop" + n, "NN", act="dgelu", aux_mode=1, colsum=True, drop=True, **c),
                    Spec("splitk-colsum-f32" + n, "NT", f32=True, bias=True, colsum=True, **c),
                    Spec("splitk-accumulate-nt" + n, "NT", f32=True, bias=True, accumulate="again", **c),
                    Spec("splitk-accumulate-nn" + n, "NN", f32=True, res=True, accumulate="first", colsum=True, **c)]
    return out


SPLITK = _splitk_cases()

# ---- (e) grids and batches whose workgroup count is not a multiple of 8: the XCD remap of gemm_kernel must stay a bijection -------
# NaN prefill: a tile no workgroup visits fails; accumulate on known values with column sums: a tile visited twice fails too
GRID_TILES = {1: (1, 1), 3: (3, 1), 7: (1, 7), 9: (3, 3), 15: (5, 3), 17: (17, 1)}


def _grid_cases():
    out = []
    for tiles, (tm, tn) in GRID_TILES.items():
        M, N = tm * 128 - 28, tn * 128 - 60
        for batch in (1, 3, 5):
            c = dict(M=M, N=N, K=128, batch=batch, tile=128, force=True, s=2)
            n = f"-{tiles}tiles-batch{batch}"
            out += [Spec("grid-nt-bias" + n, "NT", bias=True, **c),
                    Spec("grid-nn-accumulate-colsum" + n, "NN", f32=True, accumulate="first", colsum=True, **c),
                    Spec("grid-nn-bias-colsum-per-batch" + n, "NN", f32=True, bias=True, res=True, accumulate="first", colsum=True, **c),
                    Spec("grid-tn-split2" + n, "TN", f32=True, split=2, accumulate="again", **c)]
    return out


GRIDS = _grid_cases()

# ---- (f) strided views ----------------------------------------------------------------------------------------------------
VIEWS = [
    Spec("view-lda-nt", "NT", 200, 136, 192, lda_slice=True, tile=128, force=True, s=2),                 # e.g. the q columns of a [rows, 3 d] tensor
    Spec("view-lda-nn", "NN", 200, 136, 192, f32=True, lda_slice=True, tile=128, force=True, s=2),
    Spec("view-ldc-bf16", "NT", 200, 136, 192, bias=True, ldc_pad=8, tile=128, force=True, s=2),
    Spec("view-ldc-f32", "NN", 200, 136, 192, f32=True, res=True, ldc_pad=4, tile=128, force=True, s=2),
    Spec("view-ldc-tn-accumulate", "TN", 200, 136, 193, f32=True, ldc_pad=12, accumulate="again", tile=128, force=True, s=2),
    Spec("view-ldc-ldaux-gelu", "NT", 200, 136, 192, bias=True, act="gelu", aux_mode=1, ldc_pad=8, ldaux_pad=4, tile=128, force=True),
    Spec("view-ldc-ldaux-gelu-f32", "NT", 200, 136, 192, f32=True, bias=True, act="gelu", aux_mode=0, ldc_pad=4, ldaux_pad=12, tile=128, force=True),
    Spec("view-ldaux-dgelu", "NN", 200, 136, 192, act="dgelu", aux_mode=0, colsum=True, ldaux_pad=8, tile=128, force=True),
    Spec("view-ldc-ldaux-splitk", "NT", 130, 136, 768, bias=True, act="gelu", aux_mode=1, split=3, ldc_pad=8, ldaux_pad=8, tile=128, force=True),
    Spec("view-ldc-remap-splitk", "NT", 96, 136, 768, f32=True, bias=True, res=True, res_mod=16, res_off=1, seg=(16, 1, 1), split=4, ldc_pad=4,
         tile=128, force=True),
    Spec("view-batched-ldc-ldaux", "NT", 130, 72, 128, bias=True, act="gelu", aux_mode=1, batch=3, ldc_pad=8, ldaux_pad=4, tile=128, force=True),
    Spec("view-batched-drop", "NT", 130, 72, 128, f32=True, bias=True, res=True, drop=True, batch=3, tile=128, force=True, s=2),
    Spec("view-batched-remap", "NT", 48, 72, 128, f32=True, bias=True, res=True, res_mod=16, res_off=1, seg=(16, 1, 1), batch=3, tile=128, force=True, s=2),
]

ALL = SITES + EDGES + RING + TN_K + SPLITK + GRIDS + VIEWS


# ---- which kernels a case launches: a mirror of use_big_tile() and of the small branch of xvit_gemm() in csrc/gemm.hip --------------
def _uses_big_tile(s):
    if s.force or s.M < 256 or s.N < 256:
        return False
    return ((s.M + 255) // 256) * ((s.N + 255) // 256) * max(s.batch, 1) * max(s.split, 1) > 128


def _launches(s):
    t = {"NT": "false, false", "NN": "false, true", "TN": "true, true"}[s.layout]
    return {f"gemm_kernel<{t}>"} | ({"splitk_epilogue_kernel"} if s.split > 1 else set())


def _launched_in_xvit_gemm():
    src = open(GEMM_HIP).read()
    body = src[src.index('extern "C" int xvit_gemm('):]
    body = body[:body.index('return check_launch("xvit_gemm")')]
    found = {"gemm_kernel<%s>" % ", ".join(a.strip() for a in m.split(",")) for m in re.findall(r"\blaunch_small<([^>]*)>\(", body)}
    if re.search(r"\blaunch_splitk_reduce\(", body):
        found.add("splitk_epilogue_kernel")
    return found


def test_cases_cover_every_small_kernel_launch():
    """Every gemm_kernel instantiation xvit_gemm launches and the split-K reduce behind it are reached by a case of this file (the
    production sites alone reach them too), and the mirror above names nothing gemm.hip does not launch."""
    launched = _launched_in_xvit_gemm()
    assert "splitk_epilogue_kernel" in launched and len(launched) > 2, f"could not parse the launches of xvit_gemm: {launched}"
    for group, name in ((ALL, "case"), (SITES, "production site")):
        claimed = set().union(*(_launches(s) for s in group))
        assert not launched - claimed, f"launched by xvit_gemm but reached by no small-kernel {name}: {sorted(launched - claimed)}"
        assert not claimed - launched, f"the mirror of xvit_gemm's dispatch is out of date: {sorted(claimed - launched)}"


def test_no_case_runs_on_the_big_kernel():
    """The production sites run under the automatic tile choice: none of them may be routed to the 256x256 kernel (batch and split
    included in the block count), or this file would silently test the other kernel.  Every other case forces gemm_tile = 1."""
    big = [s.name for s in SITES if s.force or _uses_big_tile(s)]
    assert not big, f"sites that would not reach gemm_kernel under the automatic choice: {big}"
    unforced = [s.name for s in ALL if s not in SITES and not s.force]
    assert not unforced, f"cases that rely on the automatic choice without being in SITES: {unforced}"
    assert all(s.tile == 128 for s in ALL)
    names = [s.name for s in ALL]
    assert len(set(names)) == len(names), "duplicate case names"
    # every listed M and N with every layout and output type
    for lay, f32 in LAYOUT_DTYPES:
        got = {(s.M, s.N) for s in EDGES if s.layout == lay and s.f32 == f32}
        assert {m for m, _ in got} == set(EDGE_M) and {n for _, n in got} == set(EDGE_N)


# ---- the GPU side -------------------------------------------------------------------------------------------------------
def _ids(specs):
    return [s.name for s in specs]


@pytest.mark.gpu
@pytest.mark.parametrize("site", SITES, ids=_ids(SITES))
def test_small_kernel_site(site):
    """One GEMM of the model that lands on the 128x128 kernel under the automatic tile choice, every element checked; the cases
    without column sums (atomics) run twice and must repeat bit for bit."""
    check_site(site, repeat=not site.colsum)


@pytest.mark.gpu
@pytest.mark.parametrize("layout,f32,M", [(lay, f32, M) for lay, f32 in LAYOUT_DTYPES for M in EDGE_M],
                         ids=[f"{lay}-{'f32' if f32 else 'bf16'}-M{M}" for lay, f32 in LAYOUT_DTYPES for M in EDGE_M])
def test_tile_edges(layout, f32, M):
    """M rows against every N of EDGE_N: 1 .. 257 rows and 4 .. 260 columns around the 16 / 64 / 128 boundaries of fragment, wave and tile."""
    for s in EDGES:
        if (s.layout, s.f32, s.M) == (layout, f32, M):
            check_site(s)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RING, ids=_ids(RING))
def test_ring_prologue_and_drain(case):
    check_site(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TN_K, ids=_ids(TN_K))
def test_tn_contraction_edges(case):
    """K = 64 n + 1 and 64 n + 63, trailing splits without a K-step, splits that start beyond K (and accumulate on top)."""
    check_site(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPLITK, ids=_ids(SPLITK))
def test_split_k_reduce_epilogue(case):
    """split_k > 1: gemm_kernel writes partial tiles, splitk_epilogue_kernel runs the whole epilogue.  C is NaN before the call (the
    result must not depend on it unless accumulate is set), and so is the block the workspace comes from."""
    check_site(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRIDS, ids=_ids(GRIDS))
def test_grids_not_a_multiple_of_8(case):
    check_site(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", VIEWS, ids=_ids(VIEWS))
def test_strided_views(case):
    """lda > K, ldc > N, ldaux > N: the columns >= N of the wider destination keep what they held."""
    check_site(case)
