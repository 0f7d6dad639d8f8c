"""The fp32 residual of the 256x256 GEMM's plain bias + residual epilogue, loaded one region (16 rows) ahead of the stores
(csrc/gemm.hip: LoadCursor, big_epi_issue_res), at the sizes where a look-ahead cursor can go wrong: M just past a 256-row
tile, a 16-row region or a 64-row LDS pass, a ragged column tile, one and three K-steps, a residual row modulo that wraps
inside a region, at a region seam and across wave tiles, output segments, a batch stride.  The epilogues that keep the load
in their body (dropout, accumulate, split-K) run next to it and must stay exact.

tests/_gemm_check.py supplies exact operands, compares every output element bit for bit with the CPU reference and keeps
NaN / a sentinel around the output.  gemm_tile = 2 sends these small grids to the 256x256 kernel.
"""
import pytest
import torch

from _gemm_check import Spec, _options, check_site
from _util import assert_exact, dev, exact_grid, exact_operands

gpu = pytest.mark.gpu


def _check(spec):
    with _options(gemm_tile=2):
        check_site(spec)


@gpu
@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("N", [260, 768])
@pytest.mark.parametrize("M", [257, 273, 300, 321, 511])
@pytest.mark.parametrize("layout", ["NT", "NN"])
def test_f32_bias_residual(layout, M, N, K):
    _check(Spec("res-prefetch", layout, M, N, K, f32=True, bias=True, res=True))


@gpu
@pytest.mark.parametrize("res_off", [0, 3])
@pytest.mark.parametrize("res_mod", [5, 19, 513])
def test_residual_row_modulo(res_mod, res_off):
    """Residual row = res_off + row % res_mod: 5 wraps inside a lane's 4-row step and several times per region, 19 at and
    between region seams, 513 once, across the wave tiles of the second row tile (M = 600)."""
    _check(Spec("res-prefetch-mod", "NT", 600, 768, 64, f32=True, bias=True, res=True, res_mod=res_mod, res_off=res_off))


@gpu
def test_output_segments_with_residual():
    _check(Spec("res-prefetch-seg", "NT", 300, 260, 64, f32=True, bias=True, res=True, seg=(100, 3, 2), ldc_pad=8))


@gpu
def test_batch_with_residual():
    _check(Spec("res-prefetch-batch", "NT", 300, 260, 64, f32=True, bias=True, res=True, batch=2))


@gpu
@pytest.mark.parametrize("extra", [dict(drop=True), dict(accumulate="first"), dict(split=3)], ids=["dropout", "accumulate-first", "split3"])
def test_in_body_paths_stay_exact(extra):
    """Dropout, accumulate and split-K (NaN workspace: no residual read may replace a partial sum) keep the load in the body."""
    _check(Spec("res-in-body", "NT", 300, 260, 192, f32=True, bias=True, res=True, **extra))


@gpu
def test_patch_embed_forward_with_position_residual():
    """The PERM copy: the fused patch embedding on the smallest supported geometry with two samples (2 x 1025 rows: CLS
    rows, a position row modulo of 1025 that wraps mid-tile, a ragged last row tile) against the stand-alone patchify and
    an fp32 matmul of the same bf16 operands.  Exact operands: the reference is exact in any summation order."""
    from xvit import ops
    B, M, vol, patch, d = 2, 1, (64, 64, 64), (4, 8, 8), 256
    pd, P = 256, 1024
    unit = 2.0 ** -4
    img = exact_operands((B, M, 1) + vol, 21, 2).to(dev(), torch.bfloat16)
    w = exact_operands((d, pd), 22, 2)
    bias, pos = exact_grid((d,), 23, unit, 32), exact_grid((1 + P, d), 24, unit, 256)
    assert ops.patch_embed_supported(img, patch, d)
    x = ops.patch_embed_fwd(img, patch, w.to(dev(), torch.bfloat16), bias.to(dev()), pos.to(dev()))
    patches = ops.patchify(img, patch, pad_cls_row=True).reshape(-1, pd).float().cpu()     # zero CLS rows
    ref = patches @ w.T + bias + pos.repeat(B * M, 1)
    assert_exact(x, ref, "patch embedding forward")


@gpu
@pytest.mark.parametrize("layout,M,N,K", [("NT", 257, 260, 64), ("NN", 321, 768, 192), ("NT", 511, 768, 192)])
def test_switch_changes_no_bit(layout, M, N, K):
    """gemm_res_prefetch = 0 (one region ahead) and 1 (in the body) on random normal operands and residual: the same C."""
    g = torch.Generator().manual_seed(31)
    a = torch.randn(M, K, generator=g).to(dev(), torch.bfloat16)
    b = torch.randn((N, K) if layout == "NT" else (K, N), generator=g).to(dev(), torch.bfloat16)
    bias, res = torch.randn(N, generator=g).to(dev()), torch.randn(M, N, generator=g).to(dev())
    out = []
    for v in (0, 1):
        with _options(gemm_tile=2, gemm_res_prefetch=v) as ops:
            C = torch.full((M, N), float("nan"), device=dev())
            ops.gemm(ops.NT if layout == "NT" else ops.NN, a, b, C, bias=bias, residual=res)
            out.append(C.cpu())
    assert not torch.isnan(out[0]).any()
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)), f"{int((out[0] != out[1]).sum())} elements differ"


def test_switch_values():
    """Host only: 0 and 1 are taken, anything else is refused with the reason."""
    from xvit import _lib
    lib = _lib.load()
    try:
        assert lib.xvit_set_option(b"gemm_res_prefetch", 1) == 0
        assert lib.xvit_set_option(b"gemm_res_prefetch", 2) < 0 and b"gemm_res_prefetch" in lib.xvit_last_error_string()
        assert lib.xvit_set_option(b"gemm_res_prefetch", -1) < 0
    finally:
        assert lib.xvit_set_option(b"gemm_res_prefetch", 0) == 0
