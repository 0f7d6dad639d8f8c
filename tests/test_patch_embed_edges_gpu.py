"""GPU: the fused patch embedding (xvit_patch_embed_fwd / _wgrad / _dgrad, the gather paths of csrc/gemm.hip) bit for bit at the small
patch grids and split edges where its index arithmetic branches (tests/_pe_check.py: the cases, the exact CPU reference, the launch
through the raw C entry points with every stride free, the element-wise comparison; tests/test_pe_gate_cpu.py shows the comparison
has teeth and pins the classes the case table reaches).

Every case runs at 0.26 to 2.1 Mvoxel: mode 2 (wave-uniform K-step offsets) with every k-row pairing 64 / Dn = 1 .. 64, Hn > 1 and two
w-steps per h-row, uneven and non-positive splits; mode 3 (per-lane token placement by multiply-high division) with divisors of 1, 1 to
65 tokens per sample, K-steps over several samples and modalities, K % 64 = 0 and != 0, an empty split and splits behind K; cls_rows = 0
in both.  No tolerance anywhere: the operands make every fp32 sum exact in any order."""
import ctypes as C

import pytest
import torch

import _pe_check as P
from _util import dev

pytestmark = pytest.mark.gpu

CASE_PARAMS = [pytest.param(c, id=c.name) for c in P.CASES]


def _lib():
    from xvit import _lib
    return _lib.load()


def _last_error():
    return _lib().xvit_last_error_string().decode(errors="replace")


@pytest.mark.parametrize("case", CASE_PARAMS)
def test_forward_and_wgrad_bit_exact(case):
    L = _lib()
    g = P.geom(case)
    assert L.xvit_patch_embed_supported(C.byref(g), case.d) == 1, f"{case.tag}: the fused kernels refuse this geometry"
    k = P.classify(case)
    need = L.xvit_patch_embed_wgrad_workspace_bytes(C.byref(g), case.d)
    assert need % (4 * case.d * case.pd) == 0 and need // (4 * case.d * case.pd) == k["split"] > 1, f"{case.tag}: {need} bytes of workspace, restated split {k['split']}"
    ref = P.reference(case)
    D = P.device_operands(case, ref)
    out = P.launch(case, ref, D)
    P.compare(case, ref, out)
    again = P.launch_wgrad(case, ref, D)
    assert torch.equal(out["dW"].view(torch.int32), again["dW"].view(torch.int32)), f"{case.tag}: dW differs between two runs"
    P.compare(case, ref, again)


@pytest.mark.parametrize("case", [pytest.param(P.BY_NAME[n], id=n) for n in ("dn64-h2-w2", "m3-9tok-M1", "m3-1tok", "m3-2tok", "m3-1tok-cls0")])
def test_forward_residual_paths(case):
    """The forward without bias, without pos and without either, under both placements of the residual load (gemm_res_prefetch): a
    mode-2 case, one with a ragged last row tile, and the three whose pos table has fewer rows (2, 3, 1) than an epilogue step."""
    from xvit import ops
    ref = P.reference(case)
    D = P.device_operands(case, ref)
    try:
        for prefetch in (0, 1):
            ops.set_option("gemm_res_prefetch", prefetch)
            for bias, pos in ((True, True), (False, False), (True, False), (False, True)):
                P.compare(case, ref, P.launch_fwd(case, ref, D, bias, pos), bias, pos)
    finally:
        ops.set_option("gemm_res_prefetch", 0)


def test_refusals_launch_nothing():
    """A workspace one byte short, leading dimensions off their multiple and a pointer 8 bytes off its alignment: a nonzero return, a
    message, and destinations that still hold their prefill."""
    case = P.BY_NAME["dn8-uneven"]
    ref = P.reference(case)
    D = P.device_operands(case, ref)
    before = P.buffers(case)
    B = {k: v.to(dev()) for k, v in before.items()}
    need = P.workspace_bytes(case)

    def refused(rc, word):
        msg = _last_error()
        assert rc != 0 and word in msg, f"rc {rc}, message {msg!r}"

    refused(P.call_wgrad(case, D, B["dW"], B["ws"], ws_bytes=need - 1), "workspace")
    refused(P.call_wgrad(case, D, B["dW"], B["ws"], lddx=case.d + 4), "leading dimension")
    refused(P.call_wgrad(case, D, B["dW"], B["ws"], dx_off=8), "aligned")
    refused(P.call_fwd(case, D, B["x"], ldw=case.pd + 4), "leading dimension")
    refused(P.call_fwd(case, D, B["x"], x_off=8), "aligned")
    torch.cuda.synchronize()
    for k, v in B.items():
        assert torch.equal(v.cpu().view(torch.int32), before[k].view(torch.int32)), f"a refused call wrote to {k}"
    # and the same buffers take the accepted calls
    assert P.call_fwd(case, D, B["x"]) == 0 and P.call_wgrad(case, D, B["dW"], B["ws"]) == 0
    torch.cuda.synchronize()
    P.compare(case, ref, {k: v.cpu() for k, v in B.items()})


@pytest.mark.parametrize("case", CASE_PARAMS)
def test_dgrad_bit_exact(case):
    """xvit_patch_embed_dgrad's scatter epilogue divides by ntok, Dn, Wn and nb with the same fast_div: the check of
    tests/test_patch_embed_dgrad_gpu.py over this table (Dn = 1, Wn = 1, P = 1, cls_rows = 0 among it)."""
    P.check_dgrad(case.B, case.M, case.vol, case.patch, case.d, case.cls, seed=case.seed + 20)
