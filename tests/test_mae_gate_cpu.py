"""CPU: the teeth of the loss gates in tests/_mae_check.py (derivation there, next to the constants).

For every bounded quantity (mean, rstd, row_loss, loss_seq, loss, dpred) and at every shape, dtype pair and norm_pix setting that
tests/test_mae_kernels_gpu.py runs on the GPU:
  - the float64 reference with ONE element moved by 4x its bound is rejected, in that quantity and in no other;
  - an fp32 NumPy evaluation of the same formulas with every sum taken sequentially from the far end (not the kernel's order) is
    accepted: the reference arithmetic alone stays inside the bounds.
And the reason for the two-pass variance: on the patch whose mean is 2000x its standard deviation a one-pass fp32 sum v^2 - pd mean^2
misses the rstd bound at pd = 64 and pd = 512 by orders of magnitude."""
import numpy as np
import pytest

import _mae_check as C

CASES = [(shape, vb, pb, norm) for shape in C.LOSS_SHAPES for vb in (False, True) for pb in (False, True) for norm in (True, False)]


def _setup(shape, vol_bf16, pred_bf16, norm):
    case = C.loss_case(shape, vol_bf16, pred_bf16)
    img = np.nan_to_num(case["img"], nan=0.0)          # the reference reads the dropped patches only; NaN elsewhere is the GPU test's business
    ref = C.loss_ref64(case["pred"], img, case["patch"], case["drop_idx"], norm, C.LOSS_G)
    return case, img, ref, C.loss_bounds(ref, pred_bf16)


@pytest.mark.parametrize("shape,vol_bf16,pred_bf16,norm", CASES)
def test_another_fp32_order_is_accepted_and_a_4x_error_is_rejected(shape, vol_bf16, pred_bf16, norm):
    case, img, ref, bounds = _setup(shape, vol_bf16, pred_bf16, norm)
    assert not np.isnan(C.patch_rows(case["img"], case["patch"], case["drop_idx"])).any()      # the NaN sits in the kept patches only
    alt = C.loss_fp32_alt(case["pred"], img, case["patch"], case["drop_idx"], norm, C.LOSS_G, pred_bf16)
    got = C.violations(alt, ref, bounds)
    for k, (bad, worst) in got.items():
        print(f"mae gate {shape} vol_bf16={vol_bf16} pred_bf16={pred_bf16} norm={norm} {k}: worst |err| / bound = {worst:.3e}")
        assert bad == 0, (k, bad, worst)
    exact = {k: ref[k].copy() for k in C.BOUNDED}
    assert all(v == (0, 0.0) for v in C.violations(exact, ref, bounds).values())
    rng = np.random.default_rng(7)
    for k in C.BOUNDED:
        if not norm and k in ("mean", "rstd"):
            continue                                    # (0, 1) exactly: the bound is the denormal floor, checked below
        moved = {q: ref[q].copy() for q in C.BOUNDED}
        flat = moved[k].reshape(-1)
        i = int(rng.integers(flat.size))
        flat[i] += 4.0 * bounds[k].reshape(-1)[i] * (1 if i % 2 else -1)
        res = C.violations(moved, ref, bounds)
        assert res[k][0] == 1 and 3.9 < res[k][1] < 4.1, (k, res[k])
        assert all(res[q][0] == 0 for q in C.BOUNDED if q != k)
    if not norm:
        assert float(bounds["mean"].max()) <= 2 * C.TINY and float(bounds["rstd"].max()) <= 2 * C.TINY
        moved = {q: ref[q].copy() for q in C.BOUNDED}
        moved["rstd"][0] = np.float32(1.0) + np.float32(2.0 ** -23)
        assert C.violations(moved, ref, bounds)["rstd"][0] == 1


@pytest.mark.parametrize("shape", ["pd64", "pd512"])
def test_one_pass_variance_misses_the_rstd_bound_on_the_offset_patch(shape):
    case, img, ref, bounds = _setup(shape, False, False, True)
    r = case["special"]["offset"]
    v = C.patch_rows(img.astype(np.float32), case["patch"], case["drop_idx"])[r]
    assert abs(float(v.mean())) >= 1000 * float(v.std())
    pd = np.float32(v.size)
    mean = C._seq_sum_f32(v) / pd
    var1 = (C._seq_sum_f32(v * v) - pd * mean * mean) / (pd - np.float32(1))          # one pass: sum v^2 - pd mean^2
    rstd1 = np.float32(1.0) / np.sqrt(np.maximum(var1, np.float32(0)) + np.float32(C.EPS), dtype=np.float32)
    err = abs(float(rstd1) - ref["rstd"][r])
    print(f"mae gate {shape}: one-pass rstd error {err:.3e}, bound {bounds['rstd'][r]:.3e}, two-pass bound / rstd {bounds['rstd'][r] / ref['rstd'][r]:.3e}")
    assert err > 4 * bounds["rstd"][r]


def test_nan_is_rejected():
    case, img, ref, bounds = _setup("pd64", False, False, True)
    moved = {q: ref[q].copy() for q in C.BOUNDED}
    moved["row_loss"][3] = np.nan
    assert C.violations(moved, ref, bounds)["row_loss"][0] == 1
