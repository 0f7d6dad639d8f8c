"""The gate of the low-rank fusion kernels (tests/_head_check.py) has teeth, on the CPU.

(a) C_exp.  The float32 mirror of cls_softmax_kernel (`sm_mirror`) runs over the GPU tests' own scores; C_exp must be the power of two at or above
    4 x its largest need, and the table in _head_check's docstring is re-measured here.
(b) Every derived bound of the float64 tier is checked against torch's own fp32 arithmetic on the inputs the GPU file uses (the mirrors'
    `*_written` windows go through the very `*_check` the device's windows go through), and the exact tier's mirrors match bit for bit.
(c) Planted faults.  Each starts from the windows a correct launch would leave, plants ONE defect, and states two outcomes: the new check names it
    (always), and whether the old gate would have seen it on the same data.  The old gate is tests/test_head_linear_gpu.py's: `_util.rel` < 2e-6 on
    the fp32 products, 3e-3 on e, 1e-6 on rz and p', 1e-5 on ds and stat[2], torch.equal on the bf16 copies and the kept weights, a zero maximum over
    the padding; tests/test_kernels_gpu.py's 3e-3 on dhn.  Nothing was bent to make it miss: where it sees the fault the table says so (it
    never ran at that shape or stride), and both outcomes are asserted.

      fault                                                        new check   old gate (same data)
      head_rows: row 32 stored as a copy of row 31 (B = 33)        caught      0.24: seen
      head_rows: one element of the last row an ulp off            caught      2.1e-10: not seen
      head_rows: a padding head of the bf16 copy not zeroed        caught      seen (the maximum over the padding is NaN)
      head_rows: a store into the gap between two heads            caught      not seen (it never looks between the heads)
      head_rows: row B of out stored (the row < B test dropped)    caught      not seen (row B is outside the tensor it compares)
      head_rows: a padding head of row B zeroed in the bf16 copy   caught      not seen
      head_cols: the last K-quarter missing                        caught      0.50: seen
      head_cols: head 0 of row 0 with head 1's row scale           caught      6.9e-3: seen
      head_cols: bias_scale ignored                                caught      0.28: seen
      head_cols: a store one element past ldo                      caught      not seen
      head_cols: the bf16 copy truncated, not rounded              caught      seen (torch.equal)
      head_wgrad: the padded lanes of the tail keep their scale    caught      1.1: seen
      softmax: the mask indexed with 16 in place of H (H = 3)      caught      seen (torch.equal on the kept weights)
      softmax: rz from the unrounded weights                       caught      7.9e-5 on the 1e-6 gate: seen
      softmax: e at the arg-max row one bf16 step below 1          caught      1.4e-4 on the 3e-3 gate: not seen
      softmax: a padding column of e holds -0                      caught      not seen (|-0| = 0)
      softmax_bwd: wave 5's partial missing from dsum (N = 513)    caught      4.3e-2 on the 1e-5 gate: seen
      softmax_bwd: p' without 1 / (1 - p)                          caught      0.50: seen
      softmax_bwd: the halves of coef swapped                      caught      5.8: seen
      kv_dgrad: coefficient j = 2 H - 1 dropped (H = 5)            caught      0.33: seen
      kv_dgrad: dhn truncated to bf16, not rounded                 caught      3.3e-3 on the 3e-3 gate: seen (RNE alone is 1.7e-3)
"""
import math
import re

import pytest
import torch

import _head_check as X
from _cls_check import pow2_at_or_above
from _util import note, rel

BS, HS = (1, 31, 32, 33, 65), (1, 3, 12, 16)


def _caught(what, fn, *names):
    with pytest.raises(AssertionError) as e:
        fn()
    msg = str(e.value)
    print(f"caught: {what}: {msg[:400]}")
    for n in names:
        assert n in msg, f"{what}: the message does not name {n!r}: {msg}"
    return msg


def _old(what, value, tol, sees):
    print(f"old gate on {what}: {value:.3e} against {tol:g}")
    assert (not value < tol) == sees, f"{what}: old gate {value:.3e} against {tol:g}, recorded as {'seen' if sees else 'not seen'}"


# ---------------------------------------------------------------------------------------------------------------- (a) C_exp
def test_exp_mirror_need_sets_the_constant():
    needs = {}
    for N in X.SM_N:
        for H in X.SM_H:
            for c in X.sm_configs(N, H):
                if c.p > 0:
                    continue
                s = X.sm_scores(c)
                e32 = X.sm_mirror(c, s)[0]
                needs[c.kind] = max(needs.get(c.kind, 0.0), X.exp_need32(e32, *X.exp_ref(c, s)))
    for k, v in needs.items():
        note(f"mirror:need_exp:{k}", v)
        print(f"mirror need C_exp on {k:9s}: {v:.2f}")
    need = max(needs.values())
    # equal scores and the rows a dominant one pushes below the fp32 range need nothing.  The largest need sits at weights just below 1 (|a| -> 0, so the
    # argument term grants nothing): there a correctly rounded exp2 errs by at most half an ulp, 2^-25 = 0.5 x 2^-24 of the weight.  A weight further
    # down has a larger half-ulp (up to 1.0 x 2^-24 of it just above 1/2), but there 3 ln 2 |a| has grown past it: 1 / m - 2.08 (1 - log2 m) <= 0.5 for
    # a weight m / 2, m in [1, 2].  So the need of any host whose exp2 is correctly rounded on these arguments is in (0.25, 0.5], whatever its last digits.
    assert needs["equal"] == 0.0 and needs["dominant"] == 0.0, needs
    assert 0.25 < need <= 0.5, f"the host's exp2 is off by more than half an ulp on these arguments (need {need:.4f}): that is about this machine's torch, not the kernels"
    assert X.C_EXP == pow2_at_or_above(4 * need) == 2.0, f"mirror need {need:.3f}, C_exp {X.C_EXP:g}"


# ---------------------------------------------------------------------------------------------------------------- the mirror of the geometry
def test_geometry_mirror_reaches_every_path():
    assert sorted(set((i & 3) + 8 * (i >> 2) + 4 * hl for i in range(16) for hl in range(2))) == list(range(32))
    assert [X.tile_slot(r) for r in (0, 3, 4, 8, 31)] == [(0, 0), (3, 0), (0, 1), (4, 0), (15, 1)]
    assert [X.cols_kq(64 * H) for H in HS] == [16, 48, 192, 256]                                       # H = 1: two 8-deep steps, the unroll-4 remainder
    assert X.sm_owner(0, 0) == (0, 0, 0) and X.sm_owner(63, 15) == (1023, 15, 0) and X.sm_owner(64, 2) == (2, 0, 1) and X.sm_owner(4096, 0)[2] == 64
    assert [X.xkv_geometry(1, N, 4)[:2] for N in X.KV_N] == [(1, 1), (1, 31), (2, 32), (2, 32), (3, 22), (5, 26)]
    assert [X.xkv_geometry(3, N, 4)[:2] for N in X.KV_N] == [(1, 1), (1, 31), (2, 32), (2, 32), (3, 22), (5, 26)]
    assert X.xkv_geometry(130, 600, 1) == (8, 75, 8) and X.xkv_geometry(126, 1025, 12) == (9, 114, 24)
    assert [X.xkv_geometry(1, 1, H)[2] for H in X.KV_H] == [8, 8, 16, 16, 24, 24, 32, 32]
    assert X.sm_dominant_rows(4097, 2) == [4096, 4095] and X.sm_dominant_rows(15, 2) == [14, 14]


# ---------------------------------------------------------------------------------------------------------------- (b) the mirrors pass
WRITTEN = {"head_rows": X.rows_written, "head_cols": X.cols_written, "head_wgrad": X.wgrad_written, "head_bias_grad": X.bias_written}


def _mirror(c):
    operands, oracle, _, check = X.KERNELS[c.kernel]
    o = operands(c)
    ora = oracle(c, o)
    wins = WRITTEN[c.kernel](c, o)
    check(c, wins, ora)
    return o, ora, wins


@pytest.mark.parametrize("H", HS)
def test_head_mirrors_pass_every_case(H):
    """torch's fp32 einsum stays inside the float64 tier's bounds on the GPU file's random operands and equals the exact tier's oracle."""
    for B in BS + (64,):
        cs = X.wgrad_configs(B, H) + (X.rows_configs(B, H) + X.cols_configs(B, H) if B != 64 else [])
        for c in cs:
            if c.tier == "random" or B in (1, 33):
                _mirror(c)
    for B in (1, 65):
        for tier in ("exact", "random"):
            _mirror(X.bias_case(B, 64 * H, tier=tier))


@pytest.mark.parametrize("N", X.SM_N)
def test_softmax_mirrors_pass_every_case(N):
    for H in X.SM_H:
        for c in X.sm_configs(N, H):
            s = X.sm_scores(c)
            keep = X.sm_keep(c) if c.p > 0 else None
            w0 = X.sm_written(X.sm_case(c.B, H, N, c.kind, lds=c.lds, lde=c.lde), s) if c.p > 0 else None
            X.sm_check(c, s, X.sm_written(c, s, keep), keep, w0)
        for c in X.bw_configs(N, H):
            keep = X.sm_keep(c) if c.p > 0 else None
            i = X.bw_exact_inputs(c)
            X.bw_check(c, X.bw_written(c, i, keep), X.bw_oracle(c, i, keep))
        for p, seed in ((0.0, 0), (0.25, 5)):
            f = X.sm_case(c.B, H, N, "random", p=p, seed=seed)
            keep = X.sm_keep(f) if p > 0 else None
            _, e, _, stat = X.sm_mirror(f, X.sm_scores(f), keep)
            r = X.bw_case(c.B, H, N, lde=16, ldp=24, ldb=X.sm_lde(H, 1), p=p, seed=seed, tier="random")
            i = {"e": e, "rz": stat[0], "dp": X.bw_random_dp(r)}
            X.bw_check(r, X.bw_written(r, i, keep), X.bw_oracle(r, i, keep))


def test_kv_mirrors_pass_every_case():
    for N in X.KV_N:
        for H in X.KV_H:
            for c in X.kv_configs(N, H):
                o = X.kv_operands(c)
                X.kv_check(c, X.kv_written(c, o), X.kv_oracle(c, o))
    c = X.kv_case(130, 1, 600, wide=True)
    o = X.kv_operands(c)
    X.kv_check(c, X.kv_written(c, o), X.kv_oracle(c, o))


# ---------------------------------------------------------------------------------------------------------------- (c) planted faults
def _ulp_up(t, idx):
    t[idx] = torch.nextafter(t[idx], torch.tensor(math.inf, dtype=t.dtype))


def _trunc_bf16(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def test_rows_row_32_as_a_copy_of_row_31_is_named():
    c = X.rows_case(33, 3, "T", ob=16)
    o, ora, wins = _mirror(c)
    v = X.sview(wins["out"], *c._o)
    v[32] = v[31].clone()
    _caught("row 32 = row 31", lambda: X.rows_check(c, wins, ora), "head_rows_kernel", "32x32 tile (1, ", "sample 32")
    _old("row 32 = row 31", rel(v, ora["out"]), 2e-6, True)


def test_rows_one_ulp_in_the_last_row_is_named():
    c = X.rows_case(33, 3, "P", ob=3, wide=True)
    o, ora, wins = _mirror(c)
    v = X.sview(wins["out"], *c._o)
    _ulp_up(v, (32, 2, 191))
    _caught("one ulp in the last row", lambda: X.rows_check(c, wins, ora), "sample 32, head 2, column 191", "32x32 tile (1, 5)", "lane 31, accumulator 0")
    _old("one ulp in the last row", rel(v, ora["out"]), 2e-6, False)


def test_rows_padding_head_left_unwritten_is_named():
    c = X.rows_case(33, 3, "T", ob=16)
    o, ora, wins = _mirror(c)
    v = X.sview(wins["ob"], *c._ob)
    v[32:, 3, 32:64] = math.nan                                      # one block of the padding head 3 never ran
    _caught("padding head not zeroed", lambda: X.rows_check(c, wins, ora), "padding head 3", "padding heads 3 .. 15")
    assert not float(v[:, 3:].float().abs().max()) == 0.0            # the old test's maximum over the padding sees it


def test_rows_store_between_two_heads_is_named():
    c = X.rows_case(33, 3, "P", ob=0, wide=True)
    o, ora, wins = _mirror(c)
    wins["out"][c._o[1][1] * 2 - 1] = 0.0                             # the last float of the gap behind head 1 of sample 0
    _caught("a store between two heads", lambda: X.rows_check(c, wins, ora), "in a gap the strides leave")
    _old("a store between two heads", rel(X.sview(wins["out"], *c._o), ora["out"]), 2e-6, False)


@pytest.mark.parametrize("layout,wide", [("T", False), ("T", True), ("P", True)])
def test_rows_row_B_stored_is_named(layout, wide):
    """A lane that forgot `row < B`: row B of every head is sentinel (packed slab: of the last head, the others' row B is the next head's row 0)."""
    c = X.rows_case(33, 3, layout, ob=16, wide=wide)
    o, ora, wins = _mirror(c)
    shape, strides, off = c._o
    h = 2 if (layout, wide) == ("T", False) else 0
    wins["out"][off + 33 * strides[0] + h * strides[1] + 100] = 0.5
    _caught("row B of out stored", lambda: X.rows_check(c, wins, ora), f"(sample 33, head {h}, column 100)", "row 33 of a destination of 33 rows")
    _old("row B of out stored", rel(X.sview(wins["out"], *c._o), ora["out"]), 2e-6, False)


@pytest.mark.parametrize("wide", [False, True])
def test_rows_padding_head_of_row_B_zeroed_is_named(wide):
    """The `row < B` test of the padding-head branch: heads H .. 15 of row B must keep the sentinel."""
    c = X.rows_case(33, 3, "T", ob=16, wide=wide)
    o, ora, wins = _mirror(c)
    shape, strides, off = c._ob
    for h in (3, 15):
        w = {k: t.clone() for k, t in wins.items()}
        w["ob"][33 * strides[0] + h * strides[1]:33 * strides[0] + h * strides[1] + 32] = 0.0
        _caught("padding head of row B zeroed", lambda: X.rows_check(c, w, ora), "out_bf16", f"(sample 33, head {h}, column 0)", "row 33 of a destination of 33 rows")
    # every store a lane without the test could make lies inside the allocation, for every case the GPU file launches
    for B in BS:
        for H in HS:
            for c in X.rows_configs(B, H):
                for (shape, strides, off), buf in ((c._o, X.rows_windows(c)["out"]),) + (((c._ob, X.rows_windows(c)["ob"]),) if c._ob else ()):
                    assert off + B * strides[0] + (shape[1] - 1) * strides[1] + shape[2] - 1 < buf.numel() - X.GUARD + 1, c


@pytest.mark.parametrize("fault,sees", [("quarter", True), ("neighbour_scale", True), ("no_bias_scale", True)])
def test_cols_fault_is_named(fault, sees):
    c = X.cols_case(33, 3, rs="pow2", bias=True, bsc=True, bf=True, wide=True)
    o, ora, _ = _mirror(c)
    wins = X.cols_written(c, o, fault)
    msg = _caught(fault, lambda: X.cols_check(c, wins, ora), "head_cols_kernel", "K-quarters of 48")
    if fault == "neighbour_scale":
        assert "sample 0, head 0" in msg and 0 < int(re.search(r"(\d+) of 6336", msg).group(1)) <= 64      # only the 64 columns of head 0 in row 0
    _old(fault, rel(wins["out"][:33, :192], ora["out"]), 2e-6, sees)


def test_cols_store_past_ldo_is_named():
    c = X.cols_case(33, 3, rs="grid", bias=True, bf=True, wide=True)
    o, ora, wins = _mirror(c)
    wins["out"][5, c.d] = 1.0
    _caught("a store one element past ldo", lambda: X.cols_check(c, wins, ora), "padding between column 192", "(row 5, column 192)")
    _old("a store one element past ldo", rel(wins["out"][:33, :192], ora["out"]), 2e-6, False)


def test_cols_truncated_bf16_copy_is_named():
    c = X.cols_case(33, 3, rs="random", bias=True, bsc=True, bf=True, wide=True, tier="random")
    o, ora, wins = _mirror(c)
    out = wins["out"][:33, :192]
    assert not torch.equal(_trunc_bf16(out), out.to(torch.bfloat16))
    wins["ob"][:33, :192] = _trunc_bf16(out)
    _caught("out_bf16 truncated", lambda: X.cols_check(c, wins, ora), "out_bf16", "head_cols_kernel")


def test_wgrad_tail_that_keeps_its_scale_is_named():
    c = X.wgrad_case(33, 3, rs="pow2", wide=True)
    o, ora, _ = _mirror(c)
    wins = X.wgrad_written(c, o, fault="tail")
    _caught("padded lanes with their scale", lambda: X.wgrad_check(c, wins, ora), "head_wgrad_kernel", "31 padded lanes")
    _old("padded lanes with their scale", rel(wins["dW"][:192, :192], ora["dW"]), 2e-6, True)


def _sm(c):
    s = X.sm_scores(c)
    keep = X.sm_keep(c) if c.p > 0 else None
    wins = X.sm_written(c, s, keep)
    X.sm_check(c, s, wins, keep)
    return s, keep, wins


def test_softmax_mask_indexed_with_16_heads_is_named():
    c = X.sm_case(2, 3, 17, p=0.25, seed=20240607)
    s, keep, _ = _sm(c)
    wrong = X.sm_keep(c, heads=16)
    assert not torch.equal(wrong, keep) and torch.equal(wrong[0], keep[0])           # sample 0 is the same: b = 0 hides the fault
    wins = X.sm_written(c, s, wrong)
    _caught("the mask indexed with 16 heads", lambda: X.sm_check(c, s, wins, keep), "e_masked", "sample 1")
    assert not torch.equal(wins["em"][:34, :3].reshape(2, 17, 3), torch.where(keep, wins["e"][:34, :3].reshape(2, 17, 3), torch.zeros(2, 17, 3, dtype=torch.bfloat16)))


def test_softmax_rz_from_unrounded_weights_is_named():
    c = X.sm_case(2, 12, 513)
    s, _, _ = _sm(c)
    wins = X.sm_written(c, s, fault="unrounded_rz")
    _caught("rz from the unrounded weights", lambda: X.sm_check(c, s, wins), "stat[0]", "thread")
    e = wins["e"][:2 * 513, :12].reshape(2, 513, 12)
    _old("rz from the unrounded weights", rel(wins["stat"][0, :24].reshape(2, 12), 1.0 / e.float().sum(1)), 1e-6, True)


def test_softmax_top_weight_below_one_is_named():
    c = X.sm_case(2, 12, 513)
    s, _, wins = _sm(c)
    n = int(s[1, :, 7].argmax())
    wins["e"][513 + n, 7] = 0.99609375
    _caught("e below 1 at the arg-max row", lambda: X.sm_check(c, s, wins), "must be 1.0", "sample 1", "head 7", f"pass {n // 64}")
    ref = torch.exp(0.125 * (s - s.amax(dim=1, keepdim=True))).to(torch.bfloat16)
    _old("e below 1 at the arg-max row", rel(wins["e"][:1026, :12].float().reshape(2, 513, 12), ref.float()), 3e-3, False)


def test_softmax_negative_zero_in_the_padding_is_named():
    c = X.sm_case(2, 3, 17, lde=8)
    s, _, wins = _sm(c)
    wins["e"][20, 5] = -0.0
    _caught("-0 in a padding column", lambda: X.sm_check(c, s, wins), "padding columns 3 .. 7", "(row 20, col 5)")
    assert float(wins["e"][:34, 3:].float().abs().max()) == 0.0      # the old test's maximum does not see it


def _bw(c):
    i = X.bw_exact_inputs(c)
    keep = X.sm_keep(c) if c.p > 0 else None
    ora = X.bw_oracle(c, i, keep)
    X.bw_check(c, X.bw_written(c, i, keep), ora)
    return i, keep, ora


@pytest.mark.parametrize("fault,tol,half,sees", [("wave", 1e-5, 0, True), ("no_inv", 1e-6, 1, True), ("swapped", 1e-5, 0, True)])
def test_softmax_bwd_fault_is_named(fault, tol, half, sees):
    c = X.bw_case(2, 3, 513, lde=8, ldp=24, ldb=16, p=0.5, seed=11)
    i, keep, ora = _bw(c)
    wins = X.bw_written(c, i, keep, fault)
    msg = _caught(fault, lambda: X.bw_check(c, wins, ora), "cls_softmax_bwd coef")
    assert ("p-prime half" if fault == "no_inv" else "ds half") in msg
    if fault == "wave":
        assert "head 0" in msg
    coef = wins["coef"][0, :2 * 513 * 6].reshape(2, 513, 6)
    _old(fault, rel(coef[:, :, 3 * half:3 * half + 3], (ora["ds"], ora["pp"])[half]), tol, sees)


def _kv(c):
    o = X.kv_operands(c)
    ora = X.kv_oracle(c, o)
    X.kv_check(c, X.kv_written(c, o), ora)
    return o, ora


def test_kv_dgrad_last_coefficient_dropped_is_named():
    c = X.kv_case(3, 5, 65, wide=True)
    o, ora = _kv(c)
    wins = X.kv_written(c, o, fault="last_j")
    _caught("coefficient 2 H - 1 dropped", lambda: X.kv_check(c, wins, ora), "xattn_kv_dgrad_kernel<16>", "10 coefficients", "slice 0 of 3")
    _old("coefficient 2 H - 1 dropped", rel(wins["dhn"][:195, :320].float(), ora["dhn"]), 3e-3, True)


def test_kv_dgrad_truncated_store_is_named():
    c = X.kv_case(3, 5, 65, tier="random")
    o, ora = _kv(c)
    wins = X.kv_written(c, o)
    wins["dhn"][:195, :320] = _trunc_bf16(torch.einsum("bnj,jbc->bnc", o["coef"], o["R"]).reshape(195, 320))
    _caught("dhn truncated", lambda: X.kv_check(c, wins, ora), "xattn_kv_dgrad_kernel<16>", "outside [bf16(ref - B), bf16(ref + B)]")
    _old("dhn truncated", rel(wins["dhn"][:195, :320].float(), ora["dhn"]), 3e-3, True)
