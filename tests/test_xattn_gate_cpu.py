"""The gate of the CLS-query cross-attention kernels (tests/_xattn_check.py) has teeth, on the CPU.

(a) C_exp.  The float32 mirror of cls_xattn_fwd_kernel (`fwd_mirror`) runs over the contents of every case of tests/test_cls_xattn_edges_gpu.py
    (random, x 15, equal, dominant, the exact tier's); C_exp must be the power of two at or above 4 x its largest need, and the table in
    _xattn_check's docstring is re-measured here.
(b) Every derived bound of the float64 tier is checked against torch's own fp32 arithmetic on the inputs the GPU file uses (the mirrors' `*_written`
    windows go through the very `*_check` the device's windows go through), and the exact tier's mirrors match bit for bit.
(c) Planted faults.  Each starts from the windows a correct launch would leave, plants ONE defect, and states two outcomes: the new check names it
    (always), and what the old gate says on the same data: `_util.rel` against TOL_F32 = 1e-3 (o_f32, p, dq, coef) / TOL_BF16 = 3e-3 (dk, dv) as in
    tests/test_cls_xattn_gpu.py.  Nothing was bent to make it miss: where it sees the fault the table in _xattn_check's docstring says so, and both
    outcomes are asserted."""
import math

import pytest
import torch

import _xattn_check as X
from _cls_check import pow2_at_or_above
from _util import TOL_BF16, TOL_F32, note, rel

RANDOM_DROP = (0.25, 7)


def _caught(what, fn, *names):
    with pytest.raises(AssertionError) as e:
        fn()
    msg = str(e.value)
    print(f"caught: {what}: {msg[:500]}")
    for n in names:
        assert n in msg, f"{what}: the message does not name {n!r}: {msg}"
    return msg


def _old(what, value, tol, sees):
    print(f"old gate on {what}: {value:.3e} against {tol:g}")
    assert (not value <= tol) == sees, f"{what}: old gate {value:.3e} against {tol:g}, recorded as {'seen' if sees else 'not seen'}"


def _contents():
    """-> every (case, operands) whose scores the GPU file's forward sees, dropout off (the mask does not enter the softmax)."""
    for c, kind2 in X.all_cases() + [(X.lds_case(), None)]:
        for kind in ("random",) + ((kind2,) if kind2 else ()):
            r = X.with_(c, kind=kind)
            yield kind, r, X.random_operands(r)
        if c.N < 16385:
            e = X.with_(c, tier="exact")
            yield "exact", e, X.exact_operands_fwd(e)


# ---------------------------------------------------------------------------------------------------------------- (a) C_exp
def test_exp_mirror_need_sets_the_constant():
    needs = {}
    for kind, c, o in _contents():
        needs[kind] = max(needs.get(kind, 0.0), X.exp_need32(X.fwd_mirror(c, o["q"], o)))
    for k, v in needs.items():
        note(f"mirror:need_exp:{k}", v)
        print(f"mirror need C_exp on {k:9s}: {v:.2f}")
    need = max(needs.values())
    # the exact tier (arguments 0 and <= -369) and the rows a dominant one pushes below the fp32 range need nothing.  The largest need sits at weights just
    # below 1 (|a| -> 0, so the argument term grants nothing): a correctly rounded exp2 errs by at most half an ulp there, 0.5 x 2^-24 of the weight; further
    # down 3 ln 2 |a| has grown past the half-ulp.  So the need of any host whose exp2 is correctly rounded on these arguments is in (0.25, 0.5].
    assert set(needs) == {"random", "x15", "equal", "dominant", "exact"} and needs["exact"] == 0.0 and needs["dominant"] == 0.0, needs
    assert 0.25 < need <= 0.5, f"the host's exp2 is off by more than half an ulp on these arguments (need {need:.4f}): that is about this machine's torch, not the kernels"
    assert X.C_EXP == pow2_at_or_above(4 * need) == 2.0, f"mirror need {need:.3f}, C_exp {X.C_EXP:g}"


# ---------------------------------------------------------------------------------------------------------------- the mirror of the geometry
def test_geometry_mirror_reaches_every_path():
    assert X.pv_owner(0) == (0, 0, 0) and X.pv_owner(31) == (31, 0, 3) and X.pv_owner(32) == (0, 1, 0) and X.pv_owner(4096) == (0, 128, 0)
    assert X.sm_owner(255) == (255, 3, 0) and X.sm_owner(256) == (0, 0, 1) and X.sm_owner(512) == (0, 0, 2)
    assert X.edge_rows(1) == [0] and X.edge_rows(2) == [0, 1] and X.edge_rows(7) == [0, 6, 5, 1, 2, 3, 4]
    assert X.edge_rows(513)[:11] == [0, 512, 31, 32, 511, 255, 256, 63, 64, 1, 2] and len(X.edge_rows(513)) == 16
    assert [len(X.live_rows(N)) for N in X.NS] == [1, 2, 4, 8, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16]
    assert X.xa_lds(38908) == 160 * 1024 and X.xa_lds(38909) > 160 * 1024 and X.xa_lds(14332) <= 64 * 1024 < X.xa_lds(14333)
    assert {c.layout for c, _ in X.all_cases()} == set("abcd") and {c.H for c, _ in X.all_cases()} == set(X.HS) and {c.B for c, _ in X.all_cases()} == {1, 2, 3}
    assert {(c.layout, c.N, c.H) for c in X.layout_cases()} == {(la, N, H) for la in "abcd" for N in (33, 257) for H in (3, 20)}
    assert {k for _, k in X.all_cases() if k} == {"x15", "equal", "dominant"}
    for c, _ in X.all_cases():                # every launch of the GPU file: aligned 16-byte loads, the entry points' stride rules
        assert c.sn % 8 == 0 and c.sb % 8 == 0 and c.ld % 8 == 0 and c.koff % 8 == 0 and c.voff % 8 == 0 and c.sb >= c.N * c.sn, c
        assert max(c.koff, c.voff) + c.d <= c.sn


# ---------------------------------------------------------------------------------------------------------------- (b) the mirrors pass
def _fwd_mirror_passes(c, o, q=None):
    q = o["q"] if q is None else q
    keep = X.keep_mask(c) if c.p > 0 else None
    w0 = X.fwd_written(X.with_(c, p=0.0, seed=0), q, o) if c.p > 0 else None
    wins = X.fwd_written(c, q, o, keep)
    X.fwd_check(c, o, wins, X.fwd_oracle(c, q, o, keep), w0)
    return X.gview(wins["p"]).reshape(c.B, c.H, c.N).clone(), keep


def _bwd_mirror_passes(c, o, p, keep):
    ora = X.bwd_oracle(c, o, p, keep)
    wins = X.bwd_written(c, o, p, keep)
    X.bwd_check(c, o, wins, ora)
    return wins, ora


def _mirror_both_tiers(c, kind2=None, exact=True):
    for on in (False, True):
        if exact:
            p, seed = X.DROP if on else (0.0, 0)
            e = X.with_(c, p=p, seed=seed, tier="exact")
            _fwd_mirror_passes(e, X.exact_operands_fwd(e))
            ob = X.exact_operands_bwd(e)
            _bwd_mirror_passes(e, ob, ob["p"], X.keep_mask(e) if p > 0 else None)
        p, seed = RANDOM_DROP if on else (0.0, 0)
        for kind in ("random",) + ((kind2,) if kind2 else ()):
            r = X.with_(c, p=p, seed=seed, tier="random", kind=kind)
            o = X.random_operands(r)
            saved, keep = _fwd_mirror_passes(r, o)
            _fwd_mirror_passes(r, o, o["qb"])
            _bwd_mirror_passes(r, o, saved, keep)


@pytest.mark.parametrize("N", X.NS + (16385,))
def test_mirrors_pass_every_sequence_length(N):
    if N == 16385:
        _mirror_both_tiers(X.lds_case(), exact=False)
    else:
        _mirror_both_tiers(*X.n_cases(N))


def test_mirrors_pass_every_layout_and_head_count():
    for c in X.layout_cases() + X.h_cases():
        _mirror_both_tiers(c)


# ---------------------------------------------------------------------------------------------------------------- (c) planted faults
def _ref64(c, o, keep=None):
    """The float64 reference of tests/test_cls_xattn_gpu.py -> P [B, H, N], o [B, d]."""
    q64, k64, v64 = o["q"].double().view(c.B, c.H, 64), X._h4(c, o["k"]).double(), X._h4(c, o["v"]).double()
    P = torch.softmax(torch.einsum("bhe,bnhe->bhn", q64, k64) * c.scale, -1)
    return P, torch.einsum("bhn,bnhe->bhe", P * X.mask32(c, keep).double(), v64).reshape(c.B, c.d)


def _fwd(c, fault, keep=None):
    o = X.random_operands(c)
    ora = X.fwd_oracle(c, o["q"], o, keep)
    X.fwd_check(c, o, X.fwd_written(c, o["q"], o, keep), ora)
    return o, ora, X.fwd_written(c, o["q"], o, keep, fault)


def test_last_key_row_missing_from_the_pv_sum_is_named():
    c = X.case(1, 3, 4097)
    o, ora, wins = _fwd(c, "last_row")
    _caught("last row missing", lambda: X.fwd_check(c, o, wins, ora), "o_f32 against the float64 sum of the stored p m v", "129 passes")
    _old("last row missing", rel(wins["of"][:1, :c.d], _ref64(c, o)[1]), TOL_F32, True)


def test_slice_31_missing_from_o_is_named():
    c = X.case(2, 3, 33, "c")
    o, ora, wins = _fwd(c, "slice31")
    _caught("slice 31 missing", lambda: X.fwd_check(c, o, wins, ora), "o_f32", "sums the 32 slices in slice order")
    _old("slice 31 missing", rel(wins["of"][:2, :c.d], _ref64(c, o)[1]), TOL_F32, True)


def test_inv_from_a_sum_without_its_tail_is_named():
    c = X.case(2, 3, 257, "b")
    o, ora, wins = _fwd(c, "inv_tail")
    _caught("inv without the last N mod 256 terms", lambda: X.fwd_check(c, o, wins, ora), "p against the float64 softmax", "softmax thread")
    _old("inv without the last N mod 256 terms", rel(X.gview(wins["p"]).reshape(2, 3, 257), _ref64(c, o)[0]), TOL_F32, True)


def test_p_saved_after_dropout_is_named():
    c = X.with_(X.case(2, 3, 33), p=0.25, seed=7)
    keep = X.keep_mask(c)
    o, ora, wins = _fwd(c, "p_after_dropout", keep)
    w0 = X.fwd_written(X.with_(c, p=0.0), o["q"], o)
    _caught("p saved after dropout", lambda: X.fwd_check(c, o, wins, ora, w0), "saved before dropout")
    _caught("p saved after dropout, without the p = 0 launch", lambda: X.fwd_check(c, o, wins, ora), "p against the float64 softmax")
    _old("p saved after dropout", rel(X.gview(wins["p"]).reshape(2, 3, 33), _ref64(c, o, keep)[0]), TOL_F32, True)


def _bwd(c, tier_ops=None):
    o = X.exact_operands_bwd(c) if c.tier == "exact" else X.random_operands(c)
    keep = X.keep_mask(c) if c.p > 0 else None
    p = o["p"] if c.tier == "exact" else X.fwd_mirror(c, o["q"], o, keep)["p"]
    wins, ora = _bwd_mirror_passes(c, o, p, keep)
    return o, p, keep, ora, wins


def _dsn64(c, o, p, keep):
    return X.bwd_oracle(X.with_(c, tier="random"), o, p, keep)["dsn"]


def test_wave_missing_from_dsum_is_named():
    c = X.with_(X.case(2, 3, 513, "c"), p=0.25, seed=7)
    o, p, keep, ora, _ = _bwd(c)
    wins = X.bwd_written(c, o, p, keep, "wave")
    _caught("wave 2 missing from dsum", lambda: X.bwd_check(c, o, wins, ora), "coef[.., h] = dsn", "dsn half", "head 0")
    _old("wave 2 missing from dsum", rel(X.gview(wins["coef"]).reshape(2, 513, 6)[:, :, :3], ora["dsn"]), TOL_F32, True)


def test_swapped_halves_of_coef_are_named():
    c = X.with_(X.case(2, 3, 33), tier="exact")
    o, p, keep, ora, _ = _bwd(c)
    wins = X.bwd_written(c, o, p, keep, "swapped")
    _caught("coef halves swapped", lambda: X.bwd_check(c, o, wins, ora), "coef[.., H + h] = p m", "p-prime half")
    dk, dv = X.dkv_views(c, wins["dkv"])            # what the old tests compare is untouched
    assert torch.equal(dk, ora["dk"]) and torch.equal(dv, ora["dv"])


def test_dk_with_the_packed_stride_is_named():
    c = X.with_(X.case(2, 3, 33, "c"), tier="exact")
    o, p, keep, ora, wins = _bwd(c)
    bufs = X.dkv_windows(c)
    bufs[0].as_strided((c.B, c.N, c.d), (c.N * 2 * c.d, 2 * c.d, 1), c.koff).copy_(ora["dk"])
    X.dkv_views(c, bufs)[1].copy_(ora["dv"])
    wins["dkv"] = bufs
    _caught("dk with the packed stride", lambda: X.bwd_check(c, o, wins, ora), "dk | dv buffer", "sentinel elements were overwritten")


def test_store_behind_column_2d_is_named():
    c = X.with_(X.case(2, 3, 33, "c"), tier="exact")
    o, p, keep, ora, wins = _bwd(c)
    wins["dkv"][0][c.sb + 5 * c.sn + 2 * c.d] = 0.0
    _caught("a store behind column 2 d", lambda: X.bwd_check(c, o, wins, ora), "sample 1, row 5", "the gap behind column 384 up to the row stride 392")
    dk, dv = X.dkv_views(c, wins["dkv"])
    assert torch.equal(dk, ora["dk"]) and torch.equal(dv, ora["dv"])


@pytest.mark.parametrize("layout", "abcd")
def test_store_to_row_N_of_the_last_sample_is_named(layout):
    c = X.with_(X.case(2, 3, 33, layout), tier="exact")
    o, p, keep, ora, wins = _bwd(c)
    wins["dkv"][-1][(c.B - 1) * c.sb + c.N * c.sn + c.voff + 70] = 0.0
    _caught("a store to row N", lambda: X.bwd_check(c, o, wins, ora), "row 33 of sample 1, which has 33", "column 70 of the dv half")
    dk, dv = X.dkv_views(c, wins["dkv"])
    assert torch.equal(dk, ora["dk"]) and torch.equal(dv, ora["dv"])


def _trunc_bf16(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def test_truncated_dv_is_named():
    c = X.case(2, 3, 65, "d")
    o, p, keep, ora, wins = _bwd(c)
    coef = X.gview(wins["coef"]).reshape(2, 65, 6)
    exact = coef[:, :, 3:, None] * o["dO"].view(2, 1, 3, 64)
    assert not torch.equal(_trunc_bf16(exact), exact.to(torch.bfloat16))
    X.dkv_views(c, wins["dkv"])[1].copy_(_trunc_bf16(exact).reshape(2, 65, 192))
    _caught("dv truncated", lambda: X.bwd_check(c, o, wins, ora), "dv = bf16(coef[.., H + h] dO)", "cls_xattn_bwd dv")
    _old("dv truncated", rel(X.dkv_views(c, wins["dkv"])[1].float(), exact.double().reshape(2, 65, 192)), TOL_BF16, True)


def test_one_ulp_in_dq_is_named():
    c = X.with_(X.case(2, 3, 257, "c"), tier="exact", p=0.5, seed=20240607)
    o, p, keep, ora, wins = _bwd(c)
    assert float(wins["dq"][1, 100]) != 0.0
    wins["dq"][1, 100] = torch.nextafter(wins["dq"][1, 100], torch.tensor(math.inf))
    _caught("dq one ulp off", lambda: X.bwd_check(c, o, wins, ora), "dq", "sample 1, head 1, column 36")
    _old("dq one ulp off", rel(wins["dq"][:2, :192], ora["dq"]), TOL_F32, False)


def test_mask_indexed_with_16_heads_is_named():
    c = X.with_(X.case(2, 3, 33), p=0.25, seed=7)
    o, p, keep, ora, _ = _bwd(c)
    wrong = X.keep_mask(c, heads=16)
    assert not torch.equal(wrong, keep) and torch.equal(wrong[0], keep[0])           # sample 0 is the same: b = 0 hides the fault
    wins = X.bwd_written(c, o, p, wrong)
    _caught("the mask indexed with 16 heads", lambda: X.bwd_check(c, o, wins, ora), "coef[.., H + h] = p m", "sample 1")
    dv_ref = (ora["pr"].permute(0, 2, 1)[..., None].double() * o["dO"].double().view(2, 1, 3, 64)).reshape(2, 33, 192)
    _old("the mask indexed with 16 heads", rel(X.dkv_views(c, wins["dkv"])[1].float(), dv_ref), TOL_BF16, True)
    # the forward: the stored o_f32 is no longer the sum of the stored p with the right mask
    fw = X.fwd_written(c, o["q"], o, wrong)
    _caught("the forward's mask indexed with 16 heads", lambda: X.fwd_check(c, o, fw, X.fwd_oracle(c, o["q"], o, keep)), "o_f32 against the float64 sum", "sample 1")
