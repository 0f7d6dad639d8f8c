"""The element-wise LayerNorm / column-sum gate (tests/_ln_check.py) has teeth, on the CPU.

Not too tight: a float32 CPU mirror of the kernels' formulas (two-pass variance, plain torch sums) passes every content case at every
width under the final constants; its needs are printed and noted, and the constants are derived from them (C_k = the power of two at
or above 4 x the largest need, see _ln_check's docstring).  Not too loose: each planted fault, a mistake a LayerNorm kernel could make,
fails the gate on the case named with it."""
import pytest
import torch

import _ln_check as L
from _util import note, rt

ROWS = 257
EPS = L.f32(1e-5)


def _fwd_case(kind, d, rows=ROWS, eps=EPS, seed=0):
    x = L.content(kind, rows, d, seed=seed + d)
    g, b = L.affine(d, seed=seed + d + 1)
    return x, g, b, L.ln_ref(x, None, 0, g, b, eps)


def _bwd_case(kind, d, rows=ROWS, seed=0, with_dres=True):
    x, g, b, ref = _fwd_case(kind, d, rows, seed=seed)
    gen = torch.Generator().manual_seed(seed + 7 * d + 3)
    dy = rt(torch.randn(rows, d, generator=gen))
    dres = torch.randn(rows, d, generator=gen) if with_dres else None
    mu32, rs32 = ref["mu"].float(), ref["rs"].float()
    return x, g, dy, dres, mu32, rs32, L.ln_bwd_ref(dy, x, mu32, rs32, g, dres)


def _prefill(d, seed, names=("dgamma", "dbeta", "dxsum", "dressum")):
    gen = torch.Generator().manual_seed(seed)
    return {n: torch.randn(d, generator=gen) for n in names}


# ------------------------------------------------------------------------------------------------------------ the mirror passes
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("kind", L.CONTENT)
def test_mirror_forward_passes_and_its_needs(kind, eps):
    eps = L.f32(eps)
    for d in L.WIDTHS:
        x, g, b, ref = _fwd_case(kind, d, eps=eps)
        mu, rs, y = L.ln_fwd_mirror(x, None, 0, g, b, eps)
        needs = {"mean": L.need_of(mu, ref["mu"], ref["S_mean"]), "rstd": L.need_of(rs, ref["rs"], ref["S_rstd"], ref["E_rstd"]),
                 "y": L.need_of(y, ref["y"], ref["S_y"], ref["E_y"])}
        for k, v in needs.items():
            note(f"mirror:{kind}:eps{eps:.0e}:d{d}:need_{k}", v)
        print(f"mirror fwd {kind:10s} eps {eps:.0e} d {d:5d}: need " + ", ".join(f"{k} {v:.2f}" for k, v in needs.items()))
        L.check_fwd(ref, d, ROWS, mu, rs, y, y.to(torch.bfloat16))
        L.check_fwd(ref, d, ROWS, mu, rs, None, y.to(torch.bfloat16))


@pytest.mark.parametrize("kind", L.CONTENT)
def test_mirror_backward_passes_and_its_needs(kind):
    for d in L.WIDTHS:
        x, g, dy, dres, mu32, rs32, ref = _bwd_case(kind, d)
        pre = _prefill(d, seed=d)
        got = L.ln_bwd_mirror(dy, x, mu32, rs32, g, dres, prefill=pre)
        needs = {"dx": L.need_of(got["dx"], ref["dx"], ref["S_dx"])}
        for n in ("dgamma", "dbeta", "dressum"):
            needs[n] = L.need_of(got[n], ref[n] + pre[n].double(), ref["S_" + n] + pre[n].abs().double())
        for k, v in needs.items():
            note(f"mirror:{kind}:d{d}:need_{k}", v)
        print(f"mirror bwd {kind:10s} d {d:5d}: need " + ", ".join(f"{k} {v:.2f}" for k, v in needs.items()))
        L.check_dx(ref, d, ROWS, got["dx"], got["dx"].to(torch.bfloat16))
        L.check_cols(ref, d, ROWS, {n: got[n] for n in ("dgamma", "dbeta", "dxsum", "dressum")}, pre)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mirror_colsum_passes_and_its_needs(dtype):
    for n in (4, 252, 256, 260, 768, 3072):
        for rows in (1, 5, 77, 1026):
            x = L.content("usual", rows, n, seed=rows + n).to(dtype)
            pre = _prefill(n, seed=n)["dgamma"]
            got = L.colsum_mirror(x, pre)
            ref, S = L.colsum_ref(x)
            need = L.need_of(got, ref + pre.double(), S + pre.abs().double())
            note(f"mirror:colsum:{dtype}:n{n}:rows{rows}:need_colsum", need)
            print(f"mirror colsum {dtype} n {n:5d} rows {rows:5d}: need {need:.2f}")
            L.check_colsum(got, x, n, rows, pre)


# ------------------------------------------------------------------------------------------------------------ planted faults
def _caught(what, fn):
    """fn runs the gate on a defective output: it must fail, and the failure is reported by name."""
    with pytest.raises(AssertionError) as e:
        fn()
    print(f"caught: {what}: {str(e.value)[:200]}")


def _fwd_fault(fault, kind, d, eps=EPS, which=("rstd", "y")):
    x, g, b, ref = _fwd_case(kind, d, eps=eps)
    mu, rs, y = L.ln_fwd_mirror(x, None, 0, g, b, eps, fault=fault)
    loc = L.Loc(ROWS, d)
    if "rstd" in which:
        _caught(f"{fault} ({kind}, d = {d}): rstd", lambda: L.check_f32("rstd", "rstd", rs, ref["rs"], ref["S_rstd"], loc, chain=L.row_chain(d), extra=ref["E_rstd"]))
    if "y" in which:
        _caught(f"{fault} ({kind}, d = {d}): y", lambda: L.check_f32("y", "y", y, ref["y"], ref["S_y"], loc, chain=L.row_chain(d), extra=ref["E_y"]))
        _caught(f"{fault} ({kind}, d = {d}): y, bf16 only",
                lambda: L.check_bf16_only("y_bf16", "y", y.to(torch.bfloat16), ref["y"], ref["S_y"], loc, chain=L.row_chain(d), extra=ref["E_y"]))


@pytest.mark.parametrize("d", [w for w in L.WIDTHS if w > 4])
def test_variance_over_d_minus_1_is_caught(d):
    _fwd_fault("var_dm1", "usual", d)


@pytest.mark.parametrize("d", [768, 1024])
@pytest.mark.parametrize("kind", ["std1e-2", "std1e-3", "const"])
@pytest.mark.parametrize("fault", ["no_eps", "eps_1e-6"])
def test_wrong_eps_is_caught(fault, kind, d):
    _fwd_fault(fault, kind, d, which=("rstd", "y") if kind != "const" else ("rstd",))   # constant rows: y = beta whatever rstd is


@pytest.mark.parametrize("d", [768, 1024])
@pytest.mark.parametrize("kind", ["mean100", "mean-1000"])
def test_one_pass_variance_is_caught(kind, d):
    _fwd_fault("one_pass", kind, d)


@pytest.mark.parametrize("d", [192, 772])
def test_phantom_columns_in_the_variance_are_caught(d):
    _fwd_fault("phantom", "usual", d)


def test_x_alt_ignored_for_one_sequence_is_caught():
    rows, d, seq = 130, 256, 17
    x, alt = L.content("usual", rows, d, seed=1), L.content("usual", -(-rows // seq), d, seed=2)
    g, b = L.affine(d, seed=3)
    ref = L.ln_ref(x, alt, seq, g, b, EPS)
    mu, rs, y = L.ln_fwd_mirror(x, alt, seq, g, b, EPS)
    L.check_fwd(ref, d, rows, mu, rs, y, y.to(torch.bfloat16), seq_len=seq)
    mu, rs, y = L.ln_fwd_mirror(x, alt, seq, g, b, EPS, fault="alt_ignored_seq1")
    for name, kind, t, S in (("mean", "mean", mu, "S_mean"), ("rstd", "rstd", rs, "S_rstd"), ("y", "y", y, "S_y")):
        with pytest.raises(AssertionError, match=f"row {seq}, column .*a row from x_alt"):
            L.check_f32(name, kind, t, ref["mu" if name == "mean" else "rs" if name == "rstd" else "y"], ref[S], L.Loc(rows, d, seq_len=seq),
                        chain=L.row_chain(d))
    print("caught: x_alt ignored for sequence 1 only")


def test_unwritten_last_row_and_a_quad_past_d_are_caught():
    rows, d, ld = 33, 252, 252 + 64
    x, g, b, ref = _fwd_case("usual", d, rows)
    mu, rs, y = L.ln_fwd_mirror(x, None, 0, g, b, EPS)
    buf = L.nan_buffer(rows, ld, torch.float32)
    buf[:rows, :d] = y
    L.check_padding("y_f32", buf, rows, d)
    L.check_fwd(ref, d, rows, mu, rs, buf[:rows, :d])
    last = buf.clone()
    last[rows - 1, :d] = float("nan")
    _caught("last row not written", lambda: L.check_fwd(ref, d, rows, mu, rs, last[:rows, :d]))
    _caught("last row not written (bf16 only)", lambda: L.check_fwd(ref, d, rows, mu, rs, None, last[:rows, :d].to(torch.bfloat16)))
    past = buf.clone()
    past[5, d:d + 4] = 0.25
    _caught("one float4 written one quad past d", lambda: L.check_padding("y_f32", past, rows, d))
    over = buf.clone()
    over[rows, :4] = 0.25
    _caught("a row written behind the last one", lambda: L.check_padding("y_f32", over, rows, d))


@pytest.mark.parametrize("d", [768, 1024, 4096])
def test_backward_faults_are_caught(d):
    x, g, dy, dres, mu32, rs32, ref = _bwd_case("usual", d)
    pre = _prefill(d, seed=d)
    got = L.ln_bwd_mirror(dy, x, mu32, rs32, g, dres, prefill=pre, fault="m2_dropped")
    _caught(f"m2 term dropped from dx (d = {d})", lambda: L.check_dx(ref, d, ROWS, got["dx"]))
    got = L.ln_bwd_mirror(dy, x, mu32, rs32, g, dres, prefill=pre, fault="dres_twice_in_dxsum")
    L.check_dx(ref, d, ROWS, got["dx"])
    _caught(f"dres added twice to dxsum (d = {d})", lambda: L.check_cols(ref, d, ROWS, {"dxsum": got["dxsum"]}, pre))
    got = L.ln_bwd_mirror(dy, x, mu32, rs32, g, dres, prefill=pre, fault="dgamma_stored")
    L.check_cols(ref, d, ROWS, {"dbeta": got["dbeta"]}, pre)
    _caught(f"dgamma stored instead of added (d = {d})", lambda: L.check_cols(ref, d, ROWS, {"dgamma": got["dgamma"]}, pre))


def test_constant_rows_backward_is_pure_cancellation():
    """Constant dy g on any row: the exact dx is 0 and what a float32 kernel returns is round-off, inside the bound."""
    d = 768
    x, g, _, ref_f = _fwd_case("usual", d)
    dy = rt(torch.full((ROWS, d), 0.75))
    ones = torch.ones(d)
    mu32, rs32 = ref_f["mu"].float(), ref_f["rs"].float()
    ref = L.ln_bwd_ref(dy, x, mu32, rs32, ones)
    got = L.ln_bwd_mirror(dy, x, mu32, rs32, ones)
    assert float(ref["dx"].abs().max()) < 1e-6 and float(ref["S_dx"].min()) > 1e-2       # 0 but for the rounding of mu32
    L.check_dx(ref, d, ROWS, got["dx"])


def test_truncated_bf16_copy_is_caught():
    d = 768
    x, g, b, ref = _fwd_case("usual", d)
    mu, rs, y = L.ln_fwd_mirror(x, None, 0, g, b, EPS)
    L.check_bf16_copy("y_bf16", y.to(torch.bfloat16), y, L.Loc(ROWS, d))
    _caught("bf16 copy rounded by truncation", lambda: L.check_bf16_copy("y_bf16", L.bf16_truncate(y), y, L.Loc(ROWS, d)))


@pytest.mark.parametrize("rows", [5, 13, 17, 63, 65, 77, 1026])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_colsum_tail_rows_skipped_is_caught(dtype, rows):
    n = 768
    x = L.content("usual", rows, n, seed=rows).to(dtype)
    L.check_colsum(L.colsum_mirror(x), x, n, rows)
    _caught(f"colsum: the last rows % 4 = {rows % 4} rows skipped ({dtype}, rows = {rows})",
            lambda: L.check_colsum(L.colsum_mirror(x, fault="tail_rows_skipped"), x, n, rows))


def test_constants_are_powers_of_two_under_their_ceilings():
    for kind, c in L.C.items():
        assert c == L.pow2_at_or_above(c), kind
    for d in L.WIDTHS:
        for kind in ("mean", "rstd", "y", "dx"):
            assert L.const_of(kind, L.row_chain(d)) <= 4 * L.v_of(d) + 6
    assert L.ln_bwd_grid(12288) == 768 and L.ln_bwd_grid(12289) == 768 and L.ln_bwd_grid(12272) == 767 and L.ln_bwd_grid(1) == 1
    assert L.ln_fwd_grid(16384) == 2048 and L.ln_fwd_grid(16376) == 2047
    assert L.colsum_rows_per_block(64 * 171 + 1, 3072) == 128 and L.colsum_rows_per_block(64 * 170, 3072) == 64
