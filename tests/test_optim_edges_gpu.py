"""GPU: the fused Adam kernels, the gradient-norm partials, the step prologue and the casts, element-wise at every edge
(tests/_optim_check.py holds the oracle, the bounds and their derivation; tests/test_optim_gate_cpu.py shows the gate has teeth).

Adam: every size of _optim_check.SIZES in one launch, on every placement (both paths of adam_vec_ok), chunk lists in natural and
shuffled order and one that names a single chunk, eps 1e-8 / 1e-3, weight decay, three gradient scales, steps 1 / 2 / 1000; m and v bit
for bit on the exact tier, against float64 otherwise; the shadow is the RNE bf16 of the stored p; g and every guard come back untouched;
xvit_adam_step_dev is bit-identical to xvit_adam_step given the same fp32 numbers and writes nothing when `skip` is set."""
import functools
import math

import numpy as np
import pytest
import torch

import _optim_check as X
from _util import note

pytestmark = pytest.mark.gpu

THREE_CHUNKS = (5, 2 * X.CHUNK + 2, 1027)           # tensor 1 has three chunks; the list names only its chunk 1


def _lib():
    from xvit import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("tier", ["exact", "random"])
@pytest.mark.parametrize("placement", list(X.PLACEMENTS))
def test_adam_step_every_size_path_and_hyper(placement, tier):
    cases = [X.AdamCase(placement, tier, order=o) for o in ("natural", "shuffled")]
    worst = {}
    for i, h in enumerate(X.HYPER_EXACT if tier == "exact" else X.HYPER_RANDOM):
        case = cases[i % 2]
        rc, after = X.adam_launch(case, h)
        assert rc == 0, f"{case}: rc {rc}: {X.last_error()}"
        out = X.adam_check(case, h, after)
        for k, v in out.items():
            worst[k] = max(worst.get(k, 0.0), v)
        rc, after_dev = X.adam_launch(case, h, dev_record=True)
        assert rc == 0, f"{case}: xvit_adam_step_dev rc {rc}: {X.last_error()}"
        X.assert_same_arenas(case, f"xvit_adam_step_dev against xvit_adam_step ({h})", after_dev, after)
    for k, v in worst.items():
        note(f"optim:adam:{tier}:{placement}:{k if k.startswith('need') else k + ':max_err_over_bound'}", v)
    print(f"{placement}, {tier}: largest share of a bound {worst}")


@pytest.mark.parametrize("tier", ["exact", "random"])
@pytest.mark.parametrize("placement", list(X.PLACEMENTS))
def test_adam_single_chunk_of_a_three_chunk_tensor(placement, tier):
    """Only chunk 1 of a 2 * 16384 + 2 element tensor is listed: chunks 0 and 2 and the two other tensors come back bit-identical."""
    case = X.AdamCase(placement, tier, sizes=THREE_CHUNKS, order=[(1, 1)])
    assert int(case.listed.sum()) == X.CHUNK
    h = (X.HYPER_EXACT if tier == "exact" else X.HYPER_RANDOM)[-1]
    for dev_record in (False, True):
        rc, after = X.adam_launch(case, h, dev_record=dev_record)
        assert rc == 0, X.last_error()
        X.adam_check(case, h, after)


@pytest.mark.parametrize("placement", list(X.PLACEMENTS))
def test_adam_step_dev_with_skip_set_changes_no_byte(placement):
    case = X.AdamCase(placement, "random")
    rc, after = X.adam_launch(case, X.HYPER_RANDOM[7], dev_record=True, skip=1)
    assert rc == 0, X.last_error()
    X.assert_same_arenas(case, "a skipped step", after, case.arenas())


# ---------------------------------------------------------------------------------------------------------------- gradient-norm partials
@pytest.mark.parametrize("tier", ["exact", "random"])
@pytest.mark.parametrize("placement", list(X.PLACEMENTS))
def test_grad_sqnorm_partials_per_chunk(placement, tier):
    for order in ("natural", "shuffled"):
        case = X.AdamCase(placement, tier, order=order)
        rc, w, after = X.sqnorm_launch(case)
        assert rc == 0, X.last_error()
        worst = X.sqnorm_check(case, w, log=f"optim:sqnorm:{tier}:{placement}")
        X.assert_same_arenas(case, "the norm kernel only reads", after, case.arenas())
    print(f"{placement}, {tier}: largest share of gamma(n) {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------- prologue
def test_prologue_every_field_against_float64():
    for name, part, square, mx, step0 in X.prologue_cases():
        rec0 = np.zeros((), dtype=X.REC)
        rec0["step"], rec0["skipped"], rec0["lr"], rec0["lr_over_bc1"], rec0["inv_sqrt_bc2"], rec0["skip"] = step0, 3, 3e-3, 0.125, 0.25, 1
        rc, rec = X.prologue_launch(part, rec0, mx, 0.9, 0.98, 0)
        assert rc == 0, X.last_error()
        X.prologue_check(name, part, rec0, rec, mx, 0.9, 0.98, 0, square=square, log="optim:prologue")


@pytest.mark.parametrize("poison", [math.inf, math.nan])
@pytest.mark.parametrize("skip_nonfinite", [0, 1])
def test_prologue_nonfinite_norm(poison, skip_nonfinite):
    """An inf / NaN partial: grad_norm inf / NaN, clip_coef 0 / NaN; with skip_nonfinite the step is not counted and both corrections stay."""
    for n, at in ((1, 0), (257, 256), (1000, 511)):
        part = X.prologue_partials(n, False)
        part[at] = poison
        rec0 = np.zeros((), dtype=X.REC)
        rec0["step"], rec0["skipped"], rec0["lr"], rec0["lr_over_bc1"], rec0["inv_sqrt_bc2"] = 7, 2, 3e-3, 0.125, 0.25
        rc, rec = X.prologue_launch(part, rec0, 1.0, 0.9, 0.98, skip_nonfinite)
        assert rc == 0, X.last_error()
        X.prologue_check(f"prologue n_partials {n}, partial {at} = {poison}, skip_nonfinite {skip_nonfinite}", part, rec0, rec, 1.0, 0.9, 0.98, skip_nonfinite)
        assert int(rec["skip"]) == skip_nonfinite and int(rec["skipped"]) == 2 + skip_nonfinite and int(rec["step"]) == 8 - skip_nonfinite


def test_prologue_without_partials_takes_no_norm():
    rec0 = np.zeros((), dtype=X.REC)
    rec0["lr"], rec0["step"] = 1e-3, 4
    rc, rec = X.prologue_launch(None, rec0, 2.0, 0.9, 0.98, 1)
    assert rc == 0, X.last_error()
    assert float(rec["grad_norm"]) == 0.0 and float(rec["clip_coef"]) == 1.0
    X.prologue_check("prologue without partials", None, rec0, rec, 2.0, 0.9, 0.98, 1, square=True)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_of_the_four_entry_points_launches_nothing():
    lib = _lib()
    case = X.AdamCase("aligned, shadow 8-byte aligned", "random", sizes=(5, 1027))
    d = X.device_case(case)
    tab, ch, n, s = d["table"].data_ptr(), d["chunks"].data_ptr(), len(case.chunks), X._stream()
    part = X.partials_window(n).to(X._dev())
    rec0 = np.zeros((), dtype=X.REC)
    rec0["lr"], rec0["lr_over_bc1"], rec0["inv_sqrt_bc2"], rec0["clip_coef"], rec0["step"] = 1e-3, 1e-2, 1.0, 1.0, 1
    w = X.record_window(rec0).to(X._dev())
    st = w.data_ptr() + 8 * X.REC_GUARD
    step = lambda **k: lib.xvit_adam_step(*[{**dict(t=tab, c=ch, n=n, lr=1e-3, b1=0.9, b2=0.98, eps=1e-8, wd=0.0, step=1, gs=1.0, s=s), **k}[x]   # noqa: E731
                                            for x in ("t", "c", "n", "lr", "b1", "b2", "eps", "wd", "step", "gs", "s")])
    sdev = lambda **k: lib.xvit_adam_step_dev(*[{**dict(t=tab, c=ch, n=n, st=st, b1=0.9, b2=0.98, eps=1e-8, wd=0.0, s=s), **k}[x]   # noqa: E731
                                                for x in ("t", "c", "n", "st", "b1", "b2", "eps", "wd", "s")])
    norm = lambda **k: lib.xvit_grad_sqnorm_partials(*[{**dict(t=tab, c=ch, n=n, p=part.data_ptr(), s=s), **k}[x] for x in ("t", "c", "n", "p", "s")])   # noqa: E731
    pro = lambda **k: lib.xvit_adam_prologue(*[{**dict(p=part.data_ptr(), n=n, st=st, mx=1.0, b1=0.9, b2=0.98, sk=0, s=s), **k}[x]   # noqa: E731
                                               for x in ("p", "n", "st", "mx", "b1", "b2", "sk", "s")])
    refusals = [("xvit_adam_step", step, [dict(t=None), dict(c=None), dict(n=0), dict(n=-1), dict(step=0), dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=-0.1), dict(eps=-1e-8)]),
                ("xvit_adam_step_dev", sdev, [dict(t=None), dict(c=None), dict(st=None), dict(n=0), dict(b1=1.0), dict(b2=1.0), dict(b2=-0.1), dict(eps=-1e-8)]),
                ("xvit_grad_sqnorm_partials", norm, [dict(t=None), dict(c=None), dict(p=None), dict(n=0)]),
                ("xvit_adam_prologue", pro, [dict(st=None), dict(mx=0.0), dict(mx=-1.0), dict(b1=1.0), dict(b2=1.0), dict(b1=-0.1), dict(p=None), dict(n=0), dict(n=-3)])]
    for name, fn, bad in refusals:
        for k in bad:
            rc = fn(**k)
            assert rc != 0, f"{name} accepted {k}"
            assert name in X.last_error(), f"{name} refused {k} with a message that does not name it: {X.last_error()!r}"
    torch.cuda.synchronize()
    X.assert_same_arenas(case, "a refused call", {k: d[k].cpu() for k in case.starts}, case.arenas())
    assert X.record_of("refusals", w).tobytes() == rec0.tobytes()
    X.check_tail_guard("partials after refusals", part.cpu(), n)
    assert bool(torch.isnan(part.cpu()[:n]).all())


# ---------------------------------------------------------------------------------------------------------------- casts
CAST_BIG = 8 * 256 * 4096            # the vector body of exactly one pass of the capped grid (4096 blocks x 256 threads x 8 elements)
CAST_LEN = CAST_BIG + 4096
CAST_NS = list(range(1, 18)) + [2047, 2048, 2049] + [CAST_BIG + k for k in (-8, -1, 0, 1, 7, 8, 9)]


def _specials():
    """The list of tests/test_grad_comm_gpu.py::_specials: ties to even in both directions, subnormals, the largest finite fp32 rounding
    to inf, +-0, +-inf, NaNs."""
    f = lambda *bits: torch.tensor(list(bits), dtype=torch.int64).to(torch.int32).view(torch.float32)   # noqa: E731
    ties = []
    for b in (0x3F80, 0x3F81, 0x4049, 0xC049, 0x0001, 0x0080, 0x7F7E, 0x7F7F):
        ties += [(b << 16) | 0x8000, (b << 16) | 0x7FFF, (b << 16) | 0x8001]
    edges = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000, 0x00400000,
             0x00800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0xFFFFFFFF,
             0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF]
    x = torch.cat([f(*ties), f(*edges)])
    return torch.cat([x, -x])


@functools.lru_cache(maxsize=None)
def _cast_source():
    """One fp32 source for every cast case -> (CPU tensor, its CPU bf16, the device copy, the offset where plain random values start).
    The specials sit at the start (n = 1 .. 17 walk through the ties) and round CAST_BIG (the last vectors and the tail of the big cases)."""
    sp = _specials()
    x = torch.randn(CAST_LEN, generator=torch.Generator().manual_seed(91)) * 3.0
    x[:sp.numel()] = sp
    x[CAST_BIG - 40: CAST_BIG - 40 + sp.numel()] = sp
    assert sp.numel() > 49 and CAST_BIG - 40 + sp.numel() >= CAST_BIG + 9
    return x, x.bfloat16(), x.to(X._dev()), (sp.numel() + 7) // 8 * 8


def _cast_case(n, off):
    x, xb, xd, _ = _cast_source()
    src = xd[off: off + n + X.GUARD].clone()
    src[n:] = math.nan
    dst = torch.full((n + X.GUARD,), X.SENT, dtype=torch.bfloat16, device=X._dev())
    rc = _lib().xvit_cast_f32_bf16(src.data_ptr(), dst.data_ptr(), n, X._stream())
    assert rc == 0, X.last_error()
    got = dst.cpu()
    name = f"cast_f32_bf16 n = {n} at source offset {off}"
    X.check_tail_guard(name, got, n)
    where = lambda i: f"element {i}: " + (f"tail, thread {i - (n & ~7)}" if i >= (n & ~7) else f"vector {i // 8} (pass {i // 8 // (256 * 4096)} of the grid), lane {i % 8}")   # noqa: E731
    X.assert_bits(name, got[:n], xb[off: off + n], where, nan_ok=torch.isnan(x[off: off + n]))


@pytest.mark.parametrize("n", CAST_NS)
def test_cast_f32_bf16_bit_exact_with_tail_and_wrap(n):
    _cast_case(n, 0)
    if n < CAST_BIG - 8:
        _cast_case(n, _cast_source()[3])          # plain random values
    if n == CAST_BIG + 9:
        assert int(torch.isnan(_cast_source()[0][:n]).sum()) >= 10     # the ten NaNs of the specials (five patterns, both signs) were part of it


@pytest.mark.parametrize("n", [8, 16, 2048, 2056, CAST_BIG + 8])
def test_add_cast_f32_bf16_bit_exact(n):
    x, _, xd, _ = _cast_source()
    G = X.GUARD
    a, b = xd[:n + G].clone(), xd[2048: 2048 + n + G].clone()
    a[n:] = math.nan
    b[n:] = math.nan
    out = torch.full((n + G,), X.SENT, device=X._dev())
    outb = torch.full((n + G,), X.SENT, dtype=torch.bfloat16, device=X._dev())
    rc = _lib().xvit_add_cast_f32_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), outb.data_ptr(), n, X._stream())
    assert rc == 0, X.last_error()
    o, ob = out.cpu(), outb.cpu()
    X.check_tail_guard(f"add_cast n = {n}: out", o, n)
    X.check_tail_guard(f"add_cast n = {n}: out_bf16", ob, n)
    want = x[:n] + x[2048: 2048 + n]                                     # one fp32 add
    where = lambda i: f"element {i}: vector {i // 8} (pass {i // 8 // (256 * 4096)} of the grid), lane {i % 8}"   # noqa: E731
    X.assert_bits(f"add_cast n = {n}: out", o[:n], want, where, nan_ok=torch.isnan(want))
    X.assert_bits(f"add_cast n = {n}: out_bf16 against the stored sum", ob[:n], o[:n].bfloat16(), where, nan_ok=torch.isnan(want))
    assert n < 2048 or int(torch.isnan(want).sum()) > 0          # from n = 2048 on the NaNs of the specials are part of it


def test_add_cast_and_cast_refusals():
    lib = _lib()
    _, _, xd, _ = _cast_source()
    out = torch.full((64,), X.SENT, device=X._dev())
    outb = torch.full((64,), X.SENT, dtype=torch.bfloat16, device=X._dev())
    a, b, o, ob, s = xd.data_ptr(), xd.data_ptr() + 4096, out.data_ptr(), outb.data_ptr(), X._stream()
    for args in ((a, b, o, ob, 12), (a, b, o, ob, 0), (a + 4, b, o, ob, 8), (a, b + 8, o, ob, 8), (a, b, o + 4, ob, 8), (a, b, o, ob + 8, 8), (None, b, o, ob, 8), (a, b, o, None, 8)):
        assert lib.xvit_add_cast_f32_bf16(*args, s) != 0, f"xvit_add_cast_f32_bf16 accepted {args}"
        assert "xvit_add_cast_f32_bf16" in X.last_error()
    for args in ((a + 4, ob, 8), (a, ob + 2, 8), (a, ob, 0), (None, ob, 8), (a, None, 8)):
        assert lib.xvit_cast_f32_bf16(*args, s) != 0, f"xvit_cast_f32_bf16 accepted {args}"
        assert "xvit_cast_f32_bf16" in X.last_error()
    torch.cuda.synchronize()
    X.check_tail_guard("out after refusals", out.cpu(), 0)
    X.check_tail_guard("out_bf16 after refusals", outb.cpu(), 0)
