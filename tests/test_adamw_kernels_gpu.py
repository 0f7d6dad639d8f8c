"""GPU: xvit_adamw_step, xvit_adamw_step_dev and xvit_ema_swap element by element (oracle, bounds and arenas: tests/_adamw_check.py).

Against the plain mode of the same template (adam_kernel<., ADAM_PLAIN>): ADAM_COUPLED with every lr_scale 1, one decay and no average must
leave the arenas bit-identical to xvit_adam_step / xvit_adam_step_dev, which guards the extras table and the mode dispatch.  Against the oracle: every placement x {coupled, decoupled} x {no average, all, every other tensor} x every
hyper-parameter set of both tiers (52 launches per case), natural and shuffled chunk lists in turn."""
import itertools
import math

import numpy as np
import pytest
import torch

import _adamw_check as W
import _optim_check as X

pytestmark = pytest.mark.gpu

VEC, SCALAR, EOFF = "aligned, shadow 8-byte aligned", "shadow 2 bytes off", "ema 4 bytes off"
GRID = list(itertools.product(W.PLACEMENTS, (False, True), W.EMA_MODES))


@pytest.mark.parametrize("placement", list(X.PLACEMENTS))
@pytest.mark.parametrize("dev_record", [False, True], ids=["by value", "from the record"])
def test_coupled_without_extras_is_bit_identical_to_the_adam_kernel(placement, dev_record):
    for tier, hs in (("random", X.HYPER_RANDOM[1::7]), ("exact", X.HYPER_EXACT[3::6])):
        for b in hs:
            old = X.AdamCase(placement, tier, order="shuffled")
            rc, want = X.adam_launch(old, b, dev_record=dev_record)
            assert rc == 0, X.last_error()
            case = W.Case(placement, tier, "none", order="shuffled")
            h = W.HyperW(b, False, (1.0,), (b.wd,), w=1.0)
            rc, got = W.launch(case, h, dev_record=dev_record)
            assert rc == 0, X.last_error()
            assert case.vec_t == [old.expect_vec] * len(case.sizes)
            e = got.pop("e")
            assert bool((e == X.SENT).all())
            X.assert_same_arenas(old, f"xvit_adamw_step{'_dev' if dev_record else ''} against xvit_adam_step{'_dev' if dev_record else ''} ({b})", got, want)


@pytest.mark.parametrize("placement,decoupled,ema", GRID, ids=[f"{p}-{'decoupled' if d else 'coupled'}-ema {e}" for p, d, e in GRID])
def test_against_the_oracle(placement, decoupled, ema):
    k = GRID.index((placement, decoupled, ema))
    n = 0
    for tier in ("random", "exact"):
        for i, h in enumerate(W.hypers(tier, decoupled)):
            case = W.Case(placement, tier, ema, order=("natural", "shuffled")[(i + k) % 2])
            rc, after = W.launch(case, h)
            assert rc == 0, X.last_error()
            W.check(case, h, after, log=f"adamw:{placement}:{'dec' if decoupled else 'cpl'}:{ema}:{tier}")
            n += 1
    assert n == len(X.HYPER_RANDOM) + len(X.HYPER_EXACT) == 52


@pytest.mark.parametrize("placement", [VEC, SCALAR, EOFF])
def test_lr_scale_zero_and_no_decay_and_unlisted_chunks(placement):
    sizes = (5, 2 * X.CHUNK + 2, 1027, 16385)
    for tier, b in (("random", X.HYPER_RANDOM[-1]), ("exact", X.HYPER_EXACT[-1])):
        for dec in (False, True):
            h = W.HyperW(b, dec, (0.0,), (0.0,), w=0.5)                  # rate 0, decay 0: p stays, the moments move, the average moves towards p
            case = W.Case(placement, tier, "all", sizes=sizes)
            rc, after = W.launch(case, h)
            assert rc == 0, X.last_error()
            W.check(case, h, after)
            assert torch.equal(after["p"], case.arenas()["p"])
            h = W.hypers(tier, dec)[4]
            case = W.Case(placement, tier, "alternate", sizes=sizes, order=[(1, 1), (3, 0), (0, 0), (2, 0)])       # chunks 0 and 2 of tensor 1, chunk 1 of tensor 3 left out
            rc, after = W.launch(case, h)
            assert rc == 0, X.last_error()
            assert not bool(case.listed.all())
            W.check(case, h, after)


@pytest.mark.parametrize("warmup", [0, 1])
@pytest.mark.parametrize("step", [1, 2, 9, 10000])
def test_from_the_record(step, warmup):
    for tier, b in (("random", X.Hyper(step=step, wd=0.05, scale=1.0 / 3.0)), ("exact", X.Hyper(b1=0.5, b2=0.75, step=step, wd=2.0 ** -4, scale=0.25))):
        for k, (placement, dec, ema) in enumerate(((VEC, True, "all"), (EOFF, True, "alternate"), (SCALAR, False, "all"))):
            sc, wd = (W.SCALES_R, W.WDS_R) if tier == "random" else (W.SCALES_E, W.WDS_E)
            h = W.HyperW(b, dec, sc, wd, ema_decay=(0.999, 0.5)[k % 2], warmup=warmup)
            case = W.Case(placement, tier, ema, order="shuffled")
            rc, after = W.launch(case, h, dev_record=True)                 # asserts that the record and the words round it are untouched
            assert rc == 0, X.last_error()
            W.check(case, h, after, log=f"adamw:record:step{step}:warmup{warmup}:{tier}")
            rc, after = W.launch(case, h, dev_record=True, skip=1)
            assert rc == 0, X.last_error()
            X.assert_same_arenas(case, "a skipped step", after, case.arenas())


@pytest.mark.parametrize("ema", ["all", "alternate", "none"])
@pytest.mark.parametrize("placement", list(W.PLACEMENTS))
def test_ema_swap(placement, ema):
    h = W.hypers("random", True)[0]
    for order in ("shuffled", None):
        sizes = X.SIZES if order else (5, 2 * X.CHUNK + 2, 1027)
        case = W.Case(placement, "random", ema, sizes=sizes, order=order or [(1, 1), (2, 0)])
        once = W.swap_launch(case, h)
        X.assert_same_arenas(case, "xvit_ema_swap", once, W.swap_expected(case))       # guards, g, m, v, null-ema tensors and unlisted chunks included
        twice = W.swap_launch(case, h, times=2)
        X.assert_same_arenas(case, "xvit_ema_swap twice", twice, case.arenas())


def test_refusals_write_nothing():
    from xvit import _lib
    lib = _lib.load()
    case = W.Case(VEC, "random", "all", sizes=(5, 1027))
    h = W.hypers("random", True)[0]
    d = W.device_case(case, h)
    t, x, c, n, s = d["table"].data_ptr(), d["extras"].data_ptr(), d["chunks"].data_ptr(), len(case.chunks), X._stream()
    rec = np.zeros((), dtype=X.REC)
    rec["step"], rec["lr"], rec["lr_over_bc1"], rec["inv_sqrt_bc2"], rec["clip_coef"] = 1, 1e-3, 1e-2, 1.0, 1.0
    w = X.record_window(rec).to(X._dev())
    r = w.data_ptr() + 8 * X.REC_GUARD
    step = lambda **o: lib.xvit_adamw_step(*[o.get(k, v) for k, v in (("t", t), ("x", x), ("c", c), ("n", n), ("lr", 1e-3), ("b1", 0.9), ("b2", 0.98), ("eps", 1e-8),   # noqa: E731
                                                                       ("step", 1), ("gs", 1.0), ("dec", 1), ("w", 0.1), ("s", s))])
    stepd = lambda **o: lib.xvit_adamw_step_dev(*[o.get(k, v) for k, v in (("t", t), ("x", x), ("c", c), ("n", n), ("r", r), ("b1", 0.9), ("b2", 0.98), ("eps", 1e-8),   # noqa: E731
                                                                            ("dec", 1), ("d", 0.99), ("warm", 0), ("s", s))])
    swap = lambda **o: lib.xvit_ema_swap(*[o.get(k, v) for k, v in (("t", t), ("x", x), ("c", c), ("n", n), ("s", s))])   # noqa: E731
    bad = [(step, dict(t=None)), (step, dict(x=None)), (step, dict(c=None)), (step, dict(n=0)), (step, dict(n=-1)), (step, dict(b1=1.0)), (step, dict(b1=-0.1)),
           (step, dict(b2=1.0)), (step, dict(eps=-1e-8)), (step, dict(step=0)), (step, dict(w=-0.1)), (step, dict(w=1.5)), (step, dict(w=math.nan)),
           (stepd, dict(t=None)), (stepd, dict(x=None)), (stepd, dict(c=None)), (stepd, dict(r=None)), (stepd, dict(n=0)), (stepd, dict(b1=1.0)), (stepd, dict(b2=-0.5)),
           (stepd, dict(eps=-1.0)), (stepd, dict(d=1.0)), (stepd, dict(d=-0.1)), (stepd, dict(d=math.nan)),
           (swap, dict(t=None)), (swap, dict(x=None)), (swap, dict(c=None)), (swap, dict(n=0))]
    for fn, o in bad:
        assert fn(**o) != 0, o
        name = {step: "xvit_adamw_step:", stepd: "xvit_adamw_step_dev:", swap: "xvit_ema_swap:"}[fn]
        assert X.last_error().startswith(name), (o, X.last_error())
    torch.cuda.synchronize()
    X.assert_same_arenas(case, "after the refused calls", {k: d[k].cpu() for k in case.starts}, case.arenas())
    assert bytes(X.record_of("refusals", w).tobytes()) == rec.tobytes()
    assert step() == 0 and stepd() == 0 and swap() == 0                   # the same arguments unbroken are accepted
    torch.cuda.synchronize()
