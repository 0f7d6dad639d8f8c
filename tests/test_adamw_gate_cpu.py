"""The gate of the AdamW checks (tests/_adamw_check.py) has teeth, on the CPU: the float32 mirror of adam_kernel's per-tensor modes stays inside every stated
bound over the inputs the GPU tests use and sets the constants table of the docstring, and every planted fault is caught.

  fault                                                  caught by
  decay applied after the update                         p
  decay with lr / bc1 instead of lr (step 2)             p
  lr_scale left out of the decay factor                  p
  EMA of the old p                                       ema
  w and 1 - w swapped                                    ema
  warm-up using step - 1 (record path, step 2)           ema
  the coupled formula in decoupled mode                  m (and v, p)
  an average written for a null-ema tensor's neighbour   the slot of the null-ema tensor, which is compared like a guard"""
import pytest
import torch

import _adamw_check as W
import _optim_check as X
from _util import note

VEC, SCALAR, EOFF = "aligned, shadow 8-byte aligned", "shadow 2 bytes off", "ema 4 bytes off"


def _caught(what, fn, *needles):
    with pytest.raises(AssertionError) as e:
        fn()
    msg = str(e.value)
    print(f"caught: {what}: {msg[:400]}")
    for n in needles:
        assert n in msg, f"{what}: the message does not say {n!r}: {msg}"


def test_path_mirror_and_placements():
    a = (0x1000, 0x2000, 0x3000, 0x4000, 0x5008)
    assert W.vec_ok(*a, 0) and W.vec_ok(*a, 0x6000) and not W.vec_ok(*a, 0x6004) and not W.vec_ok(*a, 0x6008)
    assert not W.vec_ok(0x1004, 0x2000, 0x3000, 0x4000, 0, 0x6000)
    for name, pl in W.PLACEMENTS.items():
        for ema in W.EMA_MODES:
            c = W.Case(name, "random", ema)
            h = W.hypers("random", True)[0]
            base = {k: 0x100000 * (i + 1) for i, k in enumerate(W.KEYS)}
            rows, ex = c.table(base), c.extras(base["e"], h)
            want = [pl["vec"] if name != EOFF else not has for has in c.has_ema]          # per tensor: a NULL average constrains nothing
            assert [W.vec_ok(*r[:5], int(x["ema"])) for r, x in zip(rows, ex)] == want == c.vec_t, (name, ema)
            assert [int(x["ema"]) != 0 for x in ex] == c.has_ema
            assert all(s % 4 == pl["e"] and s >= X.GUARD for s in c.starts["e"])
    assert W.Case(VEC, "exact", "alternate").has_ema[:4] == [True, False, True, False]


def test_float32_mirror_stays_inside_every_bound_and_sets_the_constants():
    needs, shares, n_exact = {}, {}, 0
    for tier in ("exact", "random"):
        for dec in (False, True):
            for i, h in enumerate(W.hypers(tier, dec)):
                case = W.Case((VEC, SCALAR, EOFF)[i % 3], tier, W.EMA_MODES[1 + i % 2], order=("natural", "shuffled")[i % 2])
                out = W.check(case, h, W.written(case, h))
                needs[tier] = max(needs.get(tier, 0.0), out["need_upd"])
                for k in ("p", "m", "v", "e"):
                    shares[tier, k] = max(shares.get((tier, k), 0.0), out[k])
                n_exact += out.get("e_exact", 0)
    # the record path's own w (warm-up on and off) on both tiers
    for tier in ("exact", "random"):
        for step in (1, 2, 9, 10000):
            for warm in (0, 1):
                b = X.Hyper(b1=0.5, b2=0.75, step=step) if tier == "exact" else X.Hyper(step=step)
                h = W.HyperW(b, True, W.SCALES_E if tier == "exact" else W.SCALES_R, (0.0,), ema_decay=0.999, warmup=warm)
                case = W.Case(VEC, tier, "all")
                shares[tier, "e"] = max(shares[tier, "e"], W.check(case, h, W.written(case, h))["e"])
    print(f"mirror needs of C_u: exact {needs['exact']:.2f}, random {needs['random']:.2f}; largest shares of the bounds {shares}; {n_exact} averages compared bit for bit")
    for k, v in needs.items():
        note(f"adamw:mirror:need_upd_{k}", v)
    rows = {l.split()[0]: l.split() for l in W.__doc__.splitlines() if l.split() and l.split()[0] in ("upd_exact", "upd_random")}
    assert needs["random"] == 0.0 and rows["upd_random"][1] == "0.00"                                    # the table of the docstring
    assert X.pow2_at_or_above(4 * needs["exact"]) == W.C_UPD == float(rows["upd_exact"][6])              # the constant follows from THIS host's mirror
    assert max(shares["exact", "e"], shares["random", "e"]) <= 1.0 and n_exact > 10000
    assert shares["exact", "m"] == 0.0 and shares["exact", "v"] == 0.0


_B = X.Hyper(eps=1e-8, step=2, scale=0.25)
_WD = (0.05, 0.3, 0.01)
FORMULA = [  # fault, hyper, what the message names
    ("decay applied after the update", W.HyperW(_B, True, W.SCALES_R, _WD, w=0.1), "p ("),
    ("decay with lr / bc1", W.HyperW(_B, True, W.SCALES_R, _WD, w=0.1), "p ("),
    ("lr_scale left out of the decay factor", W.HyperW(_B, True, W.SCALES_R, _WD, w=0.1), "p ("),
    ("EMA of the old p", W.HyperW(_B, True, W.SCALES_R, _WD, w=0.1), "ema ("),
    ("w and 1 - w swapped", W.HyperW(_B, True, W.SCALES_R, _WD, w=0.1), "ema ("),
    ("warm-up using step - 1", W.HyperW(_B, True, W.SCALES_R, _WD, ema_decay=0.999, warmup=1), "ema ("),
    ("the coupled formula in decoupled mode", W.HyperW(_B, True, W.SCALES_R, _WD, w=0.1), "m ("),
]
assert [f[0] for f in FORMULA] == list(W.FAULTS)


@pytest.mark.parametrize("fault,h,names", FORMULA, ids=[f[0] for f in FORMULA])
@pytest.mark.parametrize("placement", [VEC, SCALAR, EOFF])
def test_formula_faults_are_caught_and_placed(placement, fault, h, names):
    case = W.Case(placement, "random", "all")
    W.check(case, h, W.written(case, h))                  # the unfaulted launch passes
    _caught(fault, lambda: W.check(case, h, W.written(case, h, fault)), names, "tensor ", "chunk ", "16-byte path" if placement == VEC else "scalar path", "element ")


@pytest.mark.parametrize("tier", ["exact", "random"])
def test_an_average_written_next_to_a_null_ema_tensor_is_caught(tier):
    h = W.hypers(tier, True)[3]
    case = W.Case(VEC, tier, "alternate")
    after = W.written(case, h)
    W.check(case, h, after)
    t = X.SIZES.index(1027)                               # tensor 8 has an average, tensor 9 (n = 16383) has none
    assert case.has_ema[t] and not case.has_ema[t + 1]
    after["e"][case.starts["e"][t + 1]] = 0.5
    _caught("an average written for a null-ema tensor", lambda: W.check(case, h, after), "ema is NULL", "tensor 9 (n = 16383)", "element 0")
    after = W.written(case, h)
    after["e"][case.starts["e"][t] + 1027] = 0.5           # one element behind the end of a tensor that has one
    _caught("a chunk end one too far in the average", lambda: W.check(case, h, after), "guard elements of `e`", "behind the end of tensor 8 (n = 1027)")


def test_unlisted_chunks_and_the_swap_mirror():
    h = W.hypers("random", True)[4]                       # w = 0.1 (w = 0 would leave the average where it was)
    assert h.w == 0.1
    case = W.Case(VEC, "random", "all", sizes=(5, 2 * X.CHUNK + 2, 1027), order=[(1, 1)])
    after = W.written(case, h)
    W.check(case, h, after)
    full = W.written(W.Case(VEC, "random", "all", sizes=(5, 2 * X.CHUNK + 2, 1027)), h)
    after["e"][case.starts["e"][1] + 2 * X.CHUNK] = full["e"][case.starts["e"][1] + 2 * X.CHUNK]
    _caught("the average of chunk 2 updated though only chunk 1 is listed", lambda: W.check(case, h, after), "`e` changed in a chunk the list does not name", "chunk 2 of 3")
    c = W.Case(VEC, "random", "alternate")
    a, s = c.arenas(), W.swap_expected(c)
    t0, t1 = c.starts["p"][0], c.starts["p"][1]
    assert s["p"][t0] == a["e"][c.starts["e"][0]] and s["e"][c.starts["e"][0]] == a["p"][t0] and s["sh"][c.starts["sh"][0]] == a["e"][c.starts["e"][0]].bfloat16()
    assert torch.equal(s["p"][t1:t1 + 3], a["p"][t1:t1 + 3]) and s["e"][c.starts["e"][1]] == X.SENT
