"""The gate of the optimizer, mask and cast checks (tests/_optim_check.py) has teeth, on the CPU.

Mirror needs.  The float32 CPU mirror of adam_kernel's update runs over every hyper-parameter set and operand the GPU tests use and stays
inside every stated bound; its needs are printed, noted, compared with the table in _optim_check's docstring, and C_u / C_div are
re-derived from them (the power of two at or above 4 x the need).

Planted faults.  Each starts from what a correct launch leaves (`adam_written`, `sqnorm_written`, `dropout_expected`), plants ONE defect
and states two outcomes: the new check names it (tensor, chunk, path and element), and what the existing whole-tensor gates of
tests/test_optim_gpu.py (rel-L2 < 2e-6 on every p, < 5e-6 on every moment, against float64) say on the same data.  Nothing was bent to
make them miss; both outcomes are asserted.  The sizes here are at most 32770 elements, so a one-element fault weighs more in a tensor's
norm than it does in a 768 x 768 weight.

  fault                                          new check   whole-tensor gates on the same data (largest rel-L2: p, moments)
  eps inside the root, eps = 1e-3                caught      seen on p
  decay added before the clip scale              caught      seen on p and the moments
  bias corrections of step - 1 (step 2)          caught      seen on p
  beta2 used for beta1                           caught      seen
  m and v swapped                                caught      seen
  last element of a vector body skipped          caught      seen at n = 1027: p 4.2e-6, moments 1.2e-2 (one stale moment of 1027)
  one tail element skipped                       caught      seen at n = 1027: p 1.1e-5, moments 9.6e-3
  one stale element of the 32770-element tensor  caught      seen: p 1.9e-5, moments 2.5e-3; p falls below its gate from about 3e6 elements on
  a chunk end one too far                        caught      not seen: 0, 0 (they never look behind a tensor)
  shadow taken from the old p                    caught      not seen: 0, 0 (they never look at the shadow)
  shadow truncated instead of rounded            caught      not seen: 0, 0
  g overwritten                                  caught      not seen: 0, 0 (g is not compared)
  a partial written one slot late                caught      (no whole-tensor gate sees partials)
  > for >= in keep                               caught at THRESHOLD_SEED only; any other seed of the suite gives the same mask
  thr rounded instead of truncated               caught at THIRD_SEED, p = 1/3 only
  the >> 16 of the hash dropped                  caught
  the epoch constant added instead of multiplied caught"""
import math

import numpy as np
import pytest
import torch

import _optim_check as X
from _util import note

VEC, SCALAR = "aligned, shadow 8-byte aligned", "shadow 2 bytes off"
T1027 = X.SIZES.index(1027)


def _caught(what, fn, *needles):
    with pytest.raises(AssertionError) as e:
        fn()
    msg = str(e.value)
    print(f"caught: {what}: {msg[:400]}")
    for n in needles:
        assert n in msg, f"{what}: the message does not say {n!r}: {msg}"
    return msg


# ---------------------------------------------------------------------------------------------------------------- geometry mirror
def test_path_mirror_and_where():
    assert X.vec_ok(0x1000, 0x2000, 0x3000, 0x4000, 0) and X.vec_ok(0x1000, 0x2000, 0x3000, 0x4000, 0x5008)
    assert not X.vec_ok(0x1000, 0x2000, 0x3000, 0x4000, 0x5002) and not X.vec_ok(0x1000, 0x2000, 0x3000, 0x4000, 0x5004)
    for k in range(4):
        a = [0x1000, 0x2000, 0x3000, 0x4000]
        a[k] += 4
        assert not X.vec_ok(*a, 0)
    for name, pl in X.PLACEMENTS.items():            # the arenas really put the tensors where the placement says
        c = X.AdamCase(name, "random")
        rows = c.table({k: 0x10000 * (i + 1) for i, k in enumerate(("p", "g", "m", "v", "sh"))})
        assert {X.vec_ok(*r[:5]) for r in rows} == {pl["vec"]}, name
        for k in c.starts:
            unit = 8 if k == "sh" else 4
            assert all(s % unit == pl[k] and s >= X.GUARD for s in c.starts[k])
            ends = [s + n for s, n in zip(c.starts[k], c.sizes)]
            assert all(s - e >= X.GUARD for s, e in zip(c.starts[k][1:], ends)) and c.total[k] - ends[-1] == X.GUARD
        if name == "aligned, shadow 8-byte aligned":
            assert all((2 * s) % 16 == 8 for s in c.starts["sh"])        # 8-byte aligned and NOT 16
    assert X.where(1027, 1023, True).endswith("vector body, iteration 0, thread 255, lane 3")
    assert X.where(1027, 1026, True).endswith("tail, thread 2")
    assert X.where(16387, 16386, True).startswith("chunk 1 of 2 [16384, 16387)") and X.where(16387, 16386, True).endswith("tail, thread 2")
    assert X.where(16385, 16383, True).endswith("iteration 15, thread 255, lane 3")
    assert X.where(1025, 1024, False).endswith("scalar path, element 1024: iteration 4, thread 0")
    assert [X.n_chunks(n) for n in X.SIZES] == [1] * 11 + [2, 2, 3]
    natural, shuffled = X.AdamCase(VEC, "exact"), X.AdamCase(VEC, "exact", order="shuffled")
    assert sorted(shuffled.chunks) == natural.chunks and shuffled.chunks != natural.chunks and bool(shuffled.listed.all())


# ---------------------------------------------------------------------------------------------------------------- mirror needs
def test_float32_mirror_stays_inside_every_bound_and_sets_the_constants():
    needs, shares = {}, {}
    for tier, hypers in (("exact", X.HYPER_EXACT), ("random", X.HYPER_RANDOM)):
        for i, h in enumerate(hypers):
            case = X.AdamCase((VEC, SCALAR)[i % 2], tier, order=("natural", "shuffled")[i % 2])
            out = X.adam_check(case, h, X.adam_written(case, h))
            needs[tier] = max(needs.get(tier, 0.0), out["need_upd"])
            for k in ("p", "m", "v"):
                shares[tier, k] = max(shares.get((tier, k), 0.0), out[k])
    div = X.div_mirror_need()
    print(f"mirror needs: upd exact {needs['exact']:.2f}, upd random {needs['random']:.2f}, clip_coef {div:.2f}; largest shares of the bounds {shares}")
    for k, v in (("upd_exact", needs["exact"]), ("upd_random", needs["random"]), ("div", div)):
        note(f"optim:mirror:need_{k}", v)
    assert round(needs["exact"], 2) == 2.17 and needs["random"] == 0.0 and round(div, 2) == 0.67        # the table of the docstring
    assert X.C["upd"] == X.pow2_at_or_above(4 * needs["exact"]) == 16.0
    assert X.C["div"] == X.pow2_at_or_above(4 * div) == 4.0
    assert (X.C["m"], X.C["v"], X.C["g"]) == (2.0, 3.0, 2.0) and X.NORM_ROUNDINGS == {"scalar": 72, "vec": 27}
    assert shares["exact", "m"] == 0.0 and shares["exact", "v"] == 0.0                                  # the mirror is bit-exact there too


def test_partials_and_prologue_mirrors_pass():
    for tier in ("exact", "random"):
        for pl in (VEC, SCALAR):
            case = X.AdamCase(pl, tier, order="shuffled")
            X.sqnorm_check(case, X.sqnorm_written(case))
    for name, part, square, mx, step0 in X.prologue_cases():      # the host's own arithmetic as the record a correct prologue leaves
        rec0 = np.zeros((), dtype=X.REC)
        rec0["step"], rec0["lr"], rec0["skip"] = step0, 3e-3, 1
        rec = rec0.copy()
        norm = np.float32(math.sqrt(float(part.double().sum())))
        c = np.float32(mx) / (norm + np.float32(1e-6))
        rec["grad_norm"], rec["clip_coef"], rec["step"], rec["skip"] = norm, (c if c < 1 else 1.0), step0 + 1, 0
        h = X.Hyper(lr=3e-3, step=step0 + 1)
        rec["lr_over_bc1"], rec["inv_sqrt_bc2"] = X.host_numbers(h)
        X.prologue_check(name, part, rec0, rec, mx, 0.9, 0.98, 0, square=square)
        bad = rec.copy()
        bad["step"] = step0
        _caught("prologue: step not advanced", lambda: X.prologue_check(name, part, rec0, bad, mx, 0.9, 0.98, 0, square=square), "want step")
        if not math.isinf(mx) and c < 1:
            bad = rec.copy()
            bad["clip_coef"] = np.float32(c) * np.float32(1 + 2.0 ** -20)
            _caught("prologue: clip_coef 8 ulps off", lambda: X.prologue_check(name, part, rec0, bad, mx, 0.9, 0.98, 0, square=square), "clip_coef")


# ---------------------------------------------------------------------------------------------------------------- planted faults: formula
FORMULA = [  # fault, hyper, seen by the whole-tensor gates
    ("eps inside the root", X.Hyper(eps=1e-3, wd=0.05, scale=0.25, step=2), True),
    ("decay added before the clip scale", X.Hyper(eps=1e-8, wd=0.05, scale=0.25, step=2), True),
    ("bias corrections of step - 1", X.Hyper(eps=1e-8, wd=0.0, scale=1.0, step=2), True),
    ("beta2 used for beta1", X.Hyper(eps=1e-8, wd=0.0, scale=1.0, step=2), True),
    ("m and v swapped", X.Hyper(eps=1e-8, wd=0.0, scale=1.0, step=2), True),
]


@pytest.mark.parametrize("fault,h,seen", FORMULA, ids=[f[0] for f in FORMULA])
@pytest.mark.parametrize("placement", [VEC, SCALAR])
def test_formula_faults_are_caught_and_placed(placement, fault, h, seen):
    case = X.AdamCase(placement, "random")
    after = X.adam_written(case, h, fault)
    _caught(fault, lambda: X.adam_check(case, h, after), "tensor ", "chunk ", "16-byte path" if placement == VEC else "scalar path", "element ")
    rp, rm, old = X.old_gates(case, h, after)
    print(f"{fault}: whole-tensor gates: rel p {rp:.2e}, moments {rm:.2e}: {'seen' if old else 'not seen'}")
    assert old == seen


# ---------------------------------------------------------------------------------------------------------------- planted faults: layout
def _stale(case, after, t, i, keys=("p", "m", "v", "sh")):
    before = case.arenas()
    for k in keys:
        after[k][case.starts[k][t] + i] = before[k][case.starts[k][t] + i]


def _plant_body(case, h, after):
    _stale(case, after, T1027, 1023)


def _plant_tail(case, h, after):
    _stale(case, after, T1027, 1026)


def _plant_end(case, h, after):                       # element n of tensor 1027: g there is NaN, so what is written is NaN
    for k in ("p", "m", "v"):
        after[k][case.starts[k][T1027] + 1027] = math.nan


def _plant_old_shadow(case, h, after):
    after["sh"][case.pos["sh"]] = case.arenas()["sh"][case.pos["sh"]]


def _plant_trunc_shadow(case, h, after):
    p = after["p"][case.pos["p"]]
    after["sh"][case.pos["sh"]] = (p.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)


def _plant_g(case, h, after):
    after["g"][case.starts["g"][T1027] + 5] *= 0.25


LAYOUT = [  # fault, plant, needles, seen by the whole-tensor gates
    ("the last element of a vector body skipped", _plant_body, ("tensor 8 (n = 1027)", "chunk 0 of 1", "16-byte path", "element 1023: vector body, iteration 0, thread 255, lane 3"), True),
    ("one tail element skipped", _plant_tail, ("tensor 8 (n = 1027)", "16-byte path", "element 1026: tail, thread 2"), True),
    ("a chunk end one too far", _plant_end, ("guard", "0 element(s) behind the end of tensor 8 (n = 1027)", "16-byte path"), False),
    ("shadow taken from the old p", _plant_old_shadow, ("shadow", "tensor ", "chunk ", "16-byte path", "element "), False),
    ("shadow truncated instead of rounded", _plant_trunc_shadow, ("shadow", "tensor ", "chunk ", "16-byte path", "element "), False),
    ("g overwritten", _plant_g, ("g was overwritten", "tensor 8 (n = 1027)", "chunk 0 of 1", "element 5"), False),
]


@pytest.mark.parametrize("fault,plant,needles,seen", LAYOUT, ids=[f[0] for f in LAYOUT])
@pytest.mark.parametrize("tier", ["exact", "random"])
def test_layout_faults_are_caught_and_placed(tier, fault, plant, needles, seen):
    h = (X.HYPER_EXACT if tier == "exact" else X.HYPER_RANDOM)[3]
    case = X.AdamCase(VEC, tier)
    after = X.adam_written(case, h)
    X.adam_check(case, h, after)                      # the unfaulted launch passes
    plant(case, h, after)
    _caught(fault, lambda: X.adam_check(case, h, after), *needles)
    rp, rm, old = X.old_gates(case, h, after)
    print(f"{fault} ({tier}): whole-tensor gates: rel p {rp:.2e}, moments {rm:.2e}: {'seen' if old else 'not seen'}")
    assert old == seen


def test_one_stale_element_of_the_largest_tensor_and_the_whole_tensor_gates():
    """The same stale element in the 32770-element tensor: the element-wise check names it; what the old gates say is put on record."""
    h = X.HYPER_RANDOM[3]
    case = X.AdamCase(SCALAR, "random")
    after = X.adam_written(case, h)
    _stale(case, after, len(X.SIZES) - 1, 2 * X.CHUNK + 1)
    _caught("last element of the last chunk skipped", lambda: X.adam_check(case, h, after), "tensor 13 (n = 32770)", "chunk 2 of 3", "scalar path", "element 32769: iteration 0, thread 1")
    rp, rm, old = X.old_gates(case, h, after)
    print(f"one stale element of 32770: rel p {rp:.2e} (gate 2e-6), moments {rm:.2e} (gate 5e-6)")
    assert old and 2e-6 < rp < 1e-4          # the update of one element against the norm of 32770 values: ten times the gate here, below it from ~3e6 elements on


def test_unlisted_chunk_written_is_caught():
    h = X.HYPER_RANDOM[-1]
    case = X.AdamCase(VEC, "random", sizes=(5, 2 * X.CHUNK + 2, 1027), order=[(1, 1)])
    after = X.adam_written(case, h)
    X.adam_check(case, h, after)
    full = X.adam_written(X.AdamCase(VEC, "random", sizes=(5, 2 * X.CHUNK + 2, 1027)), h)
    after["m"][case.starts["m"][1] + 2 * X.CHUNK] = full["m"][case.starts["m"][1] + 2 * X.CHUNK]
    _caught("chunk 2 updated though only chunk 1 is listed", lambda: X.adam_check(case, h, after), "a chunk the list does not name", "tensor 1 (n = 32770)", "chunk 2 of 3")


def test_a_partial_written_one_slot_late_is_caught():
    for tier in ("exact", "random"):
        case = X.AdamCase(VEC, tier)
        w = X.sqnorm_written(case)
        n = len(case.chunks)
        late = w.clone()
        late[1:n + 1] = w[:n]
        late[0] = math.nan
        _caught("a partial written one slot late", lambda: X.sqnorm_check(case, late), f"guard behind the {n} partials", f"slot {n}")
        swapped = w.clone()
        swapped[[11, 12]] = w[[12, 11]]                # the two chunks of the 16385-element tensor exchanged
        _caught("two partials exchanged", lambda: X.sqnorm_check(case, swapped), "partial 11 = tensor 11 (n = 16385), chunk 0 of 2", "16-byte path")


# ---------------------------------------------------------------------------------------------------------------- the mask mirror
HAND = [  # (seed, idx, hash32) worked out once from xvit_common.h:274 with integers of unbounded width, masked to 64 bits after each step
    (0, 0, 0x00000000), (0, 1, 0xA8397B1D), (1234, 5, 0xE3FF44B1), (2 ** 32 + 7, 2 ** 32 + 11, 0x59AB8BE6), (2 ** 64 - 1, 3, 0xF84CB272),
    (2 ** 64 - 1, 2 ** 40 + 1, 0x3D31FA6F), (8, 1752363, 0x1D400000), (13, 421518, 0xA5555555)]


def test_hash_mirror_against_hand_computed_values_and_64_bit_indices():
    for seed, idx, want in HAND:
        assert X.hash32_int(seed, idx) == want, (seed, idx)
        assert int(X.hash32_np(seed, np.array([idx], dtype=np.uint64))[0]) == want, (seed, idx)
    idx = np.array([0, 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 12345, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)
    for seed in (0, 1234, 2 ** 32 + 12345, 2 ** 64 - 1):
        assert [int(v) for v in X.hash32_np(seed, idx)] == [X.hash32_int(seed, int(i)) for i in idx]
    assert X.epoch_seed(2 ** 64 - 1, 1) == (X.EPOCH_MUL - 1) and X.epoch_seed(5, 2 ** 40 + 5) == (5 + (2 ** 40 + 5) * X.EPOCH_MUL) % 2 ** 64 and X.epoch_seed(7, None) == 7
    assert X.drop_params(0.25) == (1 << 22, np.float32(4.0) / np.float32(3.0)) and X.drop_params(0.0)[0] == 0 and X.drop_params(1.0 / 3.0)[0] == 5592405
    assert X.drop_params(0.9)[0] == int(np.float32(0.9) * np.float32(2 ** 24)) == 15099494
    assert int(X.draw24_np(X.THRESHOLD_SEED, 1, start=X.THRESHOLD_INDEX)[0]) == 1 << 22
    assert int(X.draw24_np(X.THIRD_SEED, 1, start=X.THIRD_INDEX)[0]) == 5592405


def test_mask_faults_are_caught_only_where_the_cases_reach_them():
    n = 2 * 2 ** 20 + 3
    x = torch.randn(n, generator=torch.Generator().manual_seed(3))

    def differs(p, seed, fault, epoch=None):
        want, got = X.dropout_expected(x, p, seed, epoch), X.dropout_expected(x, p, seed, epoch, fault=fault)
        try:
            X.assert_bits(fault, got, want, X.where_drop)
        except AssertionError as e:
            print(f"caught: {fault} (p {p:g}, seed {seed}): {str(e)[:200]}")
            return str(e)
        return None
    msg = differs(0.25, X.THRESHOLD_SEED, "> for >= in keep")
    assert msg and f"1 of {n} elements differ" in msg and f"element {X.THRESHOLD_INDEX}: grid-stride round 1" in msg
    assert all(differs(0.25, s, "> for >= in keep") is None for s in (0, 1, 7))           # without that seed the two cannot be told apart
    msg = differs(1.0 / 3.0, X.THIRD_SEED, "thr rounded instead of truncated")
    assert msg and f"1 of {n} elements differ" in msg and f"element {X.THIRD_INDEX}: grid-stride round 0" in msg
    assert differs(1.0 / 3.0, 0, "thr rounded instead of truncated") is None and differs(0.25, X.THRESHOLD_SEED, "thr rounded instead of truncated") is None
    assert differs(0.25, 1234, "the >> 16 of the hash dropped")
    for epoch in (0, 1, 2 ** 40 + 5):
        assert differs(0.25, 1234, "the epoch constant added instead of multiplied", epoch=epoch)
    y = X.dropout_expected(torch.tensor([-0.0, 0.0, 1.0, -1.0] * 64), 0.5, 1234)            # kept zeros keep their sign, dropped elements are +0
    keep = torch.from_numpy(X.keep_mask(256, 0.5, 1234))
    sign = torch.signbit(y)
    assert bool((sign == (keep & torch.tensor([True, False, False, True] * 64))).all()) and 64 < int(keep.sum()) < 192
