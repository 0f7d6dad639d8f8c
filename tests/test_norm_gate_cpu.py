"""CPU: the gates of tests/_norm_check.py have teeth.  The reference passes its own gate; each planted defect (a rank off by one, a sample
standard deviation, a background voxel counted, a stale bin count of 1, a clamp applied after the affine) is refused on the test inputs;
the fold gate refuses a fold in the wrong order, a touched slot and a missing clamp flag."""
import numpy as np
import pytest

import _augment_check as K
import _norm_check as NC

PCTS = [None, (0.0, 1.0), (0.005, 0.995), (0.5, 0.5)]


def _inputs():
    rng = np.random.default_rng(0)
    return [(NC.brain_like(rng, 3, (33, 31, 17), plant=(-1, 0)), True), (NC.signed_bf16(rng, 3, (33, 31, 17), plant=(-1.0, 0.0)), False)]


def _distinct_inputs():
    """Every value once: neighbouring ranks then hold different values, so a rank off by one cannot hide inside a tie."""
    rng = np.random.default_rng(4)
    ints = np.stack([rng.permutation(np.arange(-2000, 6000)) for _ in range(2)]).astype(np.int16)
    floats = np.stack([rng.permutation(np.arange(-128, 256)) for _ in range(2)]).astype(np.float32)      # all exact in bf16
    return [(ints, True), (floats, False)]


@pytest.mark.parametrize("pct", PCTS, ids=str)
@pytest.mark.parametrize("fg", [0.0, -np.inf, 100.5], ids=str)
def test_reference_passes_and_every_planted_defect_is_refused(fg, pct):
    for vols, is_int in _inputs():
        ref, mean_abs = NC.stats_ref_all(vols, fg, pct)
        NC.check_stats("reference", ref, ref, mean_abs, is_int)
        assert np.all(ref[:, NC.N] > 0) and np.all(ref[:, NC.N_W] <= ref[:, NC.N]) and np.all(ref[:, NC.LO] <= ref[:, NC.HI])
        faults = ["sample_std", ("stale_bin", 17.0)]
        if fg != -np.inf:
            faults.append("background_counted")        # with -inf there is no background to count
        for fault in faults:
            bad, _ = NC.stats_ref_all(vols, fg, pct, fault=fault)
            if fault == "sample_std" and np.all(ref[:, NC.STD] == 0):
                continue                                # (0.5, 0.5) on distinct values: a window of ties has no deviation to mis-scale
            with pytest.raises(AssertionError):
                NC.check_stats(str(fault), bad, ref, mean_abs, is_int)


@pytest.mark.parametrize("pct", PCTS[1:], ids=str)
@pytest.mark.parametrize("fg", [0.0, -np.inf, 100.5], ids=str)
def test_a_rank_off_by_one_is_refused(fg, pct):
    for vols, is_int in _distinct_inputs():
        ref, mean_abs = NC.stats_ref_all(vols, fg, pct)
        NC.check_stats("reference", ref, ref, mean_abs, is_int)
        bad, _ = NC.stats_ref_all(vols, fg, pct, fault="rank_off_by_one")
        with pytest.raises(AssertionError):
            NC.check_stats("rank_off_by_one", bad, ref, mean_abs, is_int)


def test_rank_rule_and_definitions_on_a_hand_case():
    v = np.array([0, 5, 1, 3, 3, 3, 9, -4, 0, 2], dtype=np.int16)          # F (v > 0) sorted: 1 2 3 3 3 5 9, n = 7
    rec, _ = NC.stats_ref(v, 0.0, None)
    assert rec.tolist()[:2] == [7, 7] and rec[NC.LO] == 1 and rec[NC.HI] == 9 and rec[NC.MEAN] == 26 / 7
    rec, _ = NC.stats_ref(v, 0.0, (0.3, 0.8))                              # k = ceil(2.1) = 3, ceil(5.6) = 6 -> lo = 3, hi = 5; W = 3 3 3 5
    assert rec[NC.LO] == 3 and rec[NC.HI] == 5 and rec[NC.N_W] == 4 and rec[NC.MEAN] == 3.5 and rec[NC.STD] == np.sqrt(0.75)
    assert rec[NC.MIN] == 1 and rec[NC.MAX] == 9
    rec, _ = NC.stats_ref(v, 0.0, (0.0, 0.0))                              # k = max(1, 0) = 1
    assert rec[NC.LO] == rec[NC.HI] == 1 and rec[NC.N_W] == 1 and rec[NC.STD] == 0
    rec, _ = NC.stats_ref(v, -np.inf, None)
    assert rec[NC.N] == 10 and rec[NC.MIN] == -4
    rec, _ = NC.stats_ref(np.array([0, -1, 0], dtype=np.int16), 0.0, (0.005, 0.995))
    assert not rec.any()                                                   # no foreground: a record of zeros
    rec, _ = NC.stats_ref(np.array([1.0, np.nan, -2.0], dtype=np.float32), -np.inf, None)
    assert rec[NC.N] == 2 and rec[NC.MIN] == -2 and rec[NC.MAX] == 1      # NaN is never foreground
    assert NC.rank(0.005, 2000) == 10 and NC.rank(0.995, 2000) == 1991     # the fp32 0.995 lies above 199 / 200: the product in double exceeds 1990
    assert NC.rank(0.5, 7) == 4 and NC.rank(1.0, 7) == 7 and NC.rank(0.0, 7) == 1


def test_mean_gates_separate_int16_from_bf16():
    rng = np.random.default_rng(1)
    vols = NC.brain_like(rng, 1, (16, 16, 16))
    ref, mean_abs = NC.stats_ref_all(vols)
    off = ref.copy()
    off[0, NC.MEAN] = np.nextafter(off[0, NC.MEAN], np.inf)
    NC.check_stats("one ulp, bf16 gate", off, ref, mean_abs, is_int=False)
    with pytest.raises(AssertionError, match="int64 sum"):
        NC.check_stats("one ulp, int16 gate", off, ref, mean_abs, is_int=True)
    off = ref.copy()
    off[0, NC.STD] *= 1 + 2.0 ** -35
    with pytest.raises(AssertionError, match="std"):
        NC.check_stats("std", off, ref, mean_abs, is_int=True)


def test_window_edge_values_follow_the_given_window():
    assert NC.window_edge_values(32768, 32768, bf16=False) == [-1, 0, 32767]
    assert NC.window_edge_values(33000, 1000, bf16=False) == [231, 232, 1231, 1232]
    e = NC.window_edge_values(32768, 32768, bf16=True)
    assert e[0] == -(2.0 ** -126) and e[1] == 0.0 and not np.signbit(e[1]) and np.isfinite(e[2]) and e[2] > 3e38 and len(e) == 3
    for x in e:
        assert NC.bf16_round(np.array([x]))[0] == np.float32(x)


@pytest.mark.parametrize("mode", ["zscore", "window"])
@pytest.mark.parametrize("clip", [False, True])
def test_fold_gate_has_teeth(mode, clip):
    rng = np.random.default_rng(2)
    before = rng.uniform(-2, 2, size=(3, K.NPARAM)).astype(np.float32)
    before[:, K.FLAGS] = [0.0, 1.0, 1.0]
    before[:, NC.CLAMP_LO:] = 0.0
    stats, _ = NC.stats_ref_all(NC.brain_like(rng, 3, (16, 16, 16)), 0.0, (0.005, 0.995))
    stats[2] = 0.0                                                         # a volume without foreground: its record must not change
    scale, shift, _, _, clamp = NC.fold_ref(before, stats, mode, clip)
    after = before.copy()
    after[:, K.SCALE], after[:, K.SHIFT] = scale, shift
    after[clamp, NC.CLAMP_LO], after[clamp, NC.CLAMP_HI] = stats[clamp, NC.LO], stats[clamp, NC.HI]
    after[clamp, K.FLAGS] = before[clamp, K.FLAGS] + 2
    assert clamp.tolist() == [clip, clip, False] and np.array_equal(after[2], before[2])
    NC.check_fold("reference", before, after, stats, mode, clip)

    def refused(edit):
        bad = after.copy()
        edit(bad)
        with pytest.raises(AssertionError):
            NC.check_fold("planted", before, bad, stats, mode, clip)

    a, b = before[:, K.SCALE].astype(np.float64), before[:, K.SHIFT].astype(np.float64)
    refused(lambda t: t.__setitem__((0, K.SHIFT), np.float32((shift[0] - b[0]) + b[0] * scale[0] / a[0])))     # the drawn affine first, then the normalisation
    refused(lambda t: t.__setitem__((1, K.SCALE), np.float32(scale[1] * (1 + 2.0 ** -21))))
    refused(lambda t: t.__setitem__((0, K.SIGMA), t[0, K.SIGMA] + 1))                                           # a slot outside the fold
    refused(lambda t: t.__setitem__((0, 31), 1.0))
    refused(lambda t: t.__setitem__((2, K.SCALE), 1.0))                                                         # no foreground, yet folded
    if clip:
        refused(lambda t: t.__setitem__((0, K.FLAGS), before[0, K.FLAGS]))                                      # window written, flag missing
        refused(lambda t: t.__setitem__((1, NC.CLAMP_HI), t[1, NC.CLAMP_HI] + 1))
    else:
        refused(lambda t: t.__setitem__((0, NC.CLAMP_LO), 5.0))                                                 # clip off, yet a window is written


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
def test_clamp_after_the_affine_is_refused(exact):
    rng = np.random.default_rng(3)
    s, d = (9, 10, 11), (8, 8, 16)                                          # padded along x: pad_value must land on the window floor
    src = NC.brain_like(rng, 2, s)
    m = K.identity_matrix(s, d) if exact else K.compose((0, 0, 0), (0.2, -0.1, 0.1), (1.1, 0.9, 1.0), (0.3, 0, -0.4), s, d)
    table = K.table_from(2, m, a=[1 / 700.0, 1 / 450.0], b=[-0.2, -1.5], exact=exact)
    table[:, K.FLAGS] += NC.FLAG_CLAMP
    table[:, NC.CLAMP_LO], table[:, NC.CLAMP_HI] = [40.0, 100.0], [2500.0, 2000.0]
    ref, R, ex = NC.apply_ref(src, table, d, -1.0)
    assert ex.tolist() == [exact, exact]
    lo_out = table[:, K.SCALE].astype(np.float64) * [40.0, 100.0] + table[:, K.SHIFT].astype(np.float64)
    assert np.all(ref[:, :, :, 0] == lo_out[:, None, None])                 # the padded column sits on the floor
    got = K.round_to(ref, "bf16") if exact else ref
    assert K.check("reference", got, ref, R, ex, table, "bf16") <= 1.0
    bad, _, _ = NC.apply_ref(src, table, d, -1.0, fault="clamp_after_affine")
    with pytest.raises(AssertionError):
        K.check("clamp after the affine", K.round_to(bad, "bf16") if exact else bad, ref, R, ex, table, "bf16")
    plain = table.copy()
    plain[:, K.FLAGS] -= NC.FLAG_CLAMP                                       # bit clear: exactly _augment_check.apply_ref
    a, _, _ = NC.apply_ref(src, plain, d, -1.0)
    b, _, _ = K.apply_ref(src, plain, d, -1.0)
    assert np.array_equal(a, b)
