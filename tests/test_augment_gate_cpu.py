"""CPU: the element-wise gate of the augmentation tests (tests/_augment_check.py) has teeth.  The float64 restatement against itself,
rounded to the output dtype, passes; a restatement with one planted defect, rounded the same way, is rejected: a reference shifted by one
voxel along each axis, a transposed matrix, nearest-neighbour instead of trilinear, 0 instead of pad_value outside the volume, a and b
swapped, the table row of sample 1 used for sample 0."""
import numpy as np
import pytest

import _augment_check as K

SRC, DST, PAD = (12, 11, 10), (8, 8, 16), -1.0


def _case():
    rng = np.random.default_rng(0)
    src = rng.uniform(-1000.0, 3000.0, size=(2,) + SRC)
    # two different rows: a rotation about every axis with zoom and a fractional translation that pushes part of the volume outside,
    # and a milder one; a and b differ per volume
    m0 = K.compose((0, 0, 0), (0.2, -0.15, 0.1), (0.8, 1.25, 1.0), (2.3, -1.6, 4.4), SRC, DST)
    m1 = K.compose((0, 1, 0), (-0.1, 0.05, 0.25), (1.1, 0.9, 1.2), (-0.4, 0.7, -5.5), SRC, DST)
    table = K.table_from(2, np.stack([m0, m1]), a=np.array([1.1, 0.9]), b=np.array([0.3, -0.2]))
    ref, R, exact = K.apply_ref(src, table, DST, PAD)
    return src, table, ref, R, exact


CASE = _case()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_the_rounded_reference_passes(dtype):
    src, table, ref, R, exact = CASE
    assert not exact.any() and float(R.min()) == 0.0 and float(R.max()) > 1000.0      # fully outside voxels and ordinary ones
    assert K.check("self", K.round_to(ref, dtype), ref, R, exact, table, dtype) <= 1.0


FAULTS = [("shift", 0), ("shift", 1), ("shift", 2), "transposed", "nearest", "zero_outside", "a_b_swapped", "row_of_sample_1"]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("fault", FAULTS, ids=[f if isinstance(f, str) else f"shift_axis{f[1]}" for f in FAULTS])
def test_a_planted_defect_is_rejected(fault, dtype):
    src, table, ref, R, exact = CASE
    wrong, _, _ = K.apply_ref(src, table, DST, PAD, fault=fault)
    with pytest.raises(AssertionError, match="out of bound"):
        K.check(str(fault), K.round_to(wrong, dtype), ref, R, exact, table, dtype)


def test_exact_path_gate_is_equality():
    """On a table flagged exact the gate is equality with the rounded reference: the next bf16 number is rejected."""
    rng = np.random.default_rng(1)
    src = rng.integers(-1000, 3000, size=(1,) + SRC).astype(np.float64)
    table = K.table_from(1, K.identity_matrix(SRC, DST), exact=True)
    ref, R, exact = K.apply_ref(src, table, DST, PAD)
    assert exact.all()
    good = K.round_to(ref, "bf16")
    assert K.check("exact", good, ref, R, exact, table, "bf16") == 0.0
    off = good.copy()
    off[0, 3, 4, 5] *= 1 + 2.0 ** -7      # one bf16 ulp
    with pytest.raises(AssertionError, match="equality"):
        K.check("exact", off, ref, R, exact, table, "bf16")


def test_hash_restatement_matches_a_scalar_evaluation():
    """The vectorised hash32 against the C expression evaluated with Python integers."""
    def scalar(seed, idx):
        m = (1 << 64) - 1
        z = (idx * 0x9E3779B97F4A7C15 + seed) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return ((z ^ (z >> 31)) >> 16) & 0xFFFFFFFF
    idx = [0, 1, 2, 65535, 2 ** 31, 2 ** 40 + 17]
    for seed in (0, 1, 0xDEADBEEF, 2 ** 63 + 5):
        assert [int(v) for v in K.hash32(seed, np.array(idx, dtype=np.uint64))] == [scalar(seed, i) for i in idx]


def test_noise_field_of_the_restatement_is_standard_normal():
    """n = 32768 draws: mean within 5 / sqrt(n) of 0, standard deviation within 5 / sqrt(2 n) of 1 (five standard errors)."""
    n = 32 ** 3
    f = K.normal_field(12345, n)
    assert abs(f.mean()) <= 5 / np.sqrt(n) and abs(f.std() - 1) <= 5 / np.sqrt(2 * n)
    assert np.isfinite(f).all() and np.abs(f).max() < 5.8          # sqrt(-2 ln 2^-24) = 5.77
