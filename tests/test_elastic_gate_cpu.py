"""CPU: the teeth of the elastic gate (tests/_elastic_check.py), on the builders and shapes tests/test_elastic_kernels_gpu.py uses.  The
float64 reference rounded to bf16 and to fp32 passes against itself; every planted defect of apply_ref / field_ref is rejected; the
restated draw has the statistics the header promises.  NumPy only: it passes with or without the library."""
import numpy as np
import pytest

import _augment_check as A
import _elastic_check as K

SHAPE_IDS = tuple(K.SHAPES)


def _check(shape, kind, m, got, dt):
    src, table, field, erec, (ref, R, exact, deformed, cell) = K.case(shape, kind, m)
    return K.check(f"{shape}-{kind}-{m}", got, ref, R, exact, deformed, cell, table, dt)


def test_constant_is_derived_and_cannot_swallow_a_formula_error():
    assert K.C_ELASTIC == 2.0 ** -9 and 62.1 * 2.0 ** -15 <= K.C_ELASTIC <= 2.0 ** -8
    for s, d, grid in K.SHAPES.values():
        assert max(s) < 512 and all(4 <= g <= K.MAX_GRID for g in grid)
        t = K.tables(s, d)
        assert np.abs(t[:, :12].reshape(-1, 3, 4)[:, :, :3]).sum(-1).max() <= 2.0          # what the derivation of c assumes of A
    assert K.FLAGS_ON == (1.0, 0.0, 1.0) and (K.B, K.M, K.NVOL) == (3, 2, 6)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("kind,m", [("plain", 3.0), ("plain", 12.0), ("clamp", 3.0), ("noise", 3.0)])
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_rounded_reference_passes(shape, kind, m, dt):
    src, table, field, erec, (ref, R, exact, deformed, cell) = K.case(shape, kind, m)
    assert deformed.tolist() == [True, True, False, False, True, True] and not exact.any()
    assert np.abs(field).max() <= 16.0 and np.isfinite(ref).all()
    ratio = _check(shape, kind, m, A.round_to(ref, dt), dt)
    assert ratio <= 1.0


def test_max_displacement_12_pushes_coordinates_out_of_the_source():
    """... so that pad blending is in the cases: deformed voxels depend on pad_value, and the displacement itself exceeds 3 voxels."""
    for shape in ("lx3", "lx4"):
        s, d, grid = K.SHAPES[shape]
        src, table, field, erec, (ref, R, exact, deformed, cell) = K.case(shape, "plain", 12.0)
        other = K.apply_ref(src, table, field, erec, K.M, d, -77.0)[0]
        assert (other[deformed] != ref[deformed]).any()
        assert max(np.abs(K.displacement_ref(field[b], d)).max() for b in (0, 2)) > 3.0


@pytest.mark.parametrize("fault", K.FAULTS)
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_planted_defect_is_rejected(shape, fault):
    src, table, field, erec, _ = K.case(shape, "plain", 3.0)
    s, d, grid = K.SHAPES[shape]
    bad = K.apply_ref(src, table, field, erec, K.M, d, K.PAD, fault=fault)[0]
    for dt in ("bf16", "f32"):
        with pytest.raises(AssertionError, match="out of bound|elements wrong|control cell"):
            _check(shape, "plain", 3.0, A.round_to(bad, dt), dt)


def test_failure_message_names_the_place():
    src, table, field, erec, (ref, R, exact, deformed, cell) = K.case("lx3", "plain", 3.0)
    got = A.round_to(ref, "f32")
    got[4, 7, 13, 29] += 50.0
    with pytest.raises(AssertionError) as e:
        _check("lx3", "plain", 3.0, got, "f32")
    msg = str(e.value)
    for word in ("volume 4", "z 7, y 13, x 29", "brick (0, 1, 1)", "wave 3", "run 3", "element 5", f"control cell ({cell[0][7]}, {cell[1][13]}, {cell[2][29]})"):
        assert word in msg, (word, msg)
    got = A.round_to(ref, "f32")
    got[2, 0, 0, 0] = np.nan                     # a flag-0 volume is held by _augment_check.check
    with pytest.raises(AssertionError, match="flag 0"):
        _check("lx3", "plain", 3.0, got, "f32")


def test_spike_makes_a_one_voxel_error_visible():
    """The structured source: shifting the sample position of a deformed volume by one voxel along any axis leaves the gate."""
    src, table, field, erec, (ref, R, exact, deformed, cell) = K.case("lx3", "plain", 3.0)
    s, d, grid = K.SHAPES["lx3"]
    for axis in range(3):
        t = table.copy()
        t[:, 4 * axis + 3] += 1.0
        bad = K.apply_ref(src, t, field, erec, K.M, d, K.PAD)[0]
        with pytest.raises(AssertionError):
            _check("lx3", "plain", 3.0, A.round_to(bad, "f32"), "f32")


def test_partition_of_unity_in_the_reference():
    """A constant field is the constant displacement, and composing it equals moving t by A d."""
    d_ = np.array([1.25, -2.5, 0.75])
    for shape in SHAPE_IDS:
        s, d, grid = K.SHAPES[shape]
        phi = np.broadcast_to(d_[:, None, None, None], (3,) + grid)
        u = K.displacement_ref(phi, d)
        assert np.abs(u - d_[:, None, None, None]).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------- draw
def test_draw_statistics():
    grid, m = (7, 6, 5), (3.0, 7.5, 1.0)
    cfg = K.config(prob=1.0, max_displacement=m, locked_borders=1)
    field, erec = K.field_ref(cfg, 64, grid, seed=5)
    locked = K.locked_mask(grid, 1)
    assert (erec[:, K.FLAG] == 1).all() and (erec[:, 5:] == 0).all()
    for a in range(3):
        free = field[:, a][:, ~locked].astype(np.float64)
        assert (np.abs(free) <= m[a]).all() and (field[:, a][:, locked] == 0).all()
        se = (2 * m[a] / np.sqrt(12.0)) / np.sqrt(free.size)
        assert abs(free.mean()) <= 4 * se
        assert np.float32(np.abs(free).max()) == erec[:, K.MAX_ABS + a].max()
    for L in range(4):
        f, _ = K.field_ref(K.config(locked_borders=L), 2, (8, 8, 8), seed=1)
        mask = K.locked_mask((8, 8, 8), L)
        assert (f[:, :, mask] == 0).all() and (L == 3 or (f[:, :, ~mask] != 0).any())
        assert mask.sum() == 8 ** 3 - max(8 - 2 * L, 0) ** 3


def test_draw_share_of_active_samples():
    for prob in (0.2, 0.5):
        _, erec = K.field_ref(K.config(prob=prob), 4096, (4, 4, 4), seed=11)
        share = erec[:, K.FLAG].mean()
        assert abs(share - prob) <= 4 * np.sqrt(prob * (1 - prob) / 4096)
        assert ((erec[:, K.U] < np.float32(prob)) == (erec[:, K.FLAG] == 1)).all()
    f, erec = K.field_ref(K.config(prob=0.0), 8, (4, 4, 4), seed=11)
    assert (erec[:, K.FLAG] == 0).all() and (f == 0).all() and (erec[:, 2:] == 0).all()


def test_draw_defect_and_streams():
    cfg = K.config(prob=1.0, max_displacement=5.0, locked_borders=2)
    f, e = K.field_ref(cfg, 3, (7, 7, 7), seed=3)
    fb, eb = K.field_ref(cfg, 3, (7, 7, 7), seed=3, fault="locked_ignored")
    assert not np.array_equal(f, fb) and (f[:, :, 2:5, 2:5, 2:5] == fb[:, :, 2:5, 2:5, 2:5]).all()
    f1, _ = K.field_ref(cfg, 3, (7, 7, 7), seed=3, call=1)
    assert not np.array_equal(f, f1)                                                   # call k differs from call k + 1
    assert np.array_equal(f1, K.field_ref(cfg, 3, (7, 7, 7), seed=(3 + K.COUNTER_STRIDE) & ((1 << 64) - 1))[0])
    assert K.POINT_BASE + 3 * 16 ** 3 <= K.SAMPLE_STRIDE                               # a sample's indices stay inside its stride
