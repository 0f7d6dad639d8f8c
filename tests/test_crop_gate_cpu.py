"""The teeth of the crop gate (tests/_crop_check.py), on the GPU tests' own cases: the reference passes its own gate, every planted defect
is rejected on at least one case, and the cases are what their comments claim.  No GPU, no library."""
import numpy as np
import pytest

import _augment_check as K
import _crop_check as X

BOX_FAULTS = ("hi_off_by_one", "ge", "nan_foreground", "row_x_confused")
CROP_FAULTS = ("union_is_modality_0", "empty_poisons_union", "margin_unclipped")
FOLD_FAULTS = ("offset_of_volume", "o_not_subtracted", "k_from_min", "k_not_raised", "exact_kept")
assert set(BOX_FAULTS + CROP_FAULTS + FOLD_FAULTS) == set(X.FAULTS)


def runs():
    """Every (volume set, fold case) the GPU tests run, for the 16-bit integer and a float source."""
    for dtype_name in ("int16", "bf16"):
        sets = X.volume_sets(dtype_name)
        for name, (src, M, above) in sets.items():
            yield f"{dtype_name}/{name}/boxes", src, M, above, (0, 0, 0), None, False, (4, 4, 4), "exact"
        for name, img, mode, margin, up, kind in X.FOLD_CASES:
            src, M, above = sets[name]
            yield f"{dtype_name}/{name}/{img}/{mode}/{margin}/{up}/{kind}", src, M, above, margin, mode, up, img, kind


def device_like(src, M, above, margin, mode, up, img, kind, fault=None):
    """What a kernel with the planted defect would return."""
    rng = np.random.default_rng(3)
    before = X.tables(src.shape[0], M, src.shape[1:], img, kind, rng)
    boxes = X.boxes_ref(src, above, fault if fault in BOX_FAULTS else None)
    crop = X.crop_ref(boxes, M, margin, src.shape[1:], fault if fault in CROP_FAULTS else None)
    table, _ = X.fold_ref(before, crop, M, mode, up, src.shape[1:], img, fault if fault in FOLD_FAULTS else None)
    return boxes, crop, table, before


def test_the_reference_passes_its_own_gate():
    for name, src, M, above, margin, mode, up, img, kind in runs():
        boxes, crop, table, before = device_like(src, M, above, margin, mode, up, img, kind)
        X.check_tables(name, boxes, crop, table, before, src, M, above, margin, mode, up, img)


@pytest.mark.parametrize("fault", X.FAULTS)
def test_every_planted_defect_is_rejected(fault):
    caught = []
    for name, src, M, above, margin, mode, up, img, kind in runs():
        boxes, crop, table, before = device_like(src, M, above, margin, mode, up, img, kind, fault)
        try:
            X.check_tables(name, boxes, crop, table, before, src, M, above, margin, mode, up, img)
        except AssertionError:
            caught.append(name)
    assert caught, f"the gate accepts '{fault}' on every case"


def test_a_written_slot_outside_the_fold_is_rejected():
    name, src, M, above, margin, mode, up, img, kind = next(r for r in runs() if r[5] == "fit")
    boxes, crop, table, before = device_like(src, M, above, margin, mode, up, img, kind)
    table.view(np.uint32)[0, 20] ^= 1                       # one payload bit of a NaN the fold must not touch
    with pytest.raises(AssertionError, match="slot 20 was written"):
        X.check_tables(name, boxes, crop, table, before, src, M, above, margin, mode, up, img)


def test_the_cases_are_what_they_claim():
    sets = X.volume_sets("int16")
    seen, scales, one_sided = set(), [], False
    for name, img, mode, margin, up, kind in X.FOLD_CASES:
        src, M, above = sets[name]
        shape = src.shape[1:]
        boxes = X.boxes_ref(src, above)
        crop = X.crop_ref(boxes, M, margin, shape)
        wide = X.crop_ref(boxes, M, margin, shape, fault="margin_unclipped")
        for b in range(crop.shape[0]):
            if crop[b, 6]:
                rel = tuple(np.sign((crop[b, 1:6:2] - crop[b, 0:6:2] + 1) - np.asarray(img)))
                seen.add(rel)
                scales.append((mode, up, kind, float(X.crop_scale(crop[b], mode, up, img))))
                for a in range(3):
                    one_sided |= (wide[b, 2 * a] < 0) != (wide[b, 2 * a + 1] > shape[a] - 1)
    assert any(len(set(r)) == 3 for r in seen), "s < n, s == n and s > n on the three axes of one case"
    assert one_sided, "a margin that clips on one side only"
    assert ("fit", True, "flips", 1.0) in scales, "fit with k exactly 1 on an exact record"
    assert any(m == "fit" and up and k < 1 for m, up, _, k in scales) and any(m == "fit" and k > 1 for m, _, _, k in scales)
    assert any(m == "fit" and not up and k == 1 for m, up, _, k in scales), "k raised to 1"
    thin = X.volume_sets("bf16")
    assert np.isnan(thin["threshold-0"][0]).any() and np.signbit(thin["threshold-0"][0][0, 1, 1, 1])
    assert X.chunk_rule(12, int(np.prod(X.CHUNK_SHAPE)))[0] > 1
    for es in (2, 4):                                       # the planted voxels do sit on a head, a tail and both ends of a chunk
        nvox = int(np.prod(X.CHUNK_SHAPE))
        parts, chunk = X.chunk_rule(12, nvox)
        pos = {X.edge_positions(v, 12, nvox, es)[v] for v in range(12)}
        assert {0, nvox - 1} <= pos and (chunk - 1 in pos or chunk in pos)


@pytest.mark.parametrize("name,img,margin", [("brain-9x10x37-m3", (8, 7, 16), (0, 0, 0)), ("brain-9x10x37-m2", (4, 8, 16), (1, 0, 2)),
                                             ("corners-5x6x7", (8, 8, 4), (0, 0, 0))])
def test_a_center_fold_of_the_identity_is_the_window(name, img, margin):
    """apply_ref of tests/_augment_check.py through a `center`-folded identity table is the plain slice-and-pad of window_ref, exactly."""
    src, M, above = X.volume_sets("int16")[name]
    shape = src.shape[1:]
    crop = X.crop_ref(X.boxes_ref(src, above), M, margin, shape)
    before = K.table_from(src.shape[0], K.identity_matrix(shape, img), exact=True)
    table, _ = X.fold_ref(before, crop, M, "center", False, shape, img)
    ref, _, exact = K.apply_ref(src, table, img, -7.0)
    assert exact.all() and np.array_equal(ref, X.window_ref(src, crop, M, img, -7.0))
    assert not np.array_equal(ref, K.apply_ref(src, before, img, -7.0)[0]), "the box is not where the volume's centre window is"
