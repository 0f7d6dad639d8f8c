"""CPU: the NumPy restatement of tests/_cc_check.py against scipy.ndimage.label with the 6- and 26-structures on every generated case, and
the planted defects the bit-for-bit comparison must catch."""
import numpy as np
import pytest

import _cc_check as CC

ndimage = pytest.importorskip("scipy.ndimage")

STRUCTURE = {6: ndimage.generate_binary_structure(3, 1), 26: ndimage.generate_binary_structure(3, 3)}


def scipy_labels(fg, conn):
    """scipy's labels, canonicalised to the smallest flat index of each component; -1 for background."""
    lab, n = ndimage.label(fg, structure=STRUCTURE[conn])
    flat = lab.reshape(-1)
    first = np.full(n + 1, -1, dtype=np.int64)
    idx = np.flatnonzero(flat)
    first[flat[idx[::-1]]] = idx[::-1]            # the last write per label is its smallest index
    return first[flat].reshape(fg.shape).astype(np.int32)


def scipy_tables(fg, conn, keep, min_voxels):
    comps, boxes = [], []
    for f in fg:
        lab, n = ndimage.label(f, structure=STRUCTURE[conn])
        c, b = np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
        sizes = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
        roots = np.array([np.flatnonzero(lab.reshape(-1) == k + 1)[0] for k in range(n)], dtype=np.int64)
        if n == 0:
            c[1] = -1
            kept_mask = np.zeros(f.shape, dtype=bool)
        else:
            order = sorted(range(n), key=lambda k: (-sizes[k], roots[k]))
            big = order[0]
            kept = [k for k in range(n) if sizes[k] >= min_voxels] if keep == CC.MIN_VOXELS else [big]
            kept = kept or [big]
            kept_mask = np.isin(lab, np.array(kept) + 1)
            c[:5] = n, roots[big], sizes[big], len(kept), kept_mask.sum()
        idx = np.nonzero(kept_mask)
        for a in range(3):
            b[2 * a], b[2 * a + 1] = (idx[a].min(), idx[a].max()) if idx[a].size else (f.shape[a], -1)
        b[6] = idx[0].size
        comps.append(c)
        boxes.append(b)
    return np.stack(comps), np.stack(boxes)


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("shape", CC.SHAPES + [CC.CUBE], ids=lambda s: "x".join(map(str, s)))
def test_the_restatement_agrees_with_scipy(shape, conn):
    names, fg, labels = CC.case(shape, conn)
    for v, name in enumerate(names):
        np.testing.assert_array_equal(labels[v], scipy_labels(fg[v], conn), err_msg=f"{name} {shape} connectivity {conn}")
    if np.prod(shape) > 30000:
        return                                     # the tables of the large shapes repeat the small ones' rule on the labels checked above
    n2 = max(CC.second_size(labels[names.index("brain-specks")]), 1)
    for keep, n in [(CC.LARGEST, 1), (CC.MIN_VOXELS, 1), (CC.MIN_VOXELS, n2), (CC.MIN_VOXELS, n2 + 1), (CC.MIN_VOXELS, int(np.prod(shape)) + 1)]:
        comps, boxes = CC.tables_ref(labels, keep, n)
        want_comps, want_boxes = scipy_tables(fg, conn, keep, n)
        np.testing.assert_array_equal(comps, want_comps, err_msg=f"comps {shape} {conn} keep {keep} n {n}")
        np.testing.assert_array_equal(boxes, want_boxes, err_msg=f"boxes {shape} {conn} keep {keep} n {n}")


def test_the_patterns_are_what_their_names_say():
    shape = (17, 9, 33)
    for conn in (6, 26):
        names, fg, labels = CC.case(shape, conn)
        comps, _ = CC.tables_ref(labels, CC.LARGEST, 1)
        count = dict(zip(names, comps[:, CC.COUNT]))
        assert count["empty"] == 0 and count["full"] == 1 and count["serpentine"] == 1 and count["comb"] == 1 and count["u-across-seam"] == 2
        assert count["checkerboard"] == (-(-int(np.prod(shape)) // 2) if conn == 6 else 1)
        assert count["edge-touch"] == count["corner-touch"] == (2 if conn == 6 else 1)
        assert count["corners"] == 8 and count["tie"] == 3
        tie = comps[names.index("tie")]
        assert tie[CC.LARGEST_ROOT] == 0 and tie[CC.LARGEST_SIZE] == 3, "two components of three voxels: the smaller root wins"
        assert count["brain-specks"] > 1 and count["speck-in-margin"] == 2
        u = fg[names.index("u-across-seam")]
        assert u[0, 1, :CC.TILE[2]].sum() == 0 and u[:CC.TILE[0], 8, 1].sum() == 0, "the arms meet past the first seam only"


@pytest.mark.parametrize("fault", CC.FAULTS)
def test_a_planted_defect_is_caught(fault):
    shape, conn = (17, 9, 33), 26 if fault == "6_for_26" else 6
    names, fg, labels = CC.case(shape, conn)
    caught = []
    for keep, n in [(CC.LARGEST, 1), (CC.MIN_VOXELS, 4)]:
        comps, boxes = CC.tables_ref(labels, keep, n)
        bad_labels, bad_comps, bad_boxes = CC.reference(fg, conn, keep, n, fault=fault)
        caught.append(not (np.array_equal(labels, bad_labels) and np.array_equal(comps, bad_comps) and np.array_equal(boxes, bad_boxes)))
    assert all(caught), f"{fault} passes the comparison"
    where = {"missed_seam": "u-across-seam", "wrong_tie": "tie", "6_for_26": "corner-touch"}.get(fault)
    if where:
        v = names.index(where)
        bad_labels, bad_comps, _ = CC.reference(fg[v:v + 1], conn, fault=fault)
        assert not (np.array_equal(bad_labels[0], labels[v]) and np.array_equal(bad_comps[0], CC.tables_ref(labels[v:v + 1], CC.LARGEST, 1)[0][0])), \
            f"{fault} passes on the pattern built for it ({where})"
