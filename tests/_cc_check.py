"""NumPy restatement of the connected foreground components (include/xvit.h, "Connected foreground components";
csrc/volume_components.hip) and the cases its tests share (tests/test_cc_gate_cpu.py, tests/test_cc_kernels_gpu.py,
tests/test_cc_model_gpu.py).  It needs NumPy only.

`label_ref` labels one volume by hooking (of two neighbours with different labels, the voxel that the larger label names takes the
smaller label, if that is below its own) with pointer jumping in between (lab <- lab[lab]) until no two neighbours differ; at that fixed
point neighbours hold equal labels, every label is the index of a voxel of the component that holds itself, and labels never exceed the
voxel's own index, so the label is the component's smallest flat index.  `comps_ref` takes the sizes from
np.unique, the largest with the tie to the smaller root, and the kept set; `boxes_ref` the index ranges of the kept voxels.  The sample
crop and the fold are tests/_crop_check.py's crop_ref and fold_ref, unchanged.  Everything is an integer: the comparison is bit for bit.
Planted defects (`fault=`) show that the comparison rejects them.
"""
import functools

import numpy as np

import _crop_check as X

NREC = 8
COUNT, LARGEST_ROOT, LARGEST_SIZE, KEPT, KEPT_VOXELS, STATUS = range(6)
LARGEST, MIN_VOXELS = 0, 1
TILE = (8, 8, 32)                 # the tile of csrc/volume_components.hip

FAULTS = ("missed_seam", "wrong_tie", "6_for_26", "background_labelled", "box_off_by_one", "count_includes_dropped")


def offsets(conn):
    """The half of the neighbourhood that precedes a voxel in flat order: 3 of 6, 13 of 26."""
    assert conn in (6, 26)
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) < (0, 0, 0) and (conn == 26 or abs(dz) + abs(dy) + abs(dx) == 1):
                    out.append((dz, dy, dx))
    return out


def _pair(d, n):
    """Slices of the voxels and of their neighbours at offset d along an axis of n."""
    return (slice(1, n), slice(0, n - 1)) if d < 0 else (slice(0, n - 1), slice(1, n)) if d > 0 else (slice(None), slice(None))


def label_ref(fg, conn, fault=None):
    """fg bool [Ds, Hs, Ws] -> int32 [Ds, Hs, Ws]: the smallest flat index of a foreground voxel's component, -1 for background."""
    fg = np.asarray(fg, dtype=bool)
    n = fg.size
    lab = np.where(fg, np.arange(n, dtype=np.int64).reshape(fg.shape), n)
    flat = lab.reshape(-1)
    zz = np.arange(fg.shape[0]).reshape(-1, 1, 1)
    while True:
        hooked = False
        for d in offsets(6 if fault == "6_for_26" else conn):
            sa, sb = zip(*[_pair(d[a], fg.shape[a]) for a in range(3)])
            a, b = lab[sa], lab[sb]
            differ = (a < n) & (b < n) & (a != b)
            if fault == "missed_seam" and d[0] < 0:
                differ &= (zz[sa[0]] % TILE[0] != 0)     # the pairs across a tile's first plane are not united
            if differ.any():
                hooked = True
                np.minimum.at(flat, np.maximum(a, b)[differ], np.minimum(a, b)[differ])     # the larger label's voxel takes the smaller
        if not hooked:
            break
        while True:
            nxt = np.append(flat, n)[flat]
            if np.array_equal(nxt, flat):
                break
            flat[:] = nxt
    return np.where(fg, lab, 0 if fault == "background_labelled" else -1).astype(np.int32)


def comps_ref(labels, keep, min_voxels, fault=None):
    """labels int32 [Ds, Hs, Ws] -> (comps int32 [8], the kept roots)."""
    roots, sizes = np.unique(labels[labels >= 0], return_counts=True)
    out = np.zeros(NREC, dtype=np.int32)
    if roots.size == 0:
        out[LARGEST_ROOT] = -1
        return out, roots
    top = np.flatnonzero(sizes == sizes.max())
    big = top[-1] if fault == "wrong_tie" else top[0]                  # roots ascend: a tie goes to the smaller root
    kept = np.flatnonzero(sizes >= min_voxels) if keep == MIN_VOXELS else np.array([big])
    if kept.size == 0:
        kept = np.array([big])                                          # none qualifies: the largest
    out[:5] = roots.size, roots[big], sizes[big], kept.size, sizes.sum() if fault == "count_includes_dropped" else sizes[kept].sum()
    return out, roots[kept]


def boxes_ref(labels, kept_roots, fault=None):
    """The index ranges and the count of the voxels whose label is a kept root, in xvit_volume_bbox's layout: int32 [8]."""
    idx = np.nonzero(np.isin(labels, kept_roots) & (labels >= 0))
    out = np.zeros(NREC, dtype=np.int32)
    for a in range(3):
        out[2 * a] = idx[a].min() if idx[a].size else labels.shape[a]
        out[2 * a + 1] = (idx[a].max() + (1 if fault == "box_off_by_one" else 0)) if idx[a].size else -1
    out[6] = idx[0].size
    return out


def foreground(src, above):
    """The predicate of xvit_volume_bbox: strict, NaN never, -0.0 not above 0."""
    with np.errstate(invalid="ignore"):
        return np.asarray(src).astype(np.float64) > above


def tables_ref(labels, keep, min_voxels, fault=None):
    """labels int32 [nvol, Ds, Hs, Ws] -> (comps int32 [nvol, 8], boxes int32 [nvol, 8])."""
    comps, boxes = [], []
    for lab in labels:
        c, kept = comps_ref(lab, keep, min_voxels, fault)
        comps.append(c)
        boxes.append(boxes_ref(lab, kept, fault))
    return np.stack(comps), np.stack(boxes)


def reference(fg, conn, keep=LARGEST, min_voxels=1, fault=None):
    """fg bool [nvol, Ds, Hs, Ws] -> (labels int32 [nvol, Ds, Hs, Ws], comps, boxes)."""
    labels = np.stack([label_ref(f, conn, fault) for f in fg])
    return (labels,) + tables_ref(labels, keep, min_voxels, fault)


# ---------------------------------------------------------------------------------------------------------------- shared cases
def _ellipsoid(shape, centre, radii):
    g = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return sum(((g[a] - centre[a]) / max(radii[a], .5)) ** 2 for a in range(3)) <= 1.0


def _serpentine(shape):
    """One 6-connected path through the whole volume: every other row of every other plane, joined at alternating ends."""
    D, H, W = shape
    m = np.zeros(shape, dtype=bool)
    plane = np.zeros((H, W), dtype=bool)
    plane[0::2] = True
    for y in range(1, H, 2):
        if y + 1 < H:
            plane[y, W - 1 if (y // 2) % 2 == 0 else 0] = True
    rows = (H + 1) // 2
    end = (2 * (rows - 1), W - 1 if rows % 2 == 1 else 0)              # where the path leaves the plane; it enters at (0, 0)
    m[0::2] = plane
    for z in range(1, D, 2):
        if z + 1 < D:
            m[(z,) + (end if (z // 2) % 2 == 0 else (0, 0))] = True
    return m


def _comb(shape):
    """Teeth along z on every other (y, x), joined only by the last plane."""
    m = np.zeros(shape, dtype=bool)
    m[:, 0::2, 0::2] = True
    m[-1] = True
    return m


def _u_shapes(shape):
    """Two arms along x in rows 0 and 2 of plane 0 that meet only past the first tile seam along x, and two along z in columns (y, x) =
    (H - 1, 0) and (H - 1, 2) that meet only past the first seam along z."""
    D, H, W = shape
    m = np.zeros(shape, dtype=bool)
    xe = min(W - 1, TILE[2] + 1)
    m[0, 0:3:2, :xe + 1] = True
    if H > 1:
        m[0, 1, xe] = True
    if D > 2 and H > 4 and W > 2:
        ze = min(D - 1, TILE[0] + 1)
        m[2:ze + 1, H - 1, 0:3:2] = True
        m[ze, H - 1, 1] = True
    return m


def _touching(shape, corner):
    """Two blocks that share only an edge along x (or, corner=True, only a corner): separate at 6, joined at 26."""
    D, H, W = shape
    a, b, c = max(D // 2, 1), max(H // 2, 1), max(W // 2, 1)
    m = np.zeros(shape, dtype=bool)
    m[:a, :b, :c if corner else W] = True
    m[a:, b:, c if corner else 0:] = True
    return m


def _tie(shape):
    """Two components of k voxels at opposite corners and a smaller one between them."""
    D, H, W = shape
    k = min(3, W)
    m = np.zeros(shape, dtype=bool)
    m[0, 0, :k] = True
    m[-1, -1, W - k:] = True
    m[D // 2, H // 2, W // 2] = True
    return m


def masks(shape, seed=0):
    """name -> bool [Ds, Hs, Ws]; the order is fixed: 'empty' follows a volume with foreground, so M = 2 pairs them."""
    rng = np.random.default_rng(1000 + seed)
    D, H, W = shape
    c = [(n - 1) / 2 for n in shape]
    brain = _ellipsoid(shape, (c[0] + .3, c[1] - .2, c[2] + .4), (D / 3.3, H / 3.1, W / 3.2))
    specks = brain.copy()
    for _ in range(6):
        specks[tuple(rng.integers(0, n) for n in shape)] = True
    near = brain.copy()
    zs = np.flatnonzero(brain.any(axis=(1, 2)))
    if zs.size and zs[0] >= 2:
        near[zs[0] - 2, int(round(c[1])), int(round(c[2]))] = True      # two planes in front of the brain: inside a margin of 2
    corners = np.zeros(shape, dtype=bool)
    corners[::max(D - 1, 1), ::max(H - 1, 1), ::max(W - 1, 1)] = True
    g = np.indices(shape).sum(axis=0)
    out = {"full": np.ones(shape, dtype=bool), "empty": np.zeros(shape, dtype=bool), "corners": corners, "checkerboard": g % 2 == 0,
           "edge-touch": _touching(shape, False), "corner-touch": _touching(shape, True), "serpentine": _serpentine(shape), "comb": _comb(shape),
           "u-across-seam": _u_shapes(shape), "tie": _tie(shape), "brain-specks": specks, "speck-in-margin": near}
    for p in (0.25, 0.31, 0.40, 0.08, 0.12):
        out[f"noise-{p}"] = rng.random(shape) < p
    out["empty-2"] = np.zeros(shape, dtype=bool)
    return out


def values(fg, dtype_name, bright=None, seed=0):
    """Source values for the masks fg [nvol, ...] with foreground_above = 0: positive values where fg, the largest of all where `bright`
    (a bool array like fg) is set, and a mix of 0, negatives and, for the float types, -0.0, NaN and -inf elsewhere.  int16 for 'int16',
    float32 on the bf16 grid otherwise."""
    rng = np.random.default_rng(2000 + seed)
    bright = np.zeros(fg.shape, dtype=bool) if bright is None else bright
    if dtype_name == "int16":
        v = np.where(fg, rng.integers(1, 3000, fg.shape), rng.choice(np.array([0, 0, 0, -1, -32768]), fg.shape))
        return np.where(bright & fg, 32767, v).astype(np.int16)
    bg = rng.choice(np.array([0.0, -0.0, np.nan, -1.5, -np.inf, 0.0], dtype=np.float32), fg.shape)
    v = np.where(fg, rng.choice(np.array([2.0 ** -120, 0.5, 1.0, 700.0], dtype=np.float32), fg.shape), bg)
    return X.on_bf16_grid(np.where(bright & fg, np.float32(np.inf), v).astype(np.float32))


def specks_of(names, labels):
    """bool like labels: in the two brain volumes, the voxels outside the largest component (the specks: they get the largest values)."""
    out = np.zeros(labels.shape, dtype=bool)
    for name in ("brain-specks", "speck-in-margin"):
        if name in names:
            v = names.index(name)
            c, _ = comps_ref(labels[v], LARGEST, 1)
            out[v] = (labels[v] >= 0) & (labels[v] != c[LARGEST_ROOT])
    return out


# the tile is (8, 8, 32): T - 1, T, T + 1 and 2 T + 1 along each axis, the three smallest shapes, and one of several tiles along every axis
SHAPES = [(1, 1, 1), (1, 1, 9), (3, 5, 7), (7, 9, 33), (8, 9, 33), (9, 9, 33), (17, 9, 33), (9, 7, 33), (9, 8, 33), (9, 17, 33), (9, 9, 31), (9, 9, 32),
          (9, 9, 65), (40, 36, 70)]
CUBE, CUBE_MASKS = (64, 64, 64), ("serpentine", "brain-specks", "comb")     # with the connectivity's densest noise: nvol = 4


@functools.lru_cache(maxsize=None)
def case(shape, conn):
    """Computed once and shared: leave the arrays as they are.  -> (names, fg bool [nvol, Ds, Hs, Ws], labels int32 of the same shape)."""
    ms = masks(shape)
    if shape == CUBE:
        ms = {k: ms[k] for k in CUBE_MASKS + ("noise-0.31" if conn == 6 else "noise-0.12",)}
    fg = np.stack(list(ms.values()))
    labels = np.stack([label_ref(f, conn) for f in fg])
    fg.setflags(write=False)
    labels.setflags(write=False)
    return tuple(ms), fg, labels


def second_size(labels):
    """The size of the second largest component of one volume (0 when it has fewer than two)."""
    sizes = np.sort(np.unique(labels[labels >= 0], return_counts=True)[1])
    return int(sizes[-2]) if sizes.size > 1 else 0
