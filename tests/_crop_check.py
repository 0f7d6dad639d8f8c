"""NumPy restatement of the foreground bounding box and crop (include/xvit.h, "Foreground bounding box and crop"; csrc/volume_bbox.hip), the
gate of its tests and the cases the GPU tests and the gate's own test (tests/test_crop_gate_cpu.py) share.

`boxes_ref` takes the index ranges from np.nonzero, `crop_ref` the union, margin and clip, `fold_ref` the fold in float64 with np.float32
roundings, `window_ref` a plain slice-and-pad of the source at the folded offset o'.  Planted defects (`fault=`) show that the gate rejects
them.

Gate (`check_tables`): boxes, crop, slot 31, FLAGS and the nine A slots bit for bit; the t slots bit for bit when kf == 1, else within
OFFSET_GATE = 2^-23 of tests/_augment_check.py relative to max(1, |t64|): fl32(kf (t - c - o) + cb) is one rounding of a double whose own
error is 2^-53 relative, or, contracted into a fused multiply-add, none, and the two can fall on different sides of an fp32 tie, so the
bound is the one rounding (2^-24) with a factor two to spare.  Every slot the fold must not write is compared as a bit pattern.
"""
import functools

import numpy as np

import _augment_check as K

NREC, NPARAM = 8, K.NPARAM
CROP_SCALE, FLAGS, MATRIX = 31, K.FLAGS, K.MATRIX
A_SLOTS = [4 * i + j for i in range(3) for j in range(3)]
T_SLOTS = [3, 7, 11]
FOLD_SLOTS = set(A_SLOTS + T_SLOTS + [FLAGS, CROP_SCALE])
MODES = {None: 0, "center": 1, "fit": 2}
MIN_CHUNK, MAX_GROUPS = 8192, 2048           # the chunk rule of the header

FAULTS = ("hi_off_by_one", "ge", "nan_foreground", "union_is_modality_0", "empty_poisons_union", "margin_unclipped", "offset_of_volume",
          "o_not_subtracted", "k_from_min", "k_not_raised", "exact_kept", "row_x_confused")


def chunk_rule(nvol, nvox):
    """(parts, chunk) of the header's chunk rule."""
    parts = min(max(1, MAX_GROUPS // nvol), -(-nvox // MIN_CHUNK))
    chunk = (-(-nvox // parts) + 7) // 8 * 8
    return -(-nvox // chunk), chunk


def workspace_bytes(nvol, nvox):
    return nvol * chunk_rule(nvol, nvox)[0] * NREC * 4


def boxes_ref(src, above, fault=None):
    """src [nvol, Ds, Hs, Ws] (int16 or float) -> int32 [nvol, 8]."""
    src = np.asarray(src)
    nvol, shape = src.shape[0], src.shape[1:]
    v64 = src.astype(np.float64)
    with np.errstate(invalid="ignore"):
        fg = v64 >= above if fault == "ge" else ~(v64 <= above) if fault == "nan_foreground" else v64 > above
    out = np.zeros((nvol, NREC), dtype=np.int32)
    for v in range(nvol):
        idx = np.nonzero(fg[v])
        if fault == "row_x_confused" and idx[0].size:     # (z, y) of the 8-voxel run's first voxel for all of it, x running past the row end
            flat = np.ravel_multi_index(idx, shape)
            run = flat - flat % 8
            z, y, x0 = np.unravel_index(run, shape)
            idx = (z, y, x0 + flat % 8)
        for a in range(3):
            out[v, 2 * a] = idx[a].min() if idx[a].size else shape[a]
            out[v, 2 * a + 1] = (idx[a].max() if idx[a].size else -1) + (1 if fault == "hi_off_by_one" and idx[a].size else 0)
        out[v, 6] = idx[0].size
    return out


def crop_ref(boxes, M, margin, shape, fault=None):
    """boxes int32 [nvol, 8] -> crop int32 [nvol / M, 8]."""
    B = boxes.shape[0] // M
    out = np.zeros((B, NREC), dtype=np.int32)
    for b in range(B):
        mine = boxes[b * M:b * M + M].astype(np.int64)
        full = mine[mine[:, 6] > 0]
        if fault == "union_is_modality_0":
            full = mine[:1] if mine[0, 6] > 0 else full
        if fault == "empty_poisons_union" and len(full) and len(full) < M:
            full = np.concatenate([full, np.zeros((1, NREC), dtype=np.int64)])
        for a in range(3):
            if len(full) == 0:
                out[b, 2 * a], out[b, 2 * a + 1] = 0, shape[a] - 1
                continue
            lo, hi = full[:, 2 * a].min() - margin[a], full[:, 2 * a + 1].max() + margin[a]
            if fault != "margin_unclipped":
                lo, hi = max(lo, 0), min(hi, shape[a] - 1)
            out[b, 2 * a], out[b, 2 * a + 1] = lo, hi
        out[b, 6] = int(len(full) > 0)
    return out


def crop_scale(crop_row, mode, allow_upscale, img_size, fault=None):
    """kf (np.float32) of one sample."""
    if mode != "fit":
        return np.float32(1.0)
    r = [np.float64(crop_row[2 * a + 1] - crop_row[2 * a] + 1) / np.float64(img_size[a]) for a in range(3)]
    k = min(r) if fault == "k_from_min" else max(r)
    if not allow_upscale and fault != "k_not_raised":
        k = max(k, 1.0)
    return np.float32(k)


def fold_ref(table, crop, M, mode, allow_upscale, vol_shape, img_size, fault=None):
    """table fp32 [nvol, 32] (not modified), crop int32 [B, 8] -> (folded fp32 table, t64 float64 [nvol, 3]: the t slots before their one
    rounding)."""
    out = table.copy()
    t64 = table[:, T_SLOTS].astype(np.float64)
    if mode is None:
        return out, t64
    for v in range(table.shape[0]):
        c = crop[v // M]
        if c[6] == 0:
            continue
        kf = crop_scale(c, mode, allow_upscale, img_size, fault)
        for a in range(3):
            lo, hi, n = int(c[2 * a]), int(c[2 * a + 1]), img_size[a]
            o = 0 if fault == "o_not_subtracted" else K.pad_crop_offset(vol_shape[a], n)
            t = np.float64(table[v, 4 * a + 3])
            if kf == 1:
                o2 = K.pad_crop_offset(vol_shape[a], n) if fault == "offset_of_volume" else lo + K.pad_crop_offset(hi - lo + 1, n)
                t64[v, a] = t + (o2 - o)
            else:
                for j in range(3):
                    out[v, 4 * a + j] = np.float32(np.float64(kf) * np.float64(table[v, 4 * a + j]))
                t64[v, a] = np.float64(kf) * (t - (n - 1) / 2.0 - o) + (lo + hi) / 2.0
            out[v, 4 * a + 3] = np.float32(t64[v, a])
        if kf != 1 and fault != "exact_kept":
            out[v, FLAGS] = np.float32(int(table[v, FLAGS]) & ~1)
        out[v, CROP_SCALE] = kf
    return out, t64


def window_ref(src, crop, M, img_size, pad_value):
    """The `center` crop as a slice-and-pad: dst[q] = src[q + o'] inside the volume, pad_value outside.  float64 [nvol, D, H, W]."""
    src = np.asarray(src, dtype=np.float64)
    nvol, shape = src.shape[0], src.shape[1:]
    out = np.full((nvol,) + tuple(img_size), float(pad_value))
    for v in range(nvol):
        c = crop[v // M]
        dst, srs = [], []
        for a in range(3):
            o2 = int(c[2 * a]) + K.pad_crop_offset(int(c[2 * a + 1] - c[2 * a] + 1), img_size[a])
            q0, q1 = max(0, -o2), min(img_size[a], shape[a] - o2)
            dst.append(slice(q0, max(q0, q1)))
            srs.append(slice(q0 + o2, max(q0, q1) + o2))
        out[v][tuple(dst)] = src[v][tuple(srs)]
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def check_tables(name, got_boxes, got_crop, got_table, before, src, M, above, margin, mode, allow_upscale, img_size):
    """The device's boxes, crop and folded table (None: not folded) against the reference, under the gate of the docstring."""
    shape = src.shape[1:]
    boxes = boxes_ref(src, above)
    crop = crop_ref(boxes, M, margin, shape)
    assert got_boxes.dtype == np.int32 and got_crop.dtype == np.int32
    bad = np.argwhere(got_boxes.reshape(boxes.shape) != boxes)
    assert bad.size == 0, f"{name}: boxes differ first at volume {bad[0][0]} slot {bad[0][1]}: got {got_boxes.reshape(boxes.shape)[bad[0][0]]}, want {boxes[bad[0][0]]}"
    bad = np.argwhere(got_crop != crop)
    assert bad.size == 0, f"{name}: crop differs first at sample {bad[0][0]} slot {bad[0][1]}: got {got_crop[bad[0][0]]}, want {crop[bad[0][0]]}"
    if got_table is None:
        return boxes, crop
    ref, t64 = fold_ref(before, crop, M, mode, allow_upscale, shape, img_size)
    gb, rb, bb = bits(got_table), bits(ref), bits(before)
    for v in range(ref.shape[0]):
        for s in range(NPARAM):
            if s not in FOLD_SLOTS or mode is None or crop[v // M, 6] == 0:
                assert gb[v, s] == bb[v, s], f"{name}: record {v} slot {s} was written ({bb[v, s]:#x} -> {gb[v, s]:#x})"
            elif s in T_SLOTS and ref[v, CROP_SCALE] != 1:
                a = T_SLOTS.index(s)
                err = abs(np.float64(got_table[v, s]) - t64[v, a])
                assert err <= K.OFFSET_GATE * max(1.0, abs(t64[v, a])), f"{name}: record {v} t[{a}] = {got_table[v, s]!r}, float64 {t64[v, a]!r} (error {err:.3g})"
            else:
                assert gb[v, s] == rb[v, s], f"{name}: record {v} slot {s}: got {got_table[v, s]!r} ({gb[v, s]:#x}), want {ref[v, s]!r} ({rb[v, s]:#x})"
    return boxes, crop


# ---------------------------------------------------------------------------------------------------------------- shared cases
def brain(rng, nvol, shape, centre, radii, specks=0, dtype=np.int16, empty=()):
    """An off-centre ellipsoid of positive values over an exactly-zero background; `specks` isolated bright background voxels per volume
    (the box follows them: nothing filters connected components); volumes in `empty` have no foreground."""
    g = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    out = np.zeros((nvol,) + tuple(shape), dtype=np.float64)
    for v in range(nvol):
        if v in empty:
            continue
        c = np.asarray(centre, dtype=np.float64) + rng.uniform(-.4, .4, 3)
        inside = sum(((g[a] - c[a]) / radii[a]) ** 2 for a in range(3)) <= 1.0
        out[v] = inside * rng.integers(50, 1500, shape)
        for _ in range(specks):
            out[v][tuple(rng.integers(0, n) for n in shape)] = 3000
    return out.astype(dtype)


def edge_positions(v, nvol, nvox, esize):
    """Flat voxel indices at the edges of volume v's chunks: the first and last voxel of each chunk, of its scalar head, of its 16-byte runs
    and of its scalar tail, for a source whose base is 16-byte aligned."""
    parts, chunk = chunk_rule(nvol, nvox)
    per_run = 16 // esize
    pos = []
    for j in range(parts):
        beg = j * chunk
        ln = min(nvox, beg + chunk) - beg
        head = min(ln, (-((v * nvox + beg) * esize) % 16) // esize)
        done = head + (ln - head) // per_run * per_run
        pos += [beg, beg + max(head - 1, 0), beg + min(head, ln - 1), beg + max(done - 1, 0), beg + min(done, ln - 1), beg + ln - 1]
    return pos


CHUNK_SHAPE = (9, 31, 31)          # 8649 voxels, odd: two chunks per volume by the chunk rule, later volumes 2-byte aligned


def on_bf16_grid(x):
    """float32 values rounded to the nearest bf16 (ties to even), as float32; NaN, the infinities and -0.0 stay what they are."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def volume_sets(dtype_name):
    """Computed once and shared: leave the arrays as they are.  name -> (src [nvol, Ds, Hs, Ws], M, foreground_above).  int16 for 'int16', float32 holding bf16-representable values otherwise."""
    sets = _volume_sets(dtype_name)
    return sets if dtype_name == "int16" else {k: (on_bf16_grid(s), M, above) for k, (s, M, above) in sets.items()}


def _volume_sets(dtype_name):
    f = dtype_name != "int16"
    dt = np.float32 if f else np.int16
    rng = np.random.default_rng(7)
    sets = {}
    corners = np.zeros((8, 5, 6, 7), dtype=dt)
    for v in range(8):
        corners[v, 4 * (v >> 2), 5 * ((v >> 1) & 1), 6 * (v & 1)] = 9
    sets["corners-5x6x7"] = (corners, 2, 0.0)
    small = np.zeros((4, 4, 3, 3), dtype=dt)
    small[1] = 5                                                     # sample 0: an empty volume beside a full one
    small[2, 1, 2, 0], small[2, 2, 0, 2] = 4, 1                       # sample 1: runs spanning three rows; its second modality is empty
    sets["4x3x3"] = (small, 2, 0.0)
    sets["all-empty-4x3x3"] = (np.zeros((2, 4, 3, 3), dtype=dt), 2, 0.0)
    thin = (rng.random((3, 6, 5, 1)) < .2).astype(dt) * 7
    thin[0, 0, 0, 0] = thin[2, 5, 4, 0] = 1
    sets["6x5x1"] = (thin, 3, 0.0)
    sets["brain-9x10x37-m3"] = (brain(rng, 3, (9, 10, 37), (5, 4, 21), (2.6, 3.4, 9.2), dtype=dt), 3, 0.0)
    sets["brain-9x10x37-m2"] = (brain(rng, 4, (9, 10, 37), (3, 6, 14), (2.4, 2.3, 8.1), specks=1, dtype=dt, empty=(3,)), 2, 0.0)
    nvox, nvol = int(np.prod(CHUNK_SHAPE)), 12
    assert chunk_rule(nvol, nvox)[0] == 2 and nvox % 2 == 1
    edges = np.zeros((nvol, nvox), dtype=dt)
    for v in range(nvol):
        edges[v, edge_positions(v, nvol, nvox, 4 if dtype_name == "fp32" else 2)[v]] = 3
    sets["chunk-edges-9x31x31"] = (edges.reshape((nvol,) + CHUNK_SHAPE), 3, 0.0)
    thr = np.zeros((2, 5, 6, 7), dtype=dt)
    if f:
        thr[0, 1, 1, 1], thr[0, 3, 4, 5], thr[0, 2, 2, 2] = -0.0, np.nan, -np.inf          # none of them above 0
        thr[0, 1, 2, 3], thr[0, 2, 5, 1] = np.inf, 2.0 ** -120
        thr[1, 0, 0, 0], thr[1, 4, 5, 6] = np.nan, np.nan                                    # no foreground at all
        sets["threshold-0"] = (thr, 1, 0.0)
        eq = np.full((2, 5, 6, 7), 1.5, dtype=dt)                                            # equal to the threshold: not foreground
        eq[0, 2, 3, 4], eq[0, 0, 5, 6], eq[1, 4, 0, 0] = 1.5078125, np.nan, np.inf
        sets["threshold-1.5"] = (eq, 1, 1.5)
    else:
        thr[:] = -3                                                                           # equal to the threshold
        thr[0, 1, 2, 3], thr[0, 3, 1, 6], thr[0, 2, 2, 2] = -2, 32767, -32768
        thr[1, 4, 5, 0] = 0
        sets["threshold--3"] = (thr, 1, -3.0)
    return sets


def tables(nvol, M, vol_shape, img_size, kind, rng):
    """A drawn-looking table [nvol, 32]: 'exact' identity records, 'flips' exact with reversed axes, 'general' rotation, zoom, translation;
    the spatial part is the sample's.  Slots the fold must leave alone and the kernel under test never reads carry distinct NaN payloads."""
    mats = np.empty((nvol, 3, 4))
    for b in range(nvol // M):
        if kind == "exact":
            m = K.identity_matrix(vol_shape, img_size)
        elif kind == "flips":
            m = K.compose((1, 0, 1), (0, 0, 0), (1, 1, 1), (0, 0, 0), vol_shape, img_size)
        else:
            m = K.compose(rng.integers(0, 2, 3), rng.uniform(-.26, .26, 3), rng.uniform(.9, 1.1, 3), rng.uniform(-3, 3, 3), vol_shape, img_size)
        mats[b * M:b * M + M] = m
    t = K.table_from(nvol, mats, exact=kind != "general")
    pay = t.view(np.uint32)
    for v in range(nvol):
        for s in range(NPARAM):
            if s not in FOLD_SLOTS:
                pay[v, s] = 0x7FC00000 | (v * NPARAM + s + 1)
    return t


# (volume set, img_size, mode, margin, allow_upscale, table kind): what the fold tests run.  The brain sets have boxes of about
# (5, 7, 19) and (6, 5, 34) voxels, so the sizes below put s < n, s == n and s > n on different axes (asserted by the gate's own test).
FOLD_CASES = [
    ("brain-9x10x37-m3", (8, 7, 16), "center", (0, 0, 0), False, "exact"),
    ("brain-9x10x37-m3", (8, 7, 16), "center", (1, 2, 3), False, "flips"),
    ("brain-9x10x37-m3", (8, 7, 16), "center", (0, 4, 30), False, "general"),          # margins that clip on one side only, and on both
    ("brain-9x10x37-m3", (8, 7, 16), "fit", (0, 0, 0), False, "exact"),
    ("brain-9x10x37-m3", (8, 7, 16), "fit", (1, 0, 2), False, "general"),
    ("brain-9x10x37-m3", (16, 16, 40), "fit", (0, 0, 0), False, "exact"),              # k raised to 1
    ("brain-9x10x37-m3", (16, 16, 40), "fit", (0, 0, 0), True, "general"),             # k < 1
    ("brain-9x10x37-m3", (8, 7, 32), "fit", (0, 0, 0), True, "flips"),                 # k exactly 1 (asserted): the exact record stays exact
    ("brain-9x10x37-m2", (4, 8, 16), "center", (0, 1, 0), False, "general"),
    ("brain-9x10x37-m2", (4, 8, 16), "fit", (2, 0, 1), False, "flips"),
    ("brain-9x10x37-m2", (4, 8, 16), None, (1, 1, 1), False, "general"),               # mode 0: nothing folded
    ("4x3x3", (2, 3, 4), "fit", (0, 0, 0), True, "general"),
    ("4x3x3", (2, 3, 4), "center", (0, 0, 0), False, "exact"),
    ("all-empty-4x3x3", (2, 3, 4), "fit", (1, 1, 1), True, "exact"),                   # no foreground: nothing folded
    ("corners-5x6x7", (4, 4, 4), "fit", (0, 0, 0), False, "general"),
    ("6x5x1", (4, 4, 4), "center", (0, 1, 0), False, "flips"),
    ("chunk-edges-9x31x31", (8, 16, 16), "fit", (1, 1, 1), False, "general"),
]
