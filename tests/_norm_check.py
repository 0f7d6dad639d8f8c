"""NumPy restatement of the per-volume intensity statistics and normalisation (include/xvit.h, csrc/volume_stats.hip) and the gates of
its tests.

Reference (`stats_ref`): the foreground values F = { v > foreground_above } of one volume sorted on the host, lo / hi by nearest rank
k = max(1, ceil(q n)) (q the fp32 percentile, the product in double), W = { lo <= v <= hi }, then the float64 mean and population standard
deviation of W.  For int16 the mean is the int64 sum divided once.  Planted defects (`fault=`) feed tests/test_norm_gate_cpu.py, which
shows that the gates refuse each of them.

Gates (`check_stats`), all derived, none measured:
  n, n_w, lo, hi, min, max   exact.
  mu, int16                  bit-equal to float64(int64 sum) / float64(n_w).
  mu, bf16                   |d mu| <= 2^-36 mean|v| over W: a double sum of at most 65 536 exact products h v is off by at most
                             65 536 2^-53 sum|h v| = 2^-37 n_w mean|v|, and 2^-36 leaves a factor 2 of room.
  sigma                      |d sigma| <= 2^-36 sigma: the worst case of a <= 65 536-term double sum, 65 540 2^-53 = 7.3e-12, with a
                             factor 2 of room.
`check_fold`: SCALE / SHIFT against the fold restated in float64 FROM THE DEVICE'S OWN read-back stats, |d| <= 2^-23 |a a_n| and
|d| <= 2^-23 (|a b_n| + |b|): one fp32 rounding with a factor 2 of room (the build contracts a b_n + b into an fma, so bit equality is
not promised); slots 29 / 30 and the flag exactly; every other slot bit for bit unchanged.
`apply_ref`: xvit_augment_apply with the clamp, restated on top of _augment_check.apply_ref: resample (a = 1, b = 0, no noise), clamp in
source units with fmax / fmin (a NaN becomes lo), then a v + b and the noise; checked under _augment_check.check, so exact-path volumes
must be EQUAL to clamp-then-affine-then-round.
"""
import math

import numpy as np

import _augment_check as K

NSTAT = 8
N, N_W, MEAN, STD, LO, HI, MIN, MAX = range(8)
CLAMP_LO, CLAMP_HI, FLAG_CLAMP = 29, 30, 2
MODES = {None: 0, "zscore": 1, "window": 2}
REL = 2.0 ** -36
FOLD_REL = 2.0 ** -23
FOLDED_SLOTS = (K.SCALE, K.SHIFT, K.FLAGS, CLAMP_LO, CLAMP_HI)


def rank(q, n):
    return max(1, int(math.ceil(float(np.float32(q)) * float(n))))


def stats_ref(vol, foreground_above=0.0, percentiles=None, fault=None):
    """One volume (an integer array for int16 sources, a float array of bf16-representable values otherwise) -> (record float64 [8],
    mean|v| over W).  fault: "rank_off_by_one", "sample_std", "background_counted" or ("stale_bin", value)."""
    is_int = np.issubdtype(np.asarray(vol).dtype, np.integer)
    v = np.asarray(vol, dtype=np.float64).ravel()
    fg = float(np.float32(foreground_above))
    with np.errstate(invalid="ignore"):
        fore = v > fg                        # NaN compares false
    F = v[fore]
    if fault == "background_counted":
        F = np.append(F, v[~fore & ~np.isnan(v)][:1])
    if isinstance(fault, tuple) and fault[0] == "stale_bin":
        F = np.append(F, float(fault[1]))
    F = np.sort(F)
    n = F.size
    rec = np.zeros(NSTAT)
    if n == 0:
        return rec, 0.0
    if percentiles is None:
        lo, hi = F[0], F[-1]
    else:
        k_lo, k_hi = rank(percentiles[0], n), rank(percentiles[1], n)
        if fault == "rank_off_by_one":       # the 0-based index used as if it were the rank
            k_lo, k_hi = min(n, k_lo + 1), min(n, k_hi + 1)
        lo, hi = F[k_lo - 1], F[k_hi - 1]
    W = F[(F >= lo) & (F <= hi)]
    n_w = W.size
    mu = float(int(W.astype(np.int64).sum())) / float(n_w) if is_int else float(W.mean())
    ss = float(np.sum((W - mu) ** 2))
    sd = math.sqrt(ss / (n_w - 1)) if fault == "sample_std" and n_w > 1 else math.sqrt(ss / n_w)
    rec[:] = (n, n_w, mu, sd, lo, hi, F[0], F[-1])
    return rec, float(np.abs(W).mean())


def stats_ref_all(vols, foreground_above=0.0, percentiles=None, fault=None):
    """[nvol, ...] -> (records [nvol, 8], mean|v| [nvol])."""
    out = [stats_ref(v, foreground_above, percentiles, fault) for v in vols]
    return np.stack([r for r, _ in out]), np.array([m for _, m in out])


def check_stats(name, got, ref, mean_abs, is_int):
    """Device records [nvol, 8] (float64) against the reference; raises at the first volume out of gate."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} != {ref.shape}"
    names = ("n", "n_w", "mean", "std", "lo", "hi", "min", "max")
    for v in range(ref.shape[0]):
        for k in (N, N_W, LO, HI, MIN, MAX):
            assert got[v, k] == ref[v, k], f"{name}: volume {v}: {names[k]} = {got[v, k]!r}, reference {ref[v, k]!r} (exact)"
        if is_int:
            assert got[v, MEAN] == ref[v, MEAN], f"{name}: volume {v}: mean {got[v, MEAN]!r} is not int64 sum / n_w = {ref[v, MEAN]!r}"
        else:
            d, bound = abs(got[v, MEAN] - ref[v, MEAN]), REL * mean_abs[v]
            assert d <= bound, f"{name}: volume {v}: mean {got[v, MEAN]!r}, reference {ref[v, MEAN]!r}: off by {d:.3g} > {bound:.3g}"
        d, bound = abs(got[v, STD] - ref[v, STD]), REL * ref[v, STD]
        assert d <= bound, f"{name}: volume {v}: std {got[v, STD]!r}, reference {ref[v, STD]!r}: off by {d:.3g} > {bound:.3g}"


def fold_ref(before, stats, mode, clip):
    """The fold in float64 from read-back stats: (scale64, shift64, scale bound, shift bound, clamp?) per volume."""
    a, b = before[:, K.SCALE].astype(np.float64), before[:, K.SHIFT].astype(np.float64)
    n, mu, sd, lo, hi = (stats[:, k] for k in (N, MEAN, STD, LO, HI))
    if MODES[mode] == 1:
        sp = np.where(sd > 0, sd, 1.0)
        a_n, b_n = 1.0 / sp, -mu / sp
    else:
        r = np.where(hi - lo > 0, hi - lo, 1.0)
        a_n, b_n = 1.0 / r, -lo / r
    a_n, b_n = np.where(n > 0, a_n, 1.0), np.where(n > 0, b_n, 0.0)
    return a * a_n, a * b_n + b, FOLD_REL * np.abs(a * a_n), FOLD_REL * (np.abs(a * b_n) + np.abs(b)), (n > 0) & bool(clip)


def check_fold(name, before, after, stats, mode, clip):
    """Tables fp32 [nvol, 32] before and after xvit_volume_stats, the device's stats [nvol, 8]."""
    before, after, stats = np.asarray(before), np.asarray(after), np.asarray(stats, dtype=np.float64)
    scale, shift, b_scale, b_shift, clamp = fold_ref(before, stats, mode, clip)
    for v in range(before.shape[0]):
        untouched = [k for k in range(K.NPARAM) if k not in FOLDED_SLOTS]
        assert np.array_equal(before[v, untouched].view(np.uint32), after[v, untouched].view(np.uint32)), f"{name}: volume {v}: a slot outside the fold changed"
        if stats[v, N] == 0:
            assert np.array_equal(before[v].view(np.uint32), after[v].view(np.uint32)), f"{name}: volume {v}: no foreground, yet the record changed"
            continue
        d = abs(float(after[v, K.SCALE]) - scale[v])
        assert d <= b_scale[v], f"{name}: volume {v}: SCALE {after[v, K.SCALE]!r}, float64 fold {scale[v]!r}: off by {d:.3g} > {b_scale[v]:.3g}"
        d = abs(float(after[v, K.SHIFT]) - shift[v])
        assert d <= b_shift[v], f"{name}: volume {v}: SHIFT {after[v, K.SHIFT]!r}, float64 fold {shift[v]!r}: off by {d:.3g} > {b_shift[v]:.3g}"
        flags = int(before[v, K.FLAGS]) | (FLAG_CLAMP if clamp[v] else 0)
        assert float(after[v, K.FLAGS]) == float(flags), f"{name}: volume {v}: flags {after[v, K.FLAGS]!r}, expected {flags}"
        if clamp[v]:
            assert float(after[v, CLAMP_LO]) == stats[v, LO] and float(after[v, CLAMP_HI]) == stats[v, HI], \
                f"{name}: volume {v}: clamp window ({after[v, CLAMP_LO]!r}, {after[v, CLAMP_HI]!r}) is not (lo, hi) = ({stats[v, LO]!r}, {stats[v, HI]!r})"
        else:
            assert after[v, CLAMP_LO].view(np.uint32) == before[v, CLAMP_LO].view(np.uint32) and after[v, CLAMP_HI].view(np.uint32) == before[v, CLAMP_HI].view(np.uint32), \
                f"{name}: volume {v}: clip is off, yet slot 29 / 30 changed"


def apply_ref(src, table, img_size, pad_value, fault=None):
    """xvit_augment_apply with the clamp -> (ref, R, exact) as _augment_check.apply_ref gives them.  fault: "clamp_after_affine"."""
    plain = np.array(table, dtype=np.float32, copy=True)
    plain[:, K.SCALE], plain[:, K.SHIFT], plain[:, K.SIGMA] = 1.0, 0.0, 0.0
    src = np.asarray(src, dtype=np.float64)
    missing = np.isnan(src)
    val, R, exact = K.apply_ref(np.where(missing, 0.0, src), plain, img_size, pad_value)
    if missing.any():
        # _augment_check.apply_ref writes the exact path as a trilinear blend with weights 0 and 1, in which a NaN neighbour of weight 0
        # would spread: resample the NaN mask on its own instead.  Exact path: 1 where the copied voxel is the NaN one.
        hit, _, _ = K.apply_ref(missing.astype(np.float64), plain, img_size, 0.0)
        val = np.where(hit == 1.0 if exact.all() else hit > 0.0, np.nan, val)
    ref = np.empty_like(val)
    for v in range(val.shape[0]):
        row = table[v].astype(np.float64)
        clamp = (int(row[K.FLAGS]) & FLAG_CLAMP) != 0
        lo, hi = row[CLAMP_LO], row[CLAMP_HI]
        x = val[v]
        if clamp and fault != "clamp_after_affine":
            x = np.fmin(np.fmax(x, lo), hi)
        y = row[K.SCALE] * x + row[K.SHIFT]
        if clamp and fault == "clamp_after_affine":
            y = np.fmin(np.fmax(y, lo), hi)
        if row[K.SIGMA] > 0:
            y = y + row[K.SIGMA] * K.normal_field(int(K.noise_seeds(table)[v]), y.size).reshape(y.shape)
        ref[v] = y
    return ref, R, exact


# ------------------------------------------------------------------------------------------------------------------ test inputs
def bf16_round(x):
    """float array -> the nearest bf16 values, as float32."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def bf16_of_key(key):
    """The bf16 value (as float32) of a histogram key: the inverse of the monotone key of include/xvit.h."""
    bits = (key & 0x7FFF) if key & 0x8000 else (~key & 0xFFFF)
    return np.array([bits << 16], dtype=np.uint32).view(np.float32)[0]


def window_edge_values(window_lo, window_bins, bf16):
    """Source values whose keys lie on both sides of every edge of the histogram kernel's LDS window.  For bf16 a key is moved away from
    its edge (outside keys outward, inside keys inward) past -0.0, subnormals, infinities and NaNs, which the tests keep out."""
    out = []
    for key, step in ((window_lo - 1, -1), (window_lo, 1), (window_lo + window_bins - 1, -1), (window_lo + window_bins, 1)):
        if not bf16:
            if 0 <= key < 65536:
                out.append(key - 32768)
            continue
        while 0 <= key < 65536:
            x = float(bf16_of_key(key))
            plain = math.isfinite(x) and (x == 0.0 and not math.copysign(1.0, x) < 0 or abs(x) >= 2.0 ** -126)
            if plain:
                out.append(x)
                break
            key += step
    return out


def brain_like(rng, nvol, shape, plant=()):
    """int16 volumes: about half background (0 and a few negatives), foreground mostly in 1..3000 with outliers, `plant` values three
    times each where the volume has room, and the extremes of the type."""
    nvox = int(np.prod(shape))
    v = rng.integers(1, 3001, size=(nvol, nvox))
    v = np.where(rng.random((nvol, nvox)) < 0.5, 0, v)
    v = np.where(rng.random((nvol, nvox)) < 0.05, rng.integers(-2000, 0, size=(nvol, nvox)), v)
    v = np.where(rng.random((nvol, nvox)) < 0.01, rng.integers(3000, 32767, size=(nvol, nvox)), v)
    special = [-32768, 32767] + [int(p) for p in plant for _ in range(3)]
    if nvox >= 4 * len(special):
        for i in range(nvol):
            v[i, rng.choice(nvox, size=len(special), replace=False)] = special
    return v.astype(np.int16).reshape((nvol,) + tuple(shape))


def signed_bf16(rng, nvol, shape, plant=()):
    """bf16-representable float32 volumes: the SAME magnitudes with either sign (key order against value order), +0.0 background, no
    -0.0, one NaN voxel per volume where there is room."""
    nvox = int(np.prod(shape))
    mag = bf16_round(rng.integers(1, 3001, size=(nvol, nvox)).astype(np.float32))
    v = np.where(rng.random((nvol, nvox)) < 0.5, -mag, mag)
    v = np.where(rng.random((nvol, nvox)) < 0.3, 0.0, v).astype(np.float32)
    special = [float(p) for p in plant for _ in range(3)] + [float("nan")]
    if nvox >= 4 * len(special):
        for i in range(nvol):
            v[i, rng.choice(nvox, size=len(special), replace=False)] = special
    v[v == 0] = 0.0                           # +0.0 only
    return v.reshape((nvol,) + tuple(shape))


def tied(rng, nvol, shape):
    """int16 volumes with 2000 foreground voxels whose sorted order has a heavy tie straddling every rank the percentile sets
    (0, 1), (0.005, 0.995) and (0.5, 0.5) pick: ranks 1, 10, 1000, 1990 and 2000."""
    nvox = int(np.prod(shape))
    assert nvox >= 4096
    out = np.zeros((nvol, nvox), dtype=np.int64)
    for i in range(nvol):
        F = np.concatenate([[7] * 3, [8, 9], [50] * 10, np.sort(rng.integers(60, 900, 975)), [1000] * 20, np.sort(rng.integers(1100, 2400, 975)),
                            [2500] * 10, [2600, 2700], [3000] * 3])
        assert F.size == 2000 and np.all(np.diff(F) >= 0)
        out[i, rng.choice(nvox, size=2000, replace=False)] = F
        rest = np.flatnonzero(out[i] == 0)
        out[i, rest[: rest.size // 4]] = -5     # background below zero, too
    return out.astype(np.int16).reshape((nvol,) + tuple(shape))
