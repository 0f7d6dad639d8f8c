"""float64 NumPy restatement of the augmenting input stage (include/xvit.h, csrc/augment.hip) and the element-wise gate of its tests.

`apply_ref` restates xvit_augment_apply from the table alone: p = A (z, y, x) + t in float64 from the fp32 table values, trilinear
interpolation with pad_value outside the volume, a v + b, and sigma n with n from Box-Muller on a Python restatement of hash32.  Next to
every value it returns R, the max minus min over the voxel's 8 taps (pad_value included), which the gate scales with.  `compose` restates
the draw kernel's matrix from the recorded draws.  Planted defects (`fault=`) feed tests/test_augment_gate_cpu.py, which shows that the
gate rejects each of them.

Gate for a general-path voxel:  |got - ref| <= c |a| R + eps_out |ref| + 1e-6,  eps_out = 2^-8 for bf16 and 2^-22 for fp32 outputs,
c = 2^-10: an fp32 source coordinate below 512 carries about six roundings of at most 2^-15, three axes give a weight error of at most
5.5e-4 R, and 2^-10 is the next power of two above that.  Volumes stay at or below 256 per axis so that this holds.  Exact-path voxels:
equality with the fp32 value of a v + b rounded to the output dtype.

Noise and draw gates.  They are meant to be 8 x what the first MI355X run measures (profiles/augment_measured.txt says what has been
measured).  No GPU run of these tests has been possible yet, so NOTHING below is measured: the gates are bounds derived from the number
formats, to be replaced by 8 x the measurement at the first run (XVIT_MEASURE_LOG=file records it; the tests print it).
  noise      n = sqrt(-2 ln u1) cos(2 pi u2) in fp32 against float64: logf within 1 ulp and the exact factor -2 give L = -2 ln u1 a
             relative error of 2^-23, so r = sqrt(L) carries 2^-24 of that plus one rounding of its own (2^-24, sqrtf up to 1 ulp:
             2^-23); cospif(2 u2) (its argument is exact) within 2 ulp of a value below 1, 2^-23 absolute; the product one rounding,
             2^-24 relative.  With r <= sqrt(48 ln 2) = 5.77:  |n - n64| <= 5.77 (2^-24 + 2^-23 + 2^-23 + 2^-24) = 2.1e-6.
             NOISE_GATE = 2^-18 = 3.8e-6, the next power of two above it.
  draw       the kernel composes in double and rounds once: |A - A64| <= 2^-24 |A| with |A| < 2 (zooms above 0.5): MATRIX_GATE = 2^-23;
             |t - t64| <= 2^-24 |t|: OFFSET_GATE = 2^-23 relative to max(1, |t64|) (the float64 sums on either side differ by 1e-13).
A noise gate above 1e-3 or a linear-part gate above 1e-4 would mean disagreeing draw indices or formulas, not round-off: asserted below.
"""
import numpy as np

NPARAM = 32
MATRIX, SCALE, SHIFT, SIGMA, NOISE_SEED, FLAGS, FLIPS, ANGLES, ZOOMS, TRANSLATION = 0, 12, 13, 14, 15, 16, 17, 20, 23, 26
C_WEIGHT = 2.0 ** -10

NOISE_GATE, MATRIX_GATE, OFFSET_GATE = 2.0 ** -18, 2.0 ** -23, 2.0 ** -23      # derived, not yet measured: see the docstring
assert NOISE_GATE <= 1e-3 and MATRIX_GATE <= 1e-4

_M64 = (1 << 64) - 1
COUNTER_STRIDE = 0xD1B54A32D192ED03


def hash32(seed, idx):
    """xvit_common.h hash32 on arrays of indices -> uint32 values (as uint64 arrays)."""
    with np.errstate(over="ignore"):
        z = np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(int(seed) & _M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((z ^ (z >> np.uint64(31))) >> np.uint64(16)) & np.uint64(0xFFFFFFFF)


def draw24(seed, idx):
    return hash32(seed, idx) & np.uint64(0xFFFFFF)


def normal_field(noise_seed, n):
    """The standard normal of voxels 0 .. n-1 of a volume, float64."""
    i = np.arange(n, dtype=np.uint64)
    u1 = (draw24(noise_seed, 2 * i).astype(np.float64) + 1.0) / 2.0 ** 24
    u2 = draw24(noise_seed, 2 * i + np.uint64(1)).astype(np.float64) / 2.0 ** 24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def pad_crop_offset(size, target):
    return size // 2 - target // 2 if size >= target else -((target - size) // 2)


def compose(flips, angles, zooms, translation, vol_shape, img_size):
    """The draw kernel's 3 x 4 matrix A | t in float64: L = F Rz Ry Rx diag(1 / zoom), t = c + o + translation - L c."""
    az, ay, ax = (float(v) for v in angles)
    cz, sz, cy, sy, cx, sx = np.cos(az), np.sin(az), np.cos(ay), np.sin(ay), np.cos(ax), np.sin(ax)
    Rz = np.array([[1, 0, 0], [0, cz, -sz], [0, sz, cz]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[cx, -sx, 0], [sx, cx, 0], [0, 0, 1]])
    F = np.diag([-1.0 if f else 1.0 for f in flips])
    L = F @ Rz @ Ry @ Rx @ np.diag(1.0 / np.asarray(zooms, dtype=np.float64))
    c = (np.asarray(img_size, dtype=np.float64) - 1) / 2
    o = np.array([pad_crop_offset(s, t) for s, t in zip(vol_shape, img_size)], dtype=np.float64)
    return np.concatenate([L, (c + o + np.asarray(translation, dtype=np.float64) - L @ c)[:, None]], axis=1)


def table_from(nvol, matrices, *, a=1.0, b=0.0, sigma=0.0, noise_seed=0, exact=False):
    """A hand-written fp32 table [nvol, 32]; every argument is a scalar or one value per volume (matrices: [3, 4] or [nvol, 3, 4])."""
    t = np.zeros((nvol, NPARAM), dtype=np.float32)
    t[:, MATRIX:MATRIX + 12] = np.broadcast_to(np.asarray(matrices, dtype=np.float64), (nvol, 3, 4)).reshape(nvol, 12)
    t[:, SCALE], t[:, SHIFT], t[:, SIGMA] = a, b, sigma
    t[:, NOISE_SEED] = np.broadcast_to(np.asarray(noise_seed, dtype=np.uint32), (nvol,)).view(np.float32)
    t[:, FLAGS] = np.where(np.broadcast_to(exact, (nvol,)), 1.0, 0.0)
    t[:, ZOOMS:ZOOMS + 3] = 1.0
    return t


def identity_matrix(vol_shape, img_size):
    return compose((0, 0, 0), (0, 0, 0), (1, 1, 1), (0, 0, 0), vol_shape, img_size)


def noise_seeds(table):
    return np.ascontiguousarray(table[:, NOISE_SEED]).view(np.uint32)


def apply_ref(src, table, img_size, pad_value, fault=None):
    """src [nvol, Ds, Hs, Ws] (any dtype, taken as float64), table fp32 [nvol, 32] -> (ref, R, exact), float64 [nvol, D, H, W] twice and
    bool [nvol].  The noise term is included.  fault: a planted defect (tests/test_augment_gate_cpu.py)."""
    src = np.asarray(src, dtype=np.float64)
    nvol, Ds, Hs, Ws = src.shape
    D, H, W = img_size
    size = np.array([Ds, Hs, Ws])
    zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    q = np.stack([zz, yy, xx], 0).reshape(3, -1).astype(np.float64)
    ref, R = np.empty((nvol, D * H * W)), np.empty((nvol, D * H * W))
    outside = 0.0 if fault == "zero_outside" else float(pad_value)
    for v in range(nvol):
        row = table[1 if fault == "row_of_sample_1" and v == 0 and nvol > 1 else v].astype(np.float64)
        At = row[MATRIX:MATRIX + 12].reshape(3, 4)
        A = At[:, :3].T if fault == "transposed" else At[:, :3]
        p = A @ q + At[:, 3:4]
        if isinstance(fault, tuple) and fault[0] == "shift":
            p[fault[1]] += 1.0
        if fault == "nearest":
            p = np.floor(p + 0.5)
        p = np.clip(p, -2.0, (size + 1.0)[:, None])     # beyond that every tap is outside: nothing changes
        f = np.floor(p)
        w = p - f
        i0 = f.astype(np.int64)
        taps = np.empty((8, p.shape[1]))
        for k in range(8):
            t = i0 + np.array([k >> 2, (k >> 1) & 1, k & 1])[:, None]
            inside = np.all((t >= 0) & (t < size[:, None]), axis=0)
            tc = np.where(inside, t, 0)
            taps[k] = np.where(inside, src[v, tc[0], tc[1], tc[2]], outside)
        c00, c01 = taps[0] + w[2] * (taps[1] - taps[0]), taps[2] + w[2] * (taps[3] - taps[2])
        c10, c11 = taps[4] + w[2] * (taps[5] - taps[4]), taps[6] + w[2] * (taps[7] - taps[6])
        c0, c1 = c00 + w[1] * (c01 - c00), c10 + w[1] * (c11 - c10)
        val = c0 + w[0] * (c1 - c0)
        a, b = (row[SHIFT], row[SCALE]) if fault == "a_b_swapped" else (row[SCALE], row[SHIFT])
        val = a * val + b
        if row[SIGMA] > 0:
            val = val + row[SIGMA] * normal_field(int(noise_seeds(table)[v]), D * H * W)
        ref[v], R[v] = val, taps.max(0) - taps.min(0)
    exact = (table[:, FLAGS].astype(np.int64) & 1).astype(bool)
    return ref.reshape(nvol, D, H, W), R.reshape(nvol, D, H, W), exact


def round_to(x64, dtype_name):
    """float64 -> fp32 -> the output dtype ('bf16' | 'f32'), round to nearest even, as float64 (what the kernel's single rounding gives
    on an exactly computed fp32 value)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x64)).to(torch.float32)
    if dtype_name == "bf16":
        t = t.to(torch.bfloat16)
    return t.double().numpy()


def where(shape, flat):
    v, z, y, x = np.unravel_index(flat, shape)
    lx = 4 if shape[3] > 64 else 3 if shape[3] > 32 else 2
    return (f"volume {v}, voxel (z {z}, y {y}, x {x}): brick ({x // (8 << lx)}, {y // (64 >> lx)}, {z // 4}) of {8 << lx} x {64 >> lx} x 4, "
            f"wave {z % 4}, run {x // 8 % (1 << lx)}, element {x % 8} ({'tail' if x // 8 * 8 + 8 > shape[3] else 'full run'})")


def check(name, got, ref, R, exact, table, dtype_name):
    """Every destination element against the gate; raises with the count and the place of the worst one.  got: float64 [nvol, D, H, W] of
    the device's values; exact volumes (per the table's flag) must be EQUAL to the rounded reference
    (with noise: inside the round-off of the output dtype and the noise gate).  -> worst error-to-bound ratio."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} != {ref.shape}"
    eps_out = 2.0 ** -8 if dtype_name == "bf16" else 2.0 ** -22
    a = np.abs(table[:, SCALE].astype(np.float64))[:, None, None, None]
    sigma = table[:, SIGMA].astype(np.float64)[:, None, None, None]
    noisy = sigma > 0              # the fp32 Box-Muller is off the float64 one by at most NOISE_GATE sigma (measured, see the docstring)
    bound = C_WEIGHT * a * R + eps_out * np.abs(ref) + 1e-6 + NOISE_GATE * sigma
    bound = np.where(exact[:, None, None, None], np.where(noisy, eps_out * np.abs(ref) + 1e-6 + NOISE_GATE * sigma, 0.0), bound)
    want = np.where(exact[:, None, None, None] & ~noisy, round_to(ref, dtype_name), ref)
    err = np.abs(got - want)
    bad = ~(err <= bound)          # NaN fails
    if bad.any():
        ratio = np.where(bad, np.where(bound > 0, err / np.maximum(bound, 1e-300), np.inf), 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        flat = int(ratio.argmax())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} elements out of bound; worst at {where(got.shape, flat)}: got "
                             f"{got.flat[flat]!r}, float64 reference {want.flat[flat]!r}, bound {bound.flat[flat]:.3g}, R {R.flat[flat]:.4g}"
                             f"{' (exact path: equality)' if exact[np.unravel_index(flat, got.shape)[0]] else ''}")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nan_to_num(np.where(bound > 0, err / bound, 0.0)).max())
