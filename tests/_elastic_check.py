"""float64 NumPy restatement of the elastic deformation (include/xvit.h "Elastic deformation", csrc/elastic.hip) and the gate of its tests.

`field_ref` restates xvit_elastic_draw from (config, seed, call index): the same hash, index map and fp32 fmaf range (`fma32` of
tests/_contrast_check.py), so field and record must be EQUAL slot for slot.  `displacement_ref` is u(q) on the destination grid in
float64 (exact s, exact weights).  `apply_ref` restates xvit_augment_apply_elastic: a sample whose flag is 0 goes through
_augment_check.apply_ref unchanged; a deformed one has p = A (q + u) + t and then the pieces of _augment_check (trilinear taps with
pad_value outside, a v + b, Box-Muller noise), plus the clamp window of xvit_volume_stats.  Planted defects (`fault=`, FAULTS and
DRAW_FAULTS) feed tests/test_elastic_gate_cpu.py, which shows that the gate rejects each of them.

Gate, the form of _augment_check.check:  |got - ref| <= c |a| R + eps_out |ref| + 1e-6 (+ NOISE_GATE sigma),  eps_out = 2^-8 (bf16) or
2^-22 (fp32), for every element of a deformed sample; samples whose flag is 0 are held to _augment_check.check itself.  Two differences:
  R   is max - min over the 4 x 4 x 4 source block floor(p) - 1 .. floor(p) + 2 (pad_value where it leaves the volume): a coordinate
      within round-off of an integer may land in the neighbouring cell, whose taps the block contains.
  c   from the roundings of the arithmetic csrc/elastic.hip implements, per axis of p, in units of 2^-15, for source coordinates below
      512, |phi| <= 16 and rows of A with sum_j |A_ij| <= 2 (rotations times zooms >= 0.87; every table of the tests):
        6      the existing affine coordinate: six roundings of at most 2^-15 (_augment_check).
        u_k    g = fl(i fl(s)): fl(s) is off by 2^-24 relative, the product by half an ulp of a number below 16 (2^-21):
               |dg| <= 13 x 2^-24 + 2^-21 < 1.5 x 2^-20.  |du / dg| <= max |phi_j+1 - phi_j| <= 32 (the derivative of a cubic B-spline is a
               quadratic one of the differences), so 48 x 2^-20 = 1.5 x 2^-15 per axis of the grid, 4.5 x 2^-15 for three.
               Weights: each B_j(tau) takes at most four roundings of intermediates below 6, then k = fl(1 / 6): |dB_j| <= 2^-22, so
               sum_j |dB_j| <= 2^-20 per axis.  The (z, y) reduction: sum |d(Bz By)| <= 2^-20 + 2^-20 + 2^-24 < 2^-19, times |phi| <= 16:
               2^-15; its 16 fmaf round partial sums below 16: 16 x 2^-24 x 16 = 2^-16.  The x sum: 2^-20 x 16 = 2^-16 from its weights,
               4 roundings of 2^-24 x 16 = 2^-18.  Arithmetic: (1 + 0.5 + 0.5 + 0.125) x 2^-15 < 2.25 x 2^-15.
               |du_k| <= 6.75 x 2^-15, taken as 7 x 2^-15.
        A u    sum_j |A_ij| |du_j| <= 2 x 7 = 14; its three roundings of a value below 32 (3 x 2^-24 x 32 < 0.2) and the rounding of
               p_affine + A u below 512 (2^-16 = 0.5): 14.7.
      Per axis 6 + 14.7 = 20.7 units of 2^-15 = 6.32e-4; trilinear interpolation passes a coordinate error on with at most R per axis, so
      three axes give 62.1 x 2^-15 = 1.895e-3 R.  The next power of two is C_ELASTIC = 2^-9 = 1.953e-3, asserted <= 2^-8 below so that it
      cannot swallow a formula error (tests/test_elastic_gate_cpu.py shows what it rejects).
The worst error-to-bound ratio of every GPU test is recorded under XVIT_MEASURE_LOG (profiles/elastic_measured.txt).  The constant is
derived, not fitted.  MEASURED (first MI355X run): the worst ratio over the fp32 cases was 0.084 - 0.122, below 1 / 8, and it came from
the output rounding at elements with R near 0; with the rounding allowance taken off, the smallest c that passed every element was 0.0022
of C_ELASTIC.  The constant stays as derived: it has NOT been tightened, and a later change that does so says so openly.
"""
import numpy as np

import _augment_check as A
from _contrast_check import fma32, uniform

MAX_GRID, NREC = 16, 8
FLAG, U, MAX_ABS = 0, 1, 2
CLAMP_LO, CLAMP_HI, FLAG_EXACT, FLAG_CLAMP = 29, 30, 1, 2
C_ELASTIC = 2.0 ** -9
assert 62.1 * 2.0 ** -15 <= C_ELASTIC <= 2.0 ** -8

_M64 = (1 << 64) - 1
COUNTER_STRIDE = 0xD1B54A32D192ED03
SALT = 0x00454C4153544943                 # "ELASTIC"
SAMPLE_STRIDE, POINT_BASE = 16384, 16
MEASURED = {"c_needed": 0.0}              # set by check(): the smallest c that would pass the last call's deformed elements

FAULTS = ("components_swapped", "cell+1", "b1_b2_swapped", "s_g_over_n", "no_min", "field_by_volume", "field_of_sample_1", "u_behind_A",
          "flag0_deformed")
DRAW_FAULTS = ("locked_ignored",)


# ---------------------------------------------------------------------------------------------------------------- draw
def config(prob=1.0, max_displacement=7.5, locked_borders=2):
    """The elastic arguments of VolumeAugment as fp32 values: what the draw kernel's config struct holds."""
    m = (max_displacement,) * 3 if np.isscalar(max_displacement) else tuple(max_displacement)
    return dict(prob=np.float32(prob), max_displacement=tuple(np.float32(v) for v in m), locked_borders=int(locked_borders))


def locked_mask(grid, L):
    """bool [Gz, Gy, Gx]: control points with an index < L or >= G - L along any axis."""
    m = np.zeros(grid, dtype=bool)
    for axis, G in enumerate(grid):
        idx = np.arange(G).reshape([-1 if a == axis else 1 for a in range(3)])
        m |= (idx < L) | (idx >= G - L)
    return m


def field_ref(cfg, B, grid, seed, call=0, fault=None):
    """xvit_elastic_draw restated -> (field fp32 [B, 3, Gz, Gy, Gx], erec fp32 [B, 8]), every slot as the kernel writes it."""
    s = (((int(seed) & _M64) + call * COUNTER_STRIDE) & _M64) ^ SALT
    Gz, Gy, Gx = grid
    per = Gz * Gy * Gx
    field, erec = np.zeros((B, 3, Gz, Gy, Gx), dtype=np.float32), np.zeros((B, NREC), dtype=np.float32)
    locked = locked_mask(grid, 0 if fault == "locked_ignored" else cfg["locked_borders"])
    for b in range(B):
        i0 = SAMPLE_STRIDE * b
        u0 = uniform(s, np.array([i0], dtype=np.uint64))[0]
        erec[b, U] = u0
        if not u0 < cfg["prob"]:
            continue
        erec[b, FLAG] = 1.0
        for a in range(3):
            m = cfg["max_displacement"][a]
            k = np.arange(per, dtype=np.uint64) + np.uint64(i0 + POINT_BASE + a * per)
            v = np.minimum(np.maximum(fma32(uniform(s, k), np.float32(2.0) * m, -m), -m), m).reshape(grid)
            field[b, a] = np.where(locked, np.float32(0), v)
            erec[b, MAX_ABS + a] = np.abs(field[b, a]).max()
    return field, erec


# ---------------------------------------------------------------------------------------------------------------- displacement
def bspline_weights(tau, fault=None):
    b0 = (1 - tau) ** 3 / 6
    b1 = (3 * tau ** 3 - 6 * tau ** 2 + 4) / 6
    b2 = (-3 * tau ** 3 + 3 * tau ** 2 + 3 * tau + 1) / 6
    b3 = tau ** 3 / 6
    return [b0, b2, b1, b3] if fault == "b1_b2_swapped" else [b0, b1, b2, b3]


def axis_cells(n, G, fault=None):
    """(c int [n], weights [4][n]) for the destination indices 0 .. n - 1 of an axis with G control points."""
    i = np.arange(n, dtype=np.float64)
    g = (i * G / n if fault == "s_g_over_n" else i * (G - 3) / (n - 1)) if n > 1 else 0.0 * i     # exact at the last voxel: G - 3
    c = np.floor(g).astype(np.int64)
    if fault != "no_min":
        c = np.minimum(c, G - 4)
    tau = g - c
    if fault == "cell+1":
        c = c + 1
    return c, bspline_weights(tau, fault)


def displacement_ref(phi, img_size, fault=None):
    """phi [3, Gz, Gy, Gx] -> u float64 [3, D, H, W] in destination voxels.  A read past the grid (planted defects only) gives NaN, as a read
    of foreign memory may: 0 x NaN fails the gate."""
    grid = np.shape(phi)[1:]
    phi = np.pad(np.asarray(phi, dtype=np.float64), ((0, 0), (0, 1), (0, 1), (0, 1)), constant_values=np.nan)
    cells = [axis_cells(n, G, fault) for n, G in zip(img_size, grid)]
    u = np.zeros((3,) + tuple(img_size))
    for a in range(4):
        for b in range(4):
            for c in range(4):
                iz = np.clip(cells[0][0] + a, 0, grid[0])
                iy = np.clip(cells[1][0] + b, 0, grid[1])
                ix = np.clip(cells[2][0] + c, 0, grid[2])
                w = cells[0][1][a][:, None, None] * cells[1][1][b][None, :, None] * cells[2][1][c][None, None, :]
                u += w[None] * phi[:, iz[:, None, None], iy[None, :, None], ix[None, None, :]]
    return u[::-1].copy() if fault == "components_swapped" else u


# ---------------------------------------------------------------------------------------------------------------- apply
def apply_ref(src, table, field, erec, M, img_size, pad_value, fault=None):
    """src [nvol, Ds, Hs, Ws], table fp32 [nvol, 32], field [B, 3, Gz, Gy, Gx], erec [B, 8] -> (ref, R, exact, deformed, cell): float64
    [nvol, D, H, W] twice, bool [nvol] twice (exact: the volume is held to equality, i.e. flag 0 and the table's exact bit) and the control
    cell (c_z, c_y, c_x) of every destination index per axis.  R of a deformed volume is taken over the 4 x 4 x 4 block."""
    src = np.asarray(src, dtype=np.float64)
    nvol, Ds, Hs, Ws = src.shape
    ref0, R0, exact0 = A.apply_ref(src, table, img_size, pad_value)
    if (table[:, A.FLAGS].astype(np.int64) & FLAG_CLAMP).any():            # the clamp window sits in front of a v + b: redo those volumes
        for v in np.nonzero(table[:, A.FLAGS].astype(np.int64) & FLAG_CLAMP)[0]:
            ref0[v] = _resample(src[v], table, v, None, img_size, pad_value)[0]
    ref, R, exact = ref0.copy(), R0.copy(), exact0.copy()
    deformed = np.zeros(nvol, dtype=bool)
    for v in range(nvol):
        b = v if fault == "field_by_volume" and v < field.shape[0] else v // M
        on = erec[v // M, FLAG] != 0
        if fault == "field_of_sample_1" and v // M == 0 and field.shape[0] > 1:
            b = 1
        if fault == "flag0_deformed" and not on:
            on, b = True, next(i for i in range(field.shape[0]) if erec[i, FLAG] != 0)
        if not on:
            continue
        deformed[v] = erec[v // M, FLAG] != 0
        exact[v] = exact[v] and not deformed[v]
        u = displacement_ref(field[b], img_size, fault).reshape(3, -1)
        val, Rv = _resample(src[v], table, v, u, img_size, pad_value, behind=fault == "u_behind_A")
        ref[v] = val
        if deformed[v]:
            R[v] = Rv
    cell = [axis_cells(n, G)[0] for n, G in zip(img_size, field.shape[2:])]
    return ref, R, exact, deformed, cell


def _resample(vol, table, v, u, img_size, pad_value, behind=False):
    """One volume through p = A (q + u) + t (u None: p = A q + t), the optional clamp window, a v + b and noise -> (values, R over 4^3)."""
    D, H, W = img_size
    size = np.array(vol.shape)
    zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    q = np.stack([zz, yy, xx], 0).reshape(3, -1).astype(np.float64)
    row = table[v].astype(np.float64)
    At = row[A.MATRIX:A.MATRIX + 12].reshape(3, 4)
    if u is None:
        p = At[:, :3] @ q + At[:, 3:4]
    elif behind:
        p = At[:, :3] @ q + At[:, 3:4] + u
    else:
        p = At[:, :3] @ (q + u) + At[:, 3:4]
    p = np.clip(p, -2.0, (size + 1.0)[:, None])
    f = np.floor(p)
    w = p - f
    with np.errstate(invalid="ignore"):          # a planted defect's NaN coordinate
        i0 = f.astype(np.int64)

    def tap(dz, dy, dx):
        t = i0 + np.array([dz, dy, dx])[:, None]
        inside = np.all((t >= 0) & (t < size[:, None]), axis=0)
        tc = np.where(inside, t, 0)
        return np.where(inside, vol[tc[0], tc[1], tc[2]], float(pad_value))

    taps = [tap(k >> 2, (k >> 1) & 1, k & 1) for k in range(8)]
    c00, c01 = taps[0] + w[2] * (taps[1] - taps[0]), taps[2] + w[2] * (taps[3] - taps[2])
    c10, c11 = taps[4] + w[2] * (taps[5] - taps[4]), taps[6] + w[2] * (taps[7] - taps[6])
    c0, c1 = c00 + w[1] * (c01 - c00), c10 + w[1] * (c11 - c10)
    val = c0 + w[0] * (c1 - c0)
    if int(row[A.FLAGS]) & FLAG_CLAMP:
        val = np.minimum(np.maximum(val, row[CLAMP_LO]), row[CLAMP_HI])
    val = row[A.SCALE] * val + row[A.SHIFT]
    if row[A.SIGMA] > 0:
        val = val + row[A.SIGMA] * A.normal_field(int(A.noise_seeds(table)[v]), D * H * W)
    hi = np.full(p.shape[1], -np.inf)
    lo = np.full(p.shape[1], np.inf)
    for dz in range(-1, 3):
        for dy in range(-1, 3):
            for dx in range(-1, 3):
                t = tap(dz, dy, dx)
                hi, lo = np.maximum(hi, t), np.minimum(lo, t)
    return val.reshape(D, H, W), (hi - lo).reshape(D, H, W)


def where(shape, flat, cell):
    v, z, y, x = np.unravel_index(flat, shape)
    return A.where(shape, flat) + f", control cell ({cell[0][z]}, {cell[1][y]}, {cell[2][x]})"


def check(name, got, ref, R, exact, deformed, cell, table, dtype_name):
    """Every destination element against its gate: deformed volumes under C_ELASTIC with the 4^3 R, the others as _augment_check.check
    holds them (exact ones to equality).  No element is excluded.  -> the worst error-to-bound ratio over the deformed volumes."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} != {ref.shape}"
    plain = ~deformed
    if plain.any():
        A.check(name + " (flag 0)", got[plain], ref[plain], R[plain], exact[plain], table[plain], dtype_name)
    if not deformed.any():
        return 0.0
    eps_out = 2.0 ** -8 if dtype_name == "bf16" else 2.0 ** -22
    a = np.abs(table[:, A.SCALE].astype(np.float64))[:, None, None, None]
    sigma = table[:, A.SIGMA].astype(np.float64)[:, None, None, None]
    bound = C_ELASTIC * a * R + eps_out * np.abs(ref) + 1e-6 + A.NOISE_GATE * sigma
    err = np.abs(got - ref)
    bad = ~(err <= bound) & deformed[:, None, None, None]          # NaN fails
    if bad.any():
        ratio = np.where(bad, err / bound, 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        flat = int(ratio.argmax())
        raise AssertionError(f"{name}: {int(bad.sum())} of {int(deformed.sum()) * ref[0].size} deformed elements out of bound; worst at "
                             f"{where(got.shape, flat, cell)}: got {got.flat[flat]!r}, float64 reference {ref.flat[flat]!r}, bound "
                             f"{bound.flat[flat]:.3g}, R {R.flat[flat]:.4g}")
    # what the coordinate term alone would have to be: the part of the error the output rounding and the noise gate do not cover, over
    # |a| R.  C_ELASTIC is held against this figure (MEASURED["c_needed"]), the total ratio is dominated by the output rounding where R = 0.
    rest = np.maximum(err - (eps_out * np.abs(ref) + 1e-6 + A.NOISE_GATE * sigma), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where((a * R > 0) & deformed[:, None, None, None], rest / (a * R), 0.0)
    MEASURED["c_needed"] = float(need.max())
    return float((err / bound)[deformed].max())


# ---------------------------------------------------------------------------------------------------------------- shared cases
# (source, destination, grid): the builders of tests/test_elastic_kernels_gpu.py, on which tests/test_elastic_gate_cpu.py shows the gate's teeth.
#   lx3      bricks of 64 x 8 x 4 with a W tail; the source is smaller along x and larger along z, y; 7^3 control points
#   lx4      bricks of 128 x 4 x 4; (4, 4, 4) is a single control cell
#   lx2      bricks of 32 x 16 x 4, odd H and D; (16, 5, 4): s > 1 along z, so consecutive slices skip cells
#   thin     an axis of length 1 (s = 0) and 16 control points over 9 voxels along x: a run of 8 crosses several cells (the per-voxel path)
SHAPES = {"lx3": ((14, 23, 37), (12, 20, 40), (7, 7, 7)), "lx4": ((8, 12, 64), (6, 10, 72), (4, 4, 4)), "lx2": ((11, 9, 20), (9, 7, 24), (16, 5, 4)),
          "thin": ((6, 3, 12), (5, 1, 9), (4, 4, 16))}
B, M, NVOL = 3, 2, 6
FLAGS_ON = (1.0, 0.0, 1.0)
PAD = -1.0
KINDS = ("plain", "clamp", "noise")
_CACHE = {}


def source(shape, nvol=NVOL):
    """A ramp, a checker and one isolated spike per volume, integers of at most 8 bits: exact as int16, bf16 and fp32."""
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    vols = []
    for v in range(nvol):
        s = 2.0 * ((5 * z + 3 * y + 7 * x + 11 * v) % 50) + 50.0 * ((z + y + x + v) % 2)
        s[shape[0] // 2, shape[1] // 2, (shape[2] // 2 + v) % shape[2]] = 256.0
        vols.append(s)
    return np.stack(vols)


def tables(s, d, kind="plain", nvol=NVOL):
    """One record per volume: rotation + zoom + flips + a fractional translation (the general path), a != 1, b != 0; kind "clamp" adds the
    clamp window, "noise" sigma and seeds."""
    draws = [((1, 0, 0), (0.2, -0.1, 0.15), (0.95, 1.05, 1.0), (0.3, -0.7, 1.2)), ((0, 1, 0), (-0.25, 0.0, 0.1), (1.1, 0.9, 1.05), (-1.1, 0.4, 0.0)),
             ((0, 0, 1), (0.0, 0.3, -0.2), (1.0, 1.0, 0.9), (0.0, 0.0, 0.5)), ((1, 1, 1), (0.1, 0.1, 0.1), (1.05, 1.0, 0.95), (0.6, 0.6, -0.6)),
             ((0, 0, 0), (0.3, 0.0, 0.0), (0.9, 1.1, 1.0), (0.0, -2.3, 0.0)), ((0, 1, 1), (0.0, -0.3, 0.25), (1.0, 0.92, 1.08), (1.7, 0.0, -0.9))]
    mats = np.stack([A.compose(*draws[v % 6], s, d) for v in range(nvol)])
    t = A.table_from(nvol, mats, a=np.array([1.1, 0.9, -0.5, 2.0, 1.0, 0.7])[:nvol], b=np.array([0.3, -0.2, 10.0, 0.0, 1.5, -4.0])[:nvol],
                     sigma=0.5 if kind == "noise" else 0.0, noise_seed=np.arange(nvol, dtype=np.uint32) * 2654435761 + 17)
    if kind == "clamp":
        t[:, A.FLAGS] += FLAG_CLAMP
        t[:, CLAMP_LO], t[:, CLAMP_HI] = 20.0, 120.0
    return t


def random_field(grid, m, nb=B, seed=0):
    """Hand-written control grids uniform in [-m, m] (fp32), every sample's its own; and the records, flags FLAGS_ON."""
    rng = np.random.default_rng(seed)
    field = rng.uniform(-m, m, size=(nb, 3) + tuple(grid)).astype(np.float32)
    erec = np.zeros((nb, NREC), dtype=np.float32)
    erec[:, FLAG] = np.resize(np.array(FLAGS_ON, dtype=np.float32), nb)
    erec[:, MAX_ABS:MAX_ABS + 3] = np.abs(field).reshape(nb, 3, -1).max(-1) * erec[:, FLAG:FLAG + 1]
    return field, erec


def case(shape, kind="plain", m=3.0):
    """(src float64 [6, ...], table, field, erec, (ref, R, exact, deformed, cell)) — computed once, shared by every dtype and by both test files."""
    key = (shape, kind, m)
    if key not in _CACHE:
        s, d, grid = SHAPES[shape]
        src, table = source(s), tables(s, d, kind)
        field, erec = random_field(grid, m, seed=len(shape) + int(m))
        _CACHE[key] = (src, table, field, erec, apply_ref(src, table, field, erec, M, d, PAD))
    return _CACHE[key]
