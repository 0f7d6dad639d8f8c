"""GPU: xvit_contrast_apply and xvit_contrast_draw (csrc/contrast.hip) element by element against the float64 restatement and the
two-tier gate of tests/_contrast_check.py.  Hand-written tables, at most 6 volumes per launch; EVERY destination element is checked.
The launch goes through the C ABI directly so that the test owns the buffers: dst sits inside a larger allocation of sentinels that
must survive, and NaN fills the space of a whole volume before and after src (a read outside the volumes would surface as NaN).

Sizes.  The blur path's tile is TX = 64 by TY = 16 (x, y) and it marches along z; the pointwise path works on 8-voxel runs of the flat
volume.  W in {1, 7, 8, 9, TX - 1, TX, TX + 1, 2 TX + 3}, H in {1, TY - 1, TY, TY + 1, 2 TY + 3}, D in {1, 2, 6, 13, 14, 29}, combined so
that only (29, 35, 131) is large, plus (70, 17, 9): the smallest column the host cuts into two z-segments (D / 2 >= 32).

fp32 -> fp32 results are gated (tier 1: blur alone; tier 2: with bias / gamma; flags 0: equality).  bf16 destinations are never gated by
tolerance: on bf16-representable inputs they must be RNE(fp32 result) bit for bit, and a bf16 source must give the fp32 source's bits.
The worst error-to-bound ratios are printed and recorded under XVIT_MEASURE_LOG (profiles/contrast_measured.txt)."""
import functools

import numpy as np
import pytest
import torch

import _contrast_check as K
from _util import dev, note

pytestmark = pytest.mark.gpu

TX, TY = K.TX, K.TY
SHAPES = [(29, 2 * TY + 3, 2 * TX + 3), (1, 1, 1), (2, TY - 1, 7), (6, TY, 8), (13, TY + 1, 9), (14, 1, TX - 1), (1, 2 * TY + 3, TX), (2, TY + 1, TX + 1),
          (6, TY - 1, 2 * TX + 3), (13, TY, TX), (14, 2 * TY + 3, 9), (29, 1, 8), (70, TY + 1, 9)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
SMALL = (14, TY + 1, TX + 1)          # two tiles along x and along y, tails in both, about 15 000 voxels
SENTINEL = 12345.0
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def run(src64, tab, src_dt="f32", dst_dt="f32"):
    """src64 [nvol, D, H, W] (numpy) through the table -> the destination as a torch CPU tensor of dst_dt; checks the guards."""
    from xvit import _lib, ops
    nvol, D, H, W = src64.shape
    nvox = D * H * W
    guard = (nvox + 15) // 16 * 16                                   # keeps src and dst 16-byte aligned in either dtype
    sbuf = torch.full((guard + nvol * nvox + guard,), float("nan"), dtype=DT[src_dt], device=dev())
    sbuf[guard:guard + nvol * nvox] = torch.from_numpy(np.array(src64, dtype=np.float32)).reshape(-1).to(DT[src_dt]).to(dev())
    dbuf = torch.full((guard + nvol * nvox + guard,), SENTINEL, dtype=DT[dst_dt], device=dev())
    table = torch.from_numpy(np.ascontiguousarray(tab, dtype=np.float32)).to(dev())
    src, dst = sbuf[guard:guard + nvol * nvox], dbuf[guard:guard + nvol * nvox]
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    rc = _lib.load().xvit_contrast_apply(src.data_ptr(), dst.data_ptr(), ops._dt(src), ops._dt(dst), table.data_ptr(), nvol, D, H, W, ops._stream())
    _lib.check(rc, "xvit_contrast_apply")
    torch.cuda.synchronize()
    out = dbuf.cpu()
    assert bool((out[:guard] == SENTINEL).all()) and bool((out[guard + nvol * nvox:] == SENTINEL).all()), "a store outside the destination"
    return out[guard:guard + nvol * nvox].reshape(nvol, D, H, W)


def f64(t):
    return t.float().double().numpy()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


@functools.lru_cache(maxsize=None)
def mixed_case(shape):
    src = K.volumes(6, shape, bf16=True)
    tab = K.mixed_table()
    return src, tab, K.bounds(src, tab)


def gate(name, out, src, tab, cached=None, tier=None):
    r = K.check(name, f64(out), src, tab, cached)
    if tier:
        print(f"contrast {tier}: {name}: worst error / bound = {r:.4e}")
        note(f"contrast:{tier}:{name}", r)
    return r


# ---------------------------------------------------------------------------------------------------------------- every size
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mixed_records_at_every_size_and_dtype(shape):
    """A copy next to blurs next to pointwise records in one launch; fp32 -> fp32 against the gate, the other three combinations bit for
    bit against it.  Two launches give equal bits."""
    src, tab, cached = mixed_case(shape)
    out = run(src, tab)
    gate("mixed " + "x".join(map(str, shape)), out, src, tab, cached, tier="tier2")
    assert np.array_equal(bits(out[5]), np.ascontiguousarray(src[5]).view(np.int32)), "flags 0 is a copy"
    assert np.array_equal(bits(run(src, tab)), bits(out)), "two launches differ"
    want16 = K.rne_bf16(out.numpy())
    assert np.array_equal(bits(run(src, tab, "bf16", "f32")), bits(out)), "bf16 source"
    assert np.array_equal(bits(run(src, tab, "f32", "bf16")).view(np.uint16), want16), "bf16 destination is not RNE of the fp32 result"
    assert np.array_equal(bits(run(src, tab, "bf16", "bf16")).view(np.uint16), want16), "bf16 -> bf16 is not RNE of the fp32 result"


@pytest.mark.parametrize("src_dt,dst_dt", [("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")])
def test_flags_zero_is_a_bit_exact_copy(src_dt, dst_dt):
    for shape in ((13, TY + 1, 9), (6, TY - 1, 2 * TX + 3), (1, 1, 1)):       # odd voxel counts: volumes off the 16-byte grid
        src = np.array(K.volumes(5, shape, seed=3, bf16=src_dt == "bf16"))
        src[1].flat[0], src[2].flat[-1], src[3].flat[src[3].size // 2] = np.nan, np.inf, -0.0
        out = run(src, K.table(5), src_dt, dst_dt)
        want = torch.from_numpy(src.astype(np.float32)).to(DT[src_dt]).to(DT[dst_dt])     # through the source dtype, as run() uploads it
        got_bits, want_bits = bits(out), bits(want)
        if src_dt == "f32" and dst_dt == "bf16":                                 # the one rounding: which NaN it makes of a NaN is the converter's choice
            nan = torch.isnan(want).numpy()
            assert np.array_equal(torch.isnan(out).numpy(), nan)
            got_bits, want_bits = np.where(nan, 0, got_bits), np.where(nan, 0, want_bits)
        diff = np.argwhere(got_bits != want_bits)
        assert len(diff) == 0, f"{shape}: {len(diff)} elements differ, first at {tuple(diff[0])}: {out[tuple(diff[0])]!r} != {want[tuple(diff[0])]!r}"


# ---------------------------------------------------------------------------------------------------------------- blur
def sigma_for(r):
    return (r - 0.25) / 3.0 if r else 0.0          # ceil(3 sigma) = r


@pytest.mark.parametrize("axis", [0, 1, 2], ids=["z", "y", "x"])
def test_each_radius_on_each_axis_alone(axis):
    src = K.volumes(6, SMALL, seed=1)
    for radii in ((0, 1, 2, 3, 4, 5), (6, 5, 3, 1, 6, 2)):
        sig = np.zeros((6, 3), dtype=np.float32)
        sig[:, axis] = [sigma_for(r) for r in radii]
        tab = K.table(6, sigma=sig)
        assert tab[:, K.RADIUS + axis].tolist() == [float(r) for r in radii] and (np.delete(tab[:, K.RADIUS:K.RADIUS + 3], axis, 1) == 0).all()
        out = run(src, tab)
        gate(f"axis {axis} radii {radii}", out, src, tab, tier="tier1")
        if radii[0] == 0:
            assert np.array_equal(bits(out[0]), np.ascontiguousarray(src[0]).view(np.int32)), "radius 0 on every axis: the blur path copies"


def test_three_axes_sigma_two_and_radius_beyond_the_axis():
    tab = K.table(6, sigma=[(0.5, 1.0, 1.5), (2.0, 2.0, 2.0), (1.5, 0.4, 0.9), (2.0, 0.5, 1.0), (0.7, 2.0, 0.3), (1.0, 1.0, 2.0)])
    assert tab[1, K.RADIUS:K.RADIUS + 3].tolist() == [6.0, 6.0, 6.0]
    for shape in (SMALL, (2, 3, 5), (1, 1, 1), (3, 1, TX + 1)):                  # (2, 3, 5): every radius above 1 is beyond its axis
        src = K.volumes(6, shape, seed=2)
        out = run(src, tab)
        gate("three axes " + "x".join(map(str, shape)), out, src, tab, tier="tier1")
    const = np.full((6,) + SMALL, 0.75)
    out = run(const, tab)                                                        # a constant volume stays constant (edge clamp, normalised weights)
    gate("constant", out, const, tab)
    assert float(np.abs(out.numpy() - 0.75).max()) <= K.C_BLUR * 0.75


def test_a_radius_slot_of_nine_behaves_as_six():
    src = K.volumes(4, SMALL, seed=4)
    six = K.table(4, sigma=[(2.0, 2.0, 2.0), (2.0, 0.5, 1.0), (0.5, 2.0, 2.0), (1.9, 1.9, 1.9)])
    nine = six.copy()
    nine[:, K.RADIUS:K.RADIUS + 3] = np.where(six[:, K.RADIUS:K.RADIUS + 3] == 6, 9, six[:, K.RADIUS:K.RADIUS + 3])
    nine[3, K.RADIUS:K.RADIUS + 3] = (1e9, np.inf, 7)
    weird = six.copy()
    weird[0, K.RADIUS:K.RADIUS + 3] = (-3, np.nan, -np.inf)                      # clamps to 0: that axis is skipped
    out6, out9 = run(src, six), run(src, nine)
    gate("radius 6", out6, src, six, tier="tier1")
    assert np.array_equal(bits(out9), bits(out6))
    gate("radius below 0", run(src, weird), src, weird)
    assert np.array_equal(bits(run(src, weird)[0]), np.ascontiguousarray(src[0]).view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- bias and gamma
def test_bias_alone_each_coefficient_alone():
    src = K.volumes(6, SMALL, seed=5)
    for ks in (range(0, 6), range(3, 9)):
        c = np.zeros((6, 9), dtype=np.float32)
        for v, k in enumerate(ks):
            c[v, k] = 0.3 if k % 2 else -0.27
        tab = K.table(6, bias=c)
        gate(f"bias coefficients {list(ks)}", run(src, tab), src, tab, tier="tier2-pointwise")
    one = K.volumes(3, (1, 1, 7), seed=5)                                        # n = 1 on two axes: u = 0 there
    tab = K.table(3, bias=K.MIXED_BIAS)
    gate("bias on 1x1x7", run(one, tab), one, tab)


def test_gamma_alone_and_the_window_edges():
    lo, hi = np.float32(-0.5), np.float32(1.5)
    for window in ((0.0, 1.0), (float(lo), float(hi))):
        a, b = np.float32(window[0]), np.float32(window[1])
        src = np.array(K.volumes(6, SMALL, seed=6))
        special = np.array([a, b, np.nextafter(a, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf)), np.nextafter(a, np.float32(np.inf)),
                            np.nextafter(b, np.float32(-np.inf)), -3.0, 0.0, -0.0, 0.5 * (a + b), 1e-30, -1e-30, 1e30, np.inf, -np.inf], dtype=np.float32)
        src[:, 0, 0, :len(special)] = special
        src[:, 7, 9, 8:8 + len(special)] = special                               # ... and across a run boundary
        tab = K.table(6, gamma=np.array([0.5, 1.0, 2.0, 0.7408182, 1.3498588, 3.0], dtype=np.float32), window=window)
        out = run(src, tab)
        gate(f"gamma window {window}", out, src, tab, tier="tier2-pointwise")
        o = out.numpy()
        assert (o[:, 0, 0, 0] == a).all() and (np.abs(o[:, 0, 0, 1] - b) <= np.spacing(b)).all()
        # the window is decided on the fp32 t = (v - lo) / (hi - lo) (exact divisions here: hi - lo is 1 or 2), so a value one ulp outside
        # may round onto the edge; whatever stays outside comes back unchanged, bit for bit, and whatever is inside stays inside
        with np.errstate(invalid="ignore"):
            t32 = (src.astype(np.float32) - a) / (b - a)
            inside = (t32 >= 0) & (t32 <= 1)
        assert not inside[:, 0, 0, [6, 12, 13, 14]].any() and not inside[0, 0, 0, 2] and inside[:, 0, 0, [0, 1, 4, 5, 9]].all()
        assert ((o >= a) & (o <= b))[inside].all() and np.array_equal(o[~inside].view(np.int32), src[~inside].astype(np.float32).view(np.int32))


def test_all_three_together_with_blur_on_bigger_tiles():
    shape = (13, 2 * TY + 3, TX + 1)
    src = K.volumes(4, shape, seed=7)
    tab = K.table(4, sigma=[(1.0, 1.0, 1.0), (0.5, 1.5, 2.0), (2.0, 0.6, 0.5), (1.4, 1.4, 1.4)], bias=K.MIXED_BIAS,
                  gamma=np.array([0.5, 2.0, 1.2, 0.8], dtype=np.float32), window=(-1.0, 1.0))
    gate("blur + bias + gamma", run(src, tab), src, tab, tier="tier2")


# ---------------------------------------------------------------------------------------------------------------- NaN
def test_nan_stays_where_the_reference_has_it():
    shape = SMALL
    src = np.array(K.volumes(6, shape, seed=8))
    spots = [(0, 0, 0), (7, 8, 32), (13, 16, 64), (6, 15, 63), (3, 16, 0)]
    for v in range(6):
        for z, y, x in spots:
            src[v, z, y, x] = np.nan
    tab = K.mixed_table()
    out = run(src, tab).numpy()
    ref = K.apply_ref(src, tab)
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    for v in (2, 3, 4, 5):                                                       # no blur: the planted voxels and nothing else
        assert int(np.isnan(out[v]).sum()) == len(spots)
    R = K.radii(tab[0])                                                          # blur: exactly the clamped neighbourhoods
    want = np.zeros(shape, dtype=bool)
    for z, y, x in spots:
        want[max(z - R[0], 0):z + R[0] + 1, max(y - R[1], 0):y + R[1] + 1, max(x - R[2], 0):x + R[2] + 1] = True
    assert np.array_equal(np.isnan(out[0]), want)
    K.check("NaN", out.astype(np.float64), src, tab)


# ---------------------------------------------------------------------------------------------------------------- draw
def draw(cfg_kw, B, M, seed, counter=None, advance=False):
    from xvit import _lib, ops
    cfg = K.config(**cfg_kw)
    c = _lib.ContrastConfig()
    c.blur_prob, c.bias_prob, c.gamma_prob, c.bias_coeff, c.blur_isotropic = cfg["blur_prob"], cfg["bias_prob"], cfg["gamma_prob"], cfg["bias_coeff"], int(cfg["blur_isotropic"])
    c.blur_sigma_range[:], c.log_gamma_range[:], c.gamma_window[:] = cfg["blur_sigma_range"], cfg["log_gamma_range"], cfg["gamma_window"]
    table = torch.full((B, M, K.NPARAM), float("nan"), device=dev())
    ops.contrast_draw(c, table, seed, counter, advance)
    torch.cuda.synchronize()
    return cfg, table.cpu().numpy().reshape(B * M, K.NPARAM)


CONFIGS = [dict(), dict(blur_prob=.5, bias_prob=.5, gamma_prob=.5, blur_sigma_range=(.3, 2.0), bias_coeff=.5, log_gamma_range=(-.7, .2), gamma_window=(-1.0, 3.0)),
           dict(blur_prob=1, bias_prob=1, gamma_prob=1), dict(blur_prob=0, bias_prob=0, gamma_prob=0),
           dict(blur_prob=1, blur_isotropic=True, blur_sigma_range=(1.0, 1.0), bias_prob=1, bias_coeff=0.0, gamma_prob=1, log_gamma_range=(0.25, 0.25))]


@pytest.mark.parametrize("which", range(len(CONFIGS)))
def test_draw_is_the_restatement_slot_for_slot(which):
    worst = 0.0
    for seed, (B, M) in ((0, (3, 2)), (12345, (150, 2)), (2 ** 64 - 1, (1, 1))):      # 300 volumes: more than one per thread
        cfg, got = draw(CONFIGS[which], B, M, seed)
        worst = max(worst, K.check_draw(got, K.draw_ref(cfg, B * M, seed)))
        flags = got[:, K.FLAGS]
        if which == 2:
            assert (flags == 7).all() and (got[:, K.SIGMA:K.SIGMA + 3] > 0).all() and (got[:, K.RADIUS:K.RADIUS + 3] >= 2).all()
        if which == 3:
            assert (flags == 0).all() and (got[:, K.GAMMA] == 1).all() and (np.delete(got, [K.GAMMA, K.WINDOW_HI, K.U_BLUR, K.U_BIAS, K.U_GAMMA], 1) == 0).all()
        if which == 4:
            assert (got[:, K.SIGMA:K.SIGMA + 3] == 1).all() and (got[:, K.RADIUS:K.RADIUS + 3] == 3).all() and (got[:, K.BIAS:K.BIAS + 9] == 0).all()
            assert (got[:, K.BETA] == 0.25).all()
    note(f"contrast:draw:gamma_rel:{which}", worst)


def test_draw_isotropic_and_the_counter():
    cfg, iso = draw(dict(blur_prob=1, blur_isotropic=True), 8, 2, 9)
    assert (iso[:, K.SIGMA] == iso[:, K.SIGMA + 1]).all() and (iso[:, K.SIGMA] == iso[:, K.SIGMA + 2]).all() and len(set(iso[:, K.SIGMA])) == 16
    counter = torch.zeros(1, dtype=torch.int64, device=dev())
    kw = dict(blur_prob=.5, bias_prob=.5, gamma_prob=.5)
    cfg, t0 = draw(kw, 4, 2, 77, counter, advance=False)
    assert int(counter) == 0
    cfg, t0b = draw(kw, 4, 2, 77, counter, advance=True)
    assert int(counter) == 1 and np.array_equal(t0.view(np.uint32), t0b.view(np.uint32))
    cfg, t1 = draw(kw, 4, 2, 77, counter, advance=True)
    assert int(counter) == 2 and not np.array_equal(t0, t1)
    K.check_draw(t0, K.draw_ref(cfg, 8, 77, call=0))
    K.check_draw(t1, K.draw_ref(cfg, 8, 77, call=1))
    counter.fill_(5)
    cfg, t5 = draw(kw, 4, 2, 77, counter)
    K.check_draw(t5, K.draw_ref(cfg, 8, 77, call=5))
    cfg, host = draw(kw, 4, 2, (77 + 5 * K.COUNTER_STRIDE) & (2 ** 64 - 1))      # the host-side call index of a plain stage is the same stream
    assert np.array_equal(host.view(np.uint32), t5.view(np.uint32))
