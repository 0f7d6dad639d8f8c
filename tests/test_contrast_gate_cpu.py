"""CPU: the teeth of the contrast stage's gate (tests/_contrast_check.py) and the statistics of its restated draw.

On the inputs the GPU tests use (standard-normal fp32 volumes, the six mixed records) the exact restatement passes with ratio 0 and every
planted defect is rejected.  The restated draw, over 20 000 records: decision frequencies within 4 binomial standard deviations; sigma,
beta and the bias coefficients uniform on their ranges by a chi-square over 16 bins at the 1e-4 level (15 degrees of freedom: 44.26)."""
import numpy as np
import pytest

import _contrast_check as K

SHAPE = (14, 17, 9)
CHI2_15_1E4 = 44.26


@pytest.fixture(scope="module")
def case():
    src, tab = K.volumes(6, SHAPE), K.mixed_table()
    return src, tab, K.bounds(src, tab)


def test_exact_restatement_passes_with_ratio_zero(case):
    src, tab, cached = case
    assert K.check("exact", K.apply_ref(src, tab), src, tab, cached) == 0.0


def test_fp32_rounding_of_the_reference_passes(case):
    src, tab, cached = case
    r = K.check("rounded", K.apply_ref(src, tab).astype(np.float32), src, tab, cached)
    assert 0.0 < r <= 1.0
    got = K.apply_ref(src, tab).astype(np.float32).astype(np.float64)
    got[5, 3, 4, 5] = np.nextafter(np.float32(got[5, 3, 4, 5]), np.float32(np.inf))      # the copy record: one ulp is one too many
    with pytest.raises(AssertionError, match="volume 5"):
        K.check("copy", got, src, tab, cached)


@pytest.mark.parametrize("fault", K.FAULTS)
def test_planted_defect_is_rejected(case, fault):
    src, tab, cached = case
    with pytest.raises(AssertionError, match="out of bound"):
        K.check(fault, K.apply_ref(src, tab, fault=fault), src, tab, cached)


def test_a_stray_or_missing_nan_is_rejected(case):
    src, tab, cached = case
    got = K.apply_ref(src, tab)
    got[2, 1, 1, 1] = np.nan
    with pytest.raises(AssertionError, match="volume 2"):
        K.check("stray NaN", got, src, tab, cached)
    s2 = np.array(src)
    s2[0, 7, 8, 4] = np.nan
    ref = K.apply_ref(s2, tab)
    zz, yy, xx = np.nonzero(np.isnan(ref[0]))
    assert (zz.min(), zz.max(), yy.min(), yy.max(), xx.min(), xx.max()) == (5, 9, 5, 11, 0, 8) and np.isnan(ref[0]).sum() == 5 * 7 * 9   # R = (2, 3, 5), clamped
    assert not np.isnan(ref[1:]).any()
    got = np.array(ref)
    got[0, 5, 5, 0] = 0.0
    with pytest.raises(AssertionError, match="volume 0"):
        K.check("missing NaN", got, s2, tab)


def test_where_names_tile_plane_and_lane():
    tab = K.mixed_table()
    shape = (6, 29, 35, 131)
    flat = np.ravel_multi_index((0, 7, 18, 70), shape)
    assert "tile (1, 1) of 64 x 16, plane 7, thread 33 (wave 0, lane 33), element 2" in K.where(shape, flat, tab)
    assert "pointwise path, run" in K.where(shape, np.ravel_multi_index((2, 7, 18, 70), shape), tab)


def test_fma32_is_one_rounding():
    from fractions import Fraction
    rng = np.random.default_rng(0)
    u = rng.integers(0, 1 << 24, 4000).astype(np.float64) / 2.0 ** 24
    a = rng.standard_normal(4000).astype(np.float32)
    b = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 3, 4000)).astype(np.float32)
    got = K.fma32(u, a, b)
    for i in range(4000):
        exact = Fraction(float(u[i])) * Fraction(float(a[i])) + Fraction(float(b[i]))
        g = np.float32(got[i])
        near = [np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))]
        assert all(abs(Fraction(float(g)) - exact) <= abs(Fraction(float(n)) - exact) for n in near), i


def _chi2(x, lo, hi):
    n = len(x)
    counts = np.histogram(x, bins=16, range=(lo, hi))[0]
    assert counts.sum() == n, "values outside the range"
    return float(((counts - n / 16) ** 2 / (n / 16)).sum())


def test_restated_draw_statistics():
    n = 20000
    cfg = K.config(blur_prob=.2, blur_sigma_range=(.5, 1.5), bias_prob=.2, bias_coeff=.3, gamma_prob=.3, log_gamma_range=(-.3, .3))
    t = K.draw_ref(cfg, n, seed=1234)
    flags = t[:, K.FLAGS].astype(int)
    for bit, p in ((K.FLAG_BLUR, .2), (K.FLAG_BIAS, .2), (K.FLAG_GAMMA, .3)):
        k = int((flags & bit > 0).sum())
        assert abs(k - n * p) <= 4 * np.sqrt(n * p * (1 - p)), (bit, k)
    blur, bias, gam = (flags & 1) > 0, (flags & 2) > 0, (flags & 4) > 0
    for a in range(3):
        assert _chi2(t[blur, K.SIGMA + a], .5, 1.5) < CHI2_15_1E4, a
    assert not np.array_equal(t[blur, K.SIGMA], t[blur, K.SIGMA + 1])
    for k in range(9):
        assert _chi2(t[bias, K.BIAS + k], -.3, .3) < CHI2_15_1E4, k
    assert _chi2(t[gam, K.BETA], -.3, .3) < CHI2_15_1E4
    # what a decision that came out false leaves behind
    assert (t[~blur, K.SIGMA:K.RADIUS + 3] == 0).all() and (t[~bias, K.BIAS:K.BIAS + 9] == 0).all()
    assert (t[~gam, K.GAMMA] == 1).all() and (t[~gam, K.BETA] == 0).all() and (t[:, 23:] == 0).all()
    r = t[blur, K.RADIUS:K.RADIUS + 3]
    assert set(np.unique(r)) <= {2.0, 3.0, 4.0, 5.0} and (r == np.ceil(3 * t[blur, K.SIGMA:K.SIGMA + 3].astype(np.float64))).mean() > 0.999
    iso = K.draw_ref(K.config(blur_prob=1, blur_isotropic=True), 64, seed=5)
    assert (iso[:, K.SIGMA] == iso[:, K.SIGMA + 1]).all() and (iso[:, K.SIGMA] == iso[:, K.SIGMA + 2]).all()
    assert not np.array_equal(K.draw_ref(cfg, 64, 7, call=0), K.draw_ref(cfg, 64, 7, call=1))
