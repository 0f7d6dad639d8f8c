"""CPU: foreground-ranked token selection without a GPU: what ModelCross refuses in its config, the foreground threshold's arithmetic,
the argument errors of the two entry points (host checks in front of any launch, dummy aligned addresses as in test_capi_symbols.py), and
properties of the restated ranking that the GPU tests compare the kernels with."""
import math

import numpy as np
import pytest

import ref_cpu as R
import _tokdrop_check as T
import _tokfg_check as F


# ---- ModelCross's config ----------------------------------------------------------------------------------------------------------------


def test_defaults_leave_the_model_as_it_was():
    import xvit
    model = xvit.ModelCross(R.make_config("tiny"))
    assert model.patch_select == "random" and model.eval_patch_dropout == 0.0
    assert model.patch_foreground_above == 0.0 and model.patch_foreground_min_fraction == 0.05
    assert model.last_token_occupancy is None and model.last_token_foreground is None and model.last_token_keep is None


@pytest.mark.parametrize("over,word", [
    (dict(patch_select="center"), "patch_select"),
    (dict(patch_select="foreground", eval_patch_dropout=1.0), "eval_patch_dropout"),
    (dict(patch_select="foreground", eval_patch_dropout=-0.1), "eval_patch_dropout"),
    (dict(patch_select="foreground", eval_patch_dropout=float("nan")), "eval_patch_dropout"),
    (dict(eval_patch_dropout=0.5), "random subset at validation"),
    (dict(patch_select="random", eval_patch_dropout=0.5), "random subset at validation"),
    (dict(patch_select="foreground", patch_foreground_min_fraction=1.5), "patch_foreground_min_fraction"),
    (dict(patch_select="foreground", patch_foreground_min_fraction=-0.01), "patch_foreground_min_fraction"),
    (dict(patch_select="foreground", patch_foreground_above=float("inf")), "patch_foreground_above"),
    (dict(patch_select="foreground", patch_foreground_above=float("nan")), "patch_foreground_above"),
])
def test_config_refusals(over, word):
    import xvit
    with pytest.raises(ValueError, match=word):
        xvit.ModelCross(R.make_config("tiny", **over))


def test_accepted_configs():
    import xvit
    m = xvit.ModelCross(R.make_config("tiny", patch_select="foreground", patch_dropout=0.5, eval_patch_dropout=0.75, patch_foreground_above=-1.5,
                                      patch_foreground_min_fraction=1.0))
    assert (m.patch_select, m.eval_patch_dropout, m.patch_foreground_above, m.patch_foreground_min_fraction) == ("foreground", 0.75, -1.5, 1.0)
    xvit.ModelCross(R.make_config("tiny", patch_select="foreground", patch_foreground_min_fraction=0.0))       # foreground alone switches nothing on


def test_min_count_arithmetic():
    import xvit.functional as XF
    mc = XF.foreground_min_count
    assert mc(4096, 0.05) == 205 and mc(4096, 0.05, 2) == 410           # 204.8 and 409.6, up
    assert mc(512, 0.05) == 26 and mc(512, 0.0) == 1 and mc(512, 1.0) == 512 and mc(512, 1.0, 3) == 1536
    assert mc(30, 0.1) == 3 and mc(10, 0.3) == 3 and mc(100, 0.07) == 7   # 0.1 * 30, 0.3 * 10 and 0.07 * 100 are not exact in binary: no count too many
    assert mc(1, 0.05) == 1 and mc(8, 0.125) == 1 and mc(8, 0.126) == 2
    for pd, f, m in [(4096, 0.05, 1), (512, 0.33, 3), (64, 0.5, 2), (30, 0.1, 4), (1000, 0.999, 1), (7, 0.2, 5)]:
        assert mc(pd, f, m) == F.min_count(pd, f, m) == max(1, math.ceil(round(f * pd * m, 9)))


# ---- argument errors: nothing is launched, callable without a GPU -------------------------------------------------------------------------


def _refused(rc, lib, name, word=None):
    msg = lib.xvit_last_error_string()
    assert rc < 0 and name in msg, (rc, msg)
    if word is not None:
        assert word in msg, msg


def test_patch_occupancy_argument_errors_do_not_launch():
    from xvit import _lib
    lib = _lib.load()
    A = 256   # any non-null, 16-byte aligned "address"
    name = b"xvit_patch_occupancy"
    occ = lambda img=A, dt=0, out=A, B=2, M=2, vol=(16, 16, 16), patch=(8, 8, 8), above=0.0: lib.xvit_patch_occupancy(   # noqa: E731
        img, dt, out, B, M, *vol, *patch, above, None)
    _refused(occ(img=None), lib, name, b"null")
    _refused(occ(out=None), lib, name, b"null")
    _refused(occ(dt=2), lib, name, b"dtype")                                  # XVIT_I16: raw volumes are not token input
    _refused(occ(dt=7), lib, name, b"dtype")
    _refused(occ(vol=(16, 16, 20)), lib, name, b"divisible")
    _refused(occ(vol=(12, 16, 16)), lib, name, b"divisible")
    _refused(occ(patch=(8, 0, 8)), lib, name, b"bad sizes")
    _refused(occ(B=0), lib, name, b"bad sizes")
    for bad in (float("nan"), float("inf"), -float("inf")):
        _refused(occ(above=bad), lib, name, b"finite")
    big = 1 << 11
    _refused(occ(vol=(big, big, big), patch=(1, 1, 1)), lib, name, b"too large")               # P = 2^33
    _refused(occ(vol=(big, big, big), patch=(big, big, big)), lib, name, b"too large")         # pd = 2^33
    _refused(occ(B=1 << 16, M=1 << 15), lib, name, b"too large")                               # M B = 2^31


def test_token_select_ranked_argument_errors_do_not_launch():
    from xvit import _lib
    lib = _lib.load()
    A = 256
    name = b"xvit_token_select_ranked"
    sel = lambda occ=A, keep=A, slot=A, n_fg=None, S=6, B=3, P=32, K=16, shared=0, mode=_lib.TOKEN_RANK_RANDOM, min_count=1: lib.xvit_token_select_ranked(   # noqa: E731
        occ, keep, slot, n_fg, S, B, P, K, shared, mode, min_count, 1, None)
    _refused(sel(occ=None), lib, name, b"null")
    _refused(sel(keep=None), lib, name, b"null")
    _refused(sel(slot=None), lib, name, b"null")
    _refused(sel(mode=2), lib, name, b"mode")
    _refused(sel(mode=-1), lib, name, b"mode")
    _refused(sel(min_count=-1), lib, name, b"min_count")
    _refused(sel(S=7, shared=1), lib, name, b"multiple")
    # what the plain draw refuses, under this entry point's name
    _refused(sel(S=0), lib, name, b"bad sizes")
    _refused(sel(B=0), lib, name, b"bad sizes")
    _refused(sel(P=0, K=0), lib, name, b"bad sizes")
    _refused(sel(K=0), lib, name, b"at least one")
    _refused(sel(K=33), lib, name, b"exceeds")
    _refused(sel(P=_lib.TOKEN_SELECT_MAX_P + 1), lib, name, b"too long")
    # and the plain draw still answers under its own
    assert lib.xvit_token_select_draw(A, A, 6, 3, 32, 33, 0, 1, None) < 0 and b"xvit_token_select_draw" in lib.xvit_last_error_string()


# ---- the restated ranking --------------------------------------------------------------------------------------------------------------


def _occ(S, P, hi, seed):
    return np.random.default_rng(seed).integers(0, hi, size=(S, P)).astype(np.int32)


@pytest.mark.parametrize("mode", [F.RANDOM, F.TOP])
@pytest.mark.parametrize("shared", [False, True])
def test_ranking_is_a_permutation_prefix(mode, shared):
    S, B, P = 6, 3, 257
    occ = _occ(S, P, 9, 1)
    full, slot_full, _ = F.ranked(occ, B, P, shared, mode, 4, seed=3)
    assert np.array_equal(full, np.broadcast_to(np.arange(P, dtype=np.int32), (S, P)))           # K = P keeps every patch once
    assert np.array_equal(slot_full, full)
    prev = None
    for K in (1, 100, 256):
        keep, slot, n_fg = F.ranked(occ, B, K, shared, mode, 4, seed=3)
        assert keep.shape == (S, K) and bool((keep[:, 1:] > keep[:, :-1]).all()) and keep.min() >= 0 and keep.max() < P
        assert np.array_equal(np.take_along_axis(slot, keep.astype(np.int64), axis=1), np.broadcast_to(np.arange(K), (S, K)))
        assert int((slot >= 0).sum()) == S * K
        if prev is not None:                                                                       # the ranking is one order: a larger K adds to a smaller
            assert all(set(prev[s]) <= set(keep[s]) for s in range(S))
        prev = keep
        if shared:
            assert np.array_equal(keep[:B], keep[B:]) and np.array_equal(n_fg[:B], n_fg[B:])


@pytest.mark.parametrize("shared", [False, True])
def test_no_background_patch_is_kept_while_a_foreground_one_is_dropped(shared):
    S, B, P, mc = 6, 3, 300, 5
    occ = _occ(S, P, 9, 2)
    fg = F.counts(occ, B, shared) >= mc
    for K in (1, 60, 150, 299):
        for mode in (F.RANDOM, F.TOP):
            keep, slot, n_fg = F.ranked(occ, B, K, shared, mode, mc, seed=9)
            assert np.array_equal(n_fg, fg.sum(axis=1))
            for s in range(S):
                kept = slot[s] >= 0
                assert not ((kept & ~fg[s]).any() and (~kept & fg[s]).any()), (K, mode, s)
                assert int((kept & fg[s]).sum()) == min(K, int(n_fg[s]))


def test_random_mode_is_the_plain_draw_inside_one_class():
    S, B, P, K = 6, 3, 500, 77
    occ = _occ(S, P, 9, 3)
    for shared in (False, True):
        for epoch in (None, 4):
            plain = T.draw(S, B, P, K, shared, 21, epoch)
            for mc in (0, 1000):                                                                   # every patch foreground; none
                keep, slot, n_fg = F.ranked(occ, B, K, shared, F.RANDOM, mc, seed=21, epoch=epoch)
                assert np.array_equal(keep, plain[0]) and np.array_equal(slot, plain[1])
                assert bool((n_fg == (P if mc == 0 else 0)).all())
    keep, _, _ = F.ranked(np.ones((1, T.TIE["P"]), np.int32), 1, T.TIE["K"], False, F.RANDOM, 1, seed=T.TIE["seed"])
    assert np.array_equal(keep, T.draw(1, 1, T.TIE["P"], T.TIE["K"], False, T.TIE["seed"])[0])    # equal keys: the smaller index, as there


def test_top_mode_is_monotone_in_the_count_and_ignores_the_seed():
    S, B, P, K = 4, 2, 200, 50
    occ = _occ(S, P, 30, 4)
    for shared in (False, True):
        c = F.counts(occ, B, shared)
        keep, slot, _ = F.ranked(occ, B, K, shared, F.TOP, 3, seed=1)
        assert np.array_equal(keep, F.ranked(occ, B, K, shared, F.TOP, 3, seed=2, epoch=7)[0])
        for s in range(S):
            kept = slot[s] >= 0
            lo, hi = c[s][kept].min(), c[s][~kept].max()
            assert lo >= hi                                                                        # no dropped patch holds more than a kept one
            tied_kept, tied_dropped = np.nonzero(kept & (c[s] == lo))[0], np.nonzero(~kept & (c[s] == lo))[0]
            if len(tied_dropped):
                assert tied_kept.max() < tied_dropped.min()                                        # ties at the K-th place: the smaller index
        more = occ.copy()
        s0, p0 = 1, int(np.nonzero(slot[1] < 0)[0][0])
        more[s0, p0] = 1000                                                                        # raising a dropped patch's count brings it in
        assert F.ranked(more, B, K, shared, F.TOP, 3)[1][s0, p0] >= 0


def test_occupancy_restatement_on_a_hand_counted_volume():
    import torch
    img = torch.zeros(2, 2, 1, 4, 4, 8)
    img[1, 0, 0, 2:, :2, 4:] = 1.0                 # sample 1, modality 0: patch (d 1, h 0, w 1) of the (2, 2, 4) grid, all 16 voxels
    img[0, 1, 0, 0, 3, 0] = float("nan")
    img[0, 1, 0, 0, 3, 1] = float("inf")           # sample 0, modality 1: patch (d 0, h 1, w 0), one voxel (NaN is not counted)
    img[0, 1, 0, 0, 3, 2] = -0.0
    occ = F.occupancy(img, (2, 2, 4), 0.0)
    want = np.zeros((4, 8), np.int32)              # s = m B + b; t = (h Wn + w) Dn + d with Dn = Wn = Hn = 2
    want[0 * 2 + 1, (0 * 2 + 1) * 2 + 1] = 16
    want[1 * 2 + 0, (1 * 2 + 0) * 2 + 0] = 1
    assert np.array_equal(occ, want)
    assert np.array_equal(F.occupancy(img.to(torch.bfloat16), (2, 2, 4), 0.0), want)
    assert int(F.occupancy(img, (2, 2, 4), -1.0).sum()) == img.numel() - 1                         # everything but the NaN
