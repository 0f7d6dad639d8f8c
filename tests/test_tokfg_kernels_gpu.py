"""GPU: xvit_patch_occupancy and xvit_token_select_ranked against their NumPy restatement (tests/_tokfg_check.py), bit for bit: both
kernels do integer work only.  Every output sits between sentinel-filled guard rows that must come back untouched, and is pre-filled with
a value no kernel writes, so that an element left out shows as well.

Occupancy: geometries chosen for the kernel's paths: a 16-byte run equal to one patch width, two runs per patch row, patch widths that
are no multiple of 8 and an aligned geometry from a base one element off (one voxel per lane), three different axes with a different count
in every patch (patch order), counts that depend on (sample, modality) (sequence order), 64 workgroups at 128^3, more row bands than
workgroups (the grid stride), more than 1024 patches in a row band (column chunks), and a patch width of 24 (three runs per patch).
Values: the threshold itself, NaN, both infinities and -0.0, a negative threshold, nothing and everything above it.

Ranked draw: every P at the edge of an instantiation (1, 2, 4, 8 patches per thread), K = 1, a middle value and P, both modes, per-sequence
and shared counts, 0 / K - 1 / K / K + 1 / P foreground patches, with and without a device epoch, with and without n_fg."""
import itertools

import numpy as np
import pytest
import torch

import _tokdrop_check as T
import _tokfg_check as F
from _util import dev

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -77          # int32 elements on each side of an output (256 bytes: the output keeps its 16-byte alignment)


def guarded(shape):
    """-> (buffer, the output view in its middle), all SENTINEL."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


# ---- xvit_patch_occupancy ---------------------------------------------------------------------------------------------------------------


def run_occupancy(img, patch, above):
    from xvit import ops
    B, M = img.shape[:2]
    P = int(np.prod([s // p for s, p in zip(img.shape[3:], patch)]))
    buf, out = guarded((M * B, P))
    assert ops.patch_occupancy(img, patch, above, out=out) is out
    torch.cuda.synchronize()
    assert guards_untouched(buf)
    return out.cpu().numpy()


def check_occupancy(img_cpu, patch, above):
    """img_cpu in its final dtype -> the reference, after comparing the kernel with it."""
    ref = F.occupancy(img_cpu, patch, above)
    got = run_occupancy(img_cpu.to(dev()), patch, above)
    assert got.shape == ref.shape and np.array_equal(got, ref), f"{int((got != ref).sum())} of {ref.size} counts differ; first at {np.argwhere(got != ref)[:1].tolist()}"
    return ref


def volume_with_counts(cnt, B, M, vol, patch, dtype):
    """A 0 / 1 volume whose patch t of sequence s = m B + b holds cnt[s, t] ones, in its first features."""
    (D, H, W), (dp, hp, wp) = vol, patch
    Dn, Hn, Wn = D // dp, H // hp, W // wp
    rows = (np.arange(dp * hp * wp)[None, None, :] < cnt[:, :, None]).astype(np.float32)           # [S, P, pd]
    v = rows.reshape(M, B, Hn, Wn, Dn, dp, hp, wp).transpose(1, 0, 4, 5, 2, 6, 3, 7).reshape(B, M, 1, D, H, W)
    return torch.from_numpy(np.ascontiguousarray(v)).to(dtype)


def random_volume(B, M, vol, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, M, 1, *vol, generator=g).to(dtype)


DTYPES = [torch.bfloat16, torch.float32]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("vol,patch,B,M", [
    ((16, 16, 16), (8, 8, 8), 2, 2),          # one 16-byte run = one patch width
    ((16, 16, 32), (8, 8, 16), 2, 1),         # two runs per patch row
    ((4, 6, 10), (2, 3, 5), 2, 3),            # wp % 8 != 0: one voxel per lane
    ((8, 8, 16), (4, 4, 4), 3, 2),            # ... and a patch width that divides 8
    ((4, 4, 48), (2, 2, 24), 2, 2),           # three runs per patch
    ((64, 64, 16), (2, 2, 8), 3, 2),          # 6144 row bands: more than the workgroups of a launch, walked with a grid stride
    ((2, 2, 8200), (1, 1, 8), 1, 2),          # 1025 patches in a row band: two column chunks, 16-byte runs
    ((2, 4, 2050), (1, 2, 2), 2, 1),          # ... one voxel per lane
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_occupancy_geometries(vol, patch, B, M, dtype):
    img = random_volume(B, M, vol, dtype, seed=sum(vol) + B)
    ref = check_occupancy(img, patch, 0.3)
    assert 0 < int(ref.sum()) < img.numel()
    check_occupancy(img, patch, -0.7)                                       # a negative threshold


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_occupancy_patch_and_sequence_order(dtype):
    """(8, 16, 32) / (2, 4, 8): three different axes and grid sizes, and B = 3, M = 2 with counts (t + 5 s) mod 65: every patch of a
    sequence holds another count and every sequence another arrangement, so a wrong patch order, or s = b M + m, cannot pass."""
    vol, patch, B, M = (8, 16, 32), (2, 4, 8), 3, 2
    P, pd = 64, 64
    cnt = (np.arange(P)[None, :] + 5 * np.arange(M * B)[:, None]) % (pd + 1)
    ref = check_occupancy(volume_with_counts(cnt, B, M, vol, patch, dtype), patch, 0.5)
    assert np.array_equal(ref, cnt) and all(len(np.unique(r)) == P for r in ref)
    assert not np.array_equal(ref.reshape(M, B, P).transpose(1, 0, 2).reshape(M * B, P), ref)      # the other sequence order is another table


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_occupancy_from_a_base_one_element_off_gives_the_same_integers(dtype):
    from xvit import ops
    vol, patch, B, M = (16, 16, 32), (8, 8, 16), 2, 2
    img = random_volume(B, M, vol, dtype, seed=5)
    aligned = check_occupancy(img, patch, 0.1)
    buf = torch.empty(img.numel() + 1, dtype=dtype, device=dev())
    off = buf[1:].view(img.shape)
    off.copy_(img)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    assert np.array_equal(run_occupancy(off, patch, 0.1), aligned)
    assert ops.patch_occupancy(off, patch, 0.1).shape == (M * B, 8)        # and it allocates its own output


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_occupancy_at_128_cubed(dtype):
    """(128, 128, 128) / (16, 16, 16), B = M = 1: 64 workgroups of 64 KiB (bf16) each, all 256 threads of a workgroup loading."""
    img = random_volume(1, 1, (128, 128, 128), dtype, seed=9)
    img[0, 0, 0, :, :40] = -1.0                                              # air on one side: patch counts from 0 up
    ref = check_occupancy(img, (16, 16, 16), 0.0)
    assert ref.shape == (1, 512) and int(ref.min()) == 0 and int(ref.max()) > 1500


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_occupancy_values(dtype):
    vol, patch = (8, 8, 16), (4, 4, 8)
    nan, inf = float("nan"), float("inf")
    img = torch.zeros(1, 2, 1, *vol)
    flat = img.view(2, -1)
    flat[0, :8] = torch.tensor([0.0, -0.0, nan, inf, -inf, 1.0, -1.0, 2.0 ** -126])              # against above = 0: +inf, 1 and the tiny value count
    flat[1, 3::7] = nan
    flat[1, 5::11] = inf
    img = img.to(dtype)
    ref = check_occupancy(img, patch, 0.0)
    assert int(ref[0].sum()) == 3 and int(ref[1].sum()) == int(torch.isinf(img[0, 1]).sum())      # strict, NaN never, -0.0 > 0.0 false
    ref = check_occupancy(img, patch, -0.5)                                                      # zeros now count; NaN and -inf still do not
    assert int(ref.sum()) == img.numel() - int(torch.isnan(img).sum()) - 2
    half = torch.full((1, 1, 1, *vol), 0.5).to(dtype)
    assert int(check_occupancy(half, patch, 0.5).sum()) == 0                                     # voxels equal to the threshold: not above it
    assert bool((check_occupancy(half, patch, 0.25) == 128).all())                               # everything is foreground
    assert int(check_occupancy(-half, patch, 0.0).sum()) == 0                                    # nothing is


def test_token_occupancy_is_the_public_form():
    import xvit
    img = random_volume(3, 2, (8, 16, 32), torch.bfloat16, seed=2)
    occ = xvit.token_occupancy(img.to(dev()), (2, 4, 8), above=0.2)
    assert occ.shape == (2, 3, 64) and occ.dtype == torch.int32
    assert np.array_equal(occ.cpu().numpy().reshape(6, 64), F.occupancy(img, (2, 4, 8), 0.2))
    view = img.to(dev()).transpose(0, 1).contiguous().transpose(0, 1)                            # not contiguous: served through a copy
    assert torch.equal(xvit.token_occupancy(view, (2, 4, 8), above=0.2), occ)
    with pytest.raises(ValueError, match="finite"):
        xvit.token_occupancy(img.to(dev()), (2, 4, 8), above=float("nan"))
    with pytest.raises(ValueError, match="expected"):
        xvit.token_occupancy(img[0].to(dev()), (2, 4, 8))


# ---- xvit_token_select_ranked --------------------------------------------------------------------------------------------------------------

MIN_COUNT = 5
SEQS, BATCH = 6, 3           # S = M B with M = 2, B = 3


def occ_with_foreground(P, n_fg, shared, rng):
    """int32 [SEQS, P] under which every sequence has exactly n_fg foreground patches (count >= MIN_COUNT; with `shared`: the sum over the
    two modalities of its sample), in other places per sequence.  Few distinct counts: ties everywhere."""
    rows = BATCH if shared else SEQS
    c = rng.integers(0, MIN_COUNT, size=(rows, P))
    for r in range(rows):
        c[r, rng.permutation(P)[:n_fg]] = rng.integers(MIN_COUNT, MIN_COUNT + 8, size=n_fg)
    if not shared:
        return c.astype(np.int32)
    first = rng.integers(0, c + 1)                                          # the counts split over the modalities at random
    return np.concatenate([first, c - first]).astype(np.int32)


def run_ranked(occ, K, shared, mode, seed, want_n_fg, min_count=MIN_COUNT, B=BATCH):
    from xvit import ops
    S, P = occ.shape
    (kb, keep), (sb, slot), (nb, n_fg) = guarded((S, K)), guarded((S, P)), guarded((S,))
    ops.token_select_ranked(torch.from_numpy(occ).to(dev()), keep, slot, B, shared, mode, min_count, seed, n_fg if want_n_fg else None)
    torch.cuda.synchronize()
    assert guards_untouched(kb) and guards_untouched(sb) and guards_untouched(nb)
    if not want_n_fg:
        assert bool((n_fg == SENTINEL).all())
    return keep.cpu().numpy(), slot.cpu().numpy(), n_fg.cpu().numpy()


def run_plain(S, B, P, K, shared, seed):
    from xvit import ops
    keep, slot = ops.token_select_draw(torch.empty(S, K, dtype=torch.int32, device=dev()), torch.empty(S, P, dtype=torch.int32, device=dev()), B, shared, seed)
    return keep.cpu().numpy(), slot.cpu().numpy()


@pytest.fixture
def device_epoch():
    """set(epoch | None): the dropout epoch the draws read on the device; switched off again afterwards."""
    from xvit import ops
    held = []

    def set_epoch(epoch):
        held[:] = [] if epoch is None else [torch.full((1,), epoch, dtype=torch.int64, device=dev())]
        ops.set_dropout_epoch(held[0] if held else None)

    yield set_epoch
    ops.set_dropout_epoch(None)


@pytest.mark.parametrize("P", [1, 8, 1000, 1024, 1025, 2049, 4097, 8192])
def test_ranked_draw_against_the_restatement(P, device_epoch):
    rng = np.random.default_rng(P)
    Ks = sorted({1, max(1, (P * 3) // 8), P})
    combos = 0
    for K, shared, epoch in itertools.product(Ks, (False, True), (None, 3)):
        device_epoch(epoch)
        for n_target in sorted({0, max(K - 1, 0), K, min(K + 1, P), P}):
            occ = occ_with_foreground(P, n_target, shared, rng)
            seed = 1000 + 17 * K + n_target
            plain = run_plain(SEQS, BATCH, P, K, shared, seed) if n_target in (0, P) else None
            for mode in (F.RANDOM, F.TOP):
                want_n_fg = (combos % 2 == 0)
                combos += 1
                keep, slot, n_fg = run_ranked(occ, K, shared, mode, seed, want_n_fg)
                rk, rs, rn = F.ranked(occ, BATCH, K, shared, mode, MIN_COUNT, seed, epoch)
                what = (P, K, shared, epoch, n_target, mode)
                assert bool((rn == n_target).all()), what
                assert np.array_equal(keep, rk), what
                assert np.array_equal(slot, rs), what
                if want_n_fg:
                    assert np.array_equal(n_fg, rn), what
                assert bool((keep[:, 1:] > keep[:, :-1]).all()) and keep.min() >= 0 and keep.max() < P            # strictly ascending
                assert np.array_equal(np.take_along_axis(slot, keep.astype(np.int64), axis=1), np.broadcast_to(np.arange(K), keep.shape))
                assert int((slot >= 0).sum()) == SEQS * K and int(slot.min()) >= -1                                # slot is the inverse, -1 elsewhere
                if shared:
                    assert np.array_equal(keep[:BATCH], keep[BATCH:])                                              # the modalities of a sample agree
                if mode == F.RANDOM and plain is not None:                                                        # one class only: the plain draw, bit for bit
                    assert np.array_equal(keep, plain[0]) and np.array_equal(slot, plain[1]), what
                if mode == F.TOP:                                                                                 # neither seed nor epoch
                    k2, s2, _ = run_ranked(occ, K, shared, mode, seed + 12345, False)
                    assert np.array_equal(k2, keep) and np.array_equal(s2, slot), what
    assert combos >= 16


def test_random_mode_with_equal_keys_is_the_plain_draw(device_epoch):
    """_tokdrop_check.TIE: the K-th and (K + 1)-th smallest keys of the sequence are equal; one class, so the smaller index wins as in the plain draw."""
    P, K, seed = T.TIE["P"], T.TIE["K"], T.TIE["seed"]
    device_epoch(None)
    plain = run_plain(1, 1, P, K, False, seed)
    assert np.array_equal(plain[0], T.draw(1, 1, P, K, False, seed)[0])
    for fill, n in ((MIN_COUNT, P), (0, 0)):
        keep, slot, n_fg = run_ranked(np.full((1, P), fill, np.int32), K, False, F.RANDOM, seed, True, B=1)
        assert np.array_equal(keep, plain[0]) and np.array_equal(slot, plain[1]) and int(n_fg[0]) == n


def test_top_mode_ties_at_the_kth_place_go_to_the_smaller_index():
    P, K = 1025, 300
    occ = np.zeros((1, P), np.int32)
    occ[0, 100:350] = 9                                  # 250 patches ahead of everything
    occ[0, 500:] = 7                                     # 525 tied for the remaining 50 places
    keep, slot, n_fg = run_ranked(occ, K, False, F.TOP, 0, True, B=1)
    assert np.array_equal(keep[0], np.concatenate([np.arange(100, 350), np.arange(500, 550)])) and int(n_fg[0]) == 775
    assert np.array_equal(keep, F.ranked(occ, 1, K, False, F.TOP, MIN_COUNT)[0])


def test_shared_counts_are_summed_over_the_modalities():
    """Neither modality alone reaches min_count in the patches that the sum makes foreground."""
    P, K = 64, 8
    occ = np.zeros((4, P), np.int32)                     # M = 2, B = 2
    occ[0, 10:18], occ[2, 10:18] = 3, 3                  # sample 0: 6 in patches 10 .. 17
    occ[1, 40:44], occ[3, 44:48] = 4, 4                  # sample 1: 4 in 40 .. 47, below 5
    keep, slot, n_fg = run_ranked(occ, K, True, F.TOP, 0, True, B=2)
    assert np.array_equal(keep[0], np.arange(10, 18)) and np.array_equal(keep[2], keep[0]) and np.array_equal(keep[1], np.arange(40, 48))
    assert n_fg.tolist() == [8, 0, 8, 0]
    keep, _, n_fg = run_ranked(occ, K, False, F.TOP, 0, True, B=2)          # per sequence: nothing reaches 5
    assert n_fg.tolist() == [0, 0, 0, 0] and keep[3].tolist() == [0, 1, 2, 3, 44, 45, 46, 47]


def test_refusals_name_their_entry_point_and_write_nothing():
    from xvit import _lib
    lib = _lib.load()
    img = torch.zeros(2, 2, 1, 16, 16, 16, dtype=torch.bfloat16, device=dev())
    ob, occ = guarded((4, 8))
    i, o = img.data_ptr(), occ.data_ptr()
    bad_occ = [lambda: lib.xvit_patch_occupancy(None, 0, o, 2, 2, 16, 16, 16, 8, 8, 8, 0.0, None),
               lambda: lib.xvit_patch_occupancy(i, 0, None, 2, 2, 16, 16, 16, 8, 8, 8, 0.0, None),
               lambda: lib.xvit_patch_occupancy(i, 5, o, 2, 2, 16, 16, 16, 8, 8, 8, 0.0, None),
               lambda: lib.xvit_patch_occupancy(i, 0, o, 2, 2, 16, 16, 16, 8, 8, 3, 0.0, None),
               lambda: lib.xvit_patch_occupancy(i, 0, o, 2, 2, 16, 16, 16, 8, 8, 8, float("nan"), None),
               lambda: lib.xvit_patch_occupancy(i, 0, o, 2, 2, 16, 16, 16, 8, 8, 8, float("inf"), None),
               lambda: lib.xvit_patch_occupancy(i, 0, o, 1 << 16, 1 << 15, 16, 16, 16, 8, 8, 8, 0.0, None),
               lambda: lib.xvit_patch_occupancy(i, 0, o, 2, 2, 1 << 11, 1 << 11, 1 << 11, 1, 1, 1, 0.0, None),
               lambda: lib.xvit_patch_occupancy(i, 0, o, 2, 2, 1 << 11, 1 << 11, 1 << 11, 1 << 11, 1 << 11, 1 << 11, 0.0, None)]
    for call in bad_occ:
        assert call() < 0 and b"xvit_patch_occupancy" in lib.xvit_last_error_string()
    (kb, keep), (sb, slot) = guarded((4, 4)), guarded((4, 8))
    c, k, s = occ.data_ptr(), keep.data_ptr(), slot.data_ptr()
    sel = lambda occ=c, keep=k, slot=s, S=4, B=2, P=8, K=4, shared=0, mode=0, mc=1: lib.xvit_token_select_ranked(occ, keep, slot, None, S, B, P, K, shared, mode, mc, 1, None)   # noqa: E731
    bad_sel = [dict(occ=None), dict(keep=None), dict(slot=None), dict(mode=2), dict(mc=-1), dict(S=3, shared=1), dict(S=0), dict(B=0), dict(P=0), dict(K=0), dict(K=9),
               dict(P=_lib.TOKEN_SELECT_MAX_P + 1)]
    for kw in bad_sel:
        assert sel(**kw) < 0 and b"xvit_token_select_ranked" in lib.xvit_last_error_string(), kw
    torch.cuda.synchronize()
    for buf in (ob, kb, sb):
        assert bool((buf == SENTINEL).all())
