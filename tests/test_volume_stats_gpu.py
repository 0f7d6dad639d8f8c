"""GPU: xvit_volume_stats (csrc/volume_stats.hip) against the sorted-values reference of tests/_norm_check.py, under its gates: counts,
ranks and extremes exact, the int16 mean bit-equal to int64 sum / n_w, the bf16 mean and every standard deviation within 2^-36.

Shapes: 1 x 1 x 1, the smallest volume; 3 x 5 x 7, an odd voxel count, so that with nvol = 3 volumes 1 and 2 start 2-byte aligned;
16^3 and 33 x 31 x 17, a tail behind the 16-byte loads; 96 x 96 x 40, several workgroups per volume; nvol in {1, 3, 16}.  Values on both
sides of every edge of the histogram kernel's LDS window (read from the constants include/xvit.h exports), -32768 and 32767, a constant
42^3 volume (74 088 equal voxels, more than a 16-bit counter holds), no foreground, one foreground voxel, heavy ties straddling every rank.
Every call goes through ONE workspace per test, never re-zeroed by the test: a bin left over by one call would be counted by the next."""
import functools

import numpy as np
import pytest
import torch

import _augment_check as K
import _norm_check as NC
from _util import dev

pytestmark = pytest.mark.gpu

CASES = [((1, 1, 1), 1), ((1, 1, 1), 3), ((1, 1, 1), 16), ((3, 5, 7), 1), ((3, 5, 7), 3), ((3, 5, 7), 16), ((16, 16, 16), 1), ((16, 16, 16), 3),
         ((33, 31, 17), 3), ((33, 31, 17), 16), ((96, 96, 40), 1), ((96, 96, 40), 3)]
IDS = ["%s-nvol%d" % ("x".join(map(str, s)), n) for s, n in CASES]
FGS = [0.0, -np.inf, 100.5]
PCTS = [None, (0.0, 1.0), (0.005, 0.995), (0.5, 0.5)]
SENTINEL = -12345.678


def edges(bf16):
    from xvit import _lib
    return NC.window_edge_values(_lib.STATS_WINDOW_LO, _lib.STATS_WINDOW_BINS, bf16)


@functools.lru_cache(maxsize=None)
def volumes(shape, nvol, bf16=False, seed=0):
    rng = np.random.default_rng(seed + 1000 * nvol + int(np.prod(shape)))
    return NC.signed_bf16(rng, nvol, shape, plant=tuple(edges(True))) if bf16 else NC.brain_like(rng, nvol, shape, plant=tuple(edges(False)))


@functools.lru_cache(maxsize=None)
def reference(shape, nvol, bf16, seed, fg, pct):
    return NC.stats_ref_all(volumes(shape, nvol, bf16, seed), fg, pct)


def on_gpu(vols):
    t = torch.from_numpy(np.ascontiguousarray(vols))
    return (t.to(torch.bfloat16) if t.dtype == torch.float32 else t).to(dev()).unsqueeze(1)       # [nvol, 1, D, H, W]


class Runner:
    """One workspace and one sentinel-framed stats buffer for nvol volumes, reused by every call."""

    def __init__(self, nvol):
        from xvit import ops
        self.nvol = nvol
        self.workspace = ops.volume_stats_workspace(nvol, dev())
        self.frame = torch.full((nvol * NC.NSTAT + 32,), SENTINEL, dtype=torch.float64, device=dev())
        self.stats = self.frame[16:16 + nvol * NC.NSTAT].view(nvol, 1, NC.NSTAT)

    def __call__(self, src, fg=0.0, pct=None, normalize=None, clip=False, table=None):
        from xvit import ops
        from xvit.augment import norm_config
        self.stats.fill_(SENTINEL)
        ops.volume_stats(src, norm_config(normalize, fg, pct, clip), self.stats, self.workspace, table)
        frame = self.frame.cpu().numpy()
        assert np.all(frame[:16] == SENTINEL) and np.all(frame[16 + self.nvol * NC.NSTAT:] == SENTINEL), "a write outside the stats records"
        return frame[16:16 + self.nvol * NC.NSTAT].reshape(self.nvol, NC.NSTAT).copy()

    def workspace_is_zero(self):
        return not bool(self.workspace.any())


@pytest.mark.parametrize("fg", FGS, ids=str)
@pytest.mark.parametrize("shape,nvol", CASES, ids=IDS)
def test_int16_statistics_match_the_sorted_reference(shape, nvol, fg):
    src = on_gpu(volumes(shape, nvol))
    run = Runner(nvol)
    for pct in PCTS:
        ref, mean_abs = reference(shape, nvol, False, 0, fg, pct)
        NC.check_stats(f"int16 fg {fg} percentiles {pct}", run(src, fg, pct), ref, mean_abs, is_int=True)
    assert run.workspace_is_zero()


@pytest.mark.parametrize("fg", FGS, ids=str)
@pytest.mark.parametrize("shape,nvol", [((3, 5, 7), 3), ((16, 16, 16), 1), ((33, 31, 17), 3), ((96, 96, 40), 3)], ids=["3x5x7-3", "16x16x16-1", "33x31x17-3", "96x96x40-3"])
def test_bf16_statistics_match_the_sorted_reference(shape, nvol, fg):
    vols = volumes(shape, nvol, bf16=True)
    assert not np.any(np.signbit(vols) & (vols == 0)), "no -0.0"
    if np.prod(shape) >= 64:
        assert np.all(np.isnan(vols).reshape(nvol, -1).sum(1) == 1) and np.any(vols < 0) and np.any(vols > 0)
    src = on_gpu(vols)
    run = Runner(nvol)
    for pct in PCTS:
        ref, mean_abs = reference(shape, nvol, True, 0, fg, pct)
        got = run(src, fg, pct)
        NC.check_stats(f"bf16 fg {fg} percentiles {pct}", got, ref, mean_abs, is_int=False)
        assert np.all(got[:, NC.N] < np.prod(shape)) or np.prod(shape) < 64        # the NaN voxel is never counted, not even above -inf
    assert run.workspace_is_zero()


@pytest.mark.parametrize("bf16", [False, True], ids=["int16", "bf16"])
def test_constant_volume_overflows_no_counter_and_has_no_deviation(bf16):
    vols = np.full((2, 42, 42, 42), 7, dtype=np.float32 if bf16 else np.int16)
    vols[1] = -3                                                    # counted in global memory, not in the LDS window
    run = Runner(2)
    for fg, n in ((0.0, (74088, 0)), (-np.inf, (74088, 74088))):
        for pct in PCTS:
            got = run(on_gpu(vols), fg, pct)
            ref, mean_abs = NC.stats_ref_all(vols, fg, pct)
            NC.check_stats("constant", got, ref, mean_abs, is_int=not bf16)
            assert tuple(got[:, NC.N]) == n and np.all(got[:, NC.STD] == 0) and got[0, NC.MEAN] == 7 and got[0, NC.LO] == got[0, NC.HI] == 7
    assert run.workspace_is_zero()


def test_no_foreground_one_foreground_voxel_and_the_extremes():
    rng = np.random.default_rng(5)
    vols = NC.brain_like(rng, 4, (16, 16, 16))
    vols[1] = np.minimum(vols[1], 0)                                # no foreground above 0
    vols[2] = np.minimum(vols[2], 0)
    vols[2, 3, 4, 5] = 321                                          # exactly one foreground voxel
    vols[3] = np.where(vols[3] == 32767, 0, vols[3])
    vols[3, 0, 0, 0], vols[3, 15, 15, 15] = -32768, 32767           # first and last voxel of the last volume
    run = Runner(4)
    for fg in FGS:
        for pct in PCTS:
            got = run(on_gpu(vols), fg, pct)
            ref, mean_abs = NC.stats_ref_all(vols, fg, pct)
            NC.check_stats(f"fg {fg} percentiles {pct}", got, ref, mean_abs, is_int=True)
            if fg == 0.0:
                assert not got[1].any() and got[2].tolist() == [1, 1, 321, 0, 321, 321, 321, 321]
            if fg == -np.inf:
                assert got[3, NC.MIN] == -32768 and got[3, NC.MAX] == 32767 and np.all(got[:, NC.N] == 4096)
    assert run.workspace_is_zero()


@pytest.mark.parametrize("bf16", [False, True], ids=["int16", "bf16"])
def test_heavy_ties_straddling_every_rank(bf16):
    rng = np.random.default_rng(6)
    vols = NC.tied(rng, 2, (16, 16, 16))
    if bf16:
        vols = NC.bf16_round(vols.astype(np.float32) / 8)           # rounding keeps the order and only widens the ties
    run = Runner(2)
    for pct in PCTS:
        got = run(on_gpu(vols), 0.0, pct)
        ref, mean_abs = NC.stats_ref_all(vols, 0.0, pct)
        NC.check_stats(f"ties, percentiles {pct}", got, ref, mean_abs, is_int=not bf16)
        assert np.all(got[:, NC.N] == 2000)
    if not bf16:
        assert got[0].tolist()[:2] == [2000, 20] and got[0, NC.LO] == got[0, NC.HI] == 1000          # (0.5, 0.5): the whole tie is the window
        got = run(on_gpu(vols), 0.0, (0.005, 0.995))
        assert got[0, NC.LO] == 50 and got[0, NC.HI] == 2500 and got[0, NC.N_W] == 2000 - 5 - 5


def test_one_workspace_and_stats_buffer_over_three_different_inputs():
    """The scan leaves the histogram zeroed: three calls on different data through the same buffers, each checked, nothing re-zeroed."""
    run = Runner(3)
    rng = np.random.default_rng(7)
    a = NC.brain_like(rng, 3, (33, 31, 17))
    b = (-NC.brain_like(rng, 3, (33, 31, 17)).astype(np.int32)).clip(-32768, 32767).astype(np.int16)      # mostly negative: the global path
    c = (NC.brain_like(rng, 3, (33, 31, 17)) // 7 + 11).astype(np.int16)                                  # other bins again
    for name, vols in (("first", a), ("second", b), ("third", c), ("first again", a)):
        for fg, pct in ((-np.inf, None), (0.0, (0.005, 0.995))):
            ref, mean_abs = NC.stats_ref_all(vols, fg, pct)
            NC.check_stats(f"{name} call, fg {fg}", run(on_gpu(vols), fg, pct), ref, mean_abs, is_int=True)
    assert run.workspace_is_zero()
    bf = NC.signed_bf16(rng, 3, (33, 31, 17))                                                              # and a bf16 call through the same workspace
    ref, mean_abs = NC.stats_ref_all(bf, -np.inf, (0.005, 0.995))
    NC.check_stats("bf16 after int16", run(on_gpu(bf), -np.inf, (0.005, 0.995)), ref, mean_abs, is_int=False)
    assert run.workspace_is_zero()


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("mode", ["zscore", "window"])
@pytest.mark.parametrize("bf16", [False, True], ids=["int16", "bf16"])
def test_fold_writes_slots_12_13_16_29_30_and_nothing_else(bf16, mode, clip):
    rng = np.random.default_rng(8)
    nvol, shape = 5, (16, 16, 16)
    vols = NC.signed_bf16(rng, nvol, shape) if bf16 else NC.brain_like(rng, nvol, shape)
    vols[1] = 0                                                      # no foreground: the record stays as it is
    vols[2] = 9                                                      # constant: sigma' = 1, r = 1
    before = rng.uniform(-2, 2, size=(nvol + 2, K.NPARAM)).astype(np.float32)         # every slot filled; a record of sentinels on either side
    before[:, K.FLAGS] = rng.integers(0, 2, nvol + 2)
    before[:, NC.CLAMP_LO:] = [0.0, 0.0, 7.0]                                         # slot 31 must survive too
    frame = torch.from_numpy(before).to(dev())
    table = frame[1:1 + nvol].view(nvol, 1, K.NPARAM)
    run = Runner(nvol)
    stats = run(on_gpu(vols), 0.0, (0.005, 0.995), normalize=mode, clip=clip, table=table)
    ref, mean_abs = NC.stats_ref_all(vols, 0.0, (0.005, 0.995))
    NC.check_stats("fold", stats, ref, mean_abs, is_int=not bf16)
    after = frame.cpu().numpy()
    assert np.array_equal(after[[0, -1]].view(np.uint32), before[[0, -1]].view(np.uint32)), "a write outside the table"
    NC.check_fold(f"{mode} clip {clip}", before[1:-1], after[1:-1], stats, mode, clip)
    assert stats[1, NC.N] == 0 and stats[2, NC.STD] == 0 and stats[2, NC.LO] == stats[2, NC.HI] == 9
    # mode 0 (statistics only) leaves a given table alone
    frame2 = torch.from_numpy(before).to(dev())
    run(on_gpu(vols), 0.0, None, normalize=None, clip=clip, table=frame2[1:1 + nvol].view(nvol, 1, K.NPARAM))
    assert np.array_equal(frame2.cpu().numpy().view(np.uint32), before.view(np.uint32))


def test_the_python_entry_point_and_reproducibility():
    from xvit.augment import VolumeStats, volume_stats
    vols = volumes((33, 31, 17), 16)
    src = torch.from_numpy(vols).to(dev()).reshape(8, 2, 33, 31, 17)
    s = volume_stats(src, percentiles=(0.005, 0.995))
    assert isinstance(s, VolumeStats) and s.table.shape == (8, 2, 8) and s.table.dtype == torch.float64 and s.table.is_cuda
    ref, mean_abs = reference((33, 31, 17), 16, False, 0, 0.0, (0.005, 0.995))
    NC.check_stats("volume_stats", s.table.cpu().numpy().reshape(16, 8), ref, mean_abs, is_int=True)
    assert torch.equal(s.mean, s.table[..., 2]) and torch.equal(s.lo, s.table[..., 4]) and float(s.n[3, 1]) == ref[7, NC.N]
    for _ in range(3):                                               # integer atomics: bit-reproducible, no switch
        assert torch.equal(volume_stats(src, percentiles=(0.005, 0.995)).table.view(torch.int64), s.table.view(torch.int64))
    with pytest.raises(TypeError, match="cast to bf16 or normalise beforehand"):
        volume_stats(src.float())
