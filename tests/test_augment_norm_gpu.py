"""GPU: VolumeAugment(normalize=...) end to end: draw -> statistics + fold -> apply, in train() and eval(), both modes, clip on and off,
through the gates of tests/_norm_check.py (statistics against the sorted reference, the fold against its float64 restatement from the
device's own stats, every output element against the clamped float64 restatement under the augment gate; exact-path volumes bit for bit).
normalize=None is bit-identical to a stage built without the argument.  capturable=True inside torch.cuda.graph: one process, one graph,
three replays with the static input overwritten between them."""
import numpy as np
import pytest
import torch

import _augment_check as K
import _norm_check as NC
from _util import dev

pytestmark = pytest.mark.gpu

PAD = -1.0
S, D = (20, 20, 20), (16, 16, 24)          # crop, crop, pad: padding must land on the window floor; a 16-byte run plus a tail
B, M = 2, 2


def volumes(seed, bf16=False):
    rng = np.random.default_rng(seed)
    return NC.signed_bf16(rng, B * M, S) if bf16 else NC.brain_like(rng, B * M, S)


def on_gpu(vols):
    t = torch.from_numpy(np.ascontiguousarray(vols))
    return (t.to(torch.bfloat16) if t.dtype == torch.float32 else t).to(dev()).reshape((B, M) + S)


def as64(out):
    return out.float().cpu().double().numpy().reshape((-1,) + tuple(out.shape[3:]))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def table_of(params):
    return params.table.cpu().numpy().reshape(B * M, K.NPARAM).copy()


def check_call(name, aug, plain, vols, out, mode, clip, pct, fg=0.0):
    """One forward of `aug` on `vols`: `plain` is the same stage without normalize and has drawn the table `aug` folded into."""
    stats = aug.last_stats.table.cpu().numpy().reshape(B * M, NC.NSTAT)
    ref, mean_abs = NC.stats_ref_all(vols, fg, pct)
    NC.check_stats(name, stats, ref, mean_abs, is_int=np.issubdtype(vols.dtype, np.integer))
    before, after = table_of(plain.last_params), table_of(aug.last_params)
    NC.check_fold(name, before, after, stats, mode, clip)
    want, R, exact = NC.apply_ref(vols, after, D, PAD)
    K.check(name, as64(out), want, R, exact, after, "bf16" if out.dtype == torch.bfloat16 else "f32")
    return after, exact


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("mode", ["zscore", "window"])
def test_normalised_stage_in_train_and_eval(mode, clip):
    from xvit.augment import VolumeAugment
    kw = dict(pad_value=PAD, noise_prob=0.5, intensity_scale=0.5, intensity_shift=0.25, seed=3)
    aug = VolumeAugment(D, normalize=mode, clip=clip, **kw)
    plain = VolumeAugment(D, **kw)
    vols = volumes(0)
    src = on_gpu(vols)
    for call in range(2):                                            # train(): two draws
        out = aug(src)
        plain(src)
        after, exact = check_call(f"train call {call}", aug, plain, vols, out, mode, clip, (0.005, 0.995))
        assert bool(aug.last_params.clamped.all()) == clip
    assert aug.call_index == 2
    aug.eval(), plain.eval()
    for out_dtype in (torch.bfloat16, torch.float32):                # eval(): the statistics still run; the exact path, bit for bit
        aug.out_dtype = plain.out_dtype = out_dtype
        out = aug(src)
        plain(src)
        after, exact = check_call("eval", aug, plain, vols, out, mode, clip, (0.005, 0.995))
        assert exact.all() and aug.call_index == 2
    if clip:                                                         # the padded columns sit on the window floor: a lo + b
        floor = after[:, K.SCALE].astype(np.float64) * after[:, NC.CLAMP_LO] + after[:, K.SHIFT]
        assert np.array_equal(as64(out)[:, :, :, 0], np.broadcast_to(K.round_to(floor, "f32")[:, None, None], (B * M, D[0], D[1])))
    # an explicit table stays a pure function of its arguments: no statistics are taken there
    stats_before = aug.last_stats
    again = aug.apply(src, aug.last_params)
    assert torch.equal(bits(again), bits(out)) and aug.last_stats is stats_before


@pytest.mark.parametrize("pct,fg", [(None, 0.0), ((0.0, 1.0), -np.inf), ((0.5, 0.5), 100.5)], ids=["minmax", "all-voxels", "median"])
def test_other_foregrounds_and_percentiles(pct, fg):
    from xvit.augment import VolumeAugment
    kw = dict(pad_value=PAD, seed=5)
    vols = volumes(1)
    src = on_gpu(vols)
    for mode in ("zscore", "window"):
        aug = VolumeAugment(D, normalize=mode, percentiles=pct, foreground_above=fg, **kw)
        plain = VolumeAugment(D, **kw)
        out = aug(src)
        plain(src)
        check_call(f"{mode} {pct} {fg}", aug, plain, vols, out, mode, True, pct, fg)


def test_bf16_source_and_a_nan_voxel_lands_on_the_floor():
    from xvit.augment import VolumeAugment
    vols = volumes(2, bf16=True)
    assert np.isnan(vols).sum() == B * M
    src = on_gpu(vols)
    aug = VolumeAugment(D, pad_value=PAD, normalize="window", seed=1).eval()
    plain = VolumeAugment(D, pad_value=PAD, seed=1).eval()
    out = aug(src)
    plain(src)
    after, exact = check_call("bf16 eval", aug, plain, vols, out, "window", True, (0.005, 0.995))
    assert exact.all() and bool(torch.isfinite(out.float()).all())


def test_normalize_none_is_bit_identical_to_a_stage_without_the_argument():
    from xvit.augment import VolumeAugment
    kw = dict(pad_value=PAD, noise_prob=0.5, intensity_scale=0.001, seed=9)
    a, b = VolumeAugment(D, **kw), VolumeAugment(D, normalize=None, foreground_above=50.0, percentiles=None, clip=True, **kw)
    src = on_gpu(volumes(3))
    for mode in ("train", "eval"):
        getattr(a, mode)(), getattr(b, mode)()
        oa, ob = a(src), b(src)
        assert torch.equal(bits(oa), bits(ob)) and torch.equal(bits(a.last_params.table), bits(b.last_params.table))
        assert b.last_stats is None and not bool(b.last_params.table[..., 29:].any()) and not bool(b.last_params.clamped.any())


def test_fp32_volumes_are_refused_with_the_library_message_before_anything_is_drawn():
    from xvit.augment import VolumeAugment
    aug = VolumeAugment(D, normalize="zscore")
    with pytest.raises(TypeError, match="cast to bf16 or normalise beforehand"):
        aug(on_gpu(volumes(0)).float())
    assert aug.call_index == 0 and aug.last_params is None and aug.last_stats is None
    assert VolumeAugment(D)(on_gpu(volumes(0)).float()).shape == (B, M, 1) + D          # without normalize fp32 volumes still pass


def test_capturable_stage_follows_new_data_at_every_replay():
    from xvit.augment import VolumeAugment
    kw = dict(pad_value=PAD, noise_prob=0.5, seed=11)
    static = on_gpu(volumes(10))
    aug = VolumeAugment(D, normalize="zscore", capturable=True, **kw)
    plain = VolumeAugment(D, **kw)
    aug(static)                                                      # allocates table, counter, statistics and workspace; call index 0 -> 1
    plain(static)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = aug(static)
    assert aug.call_index == 1, "a capture executes nothing"
    seen = []
    for replay in range(3):
        vols = volumes(20 + replay)
        static.copy_(on_gpu(vols))                                   # new data in the captured input
        g.replay()
        torch.cuda.synchronize()
        plain(static)
        check_call(f"replay {replay}", aug, plain, vols, out, "zscore", True, (0.005, 0.995))
        seen.append(aug.last_stats.table.cpu().numpy().copy())
    assert aug.call_index == 4
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
