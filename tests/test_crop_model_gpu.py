"""GPU: VolumeAugment(crop_foreground=...) (xvit/augment.py) against its own kernels, the NumPy restatement of tests/_crop_check.py and the
element-wise gates of tests/_augment_check.py and tests/_elastic_check.py on the folded table (the apply kernels and their gates are
unchanged: the table carries the crop).

Shapes: B = 2, M = 2 volumes of (40, 36, 27) int16 with an off-centre ellipsoid "brain" over an exactly-zero background and, in one
modality, an isolated bright background voxel that the box follows; img_size (16, 16, 16).  Source coordinates stay far below 512."""
import functools

import numpy as np
import pytest
import torch

import _augment_check as K
import _crop_check as X
import _elastic_check as E
import _norm_check as NC
from _util import dev

pytestmark = pytest.mark.gpu

S, D = (40, 36, 27), (16, 16, 16)
B, M = 2, 2
PAD = -1.0
QUIET = dict(scale_intensity_prob=0, shift_intensity_prob=0, noise_prob=0)


@functools.lru_cache(maxsize=None)
def volumes(seed=0):
    """Computed once per seed and shared: leave it as it is."""
    rng = np.random.default_rng(100 + seed)
    v = X.brain(rng, B * M, S, (24 - 3 * seed, 13 + 2 * seed, 15), (9.5, 8.2 + seed, 7.4), dtype=np.int16)
    v[1, 3 + seed, 30, 2] = 3000                           # an isolated bright voxel: sample 0's box reaches out to it
    v.setflags(write=False)
    return v


def on_gpu(vols):
    return torch.from_numpy(np.array(vols)).to(dev()).reshape((B, M) + tuple(vols.shape[1:]))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def as64(out):
    return out.float().cpu().double().numpy().reshape((-1,) + tuple(out.shape[3:]))


def table_of(params):
    return params.table.cpu().numpy().reshape(B * M, K.NPARAM).copy()


def check_crop(name, aug, plain, vols, mode, margin=(0, 0, 0), up=False, above=0.0):
    """aug.last_crop and the fold in aug.last_params against the restatement; `plain` is the same stage without the crop and has drawn the
    table `aug` folded into.  -> (folded table, crop)."""
    fb = aug.last_crop
    boxes, crop = X.check_tables(name, fb.boxes.cpu().numpy().reshape(B * M, 8), fb.crop.cpu().numpy(), table_of(aug.last_params), table_of(plain.last_params),
                                 vols, M, above, margin, mode, up, D)
    return table_of(aug.last_params), crop


def test_the_stage_equals_its_kernels_and_the_restatement():
    from xvit import _lib, ops
    from xvit.augment import VolumeAugment, foreground_boxes
    vols = volumes()
    src = on_gpu(vols)
    aug = VolumeAugment(D, pad_value=PAD, crop_foreground="fit", crop_margin=(1, 0, 2), seed=5)
    plain = VolumeAugment(D, pad_value=PAD, seed=5)
    for call in range(2):
        out = aug(src)
        plain(src)
        after, crop = check_crop(f"call {call}", aug, plain, vols, "fit", (1, 0, 2))
        assert crop[0, 3] == 30 and crop[0, 4] == 2 - 2 and crop[:, 6].all(), "the box follows the isolated voxel"
        # the kernels, called by hand on the call's seed
        table = torch.empty(B, M, _lib.AUG_NPARAM, device=dev())
        ops.augment_draw(aug.config, table, S, D, (5 + call * K.COUNTER_STRIDE) & ((1 << 64) - 1))
        assert torch.equal(bits(table), bits(plain.last_params.table))
        boxes, cr = torch.empty(B, M, 8, dtype=torch.int32, device=dev()), torch.empty(B, 8, dtype=torch.int32, device=dev())
        ops.volume_bbox(src, aug.crop_config, D, boxes, cr, ops.volume_bbox_workspace(B * M, int(np.prod(S)), dev()), table)
        assert torch.equal(bits(table), bits(aug.last_params.table)) and torch.equal(boxes, aug.last_crop.boxes) and torch.equal(cr, aug.last_crop.crop)
        assert torch.equal(bits(aug.apply(src, table)), bits(out)) and out.shape == (B, M, 1) + D
        # all modalities of a sample carry one A | t and one crop scale
        assert np.array_equal(after.reshape(B, M, 32)[:, 0, :12], after.reshape(B, M, 32)[:, 1, :12])
        assert torch.equal(aug.last_params.crop_scale[:, 0], aug.last_params.crop_scale[:, 1]) and bool((aug.last_params.crop_scale >= 1).all())
        # every element, on the folded table
        want, R, exact = K.apply_ref(vols, after, D, PAD)
        K.check(f"fit call {call}", as64(out), want, R, exact, after, "bf16")
    assert aug.call_index == 2
    alone = foreground_boxes(src, margin=(1, 0, 2))
    assert torch.equal(alone.boxes, aug.last_crop.boxes) and torch.equal(alone.crop, aug.last_crop.crop)
    assert alone.lo.tolist() == crop[:, 0:6:2].tolist() and alone.hi.tolist() == crop[:, 1:6:2].tolist()
    assert alone.nonempty.tolist() == [1, 1] and alone.count.cpu().numpy().reshape(-1).tolist() == [int((v > 0).sum()) for v in vols]


@pytest.mark.parametrize("src_dtype", ["int16", "fp32"])
def test_eval_center_is_the_plain_window_bit_for_bit(src_dtype):
    from xvit.augment import VolumeAugment
    vols = volumes()
    src = on_gpu(vols) if src_dtype == "int16" else on_gpu(vols).float()
    aug = VolumeAugment(D, pad_value=PAD, crop_foreground="center", crop_margin=1, seed=1).eval()
    plain = VolumeAugment(D, pad_value=PAD, seed=1).eval()
    out = aug(src)
    plain(src)
    after, crop = check_crop("eval center", aug, plain, vols, "center", (1, 1, 1))
    assert bool(aug.last_params.exact.all()) and bool((aug.last_params.crop_scale == 1).all()) and aug.call_index == 0
    window = X.window_ref(vols, crop, M, D, PAD)
    assert np.array_equal(as64(out), K.round_to(window, "bf16")), "the exact path copies the window"
    assert not np.array_equal(as64(out), as64(plain(src))), "the brain is not where the centre window is"
    full = vols.astype(np.int32) + 1                        # every voxel is foreground: the box is the volume, the crop is the draw's own window
    src_full = on_gpu(full.astype(np.int16)) if src_dtype == "int16" else on_gpu(full.astype(np.int16)).float()
    out_full, out_none = aug(src_full), plain(src_full)
    assert aug.last_crop.lo.tolist() == [[0, 0, 0]] * B and aug.last_crop.hi.tolist() == [[n - 1 for n in S]] * B
    assert torch.equal(bits(out_full), bits(out_none)) and torch.equal(bits(aug.last_params.table[..., :31]), bits(plain.last_params.table[..., :31]))


def test_fit_with_elastic_deformation_on_the_folded_table():
    from xvit.augment import VolumeAugment
    vols = volumes(1)
    src = on_gpu(vols)
    kw = dict(pad_value=PAD, seed=7, elastic_prob=1.0, elastic_control_points=5, elastic_max_displacement=1.5, **QUIET)
    aug = VolumeAugment(D, crop_foreground="fit", crop_upscale=True, **kw)
    plain = VolumeAugment(D, **kw)
    out = aug(src)
    plain(src)
    after, crop = check_crop("fit elastic", aug, plain, vols, "fit", up=True)
    el = aug.last_elastic
    assert el is not None and torch.equal(bits(el.field), bits(plain.last_elastic.field)), "the crop does not touch the field"
    want, R, exact, deformed, cell = E.apply_ref(vols, after, el.field.cpu().numpy(), el.record.cpu().numpy(), M, D, PAD)
    assert deformed.all() and not exact.any()
    E.check("fit elastic", as64(out), want, R, exact, deformed, cell, after, "bf16")
    assert torch.equal(bits(aug.apply(src, aug.last_params, elastic=el)), bits(out))


def test_zscore_and_crop_write_disjoint_slots_and_both_folds_are_present():
    from xvit.augment import VolumeAugment
    vols = volumes()
    src = on_gpu(vols)
    kw = dict(pad_value=PAD, seed=9, intensity_scale=0.5)
    both = VolumeAugment(D, normalize="zscore", crop_foreground="fit", **kw)
    crop_only = VolumeAugment(D, crop_foreground="fit", **kw)
    norm_only = VolumeAugment(D, normalize="zscore", **kw)
    plain = VolumeAugment(D, **kw)
    for mode in ("train", "eval"):
        for st in (both, crop_only, norm_only, plain):
            getattr(st, mode)()
        out = both(src)
        crop_only(src), norm_only(src), plain(src)
        t, c, n, p = (table_of(st.last_params).view(np.uint32) for st in (both, crop_only, norm_only, plain))
        spatial, intensity = list(range(12)) + [31], [12, 13, 29, 30]
        assert np.array_equal(t[:, spatial], c[:, spatial]) and not np.array_equal(c[:, spatial], p[:, spatial])
        assert np.array_equal(t[:, intensity], n[:, intensity]) and not np.array_equal(n[:, intensity], p[:, intensity])
        rest = [s for s in range(32) if s not in spatial + intensity + [K.FLAGS]]
        assert np.array_equal(t[:, rest], p[:, rest])
        flags = lambda st: table_of(st.last_params)[:, K.FLAGS].astype(np.int64)     # noqa: E731
        assert np.array_equal(flags(both), (flags(crop_only) & 1) | (flags(norm_only) & 2)) and (flags(both) & 2).all()
        assert torch.equal(both.last_crop.crop, crop_only.last_crop.crop) and torch.equal(both.last_stats.table, norm_only.last_stats.table)
        after = table_of(both.last_params)
        want, R, exact = NC.apply_ref(vols, after, D, PAD)                           # the clamp window in front of a v + b
        K.check(f"zscore + fit, {mode}", as64(out), want, R, exact, after, "bf16")


def test_the_default_has_no_crop():
    from xvit.augment import VolumeAugment
    src = on_gpu(volumes())
    a, b = VolumeAugment(D, seed=3), VolumeAugment(D, seed=3, crop_foreground=None, crop_margin=5, crop_upscale=True, crop_above=100.0)
    for mode in ("train", "eval"):
        getattr(a, mode)(), getattr(b, mode)()
        oa, ob = a(src), b(src)
        assert torch.equal(bits(oa), bits(ob)) and torch.equal(bits(a.last_params.table), bits(b.last_params.table))
        assert b.last_crop is None and not bool(b.last_params.crop_scale.any()) and not b._crops


def test_a_sample_without_foreground_keeps_the_volume_window():
    from xvit.augment import VolumeAugment
    vols = volumes().copy()
    vols[2:] = 0                                            # sample 1 has no foreground
    src = on_gpu(vols)
    aug = VolumeAugment(D, pad_value=PAD, crop_foreground="fit", seed=2).eval()
    plain = VolumeAugment(D, pad_value=PAD, seed=2).eval()
    out, ref = aug(src), plain(src)
    check_crop("empty sample", aug, plain, vols, "fit")
    assert aug.last_crop.nonempty.tolist() == [1, 0] and aug.last_params.crop_scale[1].tolist() == [0.0, 0.0]
    assert torch.equal(bits(out[1]), bits(ref[1])) and not torch.equal(bits(out[0]), bits(ref[0]))


def test_a_captured_stage_crops_to_the_box_of_the_data_it_is_replayed_on():
    from xvit.augment import VolumeAugment
    kw = dict(pad_value=PAD, seed=11)
    static = on_gpu(volumes(0)).clone()
    aug = VolumeAugment(D, crop_foreground="fit", crop_margin=1, capturable=True, **kw)
    plain = VolumeAugment(D, **kw)
    aug(static)                                             # allocates the table, the counter, the box tables and the workspace; call index 0 -> 1
    plain(static)
    tables = aug._crops[(B, M, static.device)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = aug(static)
    assert aug.call_index == 1, "a capture executes nothing"
    seen = []
    for replay in range(3):
        vols = volumes(replay + 1)
        static.copy_(on_gpu(vols))                          # new data in the captured input
        g.replay()
        torch.cuda.synchronize()
        plain(static)
        after, crop = check_crop(f"replay {replay}", aug, plain, vols, "fit", (1, 1, 1))
        assert aug.last_crop.boxes is tables[0] and aug.last_crop.crop is tables[1]
        assert torch.equal(bits(aug.apply(static, aug.last_params)), bits(out))
        seen.append(crop.copy())
    assert aug.call_index == 4
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
