"""GPU: VolumeAugment(crop_foreground=..., crop_component=...) (xvit/augment.py) on the speck volume of tests/test_crop_model_gpu.py: a
brain plus one isolated bright voxel.  With crop_component="largest" the crop, the table and the eval() output equal, bit for bit, those of
the same volume with the speck zeroed and no component filter; with None the box still follows the speck.  The stage equals its kernels
and the NumPy restatement of tests/_cc_check.py; z-score and elastic deformation on top; capturable inside torch.cuda.graph with the data
changed between replays; GraphedStep with the stage inside the graph.

Shapes: B = 2, M = 2 volumes of (40, 36, 27) int16, img_size (16, 16, 16)."""
import functools

import numpy as np
import pytest
import torch

import _augment_check as K
import _cc_check as CC
import _crop_check as X
from _util import dev

pytestmark = pytest.mark.gpu

S, D = (40, 36, 27), (16, 16, 16)
B, M = 2, 2
PAD = -1.0
SPECK = (1, 3, 30, 2)                                       # (volume, z, y, x) of the isolated voxel for seed 0; z moves with the seed


@functools.lru_cache(maxsize=None)
def volumes(seed=0, speck=True):
    """Computed once and shared: leave it as it is.  The volumes of tests/test_crop_model_gpu.py; speck=False: the speck zeroed."""
    rng = np.random.default_rng(100 + seed)
    v = X.brain(rng, B * M, S, (24 - 3 * seed, 13 + 2 * seed, 15), (9.5, 8.2 + seed, 7.4), dtype=np.int16)
    assert v[1, 3 + seed, 30, 2] == 0
    v[1, 3 + seed, 30, 2] = 3000 if speck else 0
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def reference(seed, conn=6):
    """(labels, comps, boxes) of volumes(seed), the largest component kept."""
    return CC.reference(CC.foreground(volumes(seed), 0.0), conn)


def on_gpu(vols):
    return torch.from_numpy(np.array(vols)).to(dev()).reshape((B, M) + tuple(vols.shape[1:]))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check_against_restatement(name, fb, seed, margin, conn=6):
    labels, comps, boxes = reference(seed, conn)
    np.testing.assert_array_equal(fb.components.labels.cpu().numpy().reshape(labels.shape), labels, err_msg=f"{name}: labels")
    np.testing.assert_array_equal(fb.components.table.cpu().numpy().reshape(comps.shape), comps, err_msg=f"{name}: comps")
    np.testing.assert_array_equal(fb.boxes.cpu().numpy().reshape(boxes.shape), boxes, err_msg=f"{name}: boxes")
    np.testing.assert_array_equal(fb.crop.cpu().numpy(), X.crop_ref(boxes, M, margin, S), err_msg=f"{name}: crop")
    assert comps[1].tolist()[:5] == [2, comps[1, 1], int((volumes(seed)[1] > 0).sum()) - 1, 1, int((volumes(seed)[1] > 0).sum()) - 1], "a brain and a speck"
    assert fb.components.status.tolist() == [[0] * M] * B


@pytest.mark.parametrize("mode", ["center", "fit"])
def test_the_largest_component_crops_as_if_the_speck_were_zeroed(mode):
    from xvit.augment import VolumeAugment
    src, clean = on_gpu(volumes()), on_gpu(volumes(0, False))
    kw = dict(pad_value=PAD, crop_foreground=mode, crop_margin=(1, 0, 2), seed=4)
    filt, plain = VolumeAugment(D, crop_component="largest", **kw), VolumeAugment(D, **kw)
    for how in ("eval", "train", "eval"):
        getattr(filt, how)(), getattr(plain, how)()
        out, want = filt(src), plain(clean)
        assert torch.equal(filt.last_crop.boxes, plain.last_crop.boxes) and torch.equal(filt.last_crop.crop, plain.last_crop.crop), how
        assert torch.equal(bits(filt.last_params.table), bits(plain.last_params.table)), f"{how}: the folded tables differ"
        if how == "eval":
            assert torch.equal(bits(out), bits(want)), "the speck lies outside the window: the eval() outputs are the same bits"
        else:                                               # it masks nothing: the same table applied to the volume that still has its speck
            assert torch.equal(bits(out), bits(filt.apply(src, plain.last_params)))
        assert plain.last_crop.components is None
        check_against_restatement(f"{mode} {how}", filt.last_crop, 0, (1, 0, 2))
        followed = plain(src)                               # without the filter the box follows the speck
        crop = plain.last_crop.crop.cpu().numpy()
        assert crop[0, 3] == SPECK[2] and crop[0, 4] == 0 and not torch.equal(plain.last_crop.crop, filt.last_crop.crop)
        assert how != "eval" or not torch.equal(bits(followed), bits(out))
        if how == "train":
            filt(src)                                       # plain was called twice in training mode: keep the call indices in step
    assert filt.call_index == plain.call_index == 2


@pytest.mark.parametrize("conn", [6, 26])
def test_the_stage_equals_its_kernels(conn):
    from xvit import _lib, ops
    from xvit.augment import VolumeAugment, foreground_boxes, foreground_components
    src = on_gpu(volumes())
    aug = VolumeAugment(D, pad_value=PAD, crop_foreground="fit", crop_margin=1, crop_component=5, crop_connectivity=conn, seed=5)
    plain = VolumeAugment(D, pad_value=PAD, seed=5)
    for call in range(2):
        out = aug(src)
        plain(src)
        table = torch.empty(B, M, _lib.AUG_NPARAM, device=dev())
        ops.augment_draw(aug.config, table, S, D, (5 + call * K.COUNTER_STRIDE) & ((1 << 64) - 1))
        assert torch.equal(bits(table), bits(plain.last_params.table))
        boxes, cr = torch.empty(B, M, 8, dtype=torch.int32, device=dev()), torch.empty(B, 8, dtype=torch.int32, device=dev())
        labels, comps = torch.empty(src.shape, dtype=torch.int32, device=dev()), torch.empty(B, M, 8, dtype=torch.int32, device=dev())
        ops.volume_bbox_components(src, aug.crop_config, aug.component_config, D, boxes, cr, labels, comps,
                                   ops.volume_components_workspace(B * M, int(np.prod(S)), dev()), table)
        fb = aug.last_crop
        assert torch.equal(bits(table), bits(aug.last_params.table)) and torch.equal(boxes, fb.boxes) and torch.equal(cr, fb.crop)
        assert torch.equal(labels, fb.components.labels) and torch.equal(comps, fb.components.table)
        assert torch.equal(bits(aug.apply(src, table)), bits(out)) and out.shape == (B, M, 1) + D
    labels, _, _ = reference(0, conn)
    want_comps, want_boxes = CC.tables_ref(labels, CC.MIN_VOXELS, 5)
    np.testing.assert_array_equal(fb.components.table.cpu().numpy().reshape(want_comps.shape), want_comps)
    np.testing.assert_array_equal(fb.boxes.cpu().numpy().reshape(want_boxes.shape), want_boxes)
    alone = foreground_boxes(src, margin=1, component=5, connectivity=conn)
    assert torch.equal(alone.boxes, fb.boxes) and torch.equal(alone.crop, fb.crop) and torch.equal(alone.components.table, fb.components.table)
    comps_alone = foreground_components(src, connectivity=conn)
    assert torch.equal(comps_alone.labels, fb.components.labels)
    assert comps_alone.count.tolist() == fb.components.count.tolist() and comps_alone.largest_size.tolist() == fb.components.largest_size.tolist()
    assert comps_alone.kept_voxels.tolist() == comps_alone.largest_size.tolist()
    assert foreground_boxes(src, margin=1).components is None


def test_zscore_on_top_keeps_the_statistics_of_the_whole_volume():
    from xvit.augment import VolumeAugment
    src, clean = on_gpu(volumes()), on_gpu(volumes(0, False))
    kw = dict(pad_value=PAD, seed=9, intensity_scale=0.5, normalize="zscore")
    both = VolumeAugment(D, crop_foreground="fit", crop_component="largest", **kw)
    crop_clean = VolumeAugment(D, crop_foreground="fit", **kw)
    norm_only = VolumeAugment(D, **kw)
    for how in ("train", "eval"):
        for st in (both, crop_clean, norm_only):
            getattr(st, how)()
        out = both(src)
        crop_clean(clean), norm_only(src)
        t, c, n = (st.last_params.table.cpu().numpy().reshape(B * M, 32).view(np.uint32) for st in (both, crop_clean, norm_only))
        spatial, intensity = list(range(12)) + [31], [12, 13, 29, 30]
        assert np.array_equal(t[:, spatial], c[:, spatial]), "the window is that of the volume without its speck"
        assert np.array_equal(t[:, intensity], n[:, intensity]), "the statistics are those of the volume with its speck: nothing is masked"
        assert not torch.equal(crop_clean.last_stats.table, norm_only.last_stats.table), "the speck counts among the foreground voxels"
        assert torch.equal(both.last_stats.table, norm_only.last_stats.table) and torch.equal(both.last_crop.crop, crop_clean.last_crop.crop)
        assert torch.equal(bits(out), bits(both.apply(src, both.last_params)))


def test_elastic_on_top():
    from xvit.augment import VolumeAugment
    src, clean = on_gpu(volumes(1)), on_gpu(volumes(1, False))
    kw = dict(pad_value=PAD, seed=7, elastic_prob=1.0, elastic_control_points=5, elastic_max_displacement=1.5, crop_foreground="fit", crop_upscale=True)
    filt, plain = VolumeAugment(D, crop_component="largest", crop_connectivity=26, **kw), VolumeAugment(D, **kw)
    out, want = filt(src), plain(clean)
    assert torch.equal(bits(filt.last_elastic.field), bits(plain.last_elastic.field)), "the filter does not touch the field"
    assert torch.equal(bits(filt.last_params.table), bits(plain.last_params.table)) and torch.equal(filt.last_crop.crop, plain.last_crop.crop)
    assert torch.equal(bits(out), bits(filt.apply(src, filt.last_params, elastic=filt.last_elastic)))
    check_against_restatement("elastic", filt.last_crop, 1, (0, 0, 0), 26)
    assert bool((filt.last_params.crop_scale != 0).all())


def test_a_captured_stage_filters_the_data_it_is_replayed_on():
    from xvit.augment import VolumeAugment
    kw = dict(pad_value=PAD, seed=11, crop_foreground="fit", crop_margin=1)
    static = on_gpu(volumes(0)).clone()
    aug = VolumeAugment(D, crop_component="largest", capturable=True, **kw)
    plain = VolumeAugment(D, **kw)
    aug(static)                                             # allocates the tables, the labels and the workspaces; call index 0 -> 1
    plain(static)
    held = aug._components[(tuple(static.shape), static.device)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = aug(static)
    assert aug.call_index == 1, "a capture executes nothing"
    seen = []
    for replay in range(3):
        static.copy_(on_gpu(volumes(replay + 1)))           # new data in the captured input
        g.replay()
        torch.cuda.synchronize()
        plain(on_gpu(volumes(replay + 1, False)))
        check_against_restatement(f"replay {replay}", aug.last_crop, replay + 1, (1, 1, 1))
        assert aug.last_crop.components.labels is held[0] and aug.last_crop.components.table is held[1]
        assert torch.equal(aug.last_crop.crop, plain.last_crop.crop) and torch.equal(bits(aug.last_params.table), bits(plain.last_params.table))
        assert torch.equal(bits(aug.apply(static, aug.last_params)), bits(out))
        seen.append(aug.last_crop.crop.cpu().numpy().copy())
    assert aug.call_index == 4
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


def test_graphed_step_with_the_stage_inside_the_graph():
    import ref_cpu as Rf
    import xvit
    from xvit.graph import GraphedStep
    cfg = Rf.make_config("tiny")
    d = tuple(cfg.img_size)
    assert cfg.num_modalities == M
    raw = on_gpu(volumes(0)).clone()
    aug = xvit.VolumeAugment(d, intensity_scale=1 / 1000, seed=1, capturable=True, crop_foreground="center", crop_component="largest")
    y = torch.tensor([0, 1], device=dev())
    example = aug(raw)
    model = xvit.ModelCross(cfg).to(dev())
    model.load_state_dict(Rf.make_state_dict(cfg, seed=0))
    model.train()
    step = GraphedStep(model, example, y, source=lambda: (aug(raw), y))
    for k in (0, 1, 2):
        raw.copy_(on_gpu(volumes(k)))
        logits, loss = step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(logits).all())
        check_against_restatement(f"step {k}", aug.last_crop, k, (0, 0, 0))
        assert torch.equal(bits(step.img), bits(aug.apply(raw, aug.last_params)))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
