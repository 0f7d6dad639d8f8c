"""GPU: VolumeAugment with elastic deformation (xvit/augment.py) against its own kernels and against the stage without it.

Shapes: sources (20, 20, 20) -> (16, 16, 24) and, for the capture, the same; B = 3, M = 2; 5 control points per axis (half a control cell is
3.75, 3.75 and 5.75 voxels there) with max_displacement 2."""
import functools

import numpy as np
import pytest
import torch

import _elastic_check as K
from _util import dev

pytestmark = pytest.mark.gpu

S, D = (20, 20, 20), (16, 16, 24)
B, M = 3, 2
EL = dict(elastic_prob=1.0, elastic_control_points=5, elastic_max_displacement=2.0)
INTENSITY_OFF = dict(scale_intensity_prob=0, shift_intensity_prob=0, noise_prob=0)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@functools.lru_cache(maxsize=None)
def source_cpu():
    g = torch.Generator().manual_seed(3)
    return torch.randint(0, 3001, (B, M) + S, generator=g).to(torch.int16)


def source():
    return source_cpu().to(dev())


def test_elastic_stage_equals_its_kernels_bit_for_bit():
    from xvit import _lib, ops
    from xvit.augment import VolumeAugment
    src = source()
    aug = VolumeAugment(D, seed=5, **EL)
    for call in range(2):
        out = aug(src)
        el, params = aug.last_elastic, aug.last_params
        assert el.field.shape == (B, 3, 5, 5, 5) and el.record.shape == (B, 8) and bool((el.active == 1).all())
        assert bool((el.max_abs <= 2.0).all()) and bool((el.max_abs > 0).all())
        # the kernels, called by hand on the call's seed
        seed = (5 + call * K.COUNTER_STRIDE) & ((1 << 64) - 1)
        field, erec = torch.empty_like(el.field), torch.empty_like(el.record)
        ops.elastic_draw(aug.elastic_config, field, erec, seed)
        table = torch.empty(B, M, _lib.AUG_NPARAM, device=dev())
        ops.augment_draw(aug.config, table, S, D, seed)
        assert torch.equal(bits(field), bits(el.field)) and torch.equal(bits(erec), bits(el.record)) and torch.equal(bits(table), bits(params.table))
        want = ops.augment_apply_elastic(src, table, field, erec, D, aug.pad_value, torch.bfloat16)
        assert out.shape == (B, M, 1) + D and torch.equal(bits(out), bits(want))
        # ... and the field is the restated draw
        ref_field, ref_erec = K.field_ref(K.config(1.0, 2.0, 2), B, (5, 5, 5), seed=5, call=call)
        assert np.array_equal(el.field.cpu().numpy().view(np.uint32), ref_field.view(np.uint32))
        assert np.array_equal(el.record.cpu().numpy().view(np.uint32), ref_erec.view(np.uint32))
    assert aug.call_index == 2


def test_elastic_prob_0_is_the_stage_without_the_arguments():
    from xvit.augment import VolumeAugment
    src = source()
    a, b = VolumeAugment(D, seed=9), VolumeAugment(D, seed=9, elastic_prob=0.0, elastic_control_points=6, elastic_max_displacement=1.0)
    for _ in range(2):
        oa, ob = a(src), b(src)
        assert torch.equal(bits(oa), bits(ob)) and torch.equal(bits(a.last_params.table), bits(b.last_params.table))
        assert a.last_elastic is None and b.last_elastic is None


def test_same_seed_same_output_and_successive_calls_differ():
    from xvit.augment import VolumeAugment
    src = source()
    a, b = VolumeAugment(D, seed=4, **EL), VolumeAugment(D, seed=4, **EL)
    oa0, fa0 = a(src), a.last_elastic.field.clone()
    ob0 = b(src)
    assert torch.equal(bits(oa0), bits(ob0)) and torch.equal(bits(fa0), bits(b.last_elastic.field))
    oa1 = a(src)
    assert not torch.equal(bits(fa0), bits(a.last_elastic.field)) and not torch.equal(bits(oa0), bits(oa1))
    assert not torch.equal(bits(VolumeAugment(D, seed=5, **EL)(src)), bits(oa0))


def test_both_modalities_of_a_sample_see_one_field():
    from xvit.augment import VolumeAugment
    one = source()[:, :1]
    src = torch.cat([one, one], dim=1).contiguous()
    aug = VolumeAugment(D, seed=2, **EL, **INTENSITY_OFF)
    out = aug(src)
    assert torch.equal(bits(out[:, 0]), bits(out[:, 1]))
    plain = aug.apply(src, aug.last_params)
    assert not torch.equal(bits(out), bits(plain))                   # ... and it is deformed


def test_eval_is_undeformed():
    from xvit.augment import VolumeAugment
    src = source()
    aug = VolumeAugment(D, seed=2, **EL).eval()
    out = aug(src)
    assert aug.last_elastic is None and aug.call_index == 0 and bool(aug.last_params.exact.all())
    assert torch.equal(bits(out), bits(VolumeAugment(D, seed=2).eval()(src)))


def test_zscore_normalisation_composes():
    from xvit import ops
    from xvit.augment import VolumeAugment
    src = source()
    aug = VolumeAugment(D, seed=6, normalize="zscore", **EL)
    out = aug(src)
    assert aug.last_stats is not None and bool(aug.last_params.clamped.all()) and bool(torch.isfinite(out.float()).all())
    want = ops.augment_apply_elastic(src, aug.last_params.table, aug.last_elastic.field, aug.last_elastic.record, D, aug.pad_value, torch.bfloat16)
    assert torch.equal(bits(out), bits(want))
    # the table is the one the stage without elastic folds the statistics into: the deformation leaves draw and statistics alone
    ref = VolumeAugment(D, seed=6, normalize="zscore")
    ref(src)
    assert torch.equal(bits(ref.last_params.table), bits(aug.last_params.table))


def test_apply_replays_a_call_exactly():
    from xvit.augment import ElasticField, VolumeAugment
    src = source()
    aug = VolumeAugment(D, seed=8, elastic_prob=0.5, elastic_control_points=5, elastic_max_displacement=2.0)
    out = aug(src)
    params, el = aug.last_params.clone(), aug.last_elastic.clone()
    aug(src)                                                         # another call in between
    assert torch.equal(bits(aug.apply(src, params, elastic=el)), bits(out))
    zero = ElasticField.zeros(B, 5, dev())
    assert torch.equal(bits(aug.apply(src, params, elastic=zero)), bits(aug.apply(src, params)))
    with pytest.raises(TypeError, match="ElasticField"):
        aug.apply(src, params, elastic=el.field)
    with pytest.raises(ValueError, match="samples"):
        aug.apply(src, params, elastic=ElasticField.zeros(B + 1, 5, dev()))


def test_capturable_stage_draws_a_new_field_at_every_replay():
    from xvit.augment import ElasticField, VolumeAugment
    static = source()
    aug = VolumeAugment(D, seed=11, capturable=True, **EL)
    aug(static)                                                      # allocates the table, the counter and the field; call index 0 -> 1
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = aug(static)
    assert aug.call_index == 1, "a capture executes nothing"
    fields = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        params, el = aug.last_params.clone(), aug.last_elastic.clone()
        assert torch.equal(bits(aug.apply(static, params, elastic=el)), bits(out))      # an eager apply of the replay's own tables
        fields.append(el)
    assert not torch.equal(bits(fields[0].field), bits(fields[1].field)) and aug.call_index == 3
    # the replays drew what a plain stage draws at call indices 1 and 2
    plain = VolumeAugment(D, seed=11, **EL)
    plain(static)
    for want in fields:
        plain(static)
        assert torch.equal(bits(plain.last_elastic.field), bits(want.field)) and torch.equal(bits(plain.last_elastic.record), bits(want.record))
    assert isinstance(aug.last_elastic, ElasticField)
