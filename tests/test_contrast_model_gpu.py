"""GPU: xvit.augment.ContrastAugment behind VolumeAugment: the stage is its two kernels with the recorded tables and nothing else,
reproducible from its seed, a new table at every call, silent in eval(), capturable with a fresh draw at every replay, and its output
trains ModelCross under GraphedStep."""
import numpy as np
import pytest
import torch

import _contrast_check as K
from _util import dev

pytestmark = pytest.mark.gpu

S, D = (20, 20, 20), (16, 16, 24)
ON = dict(blur_prob=.6, bias_prob=.6, gamma_prob=.6)


def raw_volumes(B=2, M=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1001, (B, M) + S, generator=g).to(torch.int16).to(dev())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def table_of(con):
    return con.last_params.table.cpu().numpy().reshape(-1, K.NPARAM).copy()


def test_stage_is_its_two_kernels_with_the_recorded_tables():
    from xvit.augment import ContrastAugment, ContrastParams, VolumeAugment
    raw = raw_volumes()
    aug = VolumeAugment(D, intensity_scale=1 / 1000, seed=4)
    con = ContrastAugment(seed=4, **ON)
    img = con(aug(raw))
    assert img.shape == (2, 2, 1) + D and img.dtype == torch.bfloat16 and img.is_contiguous() and isinstance(con.last_params, ContrastParams)
    p1, p2 = aug.last_params.clone(), con.last_params.clone()
    mid = aug.apply(raw, p1)
    again = con.apply(mid, p2)
    assert again.data_ptr() != mid.data_ptr() and torch.equal(bits(again), bits(img))
    assert torch.equal(bits(con.apply(mid, p2.table)), bits(img))                               # a bare table is accepted too
    assert torch.equal(bits(torch.nn.Sequential(VolumeAugment(D, intensity_scale=1 / 1000, seed=4), ContrastAugment(seed=4, **ON))(raw)), bits(img))
    # the table is the restated draw of call 0, and the output is inside the gate computed from that table (fp32 output of the bf16 input)
    tab = table_of(con)
    K.check_draw(tab, K.draw_ref(K.config(**ON), 4, 4, call=0))
    assert len(set(tab[:, K.FLAGS])) > 1, "this seed should mix records"
    out32 = con.apply(mid, p2, out_dtype=torch.float32)
    src = mid.float().cpu().numpy().reshape((4,) + D)
    K.check("stage", out32.cpu().double().numpy().reshape((4,) + D), src, tab)
    assert np.array_equal(K.rne_bf16(out32.cpu().numpy()).reshape(-1), bits(img).cpu().numpy().view(np.uint16).reshape(-1))
    # [B, M, D, H, W] in -> the same shape out; out_dtype
    five = con.apply(mid[:, :, 0], p2)
    assert five.shape == (2, 2) + D and torch.equal(bits(five), bits(img[:, :, 0]))
    assert ContrastAugment(out_dtype=torch.float32, **ON)(mid).dtype == torch.float32
    assert ContrastAugment(**ON)(mid.float()).dtype == torch.float32 and ContrastAugment(out_dtype=torch.bfloat16, **ON)(mid.float()).dtype == torch.bfloat16


def test_reproducible_from_seed_and_a_new_table_each_call():
    from xvit.augment import ContrastAugment
    img = torch.rand(2, 2, 1, *D, device=dev()).to(torch.bfloat16)
    a, b, c = ContrastAugment(seed=9, **ON), ContrastAugment(seed=9, **ON), ContrastAugment(seed=10, **ON)
    oa0, ta0 = a(img), table_of(a)
    oa1, ta1 = a(img), table_of(a)
    ob0, tb0 = b(img), table_of(b)
    assert np.array_equal(ta0.view(np.uint32), tb0.view(np.uint32)) and torch.equal(bits(oa0), bits(ob0))
    assert not np.array_equal(ta0, ta1) and not torch.equal(bits(oa0), bits(oa1))
    c(img)
    assert not np.array_equal(table_of(c), ta0)
    assert a.call_index == 2 and b.call_index == 1
    K.check_draw(ta1, K.draw_ref(K.config(**ON), 4, 9, call=1))
    # a capturable stage keeps its call index on the device and draws the same numbers
    d = ContrastAugment(seed=9, capturable=True, **ON)
    od0, td0 = d(img), table_of(d)
    od1, td1 = d(img), table_of(d)
    assert np.array_equal(td0.view(np.uint32), ta0.view(np.uint32)) and np.array_equal(td1.view(np.uint32), ta1.view(np.uint32))
    assert torch.equal(bits(od0), bits(oa0)) and torch.equal(bits(od1), bits(oa1)) and d.call_index == 2


def test_eval_launches_nothing():
    from xvit import ops
    from xvit.augment import ContrastAugment
    img = torch.rand(2, 2, 1, *D, device=dev()).to(torch.bfloat16)
    con = ContrastAugment(seed=1, blur_prob=1, bias_prob=1, gamma_prob=1).eval()
    ops.PROFILE, saved = [], ops.PROFILE
    try:
        out = con(img)
        launched = list(ops.PROFILE)
    finally:
        ops.PROFILE = saved
    assert out is img and launched == [] and con.call_index == 0 and con.last_params is None
    con.train()
    assert con(img) is not img and con.call_index == 1


def test_capturable_stage_draws_anew_at_every_replay():
    from xvit.augment import ContrastAugment
    img = torch.rand(2, 2, 1, *D, device=dev()).to(torch.bfloat16)
    con =ContrastAugment(seed=11, capturable=True, **ON)
    con(img)                                                   # allocates the table and the counter; call index 0 -> 1
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = con(img)
    assert con.call_index == 1, "a capture executes nothing"
    tables = []
    for k in (1, 2, 3):
        g.replay()
        torch.cuda.synchronize()
        tab = table_of(con)
        K.check_draw(tab, K.draw_ref(K.config(**ON), 4, 11, call=k))
        assert torch.equal(bits(out), bits(con.apply(img, torch.from_numpy(tab).reshape(2, 2, K.NPARAM).to(dev()))))
        tables.append(tab)
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[1], tables[2]) and not np.array_equal(tables[0], tables[2])
    assert con.call_index == 4


def test_graphed_step_trains_on_the_stage_output():
    import ref_cpu as Rf
    import xvit
    from xvit.graph import GraphedStep
    cfg = Rf.make_config("tiny")
    d = tuple(cfg.img_size)
    g = torch.Generator().manual_seed(2)
    raw = torch.randint(0, 1001, (4, cfg.num_modalities, d[0] + 4, d[1] - 2, d[2] + 1), generator=g).to(torch.int16).to(dev())
    aug = xvit.VolumeAugment(d, intensity_scale=1 / 1000, seed=1)
    con = xvit.ContrastAugment(seed=1, blur_prob=1, bias_prob=1, gamma_prob=1)
    img = con(aug(raw))
    assert img.shape == (4, cfg.num_modalities, 1) + d and bool(torch.isfinite(img.float()).all())
    model = xvit.ModelCross(cfg).to(dev())
    model.load_state_dict(Rf.make_state_dict(cfg, seed=0))
    model.train()
    y = torch.tensor([0, 1, 1, 0], device=dev())
    step = GraphedStep(model, img, y)
    logits, loss = step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(logits).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
