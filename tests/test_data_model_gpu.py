"""GPU: xvit.data at the oracle's tiny config.  The store round-trips host and device tensors; a sampler call is the predicted cases; two
samplers with one seed agree and another seed differs; a resumed sampler continues the stream; a captured sampler call draws anew at
every replay; and GraphedStep(source=...) trains, replay after replay, on exactly the batch the restatement predicts."""
import numpy as np
import pytest
import torch

import _data_check as D
import ref_cpu as R
from _util import dev

pytestmark = pytest.mark.gpu

CFG = R.make_config("tiny")
CASE = (CFG.num_modalities, CFG.img_size[0] + 2, CFG.img_size[1] - 2, CFG.img_size[2] + 1)    # crop, pad, crop: 12 240 bytes per case
N, B = 11, 4
LABELS = [0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0]
WEIGHTS = [1, 2, 0, 1, 3, 1, 1, 0, 2, 1, 1]


def cases(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N,) + CASE, generator=g).to(torch.int16)           # exact in bf16


@pytest.fixture(scope="module")
def filled():
    """(store, host volumes): seven cases from the host, four from the device, one of them through add()."""
    from xvit.data import VolumeStore
    vols = cases()
    store = VolumeStore(CASE, capacity=N + 2, device=dev())
    base = store.volumes.data_ptr()
    store.extend(vols[:6], LABELS[:6], WEIGHTS[:6])
    store.add(vols[6], LABELS[6], WEIGHTS[6])
    store.extend(vols[7:10].to(dev()), torch.tensor(LABELS[7:10], device=dev()), WEIGHTS[7:10])
    store.add(vols[10].to(dev()), LABELS[10], WEIGHTS[10])
    assert len(store) == N and store.volumes.data_ptr() == base
    return store, vols


def predicted(sampler, call, vols):
    cdf = D.make_cdf(WEIGHTS) if sampler.mode == "weighted" else None
    idx = D.draw_ref(sampler.mode, N, sampler.batch_size, sampler.seed, sampler.rank, sampler.world_size, call, cdf)
    return idx, vols[torch.from_numpy(idx.astype(np.int64))], torch.tensor(LABELS)[torch.from_numpy(idx.astype(np.int64))]


def check_call(sampler, raw, y, call, vols):
    idx, ref_raw, ref_y = predicted(sampler, call, vols)
    assert np.array_equal(sampler.last_indices.cpu().numpy(), idx), (call, sampler.last_indices.tolist(), idx.tolist())
    assert torch.equal(raw.cpu(), ref_raw) and torch.equal(y.cpu(), ref_y) and not bool(sampler.last_status.any())
    return idx


def test_store_round_trips_host_and_device_tensors(filled):
    store, vols = filled
    assert torch.equal(store.volumes[:N].cpu(), vols) and not bool(store.volumes[N:].any())
    assert store.labels[:N].tolist() == LABELS and store.labels_dev[:N].cpu().tolist() == LABELS and store.weights[:N].tolist() == [float(w) for w in WEIGHTS]
    raw, y = store.gather([3, 3, 10, 0])                               # a host index vector: validated, then gathered on the device
    assert raw.shape == (4,) + CASE and raw.dtype == torch.int16 and torch.equal(raw.cpu(), vols[[3, 3, 10, 0]]) and y.cpu().tolist() == [0, 0, 0, 0]
    status = torch.full((3,), 7, dtype=torch.int32, device=dev())
    raw, y = store.gather(torch.tensor([1, N, 4], dtype=torch.int32, device=dev()), status=status)     # a device vector is not read here
    assert torch.equal(raw[0].cpu(), vols[1]) and not bool(raw[1].any()) and torch.equal(raw[2].cpu(), vols[4])
    assert y.cpu().tolist() == [1, -1, 1] and status.cpu().tolist() == [0, 1, 0]
    with pytest.raises(IndexError):
        store.gather([0, N])


@pytest.mark.parametrize("mode", ["weighted", "shuffle", "sequential"])
def test_a_sampler_call_is_the_predicted_cases(filled, mode):
    from xvit.data import BatchSampler
    store, vols = filled
    s = BatchSampler(store, B, mode=mode, seed=5, rank=1, world_size=2)
    seen = []
    for call in range(4):
        raw, y = s()
        seen += check_call(s, raw, y, call, vols).tolist()
    assert s.call_index == 4
    if mode == "weighted":
        assert 2 not in seen and 7 not in seen                         # weight 0


def test_samplers_agree_by_seed_and_resume_through_their_state(filled):
    from xvit.data import BatchSampler
    store, vols = filled
    a, b, c = (BatchSampler(store, B, mode="weighted", seed=s) for s in (3, 3, 4))
    batches = [(a(), b(), c()) for _ in range(3)]
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y, _ in batches)
    assert any(not torch.equal(x[0], z[0]) for x, _, z in batches)
    state = a.state_dict()
    nxt = [a() for _ in range(2)]
    for capturable in (False, True):
        r = BatchSampler(store, B, mode="weighted", seed=3, capturable=capturable)
        if capturable:
            r()                                                        # the counter exists: the load must reach it
        r.load_state_dict(state)
        assert r.call_index == 3
        for raw, y in nxt:
            got = r()
            assert torch.equal(got[0], raw) and torch.equal(got[1], y)
        assert r.call_index == 5 and r.state_dict()["call_index"] == 5


def test_a_captured_sampler_draws_anew_at_every_replay(filled):
    from xvit.data import BatchSampler
    store, vols = filled
    s = BatchSampler(store, B, mode="shuffle", seed=11, capturable=True)
    raw0, y0 = s()                                                     # allocates the buffers and the counter; call index 0 -> 1
    check_call(s, raw0, y0, 0, vols)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        raw, y = s()
    assert s.call_index == 1, "a capture executes nothing"
    assert raw.data_ptr() == raw0.data_ptr()                           # static buffers
    batches = []
    for k in (1, 2, 3):
        g.replay()
        torch.cuda.synchronize()
        batches.append(check_call(s, raw, y, k, vols).tolist())
    assert batches[0] != batches[1] != batches[2] and s.call_index == 4
    assert sorted((batches[0] + batches[1] + batches[2])[:N - B]) == sorted(set(range(N)) - set(D.draw_ref("shuffle", N, B, 11).tolist()))   # one epoch: no repeats


def pad_crop_ref(raw, img_size, pad_value=-1.0):
    """The centre pad / crop of int16 [B, M, Ds, Hs, Ws] -> bf16 [B, M, 1, D, H, W] in torch."""
    from xvit.augment import pad_crop_offset
    out = torch.full(tuple(raw.shape[:2]) + (1,) + tuple(img_size), pad_value, dtype=torch.float32)
    src, dst = [], []
    for size, target in zip(raw.shape[2:], img_size):
        off = pad_crop_offset(size, target)
        lo = max(0, -off)
        hi = min(target, size - off)
        dst.append(slice(lo, hi))
        src.append(slice(lo + off, hi + off))
    out[(slice(None), slice(None), 0) + tuple(dst)] = raw[(slice(None), slice(None)) + tuple(src)].float()
    return out.to(torch.bfloat16)


def test_graphed_step_trains_on_the_batches_its_source_draws(filled):
    import xvit
    from xvit.data import BatchSampler
    from xvit.graph import GraphedStep
    store, vols = filled
    size = tuple(CFG.img_size)
    sampler = BatchSampler(store, B, mode="weighted", seed=2, capturable=True)
    aug = xvit.VolumeAugment(size, seed=2, capturable=True).eval()
    img0 = aug(sampler()[0])                                           # both stages allocate their static buffers here
    y0 = torch.zeros(B, dtype=torch.int64, device=dev())
    sd = R.make_state_dict(CFG, seed=0)
    model, twin = xvit.ModelCross(CFG).to(dev()), xvit.ModelCross(CFG).to(dev())
    for m in (model, twin):
        m.load_state_dict(sd)
        m.train()
    source = lambda: (lambda r, y: (aug(r), y))(*sampler())            # noqa: E731
    step = GraphedStep(model, img0, y0, source=source)
    first = sampler.call_index
    assert first == 1 + 3, "the warm-up advances the source's call index; the capture executes nothing"
    with pytest.raises(RuntimeError, match="source"):
        step(img=img0)
    with pytest.raises(RuntimeError, match="source"):
        step(labels=y0)
    assert sampler.call_index == first
    seen = []
    for k in range(3):
        logits, loss = step()
        torch.cuda.synchronize()
        idx, ref_raw, ref_y = predicted(sampler, first + k, vols)
        assert np.array_equal(sampler.last_indices.cpu().numpy(), idx)
        assert torch.equal(step.labels.cpu(), ref_y)
        ref_img = pad_crop_ref(ref_raw, size)
        assert step.img.shape == ref_img.shape and torch.equal(step.img.cpu().view(torch.int16), ref_img.view(torch.int16))
        e_logits, e_loss = twin(ref_img.to(dev()), ref_y.to(dev()))
        assert torch.equal(logits, e_logits.detach()) and torch.equal(loss, e_loss.detach())     # the gate of tests/test_graph_gpu.py
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
        seen.append((idx.tolist(), logits.clone()))
    assert sampler.call_index == first + 3
    assert seen[0][0] != seen[1][0] != seen[2][0] and not torch.equal(seen[0][1], seen[1][1]) and not torch.equal(seen[1][1], seen[2][1])
