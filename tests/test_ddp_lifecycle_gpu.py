"""GPU: the gradient reducer (xvit/ddp.py) and the captured step (xvit/graph.py) over MORE than one step, on the real model.

One RCCL rank (AVG over one rank is the identity), ModelCross "tiny", batch 4, deterministic gradients: the setting of
tests/test_grad_comm_gpu.py.  The reference is always the same model run WITHOUT a reducer, never the reducer against itself, and
every comparison is torch.equal; for the bf16 wire the reference is rounded here by the stated rule: bf16(g) after a first step,
bf16(bf16(g1) + g2) after an accumulating one.  tests/test_ddp_lifecycle_cpu.py is the CPU twin of the bookkeeping.

* gradients kept and zeroed in place, and accumulated over two backward + finish() rounds: every parameter, sink on and off;
* the documented optimizer loop (FusedAdam + reducer + GRAD_SINK + zero_grad(set_to_none=False)) ends with the parameters of the
  red.zero_grad() loop and of the loop without a reducer, eager and capturable;
* eager steps after GraphedStep(reducer=...) with the same reducer reproduce the eager steps before it; no bucket keeps an event;
* a captured step refuses to replay once model.training differs from the mode it was captured in;
* >= 2 GPUs: one accumulation round over two RCCL ranks (tests/_ddp_accum_worker.py)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

import ref_cpu as R
from _util import dev, rt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIRES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture
def rccl1(monkeypatch):
    import torch.distributed as dist
    import xvit.functional as XF
    from xvit import ops
    monkeypatch.setattr(ops, "DETERMINISTIC", True)        # XVIT_DETERMINISTIC=1: every gradient bit-reproducible run to run
    monkeypatch.setattr(XF, "GRAD_SINK", None)             # whatever a test assigns is dropped again
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_free_port()))
    monkeypatch.delenv("XVIT_GRAD_COMM", raising=False)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev())
    try:
        yield
    finally:
        dist.destroy_process_group()


def _tiny_model(**over):
    """ModelCross "tiny" with the oracle's weights, after one forward (the weights sit in their flat buffers: what grad_sink() maps), and
    the two input batches A and B"""
    import xvit
    cfg = R.make_config("tiny", **over)
    model = xvit.ModelCross(cfg).to(dev())
    model.load_state_dict(R.make_state_dict(cfg, seed=0))
    model.train()
    ins = [tuple(t.to(dev()) for t in R.make_inputs(cfg, 4, seed=s)) for s in (3, 8)]
    with torch.no_grad():
        model(*ins[0])
    return model, ins


def _backward(model, img, labels, reducer=None):
    _, loss = model(img, labels)
    loss.backward()
    if reducer is not None:
        reducer.finish()
    torch.cuda.synchronize()


_REF = []


def _ref():
    """gradients of batches A and B without a reducer: computed once (needs the rccl1 fixture's deterministic mode), on the CPU, shared"""
    if not _REF:
        model, ins = _tiny_model()
        for i in ins:
            for p in model.parameters():
                p.grad = None
            _backward(model, *i)
            _REF.append({k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()})
        assert any(not torch.equal(_REF[0][k], _REF[1][k]) for k in _REF[0])
    return _REF


def _sink_hits(monkeypatch, red):
    """[number of weight-gradient destinations handed out since it was last set to 0 that were bucket views]"""
    import xvit.functional as XF
    views = {v.data_ptr() for b in red.buckets for v in b.views}
    hits, real = [0], XF._grad_out

    def spy(like, shape, device):
        out = real(like, shape, device)
        hits[0] += out.data_ptr() in views
        return out
    monkeypatch.setattr(XF, "_grad_out", spy)
    return hits


def _events_empty(red):
    return all(len(b.events) == 0 for b in red.buckets)


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
@pytest.mark.parametrize("sink", [False, True], ids=["nosink", "sink"])
@pytest.mark.parametrize("pattern", ["kept", "accumulate"])
def test_kept_and_accumulated_gradients_equal_plain_autograd(rccl1, monkeypatch, pattern, sink, wire):
    """kept: p.grad zeroed in place between three steps (A, B, A), every step gives that batch's gradients.  accumulate: backward +
    finish() on A, then on B, nothing zeroed: g_A + g_B.  Every parameter, 1-D and 2-D.  Before the sink withheld the view of a
    parameter that has a .grad, the sink arms gave 2 * g_new for every weight matrix from the second backward on."""
    import xvit.functional as XF
    from xvit.ddp import BucketedGradReducer
    ref = _ref()
    model, ins = _tiny_model()
    red = BucketedGradReducer(list(model.parameters()), bucket_bytes=64 << 10, comm_dtype=WIRES[wire])
    assert len(red.buckets) >= 4 and max(len(b.params) for b in red.buckets) > 1
    XF.GRAD_SINK = red.grad_sink(model) if sink else None
    hits = _sink_hits(monkeypatch, red)
    wired = rt if wire == "bf16" else (lambda t: t)
    have = None
    for s, which in enumerate((0, 1, 0) if pattern == "kept" else (0, 1)):
        hits[0] = 0
        _backward(model, *ins[which], red)
        have ={k: wired(g if have is None or pattern == "kept" else have[k] + g) for k, g in ref[which].items()}
        bad = []
        for k, p in model.named_parameters():
            assert p.grad.data_ptr() == red._view_of[id(p)].data_ptr() and p.grad.dtype == torch.float32, k
            if not torch.equal(p.grad.cpu(), have[k]):
                bad.append((k, p.dim(), bool(torch.equal(p.grad.cpu(), wired(2 * ref[which][k])))))
        print(f"{pattern} sink={sink} {wire} step {s}: {len(bad)} gradients differ; (name, dim, == 2 * g_new): {bad[:3]}")
        assert not bad, (s, len(bad), bad[:3])
        # the fast path (no .grad before backward) writes into the views; a kept .grad gets fresh tensors
        assert hits[0] > 20 if sink and s == 0 else hits[0] == 0, (s, hits[0])
        if pattern == "kept":
            for p in model.parameters():
                p.grad.zero_()
    red.remove()


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
def test_documented_optimizer_loop_keeps_its_gradient_tensors(rccl1, capturable):
    """three FusedAdam(lr=1e-3) steps with the reducer, GRAD_SINK and opt.zero_grad(set_to_none=False) end with the
    parameters, bit for bit, of the same loop with red.zero_grad() and of the same loop without a reducer (fp32 wire).  capturable=True
    holds the gradients' addresses in device tables; they are the bucket views in both reducer loops, so its address check passes."""
    import xvit.functional as XF
    from xvit.ddp import BucketedGradReducer
    from xvit.optim import FusedAdam
    final = {}
    for arm in ("keep", "drop", "plain"):
        model, ins = _tiny_model()
        red = BucketedGradReducer(list(model.parameters()), bucket_bytes=64 << 10, comm_dtype=torch.float32) if arm != "plain" else None
        opt = FusedAdam(model.parameters(), lr=1e-3, capturable=capturable)
        XF.GRAD_SINK = red.grad_sink(model) if red is not None else None
        try:
            for s in range(3):
                _backward(model, *ins[s % 2], red)
                opt.step()
                if arm == "drop":
                    red.zero_grad()
                elif arm == "keep" or capturable:
                    opt.zero_grad(set_to_none=False)
                    assert all(p.grad is not None for p in model.parameters())
                else:
                    opt.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
        finally:
            XF.GRAD_SINK = None
            if red is not None:
                red.remove()
        final[arm] = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
    start = R.make_state_dict(R.make_config("tiny"), seed=0)
    assert any(not torch.equal(final["plain"][k], start[k]) for k in final["plain"])          # the loop trained something
    for arm in ("keep", "drop"):
        bad = [k for k in final["plain"] if not torch.equal(final[arm][k], final["plain"][k])]
        assert not bad, (arm, len(bad), bad[:3])


def test_eager_after_graph_with_one_reducer(rccl1):
    """Eager on A and B, GraphedStep(reducer=red), replays of B and A, then eager on A and B again with the SAME reducer: the eager
    gradients afterwards are those from before, and the replays', bit for bit.  finish() empties every bucket's events, inside the
    capture too, so an eager launch never waits for an event that was last recorded while capturing."""
    import xvit.functional as XF
    from xvit.ddp import BucketedGradReducer
    from xvit.graph import GraphedStep
    ref = _ref()
    model, ins = _tiny_model()
    red = BucketedGradReducer(list(model.parameters()), bucket_bytes=64 << 10)
    sink = red.grad_sink(model)

    def eager(which):
        XF.GRAD_SINK = sink
        try:
            red.zero_grad()
            _backward(model, *ins[which], red)
        finally:
            XF.GRAD_SINK = None
        assert _events_empty(red)
        return {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}

    def same(got, want):
        return [k for k in want if not torch.equal(got[k], want[k])]

    before = [eager(0), eager(1)]
    assert not same(before[0], ref[0]) and not same(before[1], ref[1])
    step = GraphedStep(model, *ins[0], reducer=red)
    assert _events_empty(red)
    for which in (1, 0):
        step(*ins[which])
        torch.cuda.synchronize()
        assert _events_empty(red)
        assert not same({k: p.grad.detach().cpu() for k, p in model.named_parameters()}, ref[which]), which
    for which in (0, 1):
        bad = same(eager(which), before[which])
        assert not bad, (which, len(bad), bad[:3])
    red.remove()


@pytest.mark.parametrize("captured_in", ["train", "eval"])
def test_graphed_step_refuses_another_mode(captured_in):
    """The mode is frozen into the graph (dropout epoch, patch dropout and mix draws): a replay in the other mode is refused, and after
    the mode is restored the step replays and gives the logits it gave before, for the same inputs (dropout 0)."""
    from xvit.graph import GraphedStep
    model, ins = _tiny_model()
    model.train(captured_in == "train")
    step = GraphedStep(model, *ins[0])
    want = step(*ins[1])[0].clone()
    model.train(captured_in != "train")
    with pytest.raises(RuntimeError, match="new GraphedStep"):
        step(*ins[1])
    model.train(captured_in == "train")
    step(*ins[0])
    got = step(*ins[1])[0].clone()
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.isfinite(got).all()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs >= 2 GPUs")
def test_accumulation_round_two_rccl_ranks(tmp_path):
    """Two backward + finish() rounds with p.grad kept, fp32 wire, gradient sink on: p.grad == mean(g1) + mean(g2) on both ranks, within
    3 * 2^-24 * (|acc| + |g_0| + |g_1|) element by element (acc: the reduced gradient of round 1, g_r: rank r's local gradient of round
    2): the bound derived in tests/test_ddp_gloo.py::test_bucketed_reducer_world2_accumulation, with RCCL's AVG in place of the exact
    pre-scale by 1/2 and the sum."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "XVIT_GRAD_COMM")}
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "_ddp_accum_worker.py"), str(tmp_path), "4"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "rccl ranks: 2" in r.stdout
    w0, w1 = torch.load(tmp_path / "a0.pt"), torch.load(tmp_path / "a1.pt")
    for k in w0["after"][0]:
        for rnd in range(2):
            assert torch.equal(w0["after"][rnd][k], w1["after"][rnd][k]), (rnd, k)             # the same bits on every rank
        m1 = (w0["local"][0][k].double() + w1["local"][0][k].double()) / 2
        m2 = (w0["local"][1][k].double() + w1["local"][1][k].double()) / 2
        bound = 3 * 2.0 ** -24 * (w0["after"][0][k].double().abs() + w0["local"][1][k].double().abs() + w1["local"][1][k].double().abs())
        err = (w0["after"][1][k].double() - (m1 + m2)).abs()
        assert (err <= bound).all(), (k, float((err - bound).max()))
