"""GPU: the whole training step as one HIP-graph replay: GraphedStep(..., optimizer=FusedAdam(capturable=True)) appends the gradient norm,
the clip / step prologue and Adam to the captured forward + backward.  Gates are the project's: optimizer (tests/test_optim_gpu.py:
parameters rel-L2 < 2e-6, moments < 5e-6) and gradients (tests/test_graph_gpu.py: rel < 1e-5 or absolute max < 1e-6)."""
import socket

import pytest
import torch

import ref_cpu as R
from _util import dev, rel

pytestmark = pytest.mark.gpu

P_GATE, M_GATE = 2e-6, 5e-6


def _build(kind, dropout=0.0, name="tiny"):
    import xvit
    if kind == "cross":
        cfg = R.make_config(name, dropout=dropout)
        model, sd = xvit.ModelCross(cfg), R.make_state_dict(cfg, seed=0)
    else:
        cfg = R.make_config(name, num_layers=2, dropout=dropout)
        model, sd = xvit.ModelVIT(cfg), R.make_vit_state_dict(cfg, seed=0)
    model = model.to(dev())
    model.load_state_dict(sd)
    model.train()
    return cfg, model


def _twin(kind, cfg, state):
    import xvit
    m = (xvit.ModelCross(cfg) if kind == "cross" else xvit.ModelVIT(cfg)).to(dev())
    m.load_state_dict(state)
    return m


def _inputs(cfg, batch, seeds):
    return [tuple(t.to(dev()) for t in R.make_inputs(cfg, batch, seed=s)) for s in seeds]


def _eager_grads(model, img, lab):
    for p in model.parameters():
        p.grad = None
    _, loss = model(img, lab)
    loss.backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _grad_norm(grads):
    return float(torch.cat([g.double().flatten() for g in grads]).norm())


def _opt_snapshot(opt, params):
    return ([p.detach().clone() for p in params],
            [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) if p in opt.state and opt.state[p] else None for p in params],
            {k: int(v["step"]) for k, v in opt.state_dict()["state"].items()})


class _Reference:
    """clip_grad_norm_ + torch.optim.Adam carried along the replays: each step starts from a snapshot of the model's parameters and takes
    the gradients the replay itself produced, so the comparison is of the optimizer alone (the gradients' atomic-order noise stays out)."""

    def __init__(self, params, max_norm, **hyper):
        self.ps = [torch.nn.Parameter(p.detach().clone()) for p in params]
        self.opt = torch.optim.Adam(self.ps, **hyper)
        self.max_norm = max_norm

    def step(self, snapshot, grads):
        with torch.no_grad():
            for rp, s in zip(self.ps, snapshot):
                rp.copy_(s)
        for rp, g in zip(self.ps, grads):
            rp.grad = None if g is None else g.clone()
        total = torch.nn.utils.clip_grad_norm_(self.ps, self.max_norm) if self.max_norm is not None else None
        self.opt.step()
        return total

    def compare(self, params, opt):
        for i, (p, rp) in enumerate(zip(params, self.ps)):
            assert rel(p, rp) < P_GATE, (i, tuple(p.shape), rel(p, rp))
            if rp in self.opt.state and self.opt.state[rp]:
                assert rel(opt.state[p]["exp_avg"], self.opt.state[rp]["exp_avg"]) < M_GATE, i
                assert rel(opt.state[p]["exp_avg_sq"], self.opt.state[rp]["exp_avg_sq"]) < M_GATE, i


@pytest.mark.parametrize("kind", ["cross", "vit"])
def test_construction_leaves_parameters_moments_and_step_count_untouched(kind):
    from xvit.graph import GraphedStep
    from xvit.optim import FusedAdam
    cfg, model = _build(kind)
    (img, lab), = _inputs(cfg, 4, [0])
    params = list(model.parameters())
    opt = FusedAdam(params, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0, capturable=True)
    for _ in range(2):                                     # an optimizer with a history: two eager steps (static gradient buffers)
        opt.zero_grad(set_to_none=False)
        _, loss = model(img, lab)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    p0, m0, s0 = _opt_snapshot(opt, params)
    assert set(s0.values()) == {2}
    step = GraphedStep(model, img, lab, optimizer=opt)
    torch.cuda.synchronize()
    p1, m1, s1 = _opt_snapshot(opt, params)
    assert s1 == s0
    for a, b in zip(p0, p1):
        assert torch.equal(a, b)
    for a, b in zip(m0, m1):
        assert (a is None and b is None) or (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
    step(img, lab)
    torch.cuda.synchronize()
    assert set(_opt_snapshot(opt, params)[2].values()) == {3}
    assert any(not torch.equal(a, p) for a, p in zip(p0, params))
    # a fresh optimizer: construction creates zero moments at step 0 and nothing else
    cfg, model = _build(kind)
    params = list(model.parameters())
    before = [p.detach().clone() for p in params]
    opt = FusedAdam(params, lr=1e-3, capturable=True)
    GraphedStep(model, img, lab, optimizer=opt)
    torch.cuda.synchronize()
    assert all(torch.equal(a, p) for a, p in zip(before, params))
    assert set(_opt_snapshot(opt, params)[2].values()) == {0}
    assert all(not st["exp_avg"].any() and not st["exp_avg_sq"].any() for st in opt.state.values())


@pytest.mark.parametrize("kind", ["cross", "vit"])
def test_replays_train_like_clip_grad_norm_and_torch_adam(kind):
    from xvit.graph import GraphedStep
    from xvit.optim import FusedAdam
    cfg, model = _build(kind)
    ins = _inputs(cfg, 4, [0, 9, 3, 5])
    params = list(model.parameters())
    names = [k for k, _ in model.named_parameters()]
    max_norm = _grad_norm(_eager_grads(model, *ins[0]).values()) / 3       # clipping is active from the first step
    for p in params:
        p.grad = None
    hyper = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01)
    opt = FusedAdam(params, max_grad_norm=max_norm, capturable=True, **hyper)
    step = GraphedStep(model, *ins[0], optimizer=opt)
    ref = _Reference(params, max_norm, **hyper)
    clipped = 0
    for n, (img, lab) in enumerate(ins):
        snap = [p.detach().clone() for p in params]
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        step(img, lab)
        torch.cuda.synchronize()
        grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
        total = ref.step(snap, grads)
        clipped += float(total) > max_norm
        assert abs(float(opt.last_grad_norm) - float(total)) <= 1e-5 * float(total)
        ref.compare(params, opt)
        # ... and the replay's (unclipped, untouched) gradients are those of an eager step of a model holding the snapshot
        eager = _eager_grads(_twin(kind, cfg, state), img, lab)
        for k, g in zip(names, grads):
            if g is not None:
                assert rel(g, eager[k]) < 1e-5 or float(eager[k].abs().max()) < 1e-6, (n, k)
    assert clipped >= 1
    assert {int(v["step"]) for v in opt.state_dict()["state"].values()} == {4}


@pytest.mark.parametrize("kind", ["cross", "vit"])
def test_loss_falls_and_eval_sees_the_trained_weights(kind):
    """Four replays of one batch lower the loss; an eager eval forward between and after the replays uses the weights the graph trained:
    bit-equal to a fresh model that loaded model.state_dict() (stale bf16 operand copies would show here)."""
    from xvit.graph import GraphedStep
    from xvit.optim import FusedAdam
    cfg, model = _build(kind)
    (img, lab), = _inputs(cfg, 4, [0])
    opt = FusedAdam(model.parameters(), lr=1e-3, max_grad_norm=5.0, capturable=True)
    step = GraphedStep(model, img, lab, optimizer=opt)
    losses = []
    for n in range(4):
        losses.append(float(step(img, lab)[1]))
        if n in (1, 3):
            model.eval()
            with torch.no_grad():
                got = model(img, lab)[0].clone()
                want = _twin(kind, cfg, model.state_dict()).eval()(img, lab)[0]
            model.train()
            assert torch.equal(got, want), n
    assert losses[3] < losses[0], losses
    assert losses[1] != losses[0]


def test_learning_rate_changes_between_replays_take_effect():
    from xvit.graph import GraphedStep
    from xvit.optim import FusedAdam
    cfg, model = _build("cross")
    (img, lab), = _inputs(cfg, 4, [0])
    params = list(model.parameters())
    opt = FusedAdam(params, lr=1e-3, capturable=True)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda epoch: 0.0 if epoch == 1 else 1.0)
    step = GraphedStep(model, img, lab, optimizer=opt)
    before = [p.detach().clone() for p in params]
    step(img, lab); sched.step()                           # lr 1e-3
    torch.cuda.synchronize()
    after1 = [p.detach().clone() for p in params]
    assert any(not torch.equal(a, b) for a, b in zip(before, after1))
    assert opt.param_groups[0]["lr"] == 0.0
    step(img, lab); sched.step()                           # lr 0: nothing moves, the step count does
    torch.cuda.synchronize()
    assert all(torch.equal(a, p) for a, p in zip(after1, params))
    assert {int(v["step"]) for v in opt.state_dict()["state"].values()} == {2}
    step(img, lab)                                         # lr 1e-3 again
    torch.cuda.synchronize()
    assert any(not torch.equal(a, p) for a, p in zip(after1, params))
    assert opt.lr_copies == 2


def test_dropout_still_draws_fresh_masks_with_the_optimizer_in_the_graph():
    from xvit.graph import GraphedStep
    from xvit.optim import FusedAdam
    cfg, model = _build("cross", dropout=0.1)
    (img, lab), = _inputs(cfg, 4, [0])
    torch.manual_seed(5)
    opt = FusedAdam(model.parameters(), lr=0.0, capturable=True)
    step = GraphedStep(model, img, lab, optimizer=opt)
    e0 = int(step._epoch)
    l1 = step(img, lab)[0].clone()
    l2 = step(img, lab)[0].clone()
    torch.cuda.synchronize()
    assert not torch.equal(l1, l2)                         # same weights (lr = 0), same batch: only the masks differ
    assert int(step._epoch) == e0 + 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_with_the_one_rank_rccl_reducer(monkeypatch):
    import torch.distributed as dist
    from xvit.ddp import BucketedGradReducer
    from xvit.graph import GraphedStep
    from xvit.optim import FusedAdam
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_free_port()))
    cfg, model = _build("cross", name="small")
    ins = _inputs(cfg, 6, [2, 7])
    params = list(model.parameters())
    max_norm = _grad_norm(_eager_grads(model, *ins[0]).values()) / 3
    for p in params:
        p.grad = None
    hyper = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev())
    try:
        red = BucketedGradReducer(params, bucket_bytes=128 << 10)
        opt = FusedAdam(params, max_grad_norm=max_norm, capturable=True, **hyper)
        step = GraphedStep(model, *ins[0], reducer=red, optimizer=opt)
        ref = _Reference(params, max_norm, **hyper)
        for img, lab in ins:
            snap = [p.detach().clone() for p in params]
            step(img, lab)
            torch.cuda.synchronize()
            for p in params:
                assert p.grad.data_ptr() == red._view_of[id(p)].data_ptr()
            total = ref.step(snap, [p.grad.detach().clone() for p in params])
            assert float(total) > max_norm
            ref.compare(params, opt)
        red.remove()
    finally:
        dist.destroy_process_group()


def test_other_optimizers_are_refused_before_any_capture():
    from xvit.graph import GraphedStep
    from xvit.optim import FusedAdam
    cfg, model = _build("cross")
    (img, lab), = _inputs(cfg, 4, [0])
    before = [p.detach().clone() for p in model.parameters()]
    for opt in (torch.optim.Adam(model.parameters(), lr=1e-3), FusedAdam(model.parameters(), lr=1e-3, max_grad_norm=1.0)):
        with pytest.raises(RuntimeError, match="capturable=True"):
            GraphedStep(model, img, lab, optimizer=opt)
    assert not torch.cuda.is_current_stream_capturing()
    assert all(p.grad is None for p in model.parameters())            # not even a warm-up step ran
    assert all(torch.equal(a, p) for a, p in zip(before, model.parameters()))
