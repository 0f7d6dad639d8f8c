"""GPU: xvit.optim.FusedAdamW on the tiny ModelCross against torch.optim.AdamW / Adam handed the same groups with lr * lr_scale folded into
lr and the same gradients, at the project's gates (tests/test_optim_gpu.py: parameters rel-L2 < 2e-6, moments < 5e-6); the weight average
against its float64 recursion; schedulers; the step inside GraphedStep; ema_weights() and the state-dict round trip.  Every step of the
reference starts from a snapshot of the model's parameters, so the comparison is of the optimizer alone (as tests/test_graph_optim_gpu.py)."""
import copy
import math

import pytest
import torch

import ref_cpu as R
from _util import dev, rel

pytestmark = pytest.mark.gpu

P_GATE, M_GATE = 2e-6, 5e-6
HYPER = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-8)


def _build(name="tiny"):
    import xvit
    cfg = R.make_config(name)
    model = xvit.ModelCross(cfg).to(dev())
    model.load_state_dict(R.make_state_dict(cfg, seed=0))
    model.train()
    return cfg, model


def _inputs(cfg, batch, seeds):
    return [tuple(t.to(dev()) for t in R.make_inputs(cfg, batch, seed=s)) for s in seeds]


class _Twin:
    """torch.optim.AdamW (or Adam) on clones, one group per group of `opt` with the rate folded; optionally clip_grad_norm_ first."""

    def __init__(self, opt, max_norm=None):
        self.opt_params = [p for g in opt.param_groups for p in g["params"]]
        groups = [dict(params=[torch.nn.Parameter(p.detach().clone()) for p in g["params"]], lr=g["lr"] * g["lr_scale"], weight_decay=g["weight_decay"],
                       betas=g["betas"], eps=g["eps"]) for g in opt.param_groups]
        self.ps = [p for g in groups for p in g["params"]]
        self.opt = (torch.optim.AdamW if opt.decoupled else torch.optim.Adam)(groups, lr=1e-3)
        self.max_norm = max_norm

    def step(self, snapshot, grads):
        with torch.no_grad():
            for rp, s in zip(self.ps, snapshot):
                rp.copy_(s)
        for rp, g in zip(self.ps, grads):
            rp.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(self.ps, self.max_norm) if self.max_norm is not None else None
        self.opt.step()
        return total

    def compare(self, opt, what=""):
        for i, (p, rp) in enumerate(zip(self.opt_params, self.ps)):
            assert rel(p, rp) < P_GATE, (what, i, tuple(p.shape), rel(p, rp))
            assert rel(opt.state[p]["exp_avg"], self.opt.state[rp]["exp_avg"]) < M_GATE, (what, i)
            assert rel(opt.state[p]["exp_avg_sq"], self.opt.state[rp]["exp_avg_sq"]) < M_GATE, (what, i)


class _Average:
    """The float64 recursion e += w (p' - e) over the parameters read back after each step."""

    def __init__(self, params, decay, warmup):
        self.params, self.decay, self.warmup, self.t = params, decay, warmup, 0
        self.e = [p.detach().double().clone() for p in params]

    def step(self):
        self.t += 1
        d = min(self.decay, (1 + self.t) / (10 + self.t)) if self.warmup else self.decay
        for e, p in zip(self.e, self.params):
            e += (1 - d) * (p.detach().double() - e)

    def compare(self, opt, what=""):
        for i, (e, p) in enumerate(zip(self.e, self.params)):
            assert rel(opt.state[p]["ema"], e) < M_GATE, (what, i, rel(opt.state[p]["ema"], e))


def _eager_loop(model, opt, twin, ins, steps, avg=None, sched=None, twin_sched=None):
    params = twin.opt_params
    for n in range(steps):
        opt.zero_grad(set_to_none=False)
        _, loss = model(*ins[n % len(ins)])
        loss.backward()
        snap = [p.detach().clone() for p in params]
        twin.step(snap, [p.grad for p in params])
        opt.step()
        torch.cuda.synchronize()
        twin.compare(opt, f"step {n + 1}")
        if avg is not None:
            avg.step()
            avg.compare(opt, f"step {n + 1}")
        if sched is not None:
            sched.step(); twin_sched.step()


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
@pytest.mark.parametrize("setup", ["plain", "layer decay", "coupled"])
def test_matches_torch_adamw(setup, capturable):
    from xvit.optim import FusedAdamW, layer_decay_groups
    cfg, model = _build()
    ins = _inputs(cfg, 4, [0, 9])
    if setup == "layer decay":
        opt = FusedAdamW(layer_decay_groups(model, 0.75, 0.05), capturable=capturable, ema_decay=0.9, ema_warmup=True, **HYPER)
    else:
        opt = FusedAdamW(model.parameters(), weight_decay=0.05, decoupled=setup == "plain", capturable=capturable, ema_decay=0.5 if setup == "plain" else None, **HYPER)
    twin = _Twin(opt)
    avg = _Average(twin.opt_params, opt.ema_decay, opt.ema_warmup) if opt.ema_decay is not None else None
    _eager_loop(model, opt, twin, ins, 4, avg)
    assert opt.launch_sets == 1
    assert {int(v["step"]) for v in opt.state_dict()["state"].values()} == {4}
    grp = model._flat                                              # the bf16 operand copies follow without a cast launch
    for p, v16 in zip(grp.params, grp.view16):
        assert torch.equal(v16, p.detach().to(torch.bfloat16))
    assert grp.stamp == sum(q._version for q in grp.params)


@pytest.mark.parametrize("diverge", [False, True], ids=["one lambda", "per-group lambdas"])
def test_schedulers(diverge):
    from xvit.optim import FusedAdamW, layer_decay_groups
    cfg, model = _build()
    ins = _inputs(cfg, 4, [0, 9])
    opt = FusedAdamW(layer_decay_groups(model, 0.75, 0.05), capturable=True, **HYPER)
    twin = _Twin(opt)
    n = len(opt.param_groups)
    lam = [(lambda t, k=k: 1.0 / (1.0 + 0.1 * (k + 1) * t)) for k in range(n)] if diverge else (lambda t: 1.0 / (1.0 + t))
    sched, twin_sched = torch.optim.lr_scheduler.LambdaLR(opt, lam), torch.optim.lr_scheduler.LambdaLR(twin.opt, lam)
    _eager_loop(model, opt, twin, ins, 4, sched=sched, twin_sched=twin_sched)
    assert opt.launch_sets == 1 and opt.lr_copies == 3               # the rate of the first group changed three times between the four steps
    assert (opt.scale_copies == 3) if diverge else (opt.scale_copies == 0)


def _snapshot(model, opt, params):
    torch.cuda.synchronize()
    return ([p.detach().clone() for p in params], [[opt.state[p][k].clone() for k in ("exp_avg", "exp_avg_sq", "ema")] for p in params],
            {int(v["step"]) for v in opt.state_dict()["state"].values()}, [v.clone() for v in model._flat.view16])


def _same(a, b):
    return (all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(x, y) for s, t in zip(a[1], b[1]) for x, y in zip(s, t)) and a[2] == b[2]
            and all(torch.equal(x, y) for x, y in zip(a[3], b[3])))


def test_graphed_step_construction_leaves_parameters_moments_average_and_step_count_untouched():
    from xvit.graph import GraphedStep
    from xvit.optim import FusedAdamW, layer_decay_groups
    cfg, model = _build()
    (img, lab), = _inputs(cfg, 4, [0])
    opt = FusedAdamW(layer_decay_groups(model, 0.75, 0.05), capturable=True, ema_decay=0.99, max_grad_norm=1.0, **HYPER)
    params = [p for g in opt.param_groups for p in g["params"]]
    for _ in range(2):                                             # an optimizer with a history
        opt.zero_grad(set_to_none=False)
        model(img, lab)[1].backward()
        opt.step()
    s0 = _snapshot(model, opt, params)
    assert s0[2] == {2} and any(not torch.equal(opt.state[p]["ema"], p) for p in params)
    step = GraphedStep(model, img, lab, optimizer=opt)
    assert _same(s0, _snapshot(model, opt, params))                 # construction trains nothing
    step(img, lab)
    s1 = _snapshot(model, opt, params)
    assert s1[2] == {3} and not _same(s0, s1)


def test_graphed_step_trains_like_the_eager_loop_and_skips():
    """A fresh optimizer on the inputs of tests/test_graph_optim_gpu.py's replay test, against clip_grad_norm_ + torch.optim.AdamW.  The
    whole-tensor gates are relative: they presuppose that no tensor's new moment is a near-cancellation of beta1 m against (1 - beta1) g,
    which holds on these inputs."""
    from xvit.graph import GraphedStep
    from xvit.optim import FusedAdamW, layer_decay_groups
    cfg, model = _build()
    ins = _inputs(cfg, 4, [0, 9, 3, 5])
    opt = FusedAdamW(layer_decay_groups(model, 0.75, 0.05), capturable=True, ema_decay=0.99, max_grad_norm=1.0, skip_nonfinite=True, **HYPER)
    params = [p for g in opt.param_groups for p in g["params"]]
    snapshot, same = (lambda: _snapshot(model, opt, params)), _same
    step = GraphedStep(model, *ins[0], optimizer=opt)
    twin = _Twin(opt, max_norm=1.0)
    avg = _Average(params, 0.99, False)
    clipped = 0
    for n, (img, lab) in enumerate(ins):
        snap = [p.detach().clone() for p in params]
        step(img, lab)
        torch.cuda.synchronize()
        total = twin.step(snap, [p.grad for p in params])
        clipped += float(total) > 1.0
        assert abs(float(opt.last_grad_norm) - float(total)) <= 1e-5 * float(total)
        twin.compare(opt, f"replay {n + 1}")
        avg.step()
        avg.compare(opt, f"replay {n + 1}")
    assert clipped >= 1
    # a skipped step: an inf in one of the gradient buffers the graph owns, then the optimizer's own launches on them
    s1 = snapshot()
    assert s1[2] == {4}
    params[7].grad.view(-1)[0] = math.inf
    opt.step()
    assert same(s1, snapshot()) and int(opt.skipped_steps) == 1
    # ... and the graph goes on training afterwards
    snap = [p.detach().clone() for p in params]
    step(*ins[0])
    torch.cuda.synchronize()
    twin.step(snap, [p.grad for p in params])
    twin.compare(opt, "the replay after the skipped step")
    avg.step()
    avg.compare(opt, "the replay after the skipped step")


def test_ema_weights_context_and_ema_state_dict(monkeypatch):
    import xvit
    from xvit.graph import GraphedStep
    from xvit.optim import FusedAdamW
    cfg, model = _build()
    ins = _inputs(cfg, 4, [0, 9])
    opt = FusedAdamW(model.parameters(), weight_decay=0.05, capturable=True, ema_decay=0.5, **HYPER)
    params = list(model.parameters())
    step = GraphedStep(model, *ins[0], optimizer=opt)
    twin = _Twin(opt)
    for img, lab in ins:
        snap = [p.detach().clone() for p in params]
        step(img, lab)
        torch.cuda.synchronize()
        twin.step(snap, [p.grad for p in params])
    before = [p.detach().clone() for p in params]
    before16 = [v.clone() for v in model._flat.view16]
    ema = [opt.state[p]["ema"].clone() for p in params]
    sd = opt.ema_state_dict(model)
    assert set(sd) == set(model.state_dict()) and all(torch.equal(sd[k], e) for (k, _), e in zip(model.named_parameters(), ema))
    other = xvit.ModelCross(cfg).to(dev())
    res = other.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    other.eval(); model.eval()
    with torch.no_grad():
        want = other(*ins[0])[0].clone()
        trained = model(*ins[0])[0].clone()
        with opt.ema_weights():
            assert all(torch.equal(p, e) for p, e in zip(params, ema)) and all(torch.equal(opt.state[p]["ema"], b) for p, b in zip(params, before))
            got = model(*ins[0])[0].clone()
        back = model(*ins[0])[0].clone()
    model.train()
    assert torch.equal(got, want) and not torch.equal(got, trained) and torch.equal(back, trained)
    torch.cuda.synchronize()
    assert all(torch.equal(p, b) for p, b in zip(params, before)) and all(torch.equal(opt.state[p]["ema"], e) for p, e in zip(params, ema))
    assert all(torch.equal(v, b) for v, b in zip(model._flat.view16, before16))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)       # what the exchange asks before it launches anything
    with pytest.raises(RuntimeError, match="captur"):
        with opt.ema_weights():
            pass
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(torch.equal(p, b) for p, b in zip(params, before))
    # the graph captured before the exchange still trains: one more replay against the twin, which never swapped
    snap = [p.detach().clone() for p in params]
    step(*ins[0])
    torch.cuda.synchronize()
    twin.step(snap, [p.grad for p in params])
    twin.compare(opt, "the replay after ema_weights()")
    assert any(not torch.equal(p, b) for p, b in zip(params, before))


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
def test_state_dict_round_trip(capturable):
    from xvit.optim import FusedAdam, FusedAdamW
    torch.manual_seed(0)
    shapes = [(64, 48), (3072,), (5,), (16385,), (1,)]
    gen = [[torch.randn(*s, device=dev()) for s in shapes] for _ in range(4)]

    def make(cls, src=None, one_group=False, **kw):
        ps = [torch.nn.Parameter((torch.randn(*s, device=dev()) if src is None else src[i].detach().clone())) for i, s in enumerate(shapes)]
        for p in ps:
            p.grad = torch.zeros_like(p)
        return ps, cls([dict(params=ps[:2], lr_scale=0.5), dict(params=ps[2:], weight_decay=0.0)] if cls is FusedAdamW and not one_group else ps, **kw)

    def run(ps, opt, n0, n1):
        for n in range(n0, n1):
            for p, g in zip(ps, gen[n]):
                p.grad.copy_(g)
            opt.step()
        torch.cuda.synchronize()
    kw = dict(lr=1e-2, weight_decay=0.05, capturable=capturable, ema_decay=0.9, ema_warmup=True)
    pa, a = make(FusedAdamW, **kw)
    run(pa, a, 0, 2)
    sd = copy.deepcopy(a.state_dict())              # as a checkpoint would: state_dict() hands out the live tensors
    assert all("ema" in v and int(v["step"]) == 2 for v in sd["state"].values())
    pb, b = make(FusedAdamW, src=pa, **kw)
    if capturable:
        b.prepare()                                                 # the tables exist: the values are copied into the existing buffers
        ptrs = [b.state[p]["ema"].data_ptr() for p in pb]
    b.load_state_dict(sd)
    if capturable:
        assert ptrs == [b.state[p]["ema"].data_ptr() for p in pb]
    for x, y in zip(pa, pb):
        assert all(torch.equal(a.state[x][k], b.state[y][k]) for k in ("exp_avg", "exp_avg_sq", "ema"))
    run(pa, a, 2, 4); run(pb, b, 2, 4)
    for x, y in zip(pa, pb):                                        # the same kernel on the same numbers: bit for bit, the warm-up step count included
        assert torch.equal(x, y) and all(torch.equal(a.state[x][k], b.state[y][k]) for k in ("exp_avg", "exp_avg_sq", "ema"))
    assert {int(v["step"]) for v in b.state_dict()["state"].values()} == {4}
    # a FusedAdam state has no average: it starts at the current p
    pc, c = make(FusedAdam, lr=1e-2, capturable=capturable)
    run(pc, c, 0, 2)
    pd, d = make(FusedAdamW, src=pc, one_group=True, **kw)
    if capturable:
        d.prepare()
    d.load_state_dict(copy.deepcopy(c.state_dict()))
    for x, y in zip(pc, pd):
        assert torch.equal(d.state[y]["ema"], y.detach()) and torch.equal(d.state[y]["exp_avg"], c.state[x]["exp_avg"])
    run(pd, d, 2, 3)
    assert {int(v["step"]) for v in d.state_dict()["state"].values()} == {3}
