"""GPU: FusedAdam's fused global-norm clipping (max_grad_norm), its capturable mode (every per-step number on the device, so a step can be
captured into a graph and replayed) and skip_nonfinite, against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on clones.
Tolerances are the ones of tests/test_optim_gpu.py: parameters rel-L2 < 2e-6, moments < 5e-6."""
import copy

import pytest
import torch

from _util import dev, rel

pytestmark = pytest.mark.gpu

SHAPES = [(768, 768), (3072,), (5,), (2, 3072), (1, 513, 768), (16385,), (1,)]     # the list of test_fused_adam_matches_torch_adam
HYPER = dict(lr=3e-3, betas=(0.9, 0.98), eps=1e-8)
P_GATE, M_GATE = 2e-6, 5e-6


def _params(shapes=SHAPES, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g).to(dev())) for s in shapes]


def _clones(ps):
    return [torch.nn.Parameter(p.detach().clone()) for p in ps]


def _grads(ps, n, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [[torch.randn(*p.shape, generator=g).to(dev()) for p in ps] for _ in range(n)]


def _set_grads(ps, gs, static=False):
    for p, g in zip(ps, gs):
        if static and p.grad is not None:
            p.grad.copy_(g)
        else:
            p.grad = g.clone()


def _norm64(gs):
    return float(torch.cat([g.double().flatten() for g in gs]).norm())


def _equal_state(a, ps_a, b, ps_b):
    for pa, pb in zip(ps_a, ps_b):
        assert torch.equal(pa, pb)
        if pa in a.state or pb in b.state:
            assert torch.equal(a.state[pa]["exp_avg"], b.state[pb]["exp_avg"]) and torch.equal(a.state[pa]["exp_avg_sq"], b.state[pb]["exp_avg_sq"])


def _close_state(a, ps_a, b, ps_b):
    for pa, pb in zip(ps_a, ps_b):
        assert rel(pa, pb) < P_GATE, rel(pa, pb)
    for pa, pb in zip(ps_a, ps_b):
        assert rel(a.state[pa]["exp_avg"], b.state[pb]["exp_avg"]) < M_GATE
        assert rel(a.state[pa]["exp_avg_sq"], b.state[pb]["exp_avg_sq"]) < M_GATE


def _steps_of(opt):
    return {k: int(v["step"]) for k, v in opt.state_dict()["state"].items()}


@pytest.mark.parametrize("capturable", [False, True])
def test_grad_norm_against_float64(capturable):
    """last_grad_norm against the float64 norm of the same gradients, gate 1e-5 relative.  Derivation: all terms g*g are non-negative, so
    any fp32 summation order of a chunk has a relative error of at most (roundings along the longest path) * 2^-24.  The kernel's longest
    path is the scalar one (pointer not 16-byte aligned): 64 sequential fused multiply-adds per thread (the product is not rounded
    separately), 6 levels across the wave, 2 adds across the four waves: 72 * 2^-24 = 4.3e-6 on the SUM of squares, half of that on the
    norm; the 16-byte path has 16 + 2 + 6 + 2 = 26.  Chunks are summed in double, and the result is rounded to fp32 once more (2^-24).
    1e-5 covers that bound; it is not tuned to what the kernel gives."""
    from xvit.optim import FusedAdam
    torch.manual_seed(0)
    ps = _params(SHAPES + [(5_000_003,)])
    base = torch.randn(40_000 + 1, device=dev())
    gbase = torch.randn(40_000 + 1, device=dev())
    odd = torch.nn.Parameter(base[1:])                    # 4-byte aligned, not 16
    assert odd.data_ptr() % 16 == 4 and odd.is_contiguous()
    ps.append(odd)
    gs = _grads(ps, 1)[0]
    gs[-1] = gbase[1:]
    worst = 0.0
    for group in [ps] + [[p] for p in ps]:                # all tensors together, then each alone
        idx = [i for i, p in enumerate(ps) if any(p is q for q in group)]
        for i in idx:
            ps[i].grad = gs[i] if ps[i] is odd else gs[i].clone()
        if len(idx) == len(ps) or ps[idx[0]] is odd:
            assert odd.grad.data_ptr() % 16 == 4
        opt = FusedAdam(group, max_grad_norm=1.0, capturable=capturable, **HYPER)
        opt.step()
        want = _norm64([gs[i] for i in idx])
        got = float(opt.last_grad_norm)
        err = abs(got - want) / want
        print(f"norm over {tuple(ps[idx[0]].shape) if len(idx) == 1 else 'all'}: {got!r} vs {want!r} rel {err:.2e}")
        worst = max(worst, err)
        assert err < 1e-5, (got, want)
        for p in group:
            p.grad = None
    print(f"worst relative norm error {worst:.2e}")


@pytest.mark.parametrize("capturable", [False, True])
def test_norm_and_parameters_are_bit_identical_from_run_to_run(capturable):
    from xvit.optim import FusedAdam
    ps0 = _params(SHAPES + [(1_000_001,)])
    gs = _grads(ps0, 2)
    runs = []
    for _ in range(2):
        ps = _clones(ps0)
        opt = FusedAdam(ps, max_grad_norm=5.0, capturable=capturable, **HYPER)
        norms = []
        for g in gs:
            _set_grads(ps, g, static=True)
            opt.step()
            norms.append(opt.last_grad_norm.clone())
        runs.append((ps, opt, norms))
    (pa, a, na), (pb, b, nb) = runs
    assert all(torch.equal(x, y) for x, y in zip(na, nb))
    _equal_state(a, pa, b, pb)


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_clipping_matches_clip_grad_norm_and_torch_adam(wd, capturable):
    from xvit.optim import FusedAdam
    ps_a = _params()
    ps_b = _clones(ps_a)
    gs = _grads(ps_a, 5)
    max_norm = _norm64(gs[0]) / 3                          # clipping is active at every step
    a = FusedAdam(ps_a, weight_decay=wd, max_grad_norm=max_norm, capturable=capturable, **HYPER)
    b = torch.optim.Adam(ps_b, weight_decay=wd, **HYPER)
    for step in range(5):
        _set_grads(ps_a, gs[step], static=capturable)
        _set_grads(ps_b, gs[step])
        if step == 3 and not capturable:                   # a parameter without gradient is skipped and stays out of the norm, like torch does
            ps_a[2].grad = None; ps_b[2].grad = None       # (capturable mode binds a static set of gradients and refuses this: tested below)
        before = [None if p.grad is None else p.grad.clone() for p in ps_a]
        total = torch.nn.utils.clip_grad_norm_(ps_b, max_norm)
        a.step(); b.step()
        assert float(total) > 2 * max_norm
        assert abs(float(a.last_grad_norm) - float(total)) <= 1e-5 * float(total)
        for p, g in zip(ps_a, before):                     # p.grad stays the unclipped gradient, bit for bit
            assert (p.grad is None and g is None) or torch.equal(p.grad, g)
    _close_state(a, ps_a, b, ps_b)


@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_clipping_armed_but_not_reached_is_bit_identical_to_no_clipping(wd):
    """Coefficient exactly 1: the same parameters and moments as FusedAdam without max_grad_norm, bit for bit."""
    from xvit.optim import FusedAdam
    ps_a = _params()
    ps_b = _clones(ps_a)
    gs = _grads(ps_a, 5)
    a = FusedAdam(ps_a, weight_decay=wd, max_grad_norm=10 * max(_norm64(g) for g in gs), **HYPER)
    b = FusedAdam(ps_b, weight_decay=wd, **HYPER)
    for step in range(5):
        _set_grads(ps_a, gs[step]); _set_grads(ps_b, gs[step])
        if step == 3:
            ps_a[2].grad = None; ps_b[2].grad = None
        a.step(); b.step()
    assert b.last_grad_norm is None
    _equal_state(a, ps_a, b, ps_b)


@pytest.mark.parametrize("max_grad_norm", [None, "third"])
def test_capturable_eager_matches_torch_and_a_captured_step_replays_bit_identically(max_grad_norm):
    from xvit.optim import FusedAdam
    ps0 = _params()
    gs = _grads(ps0, 5)
    if max_grad_norm == "third":
        max_grad_norm = _norm64(gs[0]) / 3
    # five eager steps in capturable mode against torch
    ps_a, ps_b = _clones(ps0), _clones(ps0)
    a = FusedAdam(ps_a, weight_decay=0.05, max_grad_norm=max_grad_norm, capturable=True, **HYPER)
    b = torch.optim.Adam(ps_b, weight_decay=0.05, **HYPER)
    for g in gs:
        _set_grads(ps_a, g, static=True); _set_grads(ps_b, g)
        if max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps_b, max_grad_norm)
        a.step(); b.step()
    _close_state(a, ps_a, b, ps_b)
    assert set(_steps_of(a).values()) == {5}
    # the same five steps as ONE captured launch sequence, replayed with new gradients copied into the static .grad buffers
    ps_c = _clones(ps0)
    c = FusedAdam(ps_c, weight_decay=0.05, max_grad_norm=max_grad_norm, capturable=True, **HYPER)
    _set_grads(ps_c, gs[0])
    c.prepare()                                            # allocation and table upload happen here, not in the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.step()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(ps_c, ps0)), "a capture executes nothing"
    for g in gs:
        _set_grads(ps_c, g, static=True)
        graph.replay()
    torch.cuda.synchronize()
    _equal_state(c, ps_c, a, ps_a)
    assert set(_steps_of(c).values()) == {5}               # the device step counter
    if max_grad_norm is not None:
        assert torch.equal(c.last_grad_norm, a.last_grad_norm)


def test_scheduler_drives_a_captured_step_and_sync_lr_copies_only_changes():
    from xvit.optim import FusedAdam
    ps0 = _params()
    gs = _grads(ps0, 6)
    ps_a, ps_b = _clones(ps0), _clones(ps0)
    a = FusedAdam(ps_a, capturable=True, **HYPER)
    b = torch.optim.Adam(ps_b, **HYPER)
    sa = torch.optim.lr_scheduler.CosineAnnealingLR(a, T_max=4, eta_min=1e-6)
    sb = torch.optim.lr_scheduler.CosineAnnealingLR(b, T_max=4, eta_min=1e-6)
    _set_grads(ps_a, gs[0])
    a.prepare()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.step()
    assert a.lr_copies == 0
    lrs = []
    for g in gs:
        _set_grads(ps_a, g, static=True); _set_grads(ps_b, g)
        a.sync_lr()
        graph.replay()
        b.step()
        lrs.append(a.param_groups[0]["lr"])
        sa.step(); sb.step()
        assert a.param_groups[0]["lr"] == pytest.approx(b.param_groups[0]["lr"], rel=1e-12)
    torch.cuda.synchronize()
    assert lrs[0] == 3e-3 and lrs[4] == pytest.approx(1e-6) and lrs[2] == pytest.approx((3e-3 + 1e-6) / 2, rel=1e-6)
    changes = sum(x != y for x, y in zip(lrs, lrs[1:]))
    assert changes == 5 and a.lr_copies == changes         # one write per change; the first replay ran at the rate the tables were built with
    _close_state(a, ps_a, b, ps_b)
    # no change, no copy
    a.sync_lr()                                            # the scheduler stepped once more after the last replay
    n = a.lr_copies
    a.sync_lr(); a.sync_lr()
    assert a.lr_copies == n


def test_skip_nonfinite_leaves_everything_untouched_and_counts():
    from xvit.optim import FusedAdam
    ps0 = _params()
    gs = _grads(ps0, 2)
    bad = [g.clone() for g in gs[1]]
    bad[4][0, 7, 3] = float("inf")
    ps_a, ps_b = _clones(ps0), _clones(ps0)
    a = FusedAdam(ps_a, weight_decay=0.05, capturable=True, skip_nonfinite=True, **HYPER)
    b = FusedAdam(ps_b, weight_decay=0.05, capturable=True, skip_nonfinite=True, **HYPER)    # never sees the bad step
    _set_grads(ps_a, gs[0]); a.step()
    _set_grads(ps_b, gs[0]); b.step()
    snap = ([p.detach().clone() for p in ps_a], [a.state[p]["exp_avg"].clone() for p in ps_a], [a.state[p]["exp_avg_sq"].clone() for p in ps_a])
    _set_grads(ps_a, bad, static=True); a.step()
    assert int(a.skipped_steps) == 1 and not torch.isfinite(a.last_grad_norm)
    assert set(_steps_of(a).values()) == {1}
    for p, p0, m0, v0 in zip(ps_a, *snap):
        assert torch.equal(p, p0) and torch.equal(a.state[p]["exp_avg"], m0) and torch.equal(a.state[p]["exp_avg_sq"], v0)
    _set_grads(ps_a, gs[1], static=True); a.step()
    _set_grads(ps_b, gs[1], static=True); b.step()
    _equal_state(a, ps_a, b, ps_b)
    assert set(_steps_of(a).values()) == {2} and int(a.skipped_steps) == 1 and int(b.skipped_steps) == 0
    assert torch.isfinite(a.last_grad_norm) and all(torch.isfinite(p).all() for p in ps_a)


@pytest.mark.parametrize("kind", ["eager-clip", "capturable", "capturable-clip"])
def test_nonfinite_gradient_without_skip_gives_what_torch_gives(kind):
    from xvit.optim import FusedAdam
    ps0 = _params()
    gs = _grads(ps0, 2)
    gs[1][4][0, 7, 3] = float("inf")
    clip = 1.0 if "clip" in kind else None
    ps_a, ps_b = _clones(ps0), _clones(ps0)
    a = FusedAdam(ps_a, max_grad_norm=clip, capturable=kind.startswith("capturable"), **HYPER)
    b = torch.optim.Adam(ps_b, **HYPER)
    for g in gs:
        _set_grads(ps_a, g, static=True); _set_grads(ps_b, g)
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(ps_b, clip)
        a.step(); b.step()
    torch.cuda.synchronize()                               # no crash
    assert not torch.isfinite(ps_b[4]).all() and not torch.isfinite(ps_a[4]).all()
    for pa, pb in zip(ps_a, ps_b):
        fa, fb = torch.isfinite(pa), torch.isfinite(pb)
        assert torch.equal(fa, fb)
        assert rel(torch.where(fa, pa, 0), torch.where(fb, pb, 0)) < P_GATE


def test_capturable_refuses_a_moved_gradient_and_names_the_parameter():
    from xvit.optim import FusedAdam
    ps = _params()
    gs = _grads(ps, 1)[0]
    opt = FusedAdam(ps, capturable=True, **HYPER)
    _set_grads(ps, gs)
    opt.step()
    before = [p.detach().clone() for p in ps]
    ps[1].grad = ps[1].grad.clone()                        # what zero_grad(set_to_none=True) + backward does
    with pytest.raises(RuntimeError, match=r"gradient of parameter 1 of group 0.*set_to_none=False"):
        opt.step()
    ps[1].grad = None
    with pytest.raises(RuntimeError, match=r"gradient of parameter 1 of group 0"):
        opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(ps, before))     # refused before any launch
    _set_grads(ps, gs)
    named = FusedAdam([{"params": ps, "param_names": [f"w{i}" for i in range(len(ps))]}], capturable=True, **HYPER)
    named.step()
    ps[5].grad = ps[5].grad.clone()
    with pytest.raises(RuntimeError, match=r"parameter 5 of group 0 \(w5\)"):
        named.step()


MODES = {"eager-clip": dict(max_grad_norm=40.0), "capturable-clip": dict(max_grad_norm=40.0, capturable=True)}


@pytest.mark.parametrize("saved", list(MODES))
@pytest.mark.parametrize("loaded", list(MODES))
def test_state_dict_round_trip_within_and_across_modes(saved, loaded):
    """Save after 3 steps, load into a fresh optimizer, continue 2 steps: bit-identical to the uninterrupted run of the same mode; across
    modes (whose bias corrections are computed by different pow implementations, host and device) at the project's optimizer gates."""
    from xvit.optim import FusedAdam
    ps0 = _params()
    gs = _grads(ps0, 5)

    def run(mode, ps, grads, opt=None):
        opt = opt or FusedAdam(ps, weight_decay=0.05, **MODES[mode], **HYPER)
        for g in grads:
            _set_grads(ps, g, static=True)
            opt.step()
        return opt

    ps_full = _clones(ps0)
    full = run(loaded, ps_full, gs)                        # uninterrupted, in the mode that continues
    ps_a = _clones(ps0)
    a = run(saved, ps_a, gs[:3])
    sd = copy.deepcopy(a.state_dict())
    assert {int(v["step"]) for v in sd["state"].values()} == {3}
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    ps_b = _clones(ps_a)
    b = FusedAdam(ps_b, weight_decay=0.05, **MODES[loaded], **HYPER)
    b.load_state_dict(sd)
    run(loaded, ps_b, gs[3:], b)
    assert set(_steps_of(b).values()) == {5}
    if saved == loaded:
        _equal_state(b, ps_b, full, ps_full)
    else:
        _close_state(b, ps_b, full, ps_full)


def test_load_state_dict_copies_into_the_buffers_a_capture_holds():
    from xvit.optim import FusedAdam
    ps0 = _params()
    gs = _grads(ps0, 5)
    kw = dict(weight_decay=0.05, max_grad_norm=40.0, capturable=True, **HYPER)
    ps_a = _clones(ps0)
    a = FusedAdam(ps_a, **kw)
    for g in gs[:3]:
        _set_grads(ps_a, g, static=True); a.step()
    sd = copy.deepcopy(a.state_dict())
    after3 = [p.detach().clone() for p in ps_a]
    for g in gs[3:]:
        _set_grads(ps_a, g, static=True); a.step()
    # an optimizer with a captured step, somewhere else in its training: load, then replay
    ps_b = _clones(ps0)
    b = FusedAdam(ps_b, **kw)
    _set_grads(ps_b, gs[4])
    b.step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.step()
    ptrs = [(b.state[p]["exp_avg"].data_ptr(), b.state[p]["exp_avg_sq"].data_ptr()) for p in ps_b]
    b.load_state_dict(sd)
    assert ptrs == [(b.state[p]["exp_avg"].data_ptr(), b.state[p]["exp_avg_sq"].data_ptr()) for p in ps_b]
    with torch.no_grad():
        for p, q in zip(ps_b, after3):
            p.copy_(q)
    for g in gs[3:]:
        _set_grads(ps_b, g, static=True)
        graph.replay()
    torch.cuda.synchronize()
    _equal_state(b, ps_b, a, ps_a)
    assert set(_steps_of(b).values()) == {5}
