"""GPU: WHICH launches FusedAdam and FusedAdamW issue, in what order and over how many chunks / partials, and where parameters of one
group at different step counts are accepted.  The numerics are checked elsewhere (test_optim_edges_gpu.py, test_adamw_kernels_gpu.py and
the model-level optimizer tests); here the library handle is wrapped in a proxy that calls through and logs (entry point, n_chunks), or
(entry point, n_partials) for the prologue.  Three fp32 parameters of 8, 20000 and 4 elements: 1 + 2 + 1 chunks of 16384 elements, in two
groups [8, 20000] and [4]."""
import pytest
import torch

from _util import dev
from xvit import _lib
from xvit.optim import CHUNK, FusedAdam, FusedAdamW

pytestmark = pytest.mark.gpu

SIZES = (8, 20000, 4)
COUNT_ARG = {"xvit_adam_step": 2, "xvit_adam_step_dev": 2, "xvit_grad_sqnorm_partials": 2, "xvit_adam_prologue": 1, "xvit_adamw_step": 3,
             "xvit_adamw_step_dev": 3, "xvit_ema_swap": 3}          # position of n_chunks (n_partials) in the C signature
STEP, STEP_DEV, NORM, PROLOGUE = "xvit_adam_step", "xvit_adam_step_dev", "xvit_grad_sqnorm_partials", "xvit_adam_prologue"
WSTEP, WSTEP_DEV, SWAP = "xvit_adamw_step", "xvit_adamw_step_dev", "xvit_ema_swap"


class _Recorder:
    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in COUNT_ARG:
            return fn

        def call(*args):
            self._log.append((name, args[COUNT_ARG[name]]))
            return fn(*args)
        return call


@pytest.fixture
def log(monkeypatch):
    assert CHUNK == 16384
    out, real = [], _lib.load()
    monkeypatch.setattr(_lib, "load", lambda: _Recorder(real, out))
    return out


def _params(sizes=SIZES):
    g = torch.Generator(device="cpu").manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g).to(dev())) for n in sizes]
    return ps, [p.detach().clone() for p in ps]


def _set_grads(ps, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(dev())


def _groups(ps, **second):
    return [dict(params=ps[:2]), dict(params=ps[2:], **second)]


def _taken(log):
    out = list(log)
    del log[:]
    return out


def _moved(ps, start):
    for p, p0 in zip(ps, start):
        assert torch.isfinite(p).all() and not torch.equal(p, p0)


NORM_THEN_PAIRS = [(NORM, 3), (NORM, 1), (PROLOGUE, 4), (STEP_DEV, 3), (PROLOGUE, 4), (STEP_DEV, 1)]


@pytest.mark.parametrize("kw, expected", [
    (dict(), [(STEP, 3), (STEP, 1)]),
    (dict(max_grad_norm=1.0), NORM_THEN_PAIRS),
], ids=["plain", "max_grad_norm"])
def test_fused_adam_eager(log, kw, expected):
    ps, start = _params()
    _set_grads(ps)
    FusedAdam(_groups(ps), lr=1e-2, **kw).step()
    assert _taken(log) == expected
    _moved(ps, start)


def test_fused_adam_eager_splits_a_group_by_step_count(log):
    ps, start = _params()
    _set_grads(ps)
    ps[1].grad = None
    opt = FusedAdam(_groups(ps), lr=1e-2)
    opt.step()
    assert _taken(log) == [(STEP, 1), (STEP, 1)]
    _set_grads(ps, seed=2)
    opt.step()
    assert _taken(log) == [(STEP, 1), (STEP, 2), (STEP, 1)]        # group 0: the 8 elements at step 2, then the 20000 at step 1; group 1
    _moved(ps, start)


@pytest.mark.parametrize("kw, expected", [
    (dict(), [(PROLOGUE, 0), (STEP_DEV, 3), (PROLOGUE, 0), (STEP_DEV, 1)]),
    (dict(skip_nonfinite=True), NORM_THEN_PAIRS),
], ids=["no norm", "skip_nonfinite"])
def test_fused_adam_capturable(log, kw, expected):
    ps, start = _params()
    _set_grads(ps)
    opt = FusedAdam(_groups(ps), lr=1e-2, capturable=True, **kw)
    for _ in range(2):
        opt.step()
        assert _taken(log) == expected
    _moved(ps, start)


@pytest.mark.parametrize("kw, second, expected", [
    (dict(), dict(), [(WSTEP, 4)]),
    (dict(max_grad_norm=1.0), dict(), [(NORM, 4), (PROLOGUE, 4), (WSTEP_DEV, 4)]),
    (dict(), dict(betas=(0.8, 0.9)), [(WSTEP, 3), (WSTEP, 1)]),
], ids=["one set", "one set, max_grad_norm", "two sets"])
def test_fused_adamw_eager(log, kw, second, expected):
    ps, start = _params()
    _set_grads(ps)
    FusedAdamW(_groups(ps, **second), lr=1e-2, **kw).step()
    assert _taken(log) == expected
    _moved(ps, start)


def test_fused_adamw_capturable_with_an_average_and_its_exchange(log):
    ps, start = _params()
    _set_grads(ps)
    opt = FusedAdamW(_groups(ps), lr=1e-2, ema_decay=0.9, capturable=True)
    for _ in range(2):
        opt.step()
        assert _taken(log) == [(PROLOGUE, 0), (WSTEP_DEV, 4)]
    with opt.ema_weights():
        assert _taken(log) == [(SWAP, 4)]
    assert _taken(log) == [(SWAP, 4)]
    _moved(ps, start)


def test_mixed_step_counts_in_one_group(log):
    ps, _ = _params(SIZES[:2])
    _set_grads(ps)
    ps[1].grad = None
    eager = FusedAdam(ps, lr=1e-2)
    eager.step()
    _set_grads(ps, seed=2)
    eager.step()
    sd = eager.state_dict()
    assert {k: v["step"] for k, v in sd["state"].items()} == {0: 2, 1: 1}

    one_per_group = FusedAdam(ps, lr=1e-2, capturable=True)
    one_per_group.load_state_dict(sd)
    with pytest.raises(ValueError, match="one step count per parameter group"):
        one_per_group.prepare()

    by_step = FusedAdamW(ps, lr=1e-2, capturable=True)
    by_step.load_state_dict(sd)
    assert by_step.launch_sets == 2
    del log[:]
    by_step.step()
    assert _taken(log) == [(PROLOGUE, 0), (WSTEP_DEV, 1), (PROLOGUE, 0), (WSTEP_DEV, 2)]
    assert by_step.launch_sets == 2
    assert {k: v["step"] for k, v in by_step.state_dict()["state"].items()} == {0: 3, 1: 2}
