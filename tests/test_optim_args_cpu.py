"""CPU: the entry points of the capturable Adam (gradient square-norm partials, step prologue, device-argument Adam) validate their
arguments on the host before any launch, and FusedAdam refuses a non-positive max_grad_norm.  Pointers are dummy addresses that are
never dereferenced: callable without a GPU."""
import math

import pytest
import torch


def _lib():
    from xvit import _lib
    return _lib.load()


P = 256   # any non-null "address"


def test_grad_sqnorm_partials_argument_errors_do_not_launch():
    lib = _lib()
    f = lib.xvit_grad_sqnorm_partials
    assert f(None, P, 4, P, None) < 0 and b"xvit_grad_sqnorm_partials" in lib.xvit_last_error_string() and b"null" in lib.xvit_last_error_string()
    assert f(P, None, 4, P, None) < 0 and b"null" in lib.xvit_last_error_string()
    assert f(P, P, 4, None, None) < 0 and b"null" in lib.xvit_last_error_string()
    assert f(P, P, 0, P, None) < 0 and b"n_chunks=0" in lib.xvit_last_error_string()
    assert f(P, P, -3, P, None) < 0 and b"n_chunks=-3" in lib.xvit_last_error_string()


def test_adam_prologue_argument_errors_do_not_launch():
    lib = _lib()
    f = lib.xvit_adam_prologue
    assert f(P, 4, None, 1.0, 0.9, 0.999, 0, None) < 0 and b"xvit_adam_prologue" in lib.xvit_last_error_string() and b"null state" in lib.xvit_last_error_string()
    assert f(P, 0, P, 1.0, 0.9, 0.999, 0, None) < 0 and b"n_partials=0" in lib.xvit_last_error_string()      # partials without a count
    assert f(None, 4, P, 1.0, 0.9, 0.999, 0, None) < 0 and b"n_partials=4" in lib.xvit_last_error_string()    # a count without partials
    assert f(P, -1, P, 1.0, 0.9, 0.999, 0, None) < 0
    assert f(P, 4, P, 0.0, 0.9, 0.999, 0, None) < 0 and b"max_norm" in lib.xvit_last_error_string()
    assert f(P, 4, P, -1.0, 0.9, 0.999, 0, None) < 0 and b"max_norm" in lib.xvit_last_error_string()
    assert f(P, 4, P, math.nan, 0.9, 0.999, 0, None) < 0 and b"max_norm" in lib.xvit_last_error_string()
    assert f(P, 4, P, 1.0, 1.0, 0.999, 0, None) < 0 and b"betas" in lib.xvit_last_error_string()
    assert f(P, 4, P, 1.0, 0.9, 1.0, 0, None) < 0 and b"betas" in lib.xvit_last_error_string()
    assert f(P, 4, P, 1.0, -0.1, 0.999, 0, None) < 0 and b"betas" in lib.xvit_last_error_string()


def test_adam_step_dev_argument_errors_do_not_launch():
    lib = _lib()
    f = lib.xvit_adam_step_dev
    assert f(None, P, 4, P, 0.9, 0.999, 1e-8, 0.0, None) < 0 and b"xvit_adam_step_dev" in lib.xvit_last_error_string() and b"null" in lib.xvit_last_error_string()
    assert f(P, None, 4, P, 0.9, 0.999, 1e-8, 0.0, None) < 0 and b"null" in lib.xvit_last_error_string()
    assert f(P, P, 4, None, 0.9, 0.999, 1e-8, 0.0, None) < 0 and b"null" in lib.xvit_last_error_string()
    assert f(P, P, 0, P, 0.9, 0.999, 1e-8, 0.0, None) < 0 and b"n_chunks=0" in lib.xvit_last_error_string()
    assert f(P, P, 4, P, 1.0, 0.999, 1e-8, 0.0, None) < 0 and b"hyper-parameters" in lib.xvit_last_error_string()
    assert f(P, P, 4, P, 0.9, 1.0, 1e-8, 0.0, None) < 0 and b"hyper-parameters" in lib.xvit_last_error_string()
    assert f(P, P, 4, P, 0.9, 0.999, -1e-8, 0.0, None) < 0 and b"hyper-parameters" in lib.xvit_last_error_string()


def test_state_record_layout_matches_the_header():
    """The Python side addresses struct xvit_adam_state (include/xvit.h) by word: 48 bytes, lr and grad_norm at fp32 words 4 and 5."""
    import os
    import re
    from xvit import optim
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xvit.h")).read()
    body = re.search(r"typedef struct xvit_adam_state \{(.*?)\} xvit_adam_state;", header, re.S).group(1)
    fields = re.findall(r"^\s*(int64_t|int32_t|float)\s+(\w+)(?:\[(\d+)\])?;", body, re.M)
    sizes = {"int64_t": 8, "int32_t": 4, "float": 4}
    offs, o = {}, 0
    for ty, name, n in fields:
        offs[name] = o
        o += sizes[ty] * int(n or 1)
    assert o == 48 == optim._REC_DTYPE.itemsize
    for name in ("step", "skipped", "lr", "grad_norm", "clip_coef", "lr_over_bc1", "inv_sqrt_bc2", "skip"):
        assert optim._REC_DTYPE.fields[name][1] == offs[name], name
    assert offs["lr"] == 4 * optim._F_LR and offs["grad_norm"] == 4 * optim._F_NORM and offs["step"] == 0 and offs["skipped"] == 8


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, math.nan, math.inf])
def test_fused_adam_refuses_a_non_positive_max_grad_norm(bad):
    from xvit.optim import FusedAdam
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam([p], lr=1e-3, max_grad_norm=bad)


def test_fused_adam_new_options_default_off_and_skip_needs_capturable():
    from xvit.optim import FusedAdam
    p = torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdam([p], lr=1e-3)
    assert opt.max_grad_norm is None and opt.capturable is False and opt.skip_nonfinite is False
    assert opt.last_grad_norm is None and opt.skipped_steps is None
    with pytest.raises(ValueError, match="capturable"):
        FusedAdam([p], lr=1e-3, skip_nonfinite=True)
    with pytest.raises(RuntimeError, match="capturable"):
        opt.prepare()


def test_graphed_step_refuses_other_optimizers_before_touching_the_gpu():
    """Anything but FusedAdam(capturable=True) is refused first thing (here: CPU tensors would be the next error, and it is not reached)."""
    from xvit.graph import GraphedStep
    from xvit.optim import FusedAdam
    lin = torch.nn.Linear(4, 2)

    class FakeCuda:
        is_cuda = True
    for opt in (torch.optim.Adam(lin.parameters()), FusedAdam(lin.parameters(), lr=1e-3)):
        with pytest.raises(RuntimeError, match="capturable=True"):
            GraphedStep(lin, FakeCuda(), None, optimizer=opt)
