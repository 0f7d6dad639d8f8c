"""CPU, one gloo rank: the gradient reducer (xvit/ddp.py) over MORE than one step, in the patterns a training loop really uses.

The forward is a stand-in autograd.Function whose backward takes the destination of its weight gradient from
xvit.functional._grad_out, the product's contract with its weight-gradient kernels.  The reference is plain autograd on the same
inputs with no reducer and no sink.  With one rank the mean is the identity (the 1/world scale is 1.0), so every comparison is
torch.equal; for the bf16 wire the reference is the stated rounding rule applied here: bf16(g) after a first step,
bf16(bf16(g1) + g2) after an accumulating one.

Covered: gradients kept and zeroed in place (optimizer.zero_grad(set_to_none=False)), accumulation over two backward + finish()
rounds, the fast path (red.zero_grad(): the weight gradient IS the bucket view, nothing is copied), the refusal of a second backward
without finish(), and the event bookkeeping (empty on the CPU, the twin of tests/test_ddp_lifecycle_gpu.py)."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-attention-vit_amd"))

OUT, IN, BATCH = 8, 16, 4
WIRES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture
def gloo1(monkeypatch):
    import xvit.functional as XF
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_free_port()))
    monkeypatch.delenv("XVIT_GRAD_COMM", raising=False)
    monkeypatch.setattr(XF, "GRAD_SINK", None)             # whatever a test assigns is dropped again
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


class _SinkLinear(torch.autograd.Function):
    """y = x w^T + b; backward writes dW = dy^T x where _grad_out says, like the HIP weight-gradient kernels do"""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return x @ w.t() + b

    @staticmethod
    def backward(ctx, dy):
        import xvit.functional as XF
        x, w = ctx.saved_tensors
        dw = XF._grad_out(w, tuple(w.shape), w.device)
        torch.mm(dy.t(), x, out=dw)
        return None, dw, dy.sum(0)


def _params():
    g = torch.Generator().manual_seed(0)
    return torch.nn.Parameter(torch.randn(OUT, IN, generator=g)), torch.nn.Parameter(torch.randn(OUT, generator=g))


def _inputs(step):
    g = torch.Generator().manual_seed(100 + step)
    return torch.randn(BATCH, IN, generator=g), torch.randn(BATCH, OUT, generator=g)


def _backward(w, b, step):
    x, t = _inputs(step)
    ((_SinkLinear.apply(x, w, b) - t) ** 2).sum().backward()


_REF = {}


def _ref(step):
    """(dW, db) of step `step` by plain autograd: no reducer, no sink.  Computed once, shared, never modified."""
    import xvit.functional as XF
    if step not in _REF:
        assert XF.GRAD_SINK is None
        w, b = _params()
        _backward(w, b, step)
        _REF[step] = (w.grad.clone(), b.grad.clone())
    return _REF[step]


def _rt(t):
    return t.to(torch.bfloat16).float()


def _reducer(w, b, sink, wire, extra=()):
    import xvit.functional as XF
    from xvit.ddp import BucketedGradReducer
    red = BucketedGradReducer([w, b, *extra], bucket_bytes=1 << 20, comm_dtype=WIRES[wire])
    assert len(red.buckets) == 1 and len(red.buckets[0].params) == 2 + len(extra)
    XF.GRAD_SINK = red.grad_sink() if sink else None
    return red


def _events_empty(red):
    return all(len(bk.events) == 0 for bk in red.buckets)


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
@pytest.mark.parametrize("sink", [False, True], ids=["nosink", "sink"])
def test_kept_gradients_zeroed_in_place(gloo1, sink, wire):
    """optimizer.zero_grad(set_to_none=False) between steps: every step's gradients equal the reference's.  Before the sink withheld the
    view of a parameter that has a .grad, the sink arms gave w.grad == 2 * dW from the second step on (AccumulateGrad added the view to
    itself); b.grad was right."""
    w, b = _params()
    red = _reducer(w, b, sink, wire)
    for step in range(3):
        _backward(w, b, step)
        red.finish()
        dw, db = _ref(step)
        if wire == "bf16":
            dw, db = _rt(dw), _rt(db)
        assert torch.equal(b.grad, db), (step, "bias")
        assert torch.equal(w.grad, dw), (step, "weight", float((w.grad / dw).mean()))
        assert _events_empty(red)
        w.grad.zero_(); b.grad.zero_()
    red.remove()


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
@pytest.mark.parametrize("sink", [False, True], ids=["nosink", "sink"])
def test_accumulation_over_two_rounds(gloo1, sink, wire):
    """Two backward + finish() rounds, nothing zeroed: p.grad == g1 + g2 (fp32 wire; the fp32 add plain autograd does), or
    bf16(bf16(g1) + g2) (bf16 wire: the first round's result is what the second adds to, and each round is rounded once on the wire).
    Before the fix the sink arms gave w.grad == 2 * g2."""
    w, b = _params()
    red = _reducer(w, b, sink, wire)
    for step in range(2):
        _backward(w, b, step)
        red.finish()
        assert _events_empty(red)
    (dw1, db1), (dw2, db2) = _ref(0), _ref(1)
    if wire == "fp32":
        want_w, want_b = dw1 + dw2, db1 + db2
    else:
        want_w, want_b = _rt(_rt(dw1) + dw2), _rt(_rt(db1) + db2)
    assert torch.equal(b.grad, want_b)
    assert torch.equal(w.grad, want_w), f"w.grad == 2 * g2: {torch.equal(w.grad, 2 * dw2) or torch.equal(w.grad, _rt(2 * dw2))}"
    red.remove()


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_fast_path_weight_gradient_is_the_bucket_view(gloo1, wire, monkeypatch):
    """red.zero_grad() between steps (p.grad is None before backward): the kernel writes into the bucket view, autograd hands that very
    tensor on, and the pack copies no 2-D gradient (fp32 wire; the CPU bf16 pack is a cast of every gradient into the wire buffer)."""
    w, b = _params()
    red = _reducer(w, b, True, wire)
    view = red._view_of[id(w)]
    copied = []
    real = torch._foreach_copy_
    monkeypatch.setattr(torch, "_foreach_copy_", lambda dsts, srcs, *a, **k: (copied.extend(srcs), real(dsts, srcs, *a, **k))[1])
    for step in range(3):
        red.zero_grad()
        assert w.grad is None and b.grad is None
        _backward(w, b, step)
        assert w.grad.data_ptr() == view.data_ptr()        # already there before finish(): written by the "kernel", not packed
        red.finish()
        dw, db = _ref(step)
        if wire == "bf16":
            dw, db = _rt(dw), _rt(db)
        assert w.grad.data_ptr() == view.data_ptr() and b.grad.data_ptr() == red._view_of[id(b)].data_ptr()
        assert torch.equal(w.grad, dw) and torch.equal(b.grad, db), step
        assert _events_empty(red)
    if wire == "fp32":
        assert len(copied) == 3 and all(s.dim() == 1 for s in copied), [tuple(s.shape) for s in copied]
    red.remove()


@pytest.mark.parametrize("unused", [False, True], ids=["launched", "pending"])
def test_second_backward_without_finish_is_refused(gloo1, unused):
    """A second backward before finish() used to drive `pending` negative: its gradients were never reduced and nothing said so.
    `launched`: the bucket's all-reduce is already on the wire.  `pending`: a parameter without a gradient keeps the bucket waiting
    for finish(), and the second gradient of the SAME parameter is refused.  After finish() and zero_grad() the reducer works again."""
    w, b = _params()
    extra = (torch.nn.Parameter(torch.ones(5)),) if unused else ()
    red = _reducer(w, b, True, "fp32", extra)
    _backward(w, b, 0)
    assert red.buckets[0].launched is (not unused)
    with pytest.raises(RuntimeError, match=r"finish\(\)"):
        _backward(w, b, 1)
    red.finish()
    red.zero_grad()
    _backward(w, b, 2)
    red.finish()
    dw, db = _ref(2)
    assert torch.equal(w.grad, dw) and torch.equal(b.grad, db)
    assert red.buckets[0].pending == len(red.buckets[0].params) and not red.buckets[0].seen and _events_empty(red)
    if unused:
        assert float(extra[0].grad.abs().max()) == 0.0
    red.remove()
