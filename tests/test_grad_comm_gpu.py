"""GPU: the bf16 wire format of the gradient reducer.

Kernels (csrc/grad_comm.hip): pack and unpack are bit-identical to the torch casts (CPU, IEEE) on random data, exact rounding ties,
+-0, subnormals, +-Inf, with scale != 1 and from 8 to millions of elements; NaN stays NaN.  A pack of more segments than one launch
holds, laid out in the reducer's 64-element (256-byte) slots, equals the table-free pack of the assembled fp32 buffer, padding zeroed.

Reducer (xvit/ddp.py, 1-rank RCCL group on this box, AVG over one rank is the identity): with XVIT_DETERMINISTIC gradients, every
p.grad of the bf16 reducer is the fp32 reducer's gradient rounded through bf16, bit for bit, eager and in the captured step; p.grad
are the fp32 bucket views; three FusedAdam steps in both formats stay within a stated distance.  Where >= 2 GPUs are visible: two
RCCL ranks end with identical parameters and bf16-reduced gradients close to the fp32-reduced ones."""
import os
import socket
import subprocess
import sys

import pytest
import torch

import ref_cpu as R
from _util import dev, note

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _assert_bf16_equal(got, want, what=""):
    """bit equality, except that a NaN only has to stay a NaN (its payload is not part of the contract)"""
    got, want = got.detach().cpu(), want.detach().cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), what


def _assert_f32_equal(got, want, what=""):
    got, want = got.detach().cpu(), want.detach().cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    assert torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan]), what


def _pack_one(x, scale, fill=0x7F7F):
    """single-segment pack of fp32 CPU data; the destination starts as garbage so the padding has to be written"""
    from xvit import ops
    slot = (x.numel() + 63) // 64 * 64
    dst = torch.full((slot,), fill, dtype=torch.int16, device=dev()).view(torch.bfloat16)
    ops.grad_pack_bf16([(x.to(dev()), 0)], dst, scale)
    torch.cuda.synchronize()
    return dst.cpu()


def _specials():
    f = lambda *bits: torch.tensor(list(bits), dtype=torch.int64).to(torch.int32).view(torch.float32)   # noqa: E731
    ties = []
    for b in (0x3F80, 0x3F81, 0x4049, 0xC049, 0x0001, 0x0080, 0x7F7E, 0x7F7F):   # bf16 patterns; b << 16 | 0x8000 sits exactly half-way
        ties += [(b << 16) | 0x8000, (b << 16) | 0x7FFF, (b << 16) | 0x8001]
    edges = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000, 0x00400000,  # +-0, subnormals
             0x00800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0xFFFFFFFF,              # +-Inf, NaNs
             0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF]                                                              # overflow to Inf
    return torch.cat([f(*ties), f(*edges)])


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0, 0.125, 3.0])
def test_pack_bit_exact_specials_ties_and_scale(scale):
    x = _specials()
    x = torch.cat([x, -x, torch.randn(37, generator=torch.Generator().manual_seed(1)) * 1e-39])   # odd total: a scalar tail
    got = _pack_one(x, scale)
    _assert_bf16_equal(got[:x.numel()], (x * scale).to(torch.bfloat16), f"scale {scale}")
    u = (x * scale).view(torch.int32).long() & 0xFFFFFFFF                  # independent RNE on the bits (NaNs excluded by the helper)
    rne = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).to(torch.int32).to(torch.int16).view(torch.bfloat16)
    _assert_bf16_equal(got[:x.numel()][~torch.isnan(x)], rne[~torch.isnan(x)], f"scale {scale}, integer RNE")
    assert torch.equal(_bits(got[x.numel():]), torch.zeros(got.numel() - x.numel(), dtype=torch.int16))     # +0 padding
    assert torch.isnan(got[:x.numel()]).sum() == torch.isnan(x * scale).sum() > 0


@pytest.mark.parametrize("n", [8, 13, 64, 65, 1000, 8191, 8193, 123457, 3_000_017])
def test_pack_bit_exact_random_sizes(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 30, (n,), generator=g).float())
    for scale in (1.0, 0.25 + 1e-3):
        got = _pack_one(x, scale)
        assert torch.equal(_bits(got[:n]), _bits((x * scale).to(torch.bfloat16))), (n, scale)
        assert not _bits(got[n:]).any()


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0, 7.0])
def test_unpack_bit_exact_every_bf16_pattern(scale):
    from xvit import ops
    b = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)          # all 65536 bf16 values
    for n in (8, 13, 65536, 65536 - 3):
        src = b[:n].to(dev())
        out = torch.full((n,), float("nan"), device=dev())
        ops.grad_unpack_bf16(src, out, scale)
        torch.cuda.synchronize()
        _assert_f32_equal(out, b[:n].float() * scale, (n, scale))


def test_unpack_bit_exact_large():
    from xvit import ops
    n = 5_000_011
    b = torch.randint(-32768, 32768, (n,), generator=torch.Generator().manual_seed(5), dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    out = torch.empty(n, device=dev())
    ops.grad_unpack_bf16(b.to(dev()), out, 0.5)
    torch.cuda.synchronize()
    _assert_f32_equal(out, b.float() * 0.5)


def test_multi_segment_pack_equals_table_free_pack():
    """More segments than one launch holds (3 launches), at the reducer's slots: some sources are the bucket's own fp32 views (what the
    GRAD_SINK kernels write), the others separate tensors (1-D p.grad).  Result == one single-segment pack of the assembled fp32 bucket
    == the torch cast, slot padding zeroed."""
    from xvit import _lib, ops
    sizes = [1, 7, 8, 63, 64, 65, 768, 3, 3072, 2304, 100_003, 5, 589_824, 16, 17, 1000] * 5
    assert len(sizes) > 2 * _lib.GRAD_PACK_MAX_SEGMENTS
    g = torch.Generator().manual_seed(11)
    offs, o = [], 0
    for n in sizes:
        offs.append(o)
        o += (n + 63) // 64 * 64
    flat = torch.zeros(o, device=dev())
    segs = []
    for i, (n, off) in enumerate(zip(sizes, offs)):
        x = (torch.randn(n, generator=g) * 10.0 ** (i % 7 - 3)).to(dev())
        if i % 3 == 0:                                                 # a "GRAD_SINK" gradient: already in its view
            flat[off:off + n] = x
            segs.append((flat[off:off + n], off))
        else:
            segs.append((x, off))
    assembled = torch.zeros_like(flat)
    for (x, off), n in zip(segs, sizes):
        assembled[off:off + n] = x
    scale = 1.0 / 8
    wire = torch.full((o,), 0x5555, dtype=torch.int16, device=dev()).view(torch.bfloat16)
    ops.grad_pack_bf16(segs, wire, scale)
    ref = torch.full((o,), 0x5555, dtype=torch.int16, device=dev()).view(torch.bfloat16)
    ops.grad_pack_bf16([(assembled, 0)], ref, scale)
    torch.cuda.synchronize()
    assert torch.equal(_bits(wire), _bits(ref))
    assert torch.equal(_bits(wire), _bits((assembled.cpu() * scale).to(torch.bfloat16)))        # padding: assembled is 0 there -> +0


# ---- the reducer on a 1-rank RCCL group --------------------------------------------------------------------------------------

def _grads(model, img, labels, reducer):
    for p in model.parameters():
        p.grad = None
    _, loss = model(img, labels)
    loss.backward()
    reducer.finish()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.fixture
def rccl1(monkeypatch):
    import torch.distributed as dist
    from xvit import ops
    monkeypatch.setattr(ops, "DETERMINISTIC", True)        # XVIT_DETERMINISTIC=1: every gradient bit-reproducible run to run
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_free_port()))
    monkeypatch.delenv("XVIT_GRAD_COMM", raising=False)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev())
    try:
        yield
    finally:
        dist.destroy_process_group()


def _tiny_model():
    import xvit
    cfg = R.make_config("tiny")
    model = xvit.ModelCross(cfg).to(dev())
    model.load_state_dict(R.make_state_dict(cfg, seed=0))
    model.train()
    ins = [tuple(t.to(dev()) for t in R.make_inputs(cfg, 4, seed=s)) for s in (3, 8)]
    return model, ins


def _rt(t):
    return t.to(torch.bfloat16).float()


def test_bf16_reducer_eager_equals_rounded_fp32_one_rank(rccl1):
    import xvit.functional as XF
    from xvit.ddp import BucketedGradReducer
    model, ins = _tiny_model()
    for sink in (False, True):                     # 1-D AND 2-D p.grad outside the buckets / weight gradients written into the views
        red32 = BucketedGradReducer(list(model.parameters()), bucket_bytes=64 << 10, comm_dtype=torch.float32)
        XF.GRAD_SINK = red32.grad_sink(model) if sink else None
        try:
            want = [_grads(model, *i, red32) for i in ins]
        finally:
            XF.GRAD_SINK = None
            red32.remove()
        red16 = BucketedGradReducer(list(model.parameters()), bucket_bytes=64 << 10, comm_dtype=torch.bfloat16)
        assert len(red16.buckets) >= 4 and max(len(b.params) for b in red16.buckets) > 1
        XF.GRAD_SINK = red16.grad_sink(model) if sink else None
        try:
            for which in (0, 1, 0):
                got = _grads(model, *ins[which], red16)
                for k, p in model.named_parameters():
                    assert p.grad.data_ptr() == red16._view_of[id(p)].data_ptr() and p.grad.dtype == torch.float32, k
                    assert torch.equal(got[k], _rt(want[which][k])), (sink, which, k)
        finally:
            XF.GRAD_SINK = None
            red16.remove()


def test_bf16_reducer_graphed_step_equals_eager_one_rank(rccl1):
    """The pack, the collective and the unpack are captured as nodes on the comm-stream fork and joined before the graph ends: the
    replayed gradients equal the eager bf16 reducer's bit for bit, across two replays with new inputs."""
    import xvit.functional as XF
    from xvit.ddp import BucketedGradReducer
    from xvit.graph import GraphedStep
    model, ins = _tiny_model()
    red = BucketedGradReducer(list(model.parameters()), bucket_bytes=64 << 10, comm_dtype=torch.bfloat16)
    XF.GRAD_SINK = red.grad_sink(model)
    try:
        eager = [_grads(model, *i, red) for i in ins]
    finally:
        XF.GRAD_SINK = None
    assert any(not torch.equal(eager[0][k], eager[1][k]) for k in eager[0])
    step = GraphedStep(model, *ins[0], reducer=red)
    for which in (1, 0, 1):
        step(*ins[which])
        torch.cuda.synchronize()
        for k, p in model.named_parameters():
            assert p.grad.data_ptr() == red._view_of[id(p)].data_ptr(), k
            assert torch.equal(p.grad, eager[which][k]), (which, k)
    red.remove()


ADAM_GAP = 2e-2      # || dtheta_bf16 - dtheta_fp32 || / || dtheta_fp32 || after three FusedAdam steps (measured on the MI355X: 5.3e-3)


def test_fused_adam_three_steps_bf16_vs_fp32_one_rank(rccl1):
    import xvit.functional as XF
    from xvit.ddp import BucketedGradReducer
    from xvit.optim import FusedAdam
    model, ins = _tiny_model()
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    final = {}
    for dt in (torch.float32, torch.bfloat16):
        model.load_state_dict(start)
        red = BucketedGradReducer(list(model.parameters()), bucket_bytes=64 << 10, comm_dtype=dt)
        opt = FusedAdam(model.parameters(), lr=1e-3)
        XF.GRAD_SINK = red.grad_sink(model)
        try:
            for s in range(3):
                _grads(model, *ins[s % 2], red)
                opt.step()
            torch.cuda.synchronize()
        finally:
            XF.GRAD_SINK = None
            red.remove()
        final[dt] = {k: p.detach().clone() for k, p in model.named_parameters()}
    d32 = torch.cat([(final[torch.float32][k] - start[k]).flatten() for k in final[torch.float32]]).double()
    d16 = torch.cat([(final[torch.bfloat16][k] - start[k]).flatten() for k in final[torch.bfloat16]]).double()
    gap = float((d16 - d32).norm() / d32.norm())
    note("fused_adam_3_steps_bf16_vs_fp32_rel", gap)
    print(f"FusedAdam, 3 steps: ||dtheta_bf16 - dtheta_fp32|| / ||dtheta_fp32|| = {gap:.3e}")
    assert 0.0 < gap < ADAM_GAP, gap


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs >= 2 GPUs")
def test_bf16_reducer_two_rccl_ranks(tmp_path):
    """Element by element, the bf16-reduced mean m16 of the two ranks' gradients g0, g1 is within the bf16_compress_hook bound of the
    fp32-reduced m32: one rounding of each rank's share (2^-8 (|g0| + |g1|) / 2) and one of the sum (2^-8 |m16|), plus fp32 slack."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "XVIT_GRAD_COMM")}
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "_ddp_bf16_worker.py"), str(tmp_path), "4"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "rccl ranks: 2" in r.stdout
    w0, w1 = torch.load(tmp_path / "w0.pt"), torch.load(tmp_path / "w1.pt")
    worst = 0.0
    for k in w0["g32"]:
        assert torch.equal(w0["l16"][k], w0["l32"][k]) and torch.equal(w1["l16"][k], w1["l32"][k]), k   # the same local gradients in both runs
        assert torch.equal(w0["g16"][k], w1["g16"][k]) and torch.equal(w0["g32"][k], w1["g32"][k]), k   # the same bits on every rank
        m16, m32 = w0["g16"][k].double(), w0["g32"][k].double()
        share = (w0["l16"][k].double().abs() + w1["l16"][k].double().abs()) / 2
        bound = 2.0 ** -8 * share * (1 + 2.0 ** -8) + 2.0 ** -8 * m16.abs() + 1e-6 * share + 1e-38
        assert ((m16 - m32).abs() <= bound).all(), (k, float(((m16 - m32).abs() - bound).max()))
        if float(m32.abs().max()) > 1e-6:
            worst = max(worst, float((m16 - m32).norm() / m32.norm()))
    note("two_rank_bf16_vs_fp32_grad_rel_worst", worst)
    print(f"two ranks: worst per-tensor ||m16 - m32|| / ||m32|| = {worst:.3e}")
    for k in w0["params"]:
        assert torch.equal(w0["params"][k], w1["params"][k]), k           # replicas stay in lock-step through 3 Adam steps
