"""CPU: the bf16 wire format of the bucketed gradient reducer (xvit/ddp.py, comm_dtype=torch.bfloat16) and the host side of its
kernels (csrc/grad_comm.hip).  World size 2 over gloo: every reduced gradient is, bit for bit, float(bf16(bf16(g0/2) + bf16(g1/2)))
of the two ranks' local gradients; the bucket plan is the fp32 one; bad wire formats are refused; the new C entry points are
exported and refuse bad arguments before any launch."""
import ctypes as C
import os
import re
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
from xvit import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _model(seed):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(24, 64), nn.GELU(), nn.LayerNorm(64), nn.Linear(64, 64), nn.GELU(), nn.Linear(64, 3))


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, os.path.join(ROOT, "cross-attention-vit_amd"))
    from xvit.ddp import BucketedGradReducer
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = _model(seed=100 + rank)
    unused = nn.Parameter(torch.ones(5))         # never receives a gradient: its bucket is launched from finish() and reduces zeros
    params = list(model.parameters()) + [unused]
    red = BucketedGradReducer(params, bucket_bytes=1 << 10, comm_dtype=torch.bfloat16)
    assert red.comm_dtype == torch.bfloat16 and len(red.buckets) >= 3
    assert all(b.wire.dtype == torch.bfloat16 and b.wire.numel() == b.flat.numel() for b in red.buckets)
    g = torch.Generator().manual_seed(7 + rank)
    x, y = torch.randn(8, 24, generator=g), torch.randint(0, 3, (8,), generator=g)
    out = {"local": [], "reduced": []}
    for step in range(2):                         # the second step reuses the wire buffers
        red.zero_grad()
        nn.functional.cross_entropy(model(x * (step + 1)), y).backward()
        out["local"].append([p.grad.clone() if p.grad is not None else torch.zeros_like(p) for p in params])
        red.finish()
        out["reduced"].append([p.grad.clone() for p in params])
        assert all(p.grad.data_ptr() == red._view_of[id(p)].data_ptr() for p in params)   # p.grad are the fp32 bucket views
        assert all(p.grad.dtype == torch.float32 for p in params)
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_bf16_reducer_world2_bit_exact(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    bf = lambda t: t.to(torch.bfloat16)           # noqa: E731
    for step in range(2):
        for i, (g0, g1) in enumerate(zip(r0["local"][step], r1["local"][step])):
            want = (bf(g0 / 2) + bf(g1 / 2)).float()
            assert torch.equal(r0["reduced"][step][i], want), (step, i)
            assert torch.equal(r1["reduced"][step][i], want), (step, i)
        assert float(r0["reduced"][step][-1].abs().max()) == 0.0
        # the wire format really is bf16: at least one reduced value differs from the fp32 mean
        assert any(not torch.equal(r, (g0 + g1) / 2) for r, g0, g1 in zip(r0["reduced"][step], r0["local"][step], r1["local"][step]))


@pytest.fixture
def world1_gloo():
    dist.init_process_group("gloo", rank=0, world_size=1, store=dist.HashStore())
    try:
        yield
    finally:
        dist.destroy_process_group()


def test_bucket_plan_is_the_fp32_plan(world1_gloo, monkeypatch):
    from xvit.ddp import BucketedGradReducer
    model = _model(seed=0)
    plans, reds = {}, []
    for dt in (torch.float32, torch.bfloat16):
        red = BucketedGradReducer(list(model.parameters()), bucket_bytes=1 << 10, comm_dtype=dt)
        plans[dt] = [([id(p) for p in b.params], b.offsets, b.flat.numel()) for b in red.buckets]
        reds.append(red)
        red.remove()
    assert plans[torch.float32] == plans[torch.bfloat16] and len(plans[torch.float32]) >= 3
    assert all(b.wire is None and b.done is None for b in reds[0].buckets)   # fp32: no wire buffer, today's path
    assert all(o % 64 == 0 for b in reds[1].buckets for o in b.offsets)
    # the environment default: XVIT_GRAD_COMM (fp32 when unset or empty), an explicit comm_dtype wins
    for env, want in ((None, torch.float32), ("", torch.float32), ("fp32", torch.float32), ("bf16", torch.bfloat16)):
        if env is None:
            monkeypatch.delenv("XVIT_GRAD_COMM", raising=False)
        else:
            monkeypatch.setenv("XVIT_GRAD_COMM", env)
        red = BucketedGradReducer(list(model.parameters()), bucket_bytes=3 << 10)
        red.remove()
        assert red.comm_dtype == want, env
    monkeypatch.setenv("XVIT_GRAD_COMM", "bf16")
    red = BucketedGradReducer(list(model.parameters()), bucket_bytes=3 << 10, comm_dtype=torch.float32)
    red.remove()
    assert red.comm_dtype == torch.float32


@pytest.mark.parametrize("bad", [torch.float16, torch.float64, "bf16", "fp32", 16, torch.int8])
def test_bad_comm_dtype_raises(bad):
    from xvit.ddp import BucketedGradReducer
    with pytest.raises(ValueError, match="comm_dtype"):
        BucketedGradReducer([nn.Parameter(torch.ones(4))], comm_dtype=bad)      # refused before any process-group call


@pytest.mark.parametrize("bad", ["fp16", "BF16", "bfloat16", "1"])
def test_bad_grad_comm_env_raises(bad, monkeypatch):
    from xvit.ddp import BucketedGradReducer
    monkeypatch.setenv("XVIT_GRAD_COMM", bad)
    with pytest.raises(ValueError, match="XVIT_GRAD_COMM"):
        BucketedGradReducer([nn.Parameter(torch.ones(4))])


def test_grad_comm_symbols_in_header_lib_and_so():
    header = open(os.path.join(ROOT, "include", "xvit.h")).read()
    lib = _lib.load()
    for name in ("xvit_grad_pack_bf16", "xvit_grad_unpack_bf16"):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _lib.SIGNATURES and name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert lib.xvit_version() >= 304
    assert int(re.search(r"#define XVIT_GRAD_PACK_MAX_SEGMENTS (\d+)", header).group(1)) == _lib.GRAD_PACK_MAX_SEGMENTS
    assert C.sizeof(_lib.GradSegment) == 24 and _lib.GradSegment.n.offset == 16     # {const float* src; int64_t dst_offset; int64_t n}


def _segs(*entries):
    t = (_lib.GradSegment * len(entries))()
    for e, (src, off, n) in zip(t, entries):
        e.src, e.dst_offset, e.n = src, off, n
    return t


def test_grad_comm_argument_errors_do_not_launch():
    """Validation on the host before any launch: callable without a GPU (the dummy addresses are never dereferenced)."""
    lib = _lib.load()
    P = 4096                                           # any non-null, 16-byte aligned "address"
    err = lambda: lib.xvit_last_error_string()        # noqa: E731
    pack = lambda segs, k, dst=P, dst_n=1024: lib.xvit_grad_pack_bf16(segs, k, dst, dst_n, 1.0, None)   # noqa: E731
    assert pack(None, 1) < 0 and b"null" in err()
    assert pack(_segs((P, 0, 8)), 1, dst=None) < 0 and b"null" in err()
    assert pack(_segs((P, 0, 8)), 0) < 0 and b"segments" in err()
    m = _lib.GRAD_PACK_MAX_SEGMENTS
    many = _segs(*[(P, 64 * i, 8) for i in range(m + 1)])
    assert pack(many, m + 1, dst_n=64 * (m + 1)) < 0 and b"segments" in err()
    assert pack(_segs((P, 0, 8)), 1, dst=P + 2) < 0 and b"aligned" in err()
    assert pack(_segs((P + 4, 0, 8)), 1) < 0 and b"aligned" in err()
    assert pack(_segs((None, 0, 8)), 1) < 0 and b"null src" in err()
    assert pack(_segs((P, 0, 0)), 1) < 0 and b"n must be positive" in err()
    assert pack(_segs((P, 0, -8)), 1) < 0
    assert pack(_segs((P, 32, 8)), 1) < 0 and b"multiple of 64" in err()
    assert pack(_segs((P, -64, 8)), 1) < 0
    assert pack(_segs((P, 0, 1025)), 1) < 0 and b"beyond dst_n" in err()      # its slot (1088) ends beyond dst_n = 1024
    assert pack(_segs((P, 1024, 1)), 1) < 0 and b"beyond dst_n" in err()
    assert pack(_segs((P, 0, 8)), 1, dst_n=0) < 0
    assert pack(_segs((P, 0, 8), (P, 960, 65)), 2) < 0 and b"segment 1" in err()   # the second segment's slot is out of range
    unpack = lambda src, dst, n: lib.xvit_grad_unpack_bf16(src, dst, n, 1.0, None)   # noqa: E731
    assert unpack(None, P, 8) < 0 and unpack(P, None, 8) < 0
    assert unpack(P, P, 0) < 0 and unpack(P, P, -1) < 0
    assert unpack(P + 2, P, 8) < 0 and b"aligned" in err()
    assert unpack(P, P + 8, 8) < 0 and b"aligned" in err()


def test_grad_comm_wrappers_refuse_cpu_tensors():
    from xvit import ops
    with pytest.raises(RuntimeError, match="not on the GPU"):
        ops.grad_pack_bf16([(torch.ones(8), 0)], torch.zeros(64, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="not on the GPU"):
        ops.grad_unpack_bf16(torch.zeros(64, dtype=torch.bfloat16), torch.zeros(64))
