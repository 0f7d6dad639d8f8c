"""GPU: xvit_batch_draw and xvit_batch_gather bit for bit against the NumPy restatement (tests/_data_check.py), with sentinels around
every output.  Draw: the three modes over store sizes, batch sizes, rank cuts and call indices (one beyond 2^32), and the device counter
with and without advance.  Gather: both paths (16 bytes per lane where case_bytes % 16 == 0, 2 bytes otherwise) at every size around
their chunk edges, duplicate and out-of-range indices, optional labels and status, a poison pattern in every unselected case, and the
store unchanged afterwards."""
import numpy as np
import pytest
import torch

import _data_check as D
from _util import dev

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 5, 64, 65, 501, 4097)
BATCHES = (1, 7, 256, 257, 1000)
CUTS = ((0, 1), (1, 2), (3, 4))
CALLS = (0, 1, 2 ** 33)
GUARD, SENTINEL = 8, -77


def guarded(B, dtype=torch.int32):
    """(whole buffer, the B-element view the kernel writes) with GUARD sentinels on both sides."""
    buf = torch.full((B + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev())
    return buf, buf[GUARD:GUARD + B]


def guards_intact(buf, B):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + B:] == SENTINEL).all())


def cdf_of(n, seed=0):
    w = np.random.default_rng(seed + n).integers(0, 5, n).astype(np.float64)       # zeros included
    w[n // 2] += 1.0
    return D.make_cdf(w)


@pytest.mark.parametrize("mode", ["weighted", "shuffle", "sequential"])
def test_draw_matches_the_restatement(mode):
    from xvit import ops
    for n in SIZES:
        cdf = cdf_of(n) if mode == "weighted" else None
        cdf_dev = torch.from_numpy(cdf).to(dev()) if cdf is not None else None
        for B in BATCHES:
            for rank, world in CUTS:
                for call in CALLS:
                    buf, idx = guarded(B)
                    ops.batch_draw(idx, D.MODES[mode], n, 9, cdf=cdf_dev, rank=rank, world=world, call=call)
                    got = idx.cpu().numpy()
                    ref = D.draw_ref(mode, n, B, 9, rank, world, call, cdf)
                    assert np.array_equal(got, ref), (mode, n, B, rank, world, call, got[:8], ref[:8])
                    assert guards_intact(buf, B) and got.min() >= 0 and got.max() < n
    if mode != "sequential":                                           # another seed, another stream
        a, b = guarded(256)[1], guarded(256)[1]
        cdf_dev = torch.from_numpy(cdf_of(501)).to(dev()) if mode == "weighted" else None
        ops.batch_draw(a, D.MODES[mode], 501, 1, cdf=cdf_dev)
        ops.batch_draw(b, D.MODES[mode], 501, 2, cdf=cdf_dev)
        assert not torch.equal(a, b)


@pytest.mark.parametrize("mode", ["weighted", "shuffle", "sequential"])
def test_draw_reads_and_advances_the_device_counter(mode):
    from xvit import ops
    n, B = 65, 7
    cdf = cdf_of(n) if mode == "weighted" else None
    cdf_dev = torch.from_numpy(cdf).to(dev()) if cdf is not None else None
    counter = torch.tensor([5], dtype=torch.int64, device=dev())
    for advance, after in ((False, 5), (True, 6), (True, 7), (False, 7)):
        before = int(counter.item())
        buf, idx = guarded(B)
        ops.batch_draw(idx, D.MODES[mode], n, 4, cdf=cdf_dev, rank=1, world=2, call=999, counter=counter, advance=advance)   # `call` is ignored
        assert np.array_equal(idx.cpu().numpy(), D.draw_ref(mode, n, B, 4, 1, 2, before, cdf)) and guards_intact(buf, B)
        assert int(counter.item()) == after
    counter.fill_(2 ** 33)
    buf, idx = guarded(B)
    ops.batch_draw(idx, D.MODES[mode], n, 4, cdf=cdf_dev, counter=counter, advance=True)
    assert np.array_equal(idx.cpu().numpy(), D.draw_ref(mode, n, B, 4, call=2 ** 33, cdf=cdf)) and int(counter.item()) == 2 ** 33 + 1


def test_draws_are_reproducible():
    from xvit import ops
    cdf_dev = torch.from_numpy(cdf_of(4097)).to(dev())
    for mode in ("weighted", "shuffle"):
        a, b = guarded(1000)[1], guarded(1000)[1]
        ops.batch_draw(a, D.MODES[mode], 4097, 3, cdf=cdf_dev, call=6)
        ops.batch_draw(b, D.MODES[mode], 4097, 3, cdf=cdf_dev, call=6)
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------------ gather
POISON = 0x7B7B
CASE_BYTES = (2, 6, 14, 16, 18, 30, 32, 210, 4096, 4098,
              D.WIDE_CHUNK + 16, 2 * D.WIDE_CHUNK + 4096,       # 16 bytes per lane: just above one workgroup chunk; a partial last chunk
              D.NARROW_CHUNK + 2, 2 * D.NARROW_CHUNK + 1026)    # 2 bytes per lane: the same two


def make_store(n, case_bytes, esize, seed):
    """capacity n + 1: the case behind the last one is poison as well.  Values in [1, 1000]: never zero, never the poison pattern."""
    tdt = torch.int16 if esize == 2 else torch.int32
    g = torch.Generator().manual_seed(seed)
    store = torch.randint(1, 1001, (n + 1, case_bytes // esize), generator=g).to(tdt)
    store[n] = POISON
    return store


def run_gather(n, case_bytes, esize, idx_list, with_labels=True, with_status=True, seed=0):
    from xvit import ops
    B, per = len(idx_list), case_bytes // esize
    host = make_store(n, case_bytes, esize, seed)
    selected = {i for i in idx_list if 0 <= i < n}
    for i in range(n):
        if i not in selected:
            host[i] = POISON
    store = host.to(dev())
    labels_host = torch.arange(100, 100 + n + 1, dtype=torch.int64)
    labels = labels_host.to(dev()) if with_labels else None
    idx = torch.tensor(idx_list, dtype=torch.int32, device=dev())
    guard = 16 // esize                                                # 16 bytes: dst stays 16-byte aligned
    buf = torch.full((B * per + 2 * guard,), SENTINEL, dtype=host.dtype, device=dev())
    out = buf[guard:guard + B * per].view(B, per)
    lbuf, lout = guarded(B, torch.int64)
    sbuf, status = guarded(B)
    got, y = ops.batch_gather(store, idx, n, labels=labels, out=out, labels_out=lout if with_labels else None, status=status if with_status else None)
    assert got is out and (y is lout if with_labels else y is None)
    ref, ref_y, ref_s = D.gather_ref(host[:n].numpy().view(np.uint8).reshape(n, case_bytes), idx_list, labels_host[:n].numpy() if with_labels else None)
    where = (n, case_bytes, esize, idx_list)
    got_bytes = out.cpu().numpy().view(np.uint8).reshape(B, case_bytes)
    assert np.array_equal(got_bytes, ref), where
    assert not bool((out == POISON).any()), where                      # nothing leaks from an unselected case
    assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + B * per:] == SENTINEL).all()), where
    assert guards_intact(lbuf, B) and guards_intact(sbuf, B), where
    assert np.array_equal(lout.cpu().numpy(), ref_y) if with_labels else bool((lout == SENTINEL).all()), where
    assert np.array_equal(status.cpu().numpy(), ref_s) if with_status else bool((status == SENTINEL).all()), where
    assert torch.equal(store.cpu(), host), where                       # the store is only read
    for b, i in enumerate(idx_list):
        if not 0 <= i < n:
            assert not got_bytes[b].any() and (not with_labels or int(lout[b]) == -1) and (not with_status or int(status[b]) == 1), where


@pytest.mark.parametrize("case_bytes", CASE_BYTES)
def test_gather_matches_the_restatement(case_bytes):
    assert D.chunks(case_bytes) == -(-case_bytes // (D.WIDE_CHUNK if case_bytes % 16 == 0 else D.NARROW_CHUNK))
    for esize in (2, 4):
        if case_bytes % esize:
            continue
        run_gather(1, case_bytes, esize, [0])
        run_gather(1, case_bytes, esize, [0, 0, 0])
        run_gather(4, case_bytes, esize, [2])
        run_gather(4, case_bytes, esize, [3, 0, 3])                                    # duplicates
        run_gather(4, case_bytes, esize, [1, 3, 3, 0, 2, 1, 1, 0, 3], seed=1)
        run_gather(4, case_bytes, esize, [1, -1, 4, 2 ** 31 - 1, 2, -2 ** 31, 5, 1, 0])  # refused indices: zeros, label -1, status 1
        run_gather(1, case_bytes, esize, [1, 0, -1])


@pytest.mark.parametrize("case_bytes", (18, 32, D.WIDE_CHUNK + 16, D.NARROW_CHUNK + 2))
def test_gather_without_labels_or_status(case_bytes):
    for with_labels, with_status in ((False, True), (True, False), (False, False)):
        run_gather(4, case_bytes, 2, [3, 4, 0], with_labels=with_labels, with_status=with_status)
        run_gather(1, case_bytes, 2, [0], with_labels=with_labels, with_status=with_status)


def test_gather_reads_its_indices_on_the_device():
    """One captured launch, replayed after the index tensor changed: another batch."""
    from xvit import ops
    store = make_store(4, 4096, 2, 3)[:4].contiguous().to(dev())
    idx = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev())
    out = torch.empty(3, 2048, dtype=torch.int16, device=dev())
    ops.batch_gather(store, idx, out=out)                              # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.batch_gather(store, idx, out=out)
    for want in ([3, 3, 1], [2, 0, 3]):
        idx.copy_(torch.tensor(want, dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, store[torch.tensor(want, device=dev())])
