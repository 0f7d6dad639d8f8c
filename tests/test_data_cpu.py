"""CPU: the device-resident volume store without a GPU.  Properties of the restatement tests/_data_check.py (the rule of include/xvit.h,
"Device-resident volume store"): the keyed permutation is a bijection, its position -> case table and the weighted draw pass a chi-square
test, the sample stream does not depend on how it is cut into ranks and calls.  Every argument error of xvit_batch_draw and
xvit_batch_gather is refused on the host before any launch (dummy aligned addresses that are never dereferenced); the constants agree
between header, xvit._lib and the restatement; the Python side refuses bad arguments and its state_dict round-trips."""
import os
import re

import numpy as np
import pytest
import torch

import _data_check as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "xvit.h")).read()
P = 4096   # any non-null, 16-byte aligned "address"
SIZES = (1, 2, 3, 5, 64, 65, 501, 4097)


def _lib():
    from xvit import _lib
    return _lib, _lib.load()


def test_constants_agree_between_header_and_binding():
    enum = dict((k, int(v)) for k, v in re.findall(r"XVIT_BATCH_([A-Z]+) = (\d+)", HEADER))
    assert enum == dict(WEIGHTED=0, SHUFFLE=1, SEQUENTIAL=2)
    assert (D.WEIGHTED, D.SHUFFLE, D.SEQUENTIAL) == (0, 1, 2)
    from xvit import _lib
    assert enum == dict(WEIGHTED=_lib.BATCH_WEIGHTED, SHUFFLE=_lib.BATCH_SHUFFLE, SEQUENTIAL=_lib.BATCH_SEQUENTIAL)


def test_new_symbols_are_exported_and_bound():
    mod, lib = _lib()
    for name, nargs in (("xvit_batch_draw", 12), ("xvit_batch_gather", 10)):
        assert name in mod.EXPORTS and hasattr(lib, name) and len(mod.SIGNATURES[name]) == nargs
        assert re.search(r"\bint " + name + r"\(", HEADER)
    assert lib.xvit_version() >= 320
    assert '"batch_store.hip"' in open(os.path.join(ROOT, "cross-attention-vit_amd", "build.py")).read()
    src = open(os.path.join(ROOT, "cross-attention-vit_amd", "csrc", "batch_store.hip")).read()
    assert f"0x{D.TAG:X}".lower() in src.lower() and f"0x{D.TAG:X}" in HEADER and f"0x{D.SEED_STRIDE:X}" in HEADER
    assert int(re.search(r"kBatchItems = (\d+);", src).group(1)) == D.GATHER_ITEMS
    import xvit
    assert xvit.data.VolumeStore and xvit.data.BatchSampler and "xvit.data" in xvit.__doc__


@pytest.mark.parametrize("n", SIZES)
def test_the_permutation_is_a_bijection(n):
    w = D.feistel_bits(n)
    assert w % 2 == 0 and w >= 2 and (1 << w) >= n and (n <= 4 or (1 << (w - 2)) < n)
    q = np.arange(n, dtype=np.uint64)
    seen = []
    for e in range(8):
        p = D.permute(n, np.full(n, e, dtype=np.uint64), q, 7)
        assert np.array_equal(np.sort(p), q), (n, e)
        seen.append(p.tolist())
        # the same through the ordinals: n consecutive samples from a multiple of n see every case once
        assert sorted(D.shuffle_ref(n, list(range(e * n, (e + 1) * n)), 7).tolist()) == list(range(n))
    if n >= 64:
        assert len(set(map(tuple, seen))) == 8                      # another permutation per epoch


def test_position_to_case_table_is_flat():
    n, epochs = 16, 4096
    e, q = np.repeat(np.arange(epochs, dtype=np.uint64), n), np.tile(np.arange(n, dtype=np.uint64), epochs)
    p = D.permute(n, e, q, 3)
    table = np.zeros((n, n))
    np.add.at(table, (q.astype(np.int64), p.astype(np.int64)), 1)
    chi = D.chi_square(table, np.full((n, n), epochs / n))
    print(f"position -> case chi-square {chi:.1f} on 225 degrees of freedom")
    assert abs(chi - 234.8) < 0.05 and chi < 300


def test_weighted_draw_follows_the_weights():
    w = np.array([1, 1, 1, 1, 4, 0, 2, 6], dtype=np.float64)
    cdf = D.make_cdf(w)
    assert cdf[-1] == 1.0 and cdf[4] == cdf[5] and np.all(np.diff(cdf) >= 0)
    idx = D.weighted_ref(cdf, list(range(65536)), 11)
    counts = np.bincount(idx, minlength=8)
    assert counts[5] == 0 and counts.sum() == 65536
    keep = [0, 1, 2, 3, 4, 6, 7]
    chi = D.chi_square(counts[keep], w[keep] / w.sum() * 65536)
    print(f"weighted draw chi-square {chi:.2f} on 6 degrees of freedom")
    assert abs(chi - 2.56) < 0.005 and chi < 22.5
    # zero weights at either end are never drawn, and the last positive weight closes the cdf at exactly 1
    edge = D.make_cdf([0, 0, 3, 1, 0, 0])
    assert edge.tolist() == [0.0, 0.0, 0.75, 1.0, 1.0, 1.0]
    assert set(D.weighted_ref(edge, list(range(4096)), 5).tolist()) == {2, 3}
    from xvit.data import make_cdf
    assert np.array_equal(make_cdf(torch.tensor(w)).numpy(), cdf) and np.array_equal(make_cdf([0, 0, 3, 1, 0, 0]).numpy(), edge)


@pytest.mark.parametrize("mode", ["weighted", "shuffle", "sequential"])
def test_the_stream_does_not_depend_on_how_it_is_cut(mode):
    n, G, calls, seed = 37, 8, 12, 5                                 # global batch 8: 1 x 8, 2 x 4, 4 x 2; 96 samples straddle epochs of 37
    cdf = D.make_cdf(np.arange(1, n + 1)) if mode == "weighted" else None
    streams = []
    for world in (1, 2, 4):
        B = G // world
        parts = [D.draw_ref(mode, n, B, seed, rank, world, call, cdf) for call in range(calls) for rank in range(world)]
        streams.append(np.concatenate(parts))
    assert np.array_equal(streams[0], streams[1]) and np.array_equal(streams[0], streams[2])
    assert np.array_equal(streams[0], D.draw_ref(mode, n, G * calls, seed, cdf=cdf))      # ... and is one long call
    if mode == "sequential":
        assert streams[0].tolist() == [k % n for k in range(G * calls)]
    if mode == "shuffle":
        assert sorted(streams[0][:n].tolist()) == list(range(n)) and sorted(streams[0][n:2 * n].tolist()) == list(range(n))
    assert not np.array_equal(streams[0], D.draw_ref(mode, n, G * calls, seed + 1, cdf=cdf)) or mode == "sequential"
    # ordinals wrap modulo 2^64 exactly
    assert D.ordinals(3, rank=1, world=2, call=2 ** 63) == [3, 4, 5]


def test_draw_argument_errors_do_not_launch():
    mod, lib = _lib()
    err = lib.xvit_last_error_string

    def draw(idx=P, cdf=2 * P, n=5, B=4, mode=0, rank=0, world=1, counter=None, advance=0):
        return lib.xvit_batch_draw(idx, cdf, n, B, mode, rank, world, 1, 0, counter, advance, None)

    assert draw(idx=None) < 0 and b"xvit_batch_draw" in err() and b"null" in err()
    for n in (0, -1, 2 ** 31, 2 ** 40):
        assert draw(n=n) < 0 and b"n_cases" in err(), n
    for B in (0, -3):
        assert draw(B=B) < 0 and b"B=" in err()
    for mode in (3, -1):
        assert draw(mode=mode) < 0 and b"unknown mode" in err()
    for rank, world in ((1, 1), (-1, 2), (4, 4), (0, 0), (0, -2)):
        assert draw(rank=rank, world=world) < 0 and b"rank" in err(), (rank, world)
    assert draw(counter=3 * P + 4) < 0 and b"8-byte aligned" in err()
    assert draw(advance=1) < 0 and b"advance needs a counter" in err()
    assert draw(cdf=None) < 0 and b"needs a cdf" in err()
    assert draw(cdf=2 * P + 4) < 0 and b"cdf" in err()
    assert draw(idx=P + 2) < 0 and b"4-byte" in err()


def test_gather_argument_errors_do_not_launch():
    mod, lib = _lib()
    err = lib.xvit_last_error_string

    def gather(store=P, cb=64, n=4, idx=2 * P, B=3, dst=3 * P, ls=4 * P, ld=5 * P, status=6 * P):
        return lib.xvit_batch_gather(store, cb, n, idx, B, dst, ls, ld, status, None)

    for kw in (dict(store=None), dict(idx=None), dict(dst=None), dict(ld=None)):
        assert gather(**kw) < 0 and b"xvit_batch_gather" in err() and b"null" in err(), kw
    for cb in (0, -16, 7, 33):
        assert gather(cb=cb) < 0 and b"multiple of 2" in err(), cb
    for n, B in ((0, 3), (-1, 3), (4, 0), (4, -2)):
        assert gather(n=n, B=B) < 0 and b"must be positive" in err(), (n, B)
    for kw in (dict(store=P + 8), dict(dst=3 * P + 2)):
        assert gather(**kw) < 0 and b"16-byte aligned" in err(), kw
    for kw in (dict(idx=2 * P + 2), dict(status=6 * P + 2), dict(ls=4 * P + 4), dict(ld=5 * P + 4)):
        assert gather(**kw) < 0 and b"aligned" in err(), kw
    # B x chunks >= 2^31 on either path: 32 KiB chunks where case_bytes % 16 == 0, 4 KiB chunks otherwise
    assert D.chunks(2 ** 40) == 2 ** 25 and D.chunks(2 ** 40 + 2) == 2 ** 28 + 1
    assert gather(cb=2 ** 40, B=64) < 0 and b"2^31" in err()
    assert gather(cb=2 ** 40 + 2, B=8) < 0 and b"2^31" in err()


def test_the_python_side_refuses_bad_arguments_and_round_trips_its_state():
    from xvit.data import BatchSampler, VolumeStore, class_balanced_weights
    with pytest.raises(ValueError, match="case_shape"):
        VolumeStore((2, 4, 4), 3, device="cpu")
    with pytest.raises(ValueError, match="capacity"):
        VolumeStore((2, 4, 4, 4), 0, device="cpu")
    with pytest.raises(TypeError, match="not supported"):
        VolumeStore((2, 4, 4, 4), 3, dtype=torch.float64, device="cpu")
    store = VolumeStore((2, 3, 4, 5), 5, device="cpu")
    base = store.volumes.data_ptr()
    g = torch.Generator().manual_seed(0)
    vols = torch.randint(-100, 1000, (4, 2, 3, 4, 5), generator=g).to(torch.int16)
    assert len(store) == 0 and store.case_bytes == 240
    with pytest.raises(RuntimeError, match="empty"):
        BatchSampler(store, 2)
    store.add(vols[0], 1, weight=2.0)
    store.extend(vols[1:4], [0, 1, 1])
    assert len(store) == 4 and store.volumes.data_ptr() == base and torch.equal(store.volumes[:4], vols)
    assert store.labels.tolist() == [1, 0, 1, 1, -1] and store.weights.tolist() == [2.0, 1.0, 1.0, 1.0, 0.0]
    with pytest.raises(ValueError, match="shape"):
        store.add(vols[0, :1], 0)
    with pytest.raises(TypeError, match="no silent conversion"):
        store.add(vols[0].float(), 0)
    with pytest.raises(ValueError, match="labels and weights"):
        store.extend(vols[:1], [0, 1])
    with pytest.raises(ValueError, match="finite and non-negative"):
        store.add(vols[0], 0, weight=-1.0)
    with pytest.raises(RuntimeError, match="capacity"):
        store.extend(vols[:2], [0, 0])
    assert len(store) == 4
    with pytest.raises(IndexError, match=r"\[0, 4\)"):
        store.gather([0, 4])
    with pytest.raises(IndexError):
        store.gather(torch.tensor([-1]))
    with pytest.raises(ValueError, match="int32 or int64"):
        store.gather(torch.tensor([0.5]))
    assert class_balanced_weights([1, 0, 1, 1]).tolist() == [1 / 3, 1.0, 1 / 3, 1 / 3]
    for kw, exc in ((dict(batch_size=0), ValueError), (dict(mode="random"), ValueError), (dict(rank=2, world_size=2), ValueError),
                    (dict(weights=[1, 2]), ValueError), (dict(mode="shuffle", weights=[1, 1, 1, 1]), ValueError), (dict(weights=[0, 0, 0, 0]), ValueError)):
        with pytest.raises(exc, match="BatchSampler"):
            BatchSampler(store, **{"batch_size": 2, **kw})
    a = BatchSampler(store, 2, mode="weighted", seed=3, rank=1, world_size=2)
    assert a.n_cases == 4 and np.array_equal(a.cdf.numpy(), D.make_cdf([2, 1, 1, 1]))
    store.add(vols[0], 0)
    assert a.n_cases == 4 and a.cdf.numel() == 4                     # a snapshot: the later add is not seen
    a.calls = 7
    state = a.state_dict()
    assert state["call_index"] == 7 and a.call_index == 7
    b = BatchSampler(store, 2, mode="weighted", weights=[2, 1, 1, 1, 0], seed=3, rank=1, world_size=2)
    with pytest.raises(ValueError, match="n_cases"):
        b.load_state_dict(state)
    c = BatchSampler(store, 2, mode="shuffle", seed=3)
    with pytest.raises(ValueError, match="mode"):
        c.load_state_dict(state)
    d = BatchSampler.__new__(BatchSampler)
    d.__dict__.update(a.__dict__)
    d.calls = 0
    d.load_state_dict(state)
    assert d.call_index == 7 and d.state_dict() == state
    with pytest.raises(RuntimeError, match="GPU"):
        a()                                                          # a host store cannot be sampled: there is no CPU path


def test_a_capturable_sampler_allocates_outside_a_capture(monkeypatch):
    from xvit.data import BatchSampler, VolumeStore
    store = VolumeStore((1, 2, 2, 2), 2, device="cpu")
    store.extend(torch.zeros(2, 1, 2, 2, 2, dtype=torch.int16), [0, 1])
    s = BatchSampler(store, 3, mode="sequential", capturable=True)
    s.load_state_dict({"call_index": 5})
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="call the sampler once before capturing it"):
        s._buffers()
    assert s._static is None and s._counter is None
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    idx, status, raw, y = s._buffers()
    assert tuple(raw.shape) == (3, 1, 2, 2, 2) and idx.dtype == status.dtype == torch.int32 and y.dtype == torch.int64
    assert s.call_index == 5 and s._buffers()[2] is raw              # the counter starts at the loaded index; the buffers are static


def test_graphed_step_refuses_a_source_that_is_not_callable():
    from xvit.graph import GraphedStep

    class FakeCuda(torch.Tensor):
        is_cuda = True

    with pytest.raises(TypeError, match="source is a callable"):
        GraphedStep(torch.nn.Linear(2, 2), torch.zeros(2, 2).as_subclass(FakeCuda), torch.zeros(2), source=3)
