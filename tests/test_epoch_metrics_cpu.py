"""CPU: the host side of the pooled epoch metrics (xvit_epoch_metrics_update / xvit_epoch_rank_stats, xvit.metrics.EpochMetrics):
refusals through the C ABI before any launch, the state-head constants, the key set of compute(), the float64 arithmetic on the integer
outputs against the restatement, and the two-rank gather of the stored rows on gloo."""
import math
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _epoch_metrics_check as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 256   # any non-null, 16-byte aligned "address": nothing is launched, so it is never dereferenced


def _update(lib, B=8, C=3, ld=None, cap=100, logits=P, labels=P, scores=P, labels32=P, preds=P, state=P):
    return lib.xvit_epoch_metrics_update(logits, C if ld is None else ld, labels, B, C, scores, labels32, preds, cap, state, None)


def _rank(lib, n_max=10, C=3, R=0, ldp=None, scores=P, labels32=P, preds=P, perm=P, n_dev=P, ranks=P, ap=P, conf=P):
    return lib.xvit_epoch_rank_stats(scores, labels32, preds, perm, n_max if ldp is None else ldp, n_dev, n_max, C, R, 0, ranks, ap, conf, None)


def test_update_refusals_do_not_launch():
    from xvit import _lib
    lib = _lib.load()
    err = lib.xvit_last_error_string
    for C in (1, 0, -3, 65):
        assert _update(lib, C=C, ld=64) < 0 and b"classes outside 2..64" in err(), C
    for B in (0, -1, 8193):
        assert _update(lib, B=B) < 0 and b"outside 1..8192" in err(), B
    for cap in (0, -5, 1 << 31):
        assert _update(lib, cap=cap) < 0 and b"capacity" in err(), cap
    assert _update(lib, C=3, ld=2) < 0 and b"row stride" in err()
    for k in ("logits", "labels", "scores", "labels32", "preds", "state"):
        assert _update(lib, **{k: None}) < 0 and b"null" in err(), k
    assert _update(lib, state=P + 4) < 0 and b"aligned" in err()


def test_rank_stats_refusals_do_not_launch():
    from xvit import _lib
    lib = _lib.load()
    err = lib.xvit_last_error_string
    limit = lib.xvit_epoch_rank_stats_max_n()
    assert limit == _lib.EPOCH_RANK_MAX_N == 65535 and limit < 2 ** 16          # a 16-bit counter cannot overflow: at most n draws hit one sample
    assert (limit + 1) * 2 + 8192 <= 160 * 1024                                  # ... and the counters fit the LDS of one CU beside the scratch
    assert _rank(lib, n_max=limit + 1, R=1) < 0 and b"bootstrap" in err() and str(limit).encode() in err()
    assert _rank(lib, n_max=1 << 31, R=0) < 0 and b"n_max" in err()
    assert _rank(lib, n_max=-1) < 0
    for C in (1, 65):
        assert _rank(lib, C=C) < 0 and b"classes outside 2..64" in err()
    assert _rank(lib, R=-1) < 0 and b"replicates" in err()
    assert _rank(lib, n_max=10, ldp=9) < 0 and b"stride" in err()
    for k in ("scores", "labels32", "preds", "perm", "n_dev", "ranks", "ap", "conf"):
        assert _rank(lib, **{k: None}) < 0 and b"null" in err(), k
    assert _rank(lib, ranks=P + 4) < 0 and b"aligned" in err()


def test_constants_match_the_header():
    from xvit import _lib
    header = open(os.path.join(ROOT, "include", "xvit.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", header).group(1))

    assert _lib.EPOCH_STATE_HEAD == define("XVIT_EPOCH_STATE_HEAD") == E.HEAD
    assert _lib.EPOCH_MAX_C == define("XVIT_EPOCH_MAX_C") and _lib.EPOCH_MAX_B == define("XVIT_EPOCH_MAX_B")
    assert _lib.EPOCH_RANK_PASS == define("XVIT_EPOCH_RANK_PASS") and _lib.EPOCH_RANK_MAX_N == define("XVIT_EPOCH_RANK_MAX_N")
    assert _lib.EPOCH_RANK_NSTAT == define("XVIT_EPOCH_RANK_NSTAT")
    enum = re.search(r"enum \{ (XVIT_EPOCH_STORED[^}]*)\}", header).group(1)
    counters = {k.strip(): int(v) for k, v in (item.split("=") for item in enum.split(","))}
    for name in ("STORED", "SEEN", "STEPS", "IGNORED", "NONFINITE", "OVERFLOW"):
        assert getattr(_lib, f"EPOCH_{name}") == counters[f"XVIT_EPOCH_{name}"] == getattr(E, name), name
    assert max(counters.values()) < _lib.EPOCH_STATE_HEAD
    enum = re.search(r"enum \{ (XVIT_EPOCH_RANK_U2[^}]*)\}", header).group(1)
    assert [s.strip() for s in enum.split(",")] == ["XVIT_EPOCH_RANK_U2 = 0", "XVIT_EPOCH_RANK_WPOS = 1", "XVIT_EPOCH_RANK_WNEG = 2"]
    assert (_lib.EPOCH_RANK_U2, _lib.EPOCH_RANK_WPOS, _lib.EPOCH_RANK_WNEG) == (0, 1, 2)
    assert _lib.load().xvit_version() >= 315


@pytest.mark.parametrize("C", [2, 3])
def test_key_set_and_host_arithmetic_match_the_restatement(C):
    """The float64 arithmetic compute() does on the kernel's integer outputs, fed with the restatement's integers: same keys, same values."""
    from xvit import metrics
    rng = np.random.default_rng(C)
    n, R = 60, 9
    scores = (np.floor(rng.random((n, C)) * 6) / 6).astype(np.float32)
    labels, preds = rng.integers(0, C, n), rng.integers(0, C, n)
    ranks, ap, conf = E.rank_stats_reference(scores, labels, preds, C, R, seed=5)
    got = metrics._scalars(torch.from_numpy(conf).double(), torch.from_numpy(ranks).double(), torch.from_numpy(ap))
    keys = metrics.epoch_metric_keys(C)
    assert set(got) == set(keys) and len(keys) == len(set(keys))
    assert ("auc_roc" in keys) == (C == 2)
    assert {"acc", "balanced_acc", "macro_auroc", "macro_ap", "macro_f1", f"auroc_{C - 1}", f"ap_0", f"npv_{C - 1}"} <= set(keys)
    for r in range(R + 1):
        ref = E.scalars(conf[r], ranks[r], ap[r])
        assert set(ref) == set(keys)
        for k in keys:
            a, b = float(got[k][r]), ref[k]
            assert (math.isnan(a) and math.isnan(b)) or abs(a - b) < 1e-12, (r, k, a, b)
    # a class without positives: its rank values are nan, never 0, and so are the macro values
    ranks[0, 0, 1] = 0
    got = metrics._scalars(torch.from_numpy(conf).double(), torch.from_numpy(ranks).double(), torch.from_numpy(ap))
    assert math.isnan(float(got["auroc_0"][0])) and math.isnan(float(got["ap_0"][0])) and math.isnan(float(got["macro_auroc"][0]))
    assert not math.isnan(float(got["auroc_1"][0])) and not math.isnan(float(got["auroc_0"][1]))
    assert metrics._nearest_rank(list(range(1, 1001)), 0.025) == 25 == E.nearest_rank(list(range(1, 1001)), 0.025)


def test_config_fields_are_optional_and_checked():
    from types import SimpleNamespace
    from xvit.metrics import epoch_metrics_config
    assert epoch_metrics_config(SimpleNamespace()) == ("reference", 0)
    assert epoch_metrics_config(SimpleNamespace(epoch_metrics="pooled", epoch_metrics_bootstrap=200)) == ("pooled", 200)
    with pytest.raises(ValueError):
        epoch_metrics_config(SimpleNamespace(epoch_metrics="exact"))
    with pytest.raises(ValueError):
        epoch_metrics_config(SimpleNamespace(epoch_metrics_bootstrap=-1))


# ---- the gather of the stored rows over two ranks (gloo, CPU tensors): ragged counts, one rank holding nothing ----
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rows(rank, count, C=3, cap=9):
    g = torch.Generator().manual_seed(50 + rank)
    scores = torch.rand(cap, C, generator=g)
    labels32 = torch.randint(0, C, (cap,), generator=g, dtype=torch.int32)
    preds = torch.randint(0, C, (cap,), generator=g, dtype=torch.int32)
    scores[count:], labels32[count:], preds[count:] = float("nan"), -7, -7       # the unused tail must not travel
    return scores, labels32, preds


def _gather_worker(rank, world, port, out_dir, counts):
    sys.path.insert(0, os.path.join(ROOT, "cross-attention-vit_amd"))
    from xvit.metrics import gather_epoch_rows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = gather_epoch_rows(*_rows(rank, counts[rank]), counts[rank])
    torch.save(out, os.path.join(out_dir, f"rows{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("counts", [(5, 0), (2, 7)])
def test_gather_of_ragged_rows_world2(tmp_path, counts):
    mp.spawn(_gather_worker, args=(2, _free_port(), str(tmp_path), counts), nprocs=2, join=True)
    got = [torch.load(tmp_path / f"rows{r}.pt") for r in range(2)]
    parts = [_rows(r, counts[r]) for r in range(2)]
    for k in range(3):
        want = torch.cat([parts[r][k][:counts[r]] for r in range(2)])
        for r in range(2):
            assert torch.equal(got[r][k], want), (r, k)                          # rank order, no padding, the same on every rank
    assert got[0][3] == got[1][3] == sum(counts)
