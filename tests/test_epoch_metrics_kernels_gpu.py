"""GPU: xvit_epoch_metrics_update and xvit_epoch_rank_stats (csrc/epoch_metrics.hip) against the restatement in
tests/_epoch_metrics_check.py, which tests/test_epoch_metrics_gate_cpu.py pins against scikit-learn.

Integers (predictions, labels, confusion, counters, pair counts, weights) are compared bit for bit.  The stored softmax scores are
compared with a float64 softmax under SCORE_BOUND (see there); the average precision under (n + 2) 2^-53 1.01 relative."""
import math

import numpy as np
import pytest
import torch

import _epoch_metrics_check as E
from _util import dev, note

pytestmark = pytest.mark.gpu

# The stored score is expf(l_c - max) / sum_k expf(l_k - max) in fp32: one expf and one division on top of a sum of C expf values.  The
# toolchain's documents state no ulp error for its device expf, so the bound is measured: the worst relative error of a stored score
# against the float64 softmax over every input of this file (C = 2 .. 64, B up to 8192, logits of standard deviation 3, the saturated rows
# included) was 34.49 units of 2^-24 (at C = 64, B = 8192); twice that is the bound.  It is far above one ulp because the error grows with the
# distance from the maximum: the fp32 difference l_c - max is rounded to half an ulp OF THE DIFFERENCE, which the exponential turns into a
# relative error of the same size (up to 16 units for a logit 30 below the maximum, 0.5 ulp(30) = 2^-20), and the device expf's own
# error grows with its argument too (22.1 units at expf(-80) in the saturated rows, whose argument is exact).  The float64 softmax has
# neither term.  The ranking is unaffected: scores are compared with each other, not with float64.
SCORE_MEASURED_ULP = 34.49
SCORE_BOUND = 2.0 * SCORE_MEASURED_ULP * 2.0 ** -24
GUARD = 64
SENT_F, SENT_I = 777.0, -12345


def _lib():
    from xvit import _lib as L
    return L


class Buffers:
    """Epoch buffers of `cap` rows inside sentinel-filled allocations: every store outside the buffers, or past the stored rows, shows."""

    def __init__(self, C, cap):
        L = _lib()
        self.C, self.cap, self.ns = C, cap, L.EPOCH_STATE_HEAD + C * C
        self.raw = [torch.full((cap * C + 2 * GUARD,), SENT_F, dtype=torch.float32, device=dev()),
                    torch.full((cap + 2 * GUARD,), SENT_I, dtype=torch.int32, device=dev()),
                    torch.full((cap + 2 * GUARD,), SENT_I, dtype=torch.int32, device=dev()),
                    torch.full((self.ns + 2 * GUARD,), SENT_I, dtype=torch.int64, device=dev())]
        self.scores = self.raw[0][GUARD:GUARD + cap * C].view(cap, C)
        self.labels32, self.preds = self.raw[1][GUARD:GUARD + cap], self.raw[2][GUARD:GUARD + cap]
        self.state = self.raw[3][GUARD:GUARD + self.ns]
        self.state.zero_()

    def update(self, logits, labels, ld=None):
        """logits / labels on the host; ld: the row stride the kernel sees (>= C)."""
        B, C = logits.shape
        ld = C if ld is None else ld
        wide = torch.full((B, ld), float("nan"), dtype=torch.float32)       # a NaN beside every row: reading past C would drop the row
        wide[:, :C] = logits
        lg, lb = wide.to(dev()), labels.to(dev(), torch.int64)
        L = _lib()
        rc = L.load().xvit_epoch_metrics_update(lg.data_ptr(), ld, lb.data_ptr(), B, C, self.scores.data_ptr(), self.labels32.data_ptr(),
                                                self.preds.data_ptr(), self.cap, self.state.data_ptr(), torch.cuda.current_stream().cuda_stream)
        L.check(rc, "xvit_epoch_metrics_update")

    def check(self, steps, what=""):
        """Everything the buffers hold against the restatement of `steps`; returns the worst score error in units of 2^-24 (relative)."""
        scores, labs, preds, conf, cnt = E.update_reference(steps, self.C, self.cap)
        L = _lib()
        state = self.state.cpu().tolist()
        got = {k: state[getattr(L, f"EPOCH_{k.upper()}")] for k in cnt}
        assert got == cnt, (what, got, cnt)
        assert state[L.EPOCH_STATE_HEAD:] == conf.reshape(-1).tolist(), what
        n = cnt["stored"]
        assert self.labels32[:n].cpu().tolist() == labs.tolist() and self.preds[:n].cpu().tolist() == preds.tolist(), what
        for raw, used, sent in zip(self.raw, (n * self.C, n, n, self.ns), (SENT_F, SENT_I, SENT_I, SENT_I)):
            r = raw.cpu()
            assert bool((r[:GUARD] == sent).all()) and bool((r[GUARD + used:] == sent).all()), f"{what}: a store outside the stored rows"
        worst = 0.0
        if n:
            g = self.scores[:n].cpu().double().numpy()
            err = np.abs(g - scores) / scores
            worst = float(err.max()) * 2.0 ** 24
            print(f"{what}: worst score error {worst:.3f} units of 2^-24 (bound {SCORE_BOUND * 2 ** 24:.2f})")
            note(f"epoch_metrics_score_ulp[{what}]", worst)
            assert float(err.max()) <= SCORE_BOUND, (what, worst)
        return worst


def _batch(seed, B, C, dirty=True):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, generator=g) * 3.0
    labels = torch.randint(0, C, (B,), generator=g)
    if dirty and B >= 8:
        labels[1], labels[B - 2] = -1, C                    # outside [0, C) on either side
        logits[3, C - 1] = float("nan")
        logits[B - 1, 0] = float("inf")
        logits[4, :] = logits[4, 0]                         # all equal: argmax is class 0
        logits[5, C - 1] = logits[5].max()                  # the maximum twice (or once, at the end)
    return logits, labels


@pytest.mark.parametrize("B", [1, 63, 64, 65, 8192])
@pytest.mark.parametrize("C", [2, 3, 5, 64])
def test_update_matches_the_restatement(C, B):
    buf = Buffers(C, cap=B + 5)
    step = _batch(100 * C + B, B, C)
    buf.update(*step, ld=C + 3)
    buf.check([step], f"C={C} B={B}")


def test_argmax_ties_go_to_the_first_maximum():
    logits = torch.tensor([[1.0, 1.0, 1.0], [0.0, 2.0, 2.0], [5.0, -1.0, 5.0], [-3.0, -3.0, -4.0], [0.5, 0.25, 0.5]])
    labels = torch.tensor([2, 2, 1, 0, 0])
    buf = Buffers(3, cap=8)
    buf.update(logits, labels)
    assert buf.preds[:5].cpu().tolist() == [0, 1, 0, 0, 0]
    buf.check([(logits, labels)], "ties")


def test_saturated_binary_scores_tie_as_in_the_reference():
    """C = 2 uses the expression of xvit_binary_metrics_step, e1 / (e0 + e1) with e = expf(l - max): a probability that rounds to 1.0 is
    exactly 1.0 and ties with every other saturated one, so the pooled AUROC of one step equals the binary kernel's."""
    from xvit.metrics import BinaryEpochMetrics
    logits = torch.tensor([[-40.0, 40.0], [-30.0, 50.0], [40.0, -40.0], [35.0, -45.0], [0.0, 0.1], [-50.0, 30.0], [2.0, 1.0]])
    labels = torch.tensor([1, 0, 0, 1, 1, 1, 0])
    buf = Buffers(2, cap=7)
    buf.update(logits, labels)
    buf.check([(logits, labels)], "saturated")
    s = buf.scores[:7].cpu()
    assert s[[0, 1, 5], 1].tolist() == [1.0, 1.0, 1.0] and s[[2, 3], 0].tolist() == [1.0, 1.0]       # bit for bit: the sum is 1 + tiny = 1
    u2, wp, wn, _ = E.rank_sums(s[:, 1].tolist(), [bool(v) for v in labels.tolist()], [1] * 7)
    ref = BinaryEpochMetrics(dev())
    ref.update(logits.to(dev()), labels.to(dev()))
    assert abs(ref.compute(sync_dist=False)["auc_roc"] - 0.5 * u2 / (wp * wn)) < 1e-12


def test_the_batch_that_crosses_the_capacity():
    steps = [_batch(1, 63, 3), _batch(2, 64, 3), _batch(3, 9, 3)]
    buf = Buffers(3, cap=100)
    for s in steps:
        buf.update(*s)
    buf.check(steps, "overflow")
    L = _lib()
    state = buf.state.cpu().tolist()
    kept = sum(state[L.EPOCH_STATE_HEAD:])
    assert state[L.EPOCH_STORED] == 100 and state[L.EPOCH_OVERFLOW] == kept - 100 > 0
    assert state[L.EPOCH_SEEN] == 136 == kept + state[L.EPOCH_IGNORED] + state[L.EPOCH_NONFINITE]


def test_two_updates_equal_one_update_of_the_concatenation():
    a, b = _batch(7, 130, 5), _batch(8, 1100, 5)
    two, one = Buffers(5, cap=1300), Buffers(5, cap=1300)
    two.update(*a)
    two.update(*b)
    one.update(torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]]))
    n = int(one.state[0])
    assert n == int(two.state[0]) > 1200
    assert torch.equal(one.scores[:n], two.scores[:n]) and torch.equal(one.labels32[:n], two.labels32[:n]) and torch.equal(one.preds[:n], two.preds[:n])
    L = _lib()
    s1, s2 = one.state.cpu().tolist(), two.state.cpu().tolist()
    s1[L.EPOCH_STEPS], s2[L.EPOCH_STEPS] = 0, 0
    assert s1 == s2
    two.check([a, b], "two updates")


def test_three_replays_of_a_captured_update_append_three_batches():
    from xvit.metrics import EpochMetrics
    logits, labels = _batch(11, 37, 3, dirty=False)
    lg, lb = logits.to(dev()), labels.to(dev())
    acc = EpochMetrics(3, dev(), capacity=200)
    acc.update(lg, lb)                                      # eager once: nothing is loaded or set up inside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc.update(lg, lb)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    state = acc.state.cpu().tolist()
    L = _lib()
    assert state[L.EPOCH_STORED] == 4 * 37 and state[L.EPOCH_STEPS] == 4 and state[L.EPOCH_SEEN] == 4 * 37
    s = acc.scores[:4 * 37]
    assert torch.equal(s[:37], s[37:74]) and torch.equal(s[:37], s[111:148])
    assert acc.labels32[:148].cpu().tolist() == labels.tolist() * 4


# ---- rank statistics --------------------------------------------------------------------------------------------------------------
def _epoch(seed, n, C, levels=5, cap=None):
    """Scores quantised to a handful of values (tie groups straddle every pass boundary), labels, predictions; NaN / junk in the tail."""
    rng = np.random.default_rng(seed)
    cap = n + 3 if cap is None else cap
    scores = np.full((cap, C), np.nan, dtype=np.float32)
    scores[:n] = (np.floor(rng.random((n, C)) * levels) / levels).astype(np.float32)
    labels = np.full(cap, -9, dtype=np.int32)
    preds = np.full(cap, 1 << 20, dtype=np.int32)
    labels[:n], preds[:n] = rng.integers(0, C, n), rng.integers(0, C, n)
    return scores, labels, preds


def _run_rank(scores, labels, preds, n, R, seed, perm=None):
    """The kernel on host arrays, its outputs inside sentinels: (ranks, ap, conf) on the host."""
    L = _lib()
    C = scores.shape[1]
    sc, lb, pr = (torch.from_numpy(a).to(dev()) for a in (scores, labels, preds))
    if perm is None:
        perm = sc[:n].t().contiguous().sort(dim=1, descending=True).indices if n else torch.zeros(C, 0, dtype=torch.int64, device=dev())
    else:
        perm = torch.from_numpy(perm).to(dev())
    n_dev = torch.tensor([n], dtype=torch.int64, device=dev())
    sizes = ((R + 1) * C * 3, (R + 1) * C, (R + 1) * C * C)
    raw = [torch.full((sizes[0] + 2 * GUARD,), SENT_I, dtype=torch.int64, device=dev()),
           torch.full((sizes[1] + 2 * GUARD,), SENT_F, dtype=torch.float64, device=dev()),
           torch.full((sizes[2] + 2 * GUARD,), SENT_I, dtype=torch.int64, device=dev())]
    out = [r[GUARD:GUARD + s] for r, s in zip(raw, sizes)]
    rc = L.load().xvit_epoch_rank_stats(sc.data_ptr(), lb.data_ptr(), pr.data_ptr(), perm.data_ptr(), max(perm.stride(0), n), n_dev.data_ptr(), n, C, R,
                                        seed, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    L.check(rc, "xvit_epoch_rank_stats")
    for r, s, sent in zip(raw, sizes, (SENT_I, SENT_F, SENT_I)):
        h = r.cpu()
        assert bool((h[:GUARD] == sent).all()) and bool((h[GUARD + s:] == sent).all()), "a store outside the outputs"
    return out[0].cpu().view(R + 1, C, 3).numpy(), out[1].cpu().view(R + 1, C).numpy(), out[2].cpu().view(R + 1, C, C).numpy()


def _check_rank(scores, labels, preds, n, R, seed, what, perm=None):
    C = scores.shape[1]
    ranks, ap, conf = _run_rank(scores, labels, preds, n, R, seed, perm)
    r_ranks, r_ap, r_conf = E.rank_stats_reference(scores[:n], labels[:n], preds[:n], C, R, seed)
    assert (ranks == r_ranks).all(), (what, ranks.tolist(), r_ranks.tolist())
    assert (conf == r_conf).all(), what
    assert np.isfinite(ap).all() and (np.abs(ap - r_ap) <= E.ap_bound(n) * r_ap).all(), (what, float(np.abs(ap - r_ap).max()))
    return ranks, ap, conf


T = 1024   # XVIT_EPOCH_RANK_PASS, asserted below


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1])
def test_rank_stats_match_the_restatement(n):
    assert T == _lib().EPOCH_RANK_PASS
    for C in (2, 3, 5):
        for R in (0, 1, 7):
            ep = _epoch(1000 * C + R + n, n, C)
            _check_rank(*ep, n, R, seed=0xC0FFEE + n, what=f"n={n} C={C} R={R}")


def test_rank_stats_at_the_bootstrap_limit():
    n = _lib().load().xvit_epoch_rank_stats_max_n()
    ep = _epoch(5, n, 2, levels=7, cap=n)
    ranks, _, conf = _check_rank(*ep, n, 2, seed=99, what="limit")
    assert (ranks[:, :, 1] + ranks[:, :, 2] == n).all() and (conf.sum(axis=(1, 2)) == n).all()      # every replicate resamples n draws


def test_rank_stats_degenerate_epochs():
    n = T + 9
    # every score equal: one tie group, u2 = wpos * wneg (AUROC 1/2) in every replicate
    sc, lb, pr = _epoch(1, n, 3)
    sc[:n] = 0.25
    ranks, _, _ = _check_rank(sc, lb, pr, n, 3, seed=4, what="all equal")
    assert (ranks[..., 0] == ranks[..., 1] * ranks[..., 2]).all()
    # two classes, every label 1: class 1 has no negatives, class 0 no positives
    sc, lb, pr = _epoch(2, n, 2)
    lb[:n] = 1
    ranks, ap, _ = _check_rank(sc, lb, pr, n, 2, seed=4, what="one class only")
    assert (ranks[:, 0, 1] == 0).all() and (ranks[:, 1, 2] == 0).all() and (ranks[..., 0] == 0).all() and (ap[:, 0] == 0).all()


def test_rank_stats_repeat_and_ignore_the_order_among_ties():
    n, C, R = 2 * T + 77, 3, 4
    sc, lb, pr = _epoch(21, n, C, levels=4)
    first = _check_rank(sc, lb, pr, n, R, seed=8, what="first")
    again = _run_rank(sc, lb, pr, n, R, 8)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()                   # bit-identical, the fp64 average precision included
    rng = np.random.default_rng(0)
    perm = np.stack([np.lexsort((rng.random(n), -sc[:n, c].astype(np.float64))) for c in range(C)]).astype(np.int64)   # ties in random order
    assert any((perm[c] != np.argsort(-sc[:n, c], kind="stable")).any() for c in range(C))
    other = _run_rank(sc, lb, pr, n, R, 8, perm=perm)
    assert other[0].tobytes() == first[0].tobytes() and other[2].tobytes() == first[2].tobytes()
    r_ap = E.rank_stats_reference(sc[:n], lb[:n], pr[:n], C, R, 8)[1]
    assert (np.abs(other[1] - r_ap) <= E.ap_bound(n) * r_ap).all()


def test_rank_stats_of_an_empty_epoch_are_zero():
    sc, lb, pr = _epoch(3, 0, 3, cap=4)
    ranks, ap, conf = _run_rank(sc, lb, pr, 0, 2, 1)
    assert not ranks.any() and not ap.any() and not conf.any()
