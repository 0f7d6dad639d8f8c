"""CPU: the restatement the pooled-epoch-metric tests compare against (tests/_epoch_metrics_check.py) is itself pinned here: against
scikit-learn's weighted roc_auc_score / average_precision_score / confusion_matrix, against a brute-force pair count, and by showing
that the comparison has teeth (four kinds of small mistakes each make it fail)."""
import math

import numpy as np
import pytest

import _epoch_metrics_check as E


def _case(seed, n, ties):
    rng = np.random.default_rng(seed)
    score = rng.random(n).astype(np.float32)
    if ties:
        score = (np.floor(score * 5) / 5).astype(np.float32)        # five distinct values: heavy ties
    pos = rng.random(n) < 0.4
    pos[:2] = (True, False)                                         # both classes occur
    w = rng.integers(0, 4, n)
    w[:2] = 1                                                       # ... with weight
    return score.tolist(), pos.tolist(), w.tolist()


def _brute_u2(score, pos, w):
    """2 * #(positive above negative) + #(equal), weighted: every pair counted."""
    u2 = 0
    for i in range(len(score)):
        if pos[i]:
            for j in range(len(score)):
                if not pos[j]:
                    u2 += w[i] * w[j] * (2 if score[i] > score[j] else (1 if score[i] == score[j] else 0))
    return u2


@pytest.mark.parametrize("ties", [False, True])
def test_rank_sums_match_scikit_learn_and_a_pair_count(ties):
    skm = pytest.importorskip("sklearn.metrics")
    for seed in range(12):
        score, pos, w = _case(seed, 40 + 7 * seed, ties)
        u2, wp, wn, ap = E.rank_sums(score, pos, w)
        assert u2 == _brute_u2(score, pos, w)
        assert wp == sum(m for m, p in zip(w, pos) if p) and wn == sum(w) - wp
        assert abs(0.5 * u2 / (wp * wn) - skm.roc_auc_score(pos, score, sample_weight=w)) < 1e-12
        assert abs(ap - skm.average_precision_score(pos, score, sample_weight=w)) < 1e-12


def test_confusion_and_scalars_match_scikit_learn():
    skm = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(3)
    C, n = 4, 120
    labels, preds, w = rng.integers(0, C, n), rng.integers(0, C, n), rng.integers(0, 3, n)
    conf = E.confusion(labels.tolist(), preds.tolist(), w.tolist(), C)
    assert (conf == skm.confusion_matrix(labels, preds, labels=list(range(C)), sample_weight=w)).all()
    s = E.scalars(conf, np.ones((C, 3), dtype=np.int64), np.zeros(C))
    assert abs(s["acc"] - skm.accuracy_score(labels, preds, sample_weight=w)) < 1e-12
    assert abs(s["balanced_acc"] - skm.balanced_accuracy_score(labels, preds, sample_weight=w)) < 1e-12
    p, r, f, _ = skm.precision_recall_fscore_support(labels, preds, labels=list(range(C)), sample_weight=w, zero_division=0)
    for c in range(C):
        assert abs(s[f"prec_{c}"] - p[c]) < 1e-12 and abs(s[f"rec_{c}"] - r[c]) < 1e-12 and abs(s[f"f1_{c}"] - f[c]) < 1e-12
    assert abs(s["macro_f1"] - f.mean()) < 1e-12


def test_the_comparison_has_teeth():
    """A swapped pair of unequal scores, one wrong multiplicity, a tie broken the wrong way and an off-by-one group boundary each change
    the integers the GPU tests compare bit for bit."""
    score = [0.9, 0.8, 0.8, 0.8, 0.5, 0.5, 0.2, 0.1]
    pos = [True, False, True, False, True, False, False, True]
    w = [1, 2, 1, 1, 3, 1, 2, 1]
    good = E.rank_sums(score, pos, w)
    assert good[0] == _brute_u2(score, pos, w)

    swapped = list(score)
    swapped[0], swapped[1] = swapped[1], swapped[0]                 # a positive and a negative with unequal scores change places
    assert E.rank_sums(swapped, pos, w)[0] != good[0]

    wrong_w = list(w)
    wrong_w[4] += 1                                                 # one multiplicity off by one
    assert E.rank_sums(score, pos, wrong_w)[:3] != good[:3]

    def walk(score, pos, w, strict_ties, boundary_shift):
        """The walk with a deliberate mistake: ties broken by position (every element its own group) or a group closed one element late."""
        order = sorted(range(len(score)), key=lambda i: -score[i])
        wneg = sum(m for m, p in zip(w, pos) if not p)
        u2 = cp = cn = 0
        j = 0
        while j < len(order):
            k = j + 1
            if not strict_ties:
                while k < len(order) and score[order[k]] == score[order[j]]:
                    k += 1
                k = min(len(order), k + boundary_shift)
            gp = sum(w[i] for i in order[j:k] if pos[i])
            gn = sum(w[i] for i in order[j:k] if not pos[i])
            cp, cn = cp + gp, cn + gn
            u2 += gp * (2 * (wneg - cn) + gn)
            j = k
        return u2

    assert walk(score, pos, w, False, 0) == good[0]                 # the faithful walk agrees
    assert walk(score, pos, w, True, 0) != good[0]                  # a tie broken the wrong way
    assert walk(score, pos, w, False, 1) != good[0]                 # an off-by-one group boundary


def test_every_replicate_resamples_n_draws():
    for n in (1, 2, 63, 1000):
        for r in range(4):
            w = E.draw_weights(12345, r, n)
            assert len(w) == n and sum(w) == n and min(w) >= 0
    assert E.draw_weights(1, 0, 5) == [1] * 5
    assert E.draw_weights(1, 1, 200) != E.draw_weights(1, 2, 200)   # replicates differ
    assert E.draw_weights(1, 1, 200) == E.draw_weights(1, 1, 200)   # ... and repeat
    assert E.hash32(0, 0) == 0 and 0 <= E.hash32(7, 9) < 2 ** 32


def test_nearest_rank_and_interval_validity():
    vals = list(range(1, 1001))
    assert E.nearest_rank(vals, 0.025) == 25 and E.nearest_rank(vals, 0.975) == 975
    assert E.nearest_rank([5.0], 0.025) == 5.0
    reps = [{"a": 1.0, "b": math.nan}] * 3 + [{"a": 2.0, "b": 1.0}] * 2
    out = E.intervals(["a", "b"], reps, 5, 0.95)
    assert out["a"] == ((1.0, 2.0), 5)
    assert out["b"][1] == 2 and all(math.isnan(v) for v in out["b"][0])     # 2 valid of 5: fewer than half
