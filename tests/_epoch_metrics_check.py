"""NumPy / Python-integer restatement of the pooled epoch metrics (include/xvit.h, "Pooled epoch metrics"; xvit.metrics.EpochMetrics).

The reference of tests/test_epoch_metrics_*: float64 softmax, integer confusion, the hash and the draw rule in Python integers, the
tie-aware sums in Python integers, the average precision in float64 (math.fsum), nearest-rank intervals.  It shares no code with the
package; tests/test_epoch_metrics_gate_cpu.py pins it against scikit-learn and a brute-force pair count."""
import math

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
HEAD, STORED, SEEN, STEPS, IGNORED, NONFINITE, OVERFLOW = 8, 0, 1, 2, 3, 4, 5      # include/xvit.h, XVIT_EPOCH_*


def hash32(seed, idx):
    """hash32 of csrc/xvit_common.h in Python integers."""
    z = (idx * GOLDEN + seed) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return ((z ^ (z >> 31)) >> 16) & 0xFFFFFFFF


def draw_weights(seed, r, n):
    """Multiplicities of replicate r over n samples: replicate 0 is all ones; r >= 1 draws n indices with replacement."""
    if r == 0:
        return [1] * n
    rs = (seed + r * GOLDEN) & M64
    w = [0] * n
    for k in range(n):
        w[(hash32(rs, k) * n) >> 32] += 1
    return w


def softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def update_reference(steps, C, cap):
    """What the epoch buffers hold after xvit_epoch_metrics_update over `steps` [(logits fp32 [B, C], labels [B]), ...]."""
    rows, labs, preds = [], [], []
    conf = np.zeros((C, C), dtype=np.int64)
    cnt = {"stored": 0, "seen": 0, "steps": 0, "ignored": 0, "nonfinite": 0, "overflow": 0}
    for logits, labels in steps:
        lg = np.asarray(logits, dtype=np.float32)
        cnt["steps"] += 1
        cnt["seen"] += len(lg)
        for row, y in zip(lg, np.asarray(labels).tolist()):
            if not 0 <= y < C:
                cnt["ignored"] += 1
            elif not np.isfinite(row).all():
                cnt["nonfinite"] += 1
            else:
                p = int(np.argmax(row))            # first maximum
                conf[y, p] += 1
                if cnt["stored"] < cap:
                    rows.append(row)
                    labs.append(y)
                    preds.append(p)
                    cnt["stored"] += 1
                else:
                    cnt["overflow"] += 1
    scores = softmax64(np.stack(rows)) if rows else np.zeros((0, C))
    return scores, np.array(labs, dtype=np.int64), np.array(preds, dtype=np.int64), conf, cnt


def rank_sums(score, pos, w):
    """Tie-aware sums of one (replicate, class): score[i] (any float), pos[i] (bool), w[i] (int multiplicity) -> (u2, wpos, wneg, ap)."""
    n = len(score)
    order = sorted(range(n), key=lambda i: -score[i])
    wpos = sum(w[i] for i in range(n) if pos[i])
    wneg = sum(w[i] for i in range(n) if not pos[i])
    u2, cp, cn, terms, j = 0, 0, 0, [], 0
    while j < n:
        k, gp, gn = j, 0, 0
        while k < n and score[order[k]] == score[order[j]]:
            if pos[order[k]]:
                gp += w[order[k]]
            else:
                gn += w[order[k]]
            k += 1
        cp += gp
        cn += gn
        u2 += gp * (2 * (wneg - cn) + gn)
        if gp > 0:
            terms.append(gp * cp / (cp + cn))
        j = k
    ap = math.fsum(terms) / wpos if wpos > 0 else 0.0
    return u2, wpos, wneg, ap


def confusion(labels, preds, w, C):
    conf = np.zeros((C, C), dtype=np.int64)
    for y, p, m in zip(labels, preds, w):
        conf[y, p] += m
    return conf


def rank_stats_reference(scores, labels, preds, C, R, seed):
    """(u2, wpos, wneg) int [R + 1, C, 3], ap float64 [R + 1, C], conf int [R + 1, C, C] of xvit_epoch_rank_stats."""
    n = len(labels)
    sc = np.asarray(scores)
    labels, preds = [int(v) for v in labels], [int(v) for v in preds]
    ranks = np.zeros((R + 1, C, 3), dtype=np.int64)
    ap = np.zeros((R + 1, C))
    conf = np.zeros((R + 1, C, C), dtype=np.int64)
    cols = [sc[:, c].tolist() if n else [] for c in range(C)]
    for r in range(R + 1):
        w = draw_weights(seed, r, n)
        assert sum(w) == n
        conf[r] = confusion(labels, preds, w, C)
        for c in range(C):
            u2, wp, wn, a = rank_sums(cols[c], [y == c for y in labels], w)
            ranks[r, c] = (u2, wp, wn)
            ap[r, c] = a
    return ranks, ap, conf


def _div(a, b):
    return a / b if b > 0 else 0.0          # torchmetrics' _safe_divide


def scalars(conf, ranks, ap):
    """Every scalar of EpochMetrics.compute() from one replicate's integers: conf [C, C], ranks [C, 3], ap [C].  nan = undefined."""
    C = conf.shape[0]
    conf = [[int(v) for v in row] for row in conf]
    total = sum(map(sum, conf))
    out = {"acc": _div(sum(conf[c][c] for c in range(C)), total)}
    per = {k: [] for k in ("prec", "rec", "spec", "f1", "npv")}
    present = []
    for c in range(C):
        tp = conf[c][c]
        fn = sum(conf[c]) - tp
        fp = sum(conf[k][c] for k in range(C)) - tp
        tn = total - tp - fn - fp
        vals = {"prec": _div(tp, tp + fp), "rec": _div(tp, tp + fn), "spec": _div(tn, tn + fp), "f1": _div(2 * tp, 2 * tp + fp + fn), "npv": _div(tn, tn + fn)}
        for k, v in vals.items():
            out[f"{k}_{c}"] = v
            per[k].append(v)
        if tp + fn > 0:
            present.append(vals["rec"])
    out["balanced_acc"] = math.fsum(present) / len(present) if present else 0.0      # recall averaged over the classes that occur
    for k, v in per.items():
        out[f"macro_{k}"] = math.fsum(v) / C
    au, aps = [], []
    for c in range(C):
        u2, wp, wn = (int(v) for v in ranks[c])
        ok = wp > 0 and wn > 0
        au.append(0.5 * u2 / (wp * wn) if ok else math.nan)
        aps.append(float(ap[c]) if ok else math.nan)
        out[f"auroc_{c}"], out[f"ap_{c}"] = au[-1], aps[-1]
    out["macro_auroc"] = math.fsum(au) / C      # nan as soon as one class is undefined
    out["macro_ap"] = math.fsum(aps) / C
    if C == 2:
        out["auc_roc"] = out["auroc_1"]
    return out


def nearest_rank(values, q):
    """The max(1, ceil(q m))-th smallest of the m values (q m rounded to 1e-9 first, so that 0.025 * 1000 is 25)."""
    v = sorted(values)
    k = max(1, math.ceil(round(q * len(v), 9)))
    return v[min(k, len(v)) - 1]


def intervals(point_keys, replicate_scalars, R, ci):
    """{key: ((lo, hi), valid)} over the replicates' scalars; fewer valid replicates than R / 2 give nan bounds."""
    out = {}
    for k in point_keys:
        vals = [s[k] for s in replicate_scalars if not math.isnan(s[k])]
        if 2 * len(vals) < R or not vals:
            out[k] = ((math.nan, math.nan), len(vals))
        else:
            out[k] = ((nearest_rank(vals, (1.0 - ci) / 2.0), nearest_rank(vals, (1.0 + ci) / 2.0)), len(vals))
    return out


def epoch_reference(scores, labels, preds, C, R=0, seed=0, ci=0.95):
    """Point scalars and intervals of an epoch whose kept rows are (scores, labels, preds): ({key: value}, {key: ((lo, hi), valid)})."""
    ranks, ap, conf = rank_stats_reference(scores, labels, preds, C, R, seed)
    point = scalars(conf[0], ranks[0], ap[0])
    reps = [scalars(conf[r], ranks[r], ap[r]) for r in range(1, R + 1)]
    return point, (intervals(point.keys(), reps, R, ci) if R > 0 else {})


def ap_bound(n):
    """Relative bound on the fp64 average precision: one division per term and at most n additions of non-negative terms."""
    return (n + 2) * 2.0 ** -53 * 1.01
