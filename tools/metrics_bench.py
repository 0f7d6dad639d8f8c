#!/usr/bin/env python3
"""What the pooled epoch metrics (xvit.metrics.EpochMetrics, csrc/epoch_metrics.hip) cost:

  1. the per-step launch, xvit_epoch_metrics_update, at B = 126 and B = 8 for C = 2 and C = 3, beside xvit_binary_metrics_step at the same
     shapes (C = 2).  The new kernel also appends the rows, so the two are written side by side with no required ratio; what matters is
     that a step stays one launch with no host synchronisation;
  2. the epoch end at (n, C, R): the per-class sort (torch.sort), xvit_epoch_rank_stats, and the host's float64 arithmetic on the
     (R + 1) x C outputs, each on its own, and compute() as a whole;
  3. the same replicates through the NumPy / Python-integer restatement of the tests (tests/_epoch_metrics_check.py) on the host CPU:
     `--reference-replicates` replicates are timed and the time per replicate is scaled to R.

The arms of a table are interleaved: every round times each arm once; the table gives the median, minimum and maximum of the rounds.
Kernels are timed with device events around `--launches` launches (update) or one launch (rank statistics), host work with the host
clock between two device synchronisations.

    python tools/metrics_bench.py [--out FILE] [--rounds 9] [--launches 200] [--reference-replicates 2]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-attention-vit_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from xvit import _lib, metrics, ops  # noqa: E402
import _epoch_metrics_check as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reference-replicates", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench: needs a GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def events(fn, reps=1):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / reps          # microseconds per call

    def host(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e6, out

    def table(arms, rounds, prepare=None):
        times = {k: [] for k in arms}
        for _ in range(rounds + 1):                    # the first round warms every arm up and is dropped
            for k, fn in arms.items():
                if prepare:
                    prepare()
                times[k].append(fn())
        return {k: (statistics.median(v[1:]), min(v[1:]), max(v[1:])) for k, v in times.items()}

    say(f"# metrics_bench on {torch.cuda.get_device_name(0)}; library version {_lib.load().xvit_version()}; microseconds")
    say()
    say(f"## 1. per-step launch (device events around {a.launches} launches, {a.rounds} interleaved rounds: median [min, max] per launch)")
    g = torch.Generator().manual_seed(0)
    for B in (126, 8):
        arms, accs = {}, []
        for C in (2, 3):
            lg, lb = torch.randn(B, C, generator=g).to(dev), torch.randint(0, C, (B,), generator=g).to(dev)
            acc = metrics.EpochMetrics(C, dev, capacity=B * a.launches)
            accs.append(acc)
            arms[f"xvit_epoch_metrics_update C={C}"] = (lambda acc=acc, lg=lg, lb=lb: events(lambda: acc.update(lg, lb), a.launches))
            if C == 2:
                ref = metrics.BinaryEpochMetrics(dev)
                arms["xvit_binary_metrics_step  C=2"] = (lambda ref=ref, lg=lg, lb=lb: events(lambda: ref.update(lg, lb), a.launches))
        res = table(arms, a.rounds, prepare=lambda: [x.reset() for x in accs])
        for k, (med, lo, hi) in res.items():
            say(f"B={B:4d}  {k}: {med:7.2f} [{lo:7.2f}, {hi:7.2f}]")
    say("   (back-to-back launches from Python: both arms include the host's enqueue cost where that exceeds the kernel)")
    say()

    say(f"## 2. epoch end ({a.rounds} rounds: median [min, max]); 3. the restatement on the host CPU, scaled from {a.reference_replicates} replicates")
    limit = ops.epoch_rank_stats_max_n()
    for n, C, R in ((512, 2, 1000), (8192, 3, 1000), (limit, 3, 0), (limit, 3, 1000)):
        acc = metrics.EpochMetrics(C, dev, capacity=n, bootstrap=R, seed=1)
        logits, labels = torch.randn(n, C, generator=g), torch.randint(0, C, (n,), generator=g)
        for i in range(0, n, 8192):
            acc.update(logits[i:i + 8192].to(dev), labels[i:i + 8192].to(dev))
        n_dev = acc.state[:1]
        perm = [None]
        out = [None]

        def sort():
            perm[0] = acc.scores[:n].t().contiguous().sort(dim=1, descending=True).indices

        def rank():
            out[0] = ops.epoch_rank_stats(acc.scores, acc.labels32, acc.preds, perm[0], n_dev, n, R, 1)

        def host_part():
            ranks, apv, conf = (t.cpu() for t in out[0])
            vals = metrics._scalars(conf.double(), ranks.double(), apv)
            for v in vals.values():
                reps = sorted(v[1:][~torch.isnan(v[1:])].tolist())
                if reps:
                    metrics._nearest_rank(reps, 0.025), metrics._nearest_rank(reps, 0.975)
            return vals

        sort()
        res = table({"sort": lambda: events(sort), "rank kernel": lambda: events(rank), "host float64": lambda: host(host_part)[0],
                     "compute() in all": lambda: host(lambda: acc.compute(sync_dist=False))[0]}, a.rounds)
        say(f"n={n:6d} C={C} R={R:5d}  " + "  ".join(f"{k}: {med:9.1f} [{lo:9.1f}, {hi:9.1f}]" for k, (med, lo, hi) in res.items()))
        k = min(a.reference_replicates, R)
        sc, lb, pr = acc.scores[:n].cpu().numpy(), acc.labels32[:n].cpu().numpy(), acc.preds[:n].cpu().numpy()
        t = time.perf_counter()
        E.rank_stats_reference(sc, lb, pr, C, k, 1)
        per = (time.perf_counter() - t) * 1e6 / (k + 1)
        gpu = res["sort"][0] + res["rank kernel"][0]
        say(f"                          restatement: {per:.0f} per replicate, {per * (R + 1):.3e} for R + 1 = {R + 1} (scaled); "
            f"sort + kernel = {gpu:.1f}: ratio {per * (R + 1) / gpu:.0f}x")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
