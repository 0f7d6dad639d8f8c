#!/usr/bin/env python3
"""What the device-resident volume store (xvit.data, csrc/batch_store.hip) costs, on a 64-case store at B = 8, M = 2, 240 x 240 x 155 int16:

  1. xvit_batch_gather beside torch.index_select(store, 0, idx) and beside raw.clone() (the copy floor);
  2. xvit_batch_draw in its three modes;
  3. the captured training step with the input stage inside the graph, GraphedStep(source=...), at batch 8 with
     VolumeAugment(normalize="zscore") on the base model (128^3, 16^3 patches), beside the same work as eager aug(sampler()) followed by
     step(img, y) on a step captured without a source: wall time per step, host time per step in the running loop (until the last
     launch is issued; a replay waits there for room in the queue, so this follows the wall time), and the host time to issue ONE step on
     an idle GPU (what the host itself spends per step).

The arms of a table are interleaved: every round times each arm once; the table gives the median, minimum and maximum of the rounds in
microseconds (device events around the launches of one timing) and TB/s of source + destination bytes at the median.

    python tools/data_bench.py [--out FILE] [--rounds 7] [--launches 10] [--steps 30] [--cases 64]"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-attention-vit_amd"))
import xvit  # noqa: E402
from xvit import _lib, ops  # noqa: E402
from xvit.data import BatchSampler, VolumeStore, class_balanced_weights  # noqa: E402
from xvit.graph import GraphedStep  # noqa: E402
from xvit.optim import FusedAdam  # noqa: E402

CASE = (2, 240, 240, 155)


def base_config():
    return SimpleNamespace(hidden_dim=768, mlp_dim=3072, num_heads=12, num_multi_blocks=2, num_self_blocks=2, img_size=(128, 128, 128),
                           patch_size=(16, 16, 16), num_modalities=2, attn_order={"0": "1", "1": "0"}, num_classes=2, dropout=0.0, lr=1e-4,
                           weight_decay=0.0, optim_params={"T_max": 1, "eta_min": 0.0}, label_smoothing=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--cases", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("data_bench: needs a GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def events(fn, reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / reps          # microseconds per call

    def table(title, arms, nbytes=None):
        """arms: [(name, fn, launches)]; interleaved rounds after one warm-up call of each."""
        for _, fn, _ in arms:
            fn()
        times = {name: [] for name, _, _ in arms}
        for _ in range(a.rounds):
            for name, fn, reps in arms:
                times[name].append(events(fn, reps))
        say(f"{title}")
        for name, _, _ in arms:
            t = times[name]
            med = statistics.median(t)
            rate = f"  {nbytes / med / 1e6:6.2f} TB/s" if nbytes else ""
            say(f"  {name:<52s} median {med:10.1f} us   min {min(t):10.1f}   max {max(t):10.1f}{rate}")
        return {name: statistics.median(t) for name, t in times.items()}

    B, n = a.batch, a.cases
    say(f"# data_bench on {torch.cuda.get_device_name(0)}; library version {_lib.load().xvit_version()}; store of {n} cases of "
        f"{' x '.join(map(str, CASE))} int16, B = {B}; {a.rounds} interleaved rounds, {a.launches} launches per timing")
    store = VolumeStore(CASE, capacity=n, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for lo in range(0, n, 8):                                         # filled on the device: the bench is about what happens after loading
        k = min(8, n - lo)
        store.extend(torch.randint(0, 1001, (k,) + CASE, generator=g, device=dev, dtype=torch.int16), [(lo + i) % 2 for i in range(k)])
    nbytes = 2 * B * store.case_bytes
    say(f"\n## gather: {nbytes / 2e6:.1f} MB read + {nbytes / 2e6:.1f} MB written per call")
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:B].to(torch.int32).to(dev)
    idx64 = idx.to(torch.int64)
    out, y, status = torch.empty((B,) + CASE, dtype=torch.int16, device=dev), torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    sel_out = torch.empty_like(out)
    gather = table("gather", [
        ("raw.clone() (the copy floor)", lambda: out.clone(), a.launches),
        ("torch.index_select(store, 0, idx)", lambda: torch.index_select(store.volumes, 0, idx64), a.launches),
        ("torch.index_select(store, 0, idx, out=static)", lambda: torch.index_select(store.volumes, 0, idx64, out=sel_out), a.launches),
        ("xvit_batch_gather (+ labels, status)", lambda: ops.batch_gather(store.volumes, idx, n, labels=store.labels_dev, out=out, labels_out=y, status=status), a.launches),
    ], nbytes)
    assert torch.equal(out, torch.index_select(store.volumes, 0, idx64))
    ratio = gather["xvit_batch_gather (+ labels, status)"] / min(gather["torch.index_select(store, 0, idx)"], gather["torch.index_select(store, 0, idx, out=static)"])
    say(f"  xvit_batch_gather / torch.index_select (the faster form): {ratio:.3f}")
    del sel_out

    say("\n## draw")
    cdf = xvit.data.make_cdf(class_balanced_weights(store.labels[:n])).to(dev)
    ibuf = torch.empty(B, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    table("draw", [(f"xvit_batch_draw {name} (device counter, advance)",
                    (lambda m: lambda: ops.batch_draw(ibuf, m, n, 0, cdf=cdf, counter=counter, advance=True))(mode), 200)
                   for name, mode in (("weighted", _lib.BATCH_WEIGHTED), ("shuffle", _lib.BATCH_SHUFFLE), ("sequential", _lib.BATCH_SEQUENTIAL))])

    say(f"\n## training step at batch {B}: base model (128^3, 16^3 patches), FusedAdam(capturable) in the graph, VolumeAugment(normalize='zscore')")
    cfg = base_config()
    weights = class_balanced_weights(store.labels[:n])

    def build(with_source):
        torch.manual_seed(0)
        model = xvit.ModelCross(cfg).to(dev)
        model.train()
        opt = FusedAdam(model.parameters(), lr=1e-4, max_grad_norm=1.0, capturable=True)
        sampler = BatchSampler(store, B, mode="weighted", weights=weights, seed=0, capturable=True)
        aug = xvit.VolumeAugment(cfg.img_size, normalize="zscore", seed=0, capturable=True)
        img0 = aug(sampler()[0])
        y0 = sampler()[1].clone()
        if with_source:
            step = GraphedStep(model, img0, y0, optimizer=opt, source=lambda: (lambda r, t: (aug(r), t))(*sampler()))
            return step, (lambda: step())
        step = GraphedStep(model, img0, y0, optimizer=opt)

        def eager_input_then_replay():
            raw, t = sampler()
            step(aug(raw), t)
        return step, eager_input_then_replay

    def wall_and_host(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        idle = []
        for _ in range(a.steps):
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            fn()
            idle.append((time.perf_counter() - t3) * 1e3)
        torch.cuda.synchronize()
        return (t2 - t0) / a.steps * 1e3, (t1 - t0) / a.steps * 1e3, statistics.median(idle)

    arms = {}
    for name, with_source in (("captured step with source= (draw, gather, augment in the graph)", True),
                              ("eager aug(sampler()) + step(img, y)", False)):
        step, fn = build(with_source)
        arms[name] = (step, fn)
    results = {name: [] for name in arms}
    for _ in range(a.rounds):
        for name, (_, fn) in arms.items():
            results[name].append(wall_and_host(fn))
    for name, r in results.items():
        wall, host, idle = ([t[i] for t in r] for i in range(3))
        say(f"  {name:<68s} wall {statistics.median(wall):7.3f} ms/step (min {min(wall):7.3f}, max {max(wall):7.3f})   "
            f"host in the loop {statistics.median(host):7.3f} ms/step (min {min(host):7.3f}, max {max(host):7.3f})   "
            f"host to issue one step, GPU idle {statistics.median(idle):7.3f} ms (min {min(idle):7.3f}, max {max(idle):7.3f})")
    say(f"  ({a.steps} steps per timing after 3 untimed; host in the loop = until the last launch of the timing is issued, before the synchronisation; "
        "idle = one step issued after a synchronisation, median of the steps)")

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
