#!/usr/bin/env python3
"""What the contrast stage (xvit.augment.ContrastAugment, csrc/contrast.hip) costs, at B = 8 and B = 126, M = 2, 128^3 bf16:

  1. xvit_contrast_apply on copy records (flags 0), on bias + gamma records (pointwise path) and on blur + bias + gamma records with
     sigma 0.5, 1.0 and 2.0 on the three axes, beside x.clone() and beside the same transform composed of torch ops: three separable
     F.conv3d with replicate padding, an exp field multiply and a masked pow;
  2. xvit_contrast_draw;
  3. the whole stage con(aug(raw)) beside aug(raw) alone.

The arms of a table are interleaved: every round times each arm once; the table gives the median, minimum and maximum of the rounds in
microseconds (device events around `--launches` launches) and TB/s of source + destination bytes at the median.  The torch composition
works sample by sample (conv3d on the whole batch would need several more copies of it) and is timed with fewer launches.

    python tools/contrast_bench.py [--out FILE] [--rounds 7] [--launches 10] [--batches 8 126]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-attention-vit_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from xvit import _lib, augment, ops  # noqa: E402
import _contrast_check as K  # noqa: E402

BIAS = K.MIXED_BIAS


def torch_composition(x, sigma, bias, g, lo, hi):
    """The transform of one blur + bias + gamma record on x [N, 1, D, H, W] with torch ops (bf16 in and out, fp32 inside)."""
    v = x.float()
    for axis, s in zip((4, 3, 2), sigma[::-1]):                       # x, then y, then z
        R = min(int(np.ceil(3 * s)), 6)
        k = torch.arange(-R, R + 1, device=x.device, dtype=torch.float32)
        w = torch.exp(-k * k / (2 * s * s))
        w = (w / w.sum()).reshape([1, 1] + [2 * R + 1 if a == axis else 1 for a in (2, 3, 4)])
        pad = [0, 0, 0, 0, 0, 0]
        pad[2 * (4 - axis)] = pad[2 * (4 - axis) + 1] = R
        v = F.conv3d(F.pad(v, pad, mode="replicate"), w)
    D, H, W = v.shape[2:]
    uz, uy, ux = (torch.linspace(-1, 1, n, device=x.device).reshape([n if a == i else 1 for a in range(3)]) for i, n in enumerate((D, H, W)))
    m = (uz, uy, ux, uz * uz, uy * uy, ux * ux, uz * uy, uz * ux, uy * ux)
    v = v * torch.exp(sum(float(c) * t for c, t in zip(bias, m)))
    t = (v - lo) / (hi - lo)
    inside = (t >= 0) & (t <= 1)
    v = torch.where(inside, lo + (hi - lo) * t.clamp(0, 1).pow(g), v)
    return v.to(x.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 126])
    ap.add_argument("--size", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrast_bench: needs a GPU (no number is produced without one)")
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
            say(f"  {name:<44s} median {med:10.1f} us   min {min(t):10.1f}   max {max(t):10.1f}{rate}")
        return {name: statistics.median(t) for name, t in times.items()}

    say(f"# contrast_bench on {torch.cuda.get_device_name(0)}; library version {_lib.load().xvit_version()}; M = 2, {a.size}^3 bf16; "
        f"{a.rounds} interleaved rounds, {a.launches} launches per timing")
    n = a.size
    for B in a.batches:
        M = 2
        x = torch.rand(B, M, 1, n, n, n, device=dev).to(torch.bfloat16)
        nbytes = 2 * x.numel() * 2
        con = augment.ContrastAugment()

        def records(**kw):
            return torch.from_numpy(K.table(B * M, **kw)).reshape(B, M, K.NPARAM).to(dev)

        tabs = {"copy records (flags 0)": records(), "bias + gamma (pointwise path)": records(bias=BIAS, gamma=1.3)}
        for s in (0.5, 1.0, 2.0):
            tabs[f"blur sigma {s} + bias + gamma"] = records(sigma=(s, s, s), bias=BIAS, gamma=1.3)
        tabs["blur sigma 1.0 alone"] = records(sigma=(1.0, 1.0, 1.0))
        mixed = K.draw_ref(K.config(), B * M, seed=0)
        tabs["default mix (restated draw, seed 0)"] = torch.from_numpy(mixed).reshape(B, M, K.NPARAM).to(dev)
        arms = [("x.clone()", lambda: x.clone(), a.launches)]
        arms += [(f"contrast_apply: {name}", (lambda t: lambda: con.apply(x, t))(t), a.launches) for name, t in tabs.items()]

        def composed(s):
            def fn():
                for b in range(B):
                    torch_composition(x[b], (s, s, s), BIAS, 1.3, 0.0, 1.0)
            return fn

        arms += [(f"torch composition: blur sigma {s} + bias + gamma", composed(s), 1) for s in (0.5, 2.0)]
        say()
        flags = mixed[:, K.FLAGS].astype(int)
        say(f"## B = {B}: {B * M} volumes, {nbytes / 1e9:.3f} GB read + written per call "
            f"(default mix: {(flags & 1 > 0).sum()} blur, {(flags == 0).sum()} copy, {((flags & 1 == 0) & (flags > 0)).sum()} pointwise records)")
        table("apply", arms, nbytes)
        del arms, tabs

        params = torch.empty(B, M, K.NPARAM, device=dev)
        table("draw", [("contrast_draw", lambda: ops.contrast_draw(con.config, params, 0), 200)])

        raw = torch.randint(0, 1001, (B, M, n + 8, n - 4, n + 2), dtype=torch.int16, device=dev)
        aug = augment.VolumeAugment((n, n, n), intensity_scale=1 / 1000)
        stage = augment.ContrastAugment()
        table("stage", [("aug(raw)", lambda: aug(raw), a.launches), ("con(aug(raw))", lambda: stage(aug(raw)), a.launches)])
        del x, raw
        torch.cuda.empty_cache()

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
