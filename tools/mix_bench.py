#!/usr/bin/env python3
"""What Mixup / CutMix (ModelCross(config.mixup_alpha / cutmix_alpha), csrc/mix.hip) costs at configs[1], at batch 126 (eager) and 8
(captured):

  1. xvit_mix_apply on a whole batch of mixup records, of CutMix records and of copy records, against the torch composition of the same
     result: lam * x + (1 - lam) * x[perm], and a clone with the partner's box slice-assigned into it;
  2. xvit_mean_ce_mix against xvit_mean_ce;
  3. the eager training step (fwd + bwd) and the captured one with mixing off and on.

The arms of a table are interleaved: every round times each arm once, so drift of the machine lands on all of them alike; the table gives
the median, minimum and maximum of the rounds.  Kernels are timed with device events around `--launches` launches, steps with the host
clock between two device synchronisations.  Bytes are the ones the algorithm needs, from the shapes: a mixup voxel is two reads and a write,
a CutMix or copied voxel one read and one write.

    python tools/mix_bench.py [--out FILE] [--rounds 7] [--launches 10] [--steps 10]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-attention-vit_amd"))
sys.path.insert(0, ROOT)
import xvit  # noqa: E402
from xvit import _lib, ops  # noqa: E402
from bench import base_config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--eager-batch", type=int, default=126)
    ap.add_argument("--graph-batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: needs a GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cfg0 = base_config()
    M = cfg0.num_modalities
    D, H, W = cfg0.img_size

    def inputs(B):
        g = torch.Generator().manual_seed(1)
        return torch.randn(B, M, 1, D, H, W, generator=g).to(dev, torch.bfloat16), torch.randint(0, cfg0.num_classes, (B,), generator=g).to(dev)

    def events(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(a.launches):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.launches * 1e3     # us

    def host(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3   # ms

    def table(title, arms, timer, unit, nbytes=None):
        say(title)
        for _ in range(3):                      # warm every arm: code objects, allocator pools
            for fn in arms.values():
                fn()
        samples = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                samples[k].append(timer(fn))
        med = {k: statistics.median(v) for k, v in samples.items()}
        for k in arms:
            rate = f"   {nbytes[k] / med[k] / 1e3:8.1f} GB/s" if nbytes and nbytes.get(k) and unit == "us" else ""
            say(f"  {k:44s} median {med[k]:10.3f} {unit}  (min {min(samples[k]):10.3f}, max {max(samples[k]):10.3f}){rate}")
        return med

    say(f"mix_bench: configs[1] volumes {M} x {D}x{H}x{W} bf16; {a.rounds} rounds, interleaved; kernels: device events around {a.launches} launches; "
        f"steps: host clock around {a.steps} steps between device synchronisations")

    def record(mode, partner, lam, box=(0,) * 6):
        r = [0.0] * _lib.MIX_NPARAM
        r[_lib.MIX_MODE], r[_lib.MIX_PARTNER], r[_lib.MIX_LAM], r[_lib.MIX_OML] = mode, partner, lam, 1.0 - lam
        r[_lib.MIX_BOX:_lib.MIX_BOX + 6] = box
        return r

    for B in (a.eager_batch, a.graph_batch):
        img, labels = inputs(B)
        size = img.numel() * img.element_size()
        out = torch.empty_like(img)
        perm = (torch.arange(B, device=dev) + 1) % B
        lam = 0.3
        ext = [int(s * 0.5 ** (1.0 / 3.0)) for s in (D, H, W)]                   # lam0 = 0.5: the box holds half the volume
        box = tuple(v for s, e in zip((D, H, W), ext) for v in ((s - e) // 2, (s - e) // 2 + e))
        frac = ext[0] * ext[1] * ext[2] / (D * H * W)
        tab = {k: torch.tensor(v, dtype=torch.float32, device=dev) for k, v in {
            "mixup": [record(1, (b + 1) % B, lam) for b in range(B)], "cutmix": [record(2, (b + 1) % B, 1.0 - frac, box) for b in range(B)],
            "copy": [record(0, b, 1.0) for b in range(B)]}.items()}
        lam_t = torch.full((B, 1, 1, 1, 1, 1), lam, dtype=torch.bfloat16, device=dev)
        d0, d1, h0, h1, w0, w1 = box

        def torch_mixup():
            return lam_t * img + (1 - lam_t) * img[perm]

        def torch_cutmix():
            y = img.clone()
            y[:, :, :, d0:d1, h0:h1, w0:w1] = img[perm][:, :, :, d0:d1, h0:h1, w0:w1]
            return y

        arms = {"xvit_mix_apply, mixup records": lambda: ops.mix_apply(img, tab["mixup"], out=out),
                "torch lam * x + (1 - lam) * x[perm]": torch_mixup,
                "xvit_mix_apply, CutMix records": lambda: ops.mix_apply(img, tab["cutmix"], out=out),
                "torch clone + box slice-assign of x[perm]": torch_cutmix,
                "xvit_mix_apply, copy records": lambda: ops.mix_apply(img, tab["copy"], out=out),
                "torch x.clone()": lambda: img.clone(),
                "xvit_mix_apply, mixup records (again)": lambda: ops.mix_apply(img, tab["mixup"], out=out)}
        nbytes = {k: (3 if "mixup" in k or "lam" in k else 2) * size for k in arms}
        med = table(f"\n1. apply, batch {B}: {size / 1e6:.1f} MB of volumes; mixup moves {3 * size / 1e9:.2f} GB, CutMix and copy {2 * size / 1e9:.2f} GB "
                    f"(GB/s = those bytes over the time, for the torch arms too, whatever they really move); box {box} = {frac:.3f} of the volume",
                    arms, events, "us", nbytes)
        say(f"  mixup: kernel / torch = {med['xvit_mix_apply, mixup records'] / med['torch lam * x + (1 - lam) * x[perm]']:.3f};  "
            f"CutMix: kernel / torch = {med['xvit_mix_apply, CutMix records'] / med['torch clone + box slice-assign of x[perm]']:.3f};  "
            f"the two identical mixup arms differ by {abs(med['xvit_mix_apply, mixup records'] - med['xvit_mix_apply, mixup records (again)']):.2f} us")

        lm = torch.randn(M, B, cfg0.num_classes, device=dev)
        table(f"\n2. loss, batch {B} (M = {M}, C = {cfg0.num_classes})",
              {"xvit_mean_ce": lambda: ops.mean_ce(lm, labels, 0.1), "xvit_mean_ce_mix, mixup records": lambda: ops.mean_ce_mix(lm, labels, tab["mixup"], 0.1),
               "xvit_mean_ce (again)": lambda: ops.mean_ce(lm, labels, 0.1)}, events, "us")
        cfgd = _lib.MixConfig(0.8, 1.0, 1.0, 0.5, 1)
        drawn = torch.empty(B, _lib.MIX_NPARAM, dtype=torch.float32, device=dev)
        table(f"\n   draw, batch {B}", {"xvit_mix_draw (both alphas, per sample)": lambda: ops.mix_draw(cfgd, drawn, (D, H, W), 12345)}, events, "us")
        del img, out, tab
        torch.cuda.empty_cache()

    # 3. the training step, mixing off and on (timm's usual pair: mixup 0.8, cutmix 1.0, switch 0.5, per batch)
    torch.manual_seed(0)
    models = {}
    for name, over in (("mixing off", {}), ("mixup 0.8 + cutmix 1.0", dict(mixup_alpha=0.8, cutmix_alpha=1.0)), ("mixup 0.8 alone", dict(mixup_alpha=0.8))):
        cfg = base_config()
        for k, v in over.items():
            setattr(cfg, k, v)
        models[name] = xvit.ModelCross(cfg).to(dev)
        if len(models) > 1:
            models[name].load_state_dict(models["mixing off"].state_dict())
        models[name].train()
    models["mixing off (again)"] = models["mixing off"]

    img, labels = inputs(a.eager_batch)

    def eager(model):
        def fn():
            for p in model.parameters():
                p.grad = None
            xvit.invalidate_shadows()           # the weights change every step in training: re-cast them
            model(img, labels)[1].backward()
        return fn

    table(f"\n3. eager training step (fwd + bwd), batch {a.eager_batch}", {k: eager(m) for k, m in models.items()}, host, "ms")
    del img, labels
    torch.cuda.empty_cache()

    from xvit.graph import GraphedStep
    img, labels = inputs(a.graph_batch)
    steps = {k: GraphedStep(m, img, labels) for k, m in models.items() if "again" not in k}
    steps["mixing off (again)"] = steps["mixing off"]
    table(f"\n4. captured training step (one HIP graph, fwd + bwd), batch {a.graph_batch}", {k: (lambda s=s: s(img, labels)) for k, s in steps.items()}, host, "ms")
    say(f"\npeak memory over the whole run {torch.cuda.max_memory_allocated() / 1e9:.1f} GB")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
