#!/usr/bin/env python3
"""What masked-volume pretraining (xvit.MaskedVolumeModel, csrc/mae.hip) costs at configs[1]:

  1. the eager pretraining step (fwd + bwd) at mask ratio 0.5 and 0.75 beside the supervised ModelCross step at the same batch: the
     largest of --eager-batches that fits;
  2. the same three as one HIP graph each at --graph-batch;
  3. the loss stage alone (xvit_mae_loss_fwd + xvit_mae_loss_bwd) at the eager batch and mask ratio 0.75, with its algorithmic bytes from
     the shapes (voxels read twice, pred read twice, dpred written once) over the time, as a share of 6.3 TB/s, against the composed
     alternative: xvit_patchify_select on drop_idx to a stored target, then torch mean / var / mse and their autograd backward.

The arms of a table are interleaved (every round times each arm once), timed with device events around --steps steps, after a warm-up
of every arm; the table gives the median, minimum and maximum of the rounds.

    python tools/mae_bench.py [--out FILE] [--rounds 5] [--steps 3]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-attention-vit_amd"))
sys.path.insert(0, ROOT)
import xvit  # noqa: E402
from xvit import ops  # noqa: E402
from bench import base_config  # noqa: E402

HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--eager-batches", type=int, nargs="+", default=[126, 64, 32])
    ap.add_argument("--graph-batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-graph", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mae_bench: needs a GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cfg = base_config()
    M, patch = cfg.num_modalities, tuple(cfg.patch_size)
    P, pd = 1, patch[0] * patch[1] * patch[2]
    for s, p in zip(cfg.img_size, cfg.patch_size):
        P *= s // p
    torch.manual_seed(0)
    sup = xvit.ModelCross(base_config()).to(dev).train()
    maes = {r: xvit.MaskedVolumeModel(base_config(), mask_ratio=r).to(dev).train() for r in (0.5, 0.75)}

    def inputs(B):
        g = torch.Generator().manual_seed(1)
        return torch.randn(B, M, 1, *cfg.img_size, generator=g).to(dev, torch.bfloat16), torch.randint(0, 2, (B,), generator=g).to(dev)

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(a.steps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.steps

    def table(title, arms, base_key, extra=None):
        say(title)
        for _ in range(2):                      # warm every arm: code objects, allocator pools, tile choices
            for fn in arms.values():
                fn()
        samples = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                samples[k].append(timed(fn))
        base = statistics.median(samples[base_key])
        for k in arms:
            med = statistics.median(samples[k])
            say(f"  {k:34s} median {med:9.3f} ms  (min {min(samples[k]):9.3f}, max {max(samples[k]):9.3f})   {med / base:6.3f} x {base_key}" + (extra(k, med) if extra else ""))
        return {k: statistics.median(v) for k, v in samples.items()}

    def eager(model):
        def fn():
            for p in model.parameters():
                p.grad = None
            xvit.invalidate_shadows()           # the weights change every step in training: re-cast them
            model(img, labels)[1].backward()
        return fn

    say(f"mae_bench: configs[1] (d = {cfg.hidden_dim}, {M} x {'x'.join(map(str, cfg.img_size))}, {'x'.join(map(str, patch))} patches, P = {P}, pd = {pd}); decoder 512 x 2; "
        f"{a.rounds} rounds x {a.steps} steps per arm, interleaved; device events")

    # 1. eager fwd + bwd at the largest batch that fits
    B = None
    for cand in a.eager_batches:
        try:
            img, labels = inputs(cand)
            for fn in (eager(sup), eager(maes[0.5]), eager(maes[0.75])):
                fn()
            torch.cuda.synchronize()
            B = cand
            break
        except torch.cuda.OutOfMemoryError:
            say(f"  (batch {cand} does not fit)")
            img = labels = None
            for m in (sup, *maes.values()):
                for p in m.parameters():
                    p.grad = None
            torch.cuda.empty_cache()
    if B is None:
        raise SystemExit("mae_bench: none of the eager batches fits")
    arms = {"supervised ModelCross": eager(sup)}
    arms.update({f"MAE mask_ratio {r:.2f} (K = {maes[r].num_kept})": eager(maes[r]) for r in maes})
    table(f"\n1. eager training step (fwd + bwd), batch {B}", arms, "supervised ModelCross")

    # 3. the loss stage alone at this batch, mask ratio 0.75
    K, Rm = maes[0.75].num_kept, maes[0.75].num_dropped
    S = M * B
    rows = S * Rm
    keep_idx, slot = torch.empty(S, K, dtype=torch.int32, device=dev), torch.empty(S, P, dtype=torch.int32, device=dev)
    ops.token_select_draw(keep_idx, slot, B, False, 12345)
    drop_idx, _ = ops.token_select_complement(slot, K)
    g = torch.Generator().manual_seed(2)
    pred = torch.randn(rows, pd, generator=g).to(dev, torch.bfloat16)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    dpred = torch.empty_like(pred)
    algo = rows * pd * (2 * img.element_size() + 2 * pred.element_size() + pred.element_size())

    def fused():
        _, _, _, stats = ops.mae_loss_fwd(pred, drop_idx, img, patch, True)
        ops.mae_loss_bwd(pred, drop_idx, img, patch, stats, one, out=dpred)

    def composed():
        target = ops.patchify_select(img, patch, drop_idx).reshape(S, Rm + 1, pd)[:, 1:].reshape(rows, pd).float()      # the stored target matrix
        mean = target.mean(dim=1, keepdim=True)
        target = (target - mean) / torch.sqrt(target.var(dim=1, unbiased=True, keepdim=True) + 1e-6)
        p = pred.detach().requires_grad_()
        ((p.float() - target) ** 2).mean().backward()

    def share(k, med):
        return f"   {algo / 1e9:.2f} GB algorithmic -> {algo / med / 1e9:.2f} TB/s = {100 * algo / med / 1e9 / HBM_TBS:.0f} % of {HBM_TBS} TB/s" if k.startswith("fused") else ""

    table(f"\n3. loss stage alone (fwd + bwd), batch {B}, mask ratio 0.75: {rows} rows of {pd} voxels, bf16 volume and prediction, norm_pix",
          {"fused xvit_mae_loss_fwd + _bwd": fused, "composed (stored target + torch)": composed}, "fused xvit_mae_loss_fwd + _bwd", share)
    del pred, dpred, img, labels
    for m in (sup, *maes.values()):
        for p in m.parameters():
            p.grad = None
    torch.cuda.empty_cache()

    # 2. the captured step
    if not a.skip_graph:
        from xvit.graph import GraphedStep
        img, labels = inputs(a.graph_batch)
        steps = {"supervised ModelCross": GraphedStep(sup, img, labels)}
        steps.update({f"MAE mask_ratio {r:.2f} (K = {maes[r].num_kept})": GraphedStep(maes[r], img, labels) for r in maes})
        table(f"\n2. captured training step (one HIP graph, fwd + bwd), batch {a.graph_batch}", {k: (lambda s=s: s(img, labels)) for k, s in steps.items()}, "supervised ModelCross")
    say(f"\npeak memory over the whole run {torch.cuda.max_memory_allocated() / 1e9:.1f} GB (three models resident)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
