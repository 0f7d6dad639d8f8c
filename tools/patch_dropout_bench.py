#!/usr/bin/env python3
"""What patch dropout (ModelCross(config.patch_dropout), csrc/token_select.hip) buys at configs[1]: the fwd+bwd training step at
patch_dropout 0 / 0.25 / 0.5 / 0.75, eagerly at batch 126 and as one HIP graph at batch 8, and the embedding stage alone (draw +
patchify_select + NT GEMM + embed_select_fwd) against the fused gather embedding it bypasses.

The arms are interleaved: every round times each rate once (`--steps` steps between two device synchronisations), so drift of the machine
lands on all of them alike; the table gives the median, minimum and maximum of the rounds.  Rate 0 launches nothing new: it is the
baseline the other rows are divided by, and the number to hold against the step time of the commit before this feature.

    python tools/patch_dropout_bench.py [--out FILE] [--rounds 7] [--steps 10]"""
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
import xvit.functional as XF  # noqa: E402
from xvit import ops  # noqa: E402
from bench import base_config  # noqa: E402

RATES = (0.0, 0.25, 0.5, 0.75)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--eager-batch", type=int, default=126)
    ap.add_argument("--graph-batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("patch_dropout_bench: needs a GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cfg0 = base_config()
    M, d = cfg0.num_modalities, cfg0.hidden_dim
    P = 1
    for s, p in zip(cfg0.img_size, cfg0.patch_size):
        P *= s // p
    torch.manual_seed(0)
    models = {}
    for rate in RATES:
        cfg = base_config()
        cfg.patch_dropout = rate
        models[rate] = xvit.ModelCross(cfg).to(dev)
        if rate != RATES[0]:
            models[rate].load_state_dict(models[RATES[0]].state_dict())
        models[rate].train()
    keep = {rate: P if rate == 0.0 else XF.patch_keep_count(P, rate) for rate in RATES}

    def inputs(B):
        g = torch.Generator().manual_seed(1)
        return torch.randn(B, M, 1, *cfg0.img_size, generator=g).to(dev, torch.bfloat16), torch.randint(0, 2, (B,), generator=g).to(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3

    def table(title, arms, unit="ms"):
        say(title)
        for _ in range(3):                      # warm every arm: code objects, allocator pools, tile choices
            for fn in arms.values():
                fn()
        samples = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                samples[k].append(timed(fn))
        base = statistics.median(samples[RATES[0]])
        for k in arms:
            med = statistics.median(samples[k])
            say(f"  patch_dropout {k:4.2f}   K = {keep[k]:4d}  N = {keep[k] + 1:4d}   median {med:8.3f} {unit}  (min {min(samples[k]):8.3f}, max {max(samples[k]):8.3f})   {med / base:5.3f} x rate 0")
        return samples

    say(f"patch_dropout_bench: configs[1] (d = {d}, {M} x {'x'.join(map(str, cfg0.img_size))}, {'x'.join(map(str, cfg0.patch_size))} patches, P = {P}); "
        f"{a.rounds} rounds x {a.steps} steps per arm, interleaved; host clock between device synchronisations")

    # 1. eager fwd + bwd
    img, labels = inputs(a.eager_batch)

    def eager(model):
        def fn():
            for p in model.parameters():
                p.grad = None
            xvit.invalidate_shadows()           # the weights change every step in training: re-cast them
            model(img, labels)[1].backward()
        return fn

    table(f"\n1. eager training step (fwd + bwd), batch {a.eager_batch}", {r: eager(models[r]) for r in RATES})

    # 2. the embedding stage alone at the same batch (forward only): its launches back to back, timed like the steps
    w_b = models[0.0].patch_to_embedding.weight.detach().to(torch.bfloat16)
    bias, cls = models[0.0].patch_to_embedding.bias.detach(), models[0.0].cls_token.detach().reshape(d)
    pos = models[0.0].pos_embedding.detach().reshape(P + 1, d)
    patch = tuple(cfg0.patch_size)
    S = M * a.eager_batch
    fused_ok = ops.patch_embed_supported(img, patch, d)

    def embed_parent():
        if fused_ok:
            x = ops.patch_embed_fwd(img, patch, w_b, bias, pos)
        else:
            x = torch.empty(S * (P + 1), d, dtype=torch.float32, device=dev)
            ops.gemm(ops.NT, ops.patchify(img, patch, pad_cls_row=True).reshape(S * (P + 1), -1), w_b, x, bias=bias, residual=pos, res_row_mod=P + 1, res_row_off=0)
        ops.cls_row_fwd(cls, pos, x, S, P + 1, d)

    def embed_selected(K):
        keep_idx, slot = torch.empty(S, K, dtype=torch.int32, device=dev), torch.empty(S, P, dtype=torch.int32, device=dev)

        def fn():
            ops.token_select_draw(keep_idx, slot, a.eager_batch, False, 12345)
            patches = ops.patchify_select(img, patch, keep_idx).reshape(S * (K + 1), -1)
            x = torch.empty(S * (K + 1), d, dtype=torch.float32, device=dev)
            ops.gemm(ops.NT, patches, w_b, x, bias=bias)
            ops.embed_select_fwd(x, cls, pos, keep_idx)
        return fn

    arms = {0.0: embed_parent}
    arms.update({r: embed_selected(keep[r]) for r in RATES[1:]})
    table(f"\n2. embedding stage alone, forward, batch {a.eager_batch}: rate 0 = the {'fused gather embedding' if fused_ok else 'stored-matrix embedding'} + CLS row "
          "(what rate 0 runs); other rates = draw + patchify_select + NT GEMM + embed_select_fwd", arms)
    del img, labels, arms
    torch.cuda.empty_cache()

    # 3. the captured step
    from xvit.graph import GraphedStep
    img, labels = inputs(a.graph_batch)
    steps = {r: GraphedStep(models[r], img, labels) for r in RATES}
    table(f"\n3. captured training step (one HIP graph, fwd + bwd), batch {a.graph_batch}", {r: (lambda s=steps[r]: s(img, labels)) for r in RATES})
    say(f"\npeak memory over the whole run {torch.cuda.max_memory_allocated() / 1e9:.1f} GB (four models resident)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
