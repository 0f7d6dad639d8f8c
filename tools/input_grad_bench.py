#!/usr/bin/env python3
"""Input-volume gradient: the fused scatter dgrad (xvit_patch_embed_dgrad) against the NN GEMM + xvit_unpatchify fallback at configs[1]
(B = 8 and 126), mist and ucsf, both interleaved in one process (HIP events, median of the rounds); an eager training step at configs[1],
B = 8, with and without img.requires_grad; input_attributions(..., steps=32) at B = 1.
    python tools/input_grad_bench.py [rounds]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-attention-vit_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_cpu as R  # noqa: E402
import xvit  # noqa: E402
from xvit import functional as XF  # noqa: E402
from xvit import ops  # noqa: E402

dev = torch.device("cuda:0")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def interleaved(fns, rounds=ROUNDS):
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(event_ms(fn))
    return {k: statistics.median(v) for k, v in t.items()}


def dgrad_case(name, B, M, vol, patch, d):
    P, pd = (vol[0] // patch[0]) * (vol[1] // patch[1]) * (vol[2] // patch[2]), patch[0] * patch[1] * patch[2]
    shape = (B, M, 1, *vol)
    dx = torch.randn(M * B * (1 + P), d, device=dev).bfloat16()
    w = (torch.randn(d, pd, device=dev) / d ** 0.5).bfloat16()
    out = torch.empty(shape, device=dev)

    def fallback():
        os.environ["XVIT_PATCH_EMBED"] = "unfused"
        try:
            XF._input_grad(dx, w, shape, patch, False, torch.float32)
        finally:
            del os.environ["XVIT_PATCH_EMBED"]

    t = interleaved({"fused": lambda: ops.patch_embed_dgrad(dx, w, shape, patch, torch.float32, out=out), "fallback": fallback})
    flop = 2.0 * M * B * P * d * pd
    byts = dx.numel() * 2 + w.numel() * 2 + out.numel() * 4
    print(f"{name:14s} rows {dx.shape[0]:7d}  fused {t['fused'] * 1e3:8.1f} us ({flop / t['fused'] / 1e9:5.0f} TFLOP/s, {byts / t['fused'] / 1e6:5.0f} GB/s)"
          f"   fallback {t['fallback'] * 1e3:8.1f} us   x{t['fallback'] / t['fused']:.2f}", flush=True)
    del dx, out
    torch.cuda.empty_cache()


def step_case():
    cfg = R.make_config("base")
    model = xvit.ModelCross(cfg).to(dev)
    model.load_state_dict(R.make_state_dict(cfg, seed=0))
    model.train()
    img, labels = R.make_inputs(cfg, 8, seed=0)
    img, labels = img.to(dev).bfloat16(), labels.to(dev)

    def step(want):
        x = img.detach().requires_grad_(want)
        model(x, labels)[1].backward()
        model.zero_grad(set_to_none=True)

    t = interleaved({"plain": lambda: step(False), "img grad": lambda: step(True)})
    print(f"eager step configs[1] B = 8: {t['plain']:.2f} ms, with img.requires_grad {t['img grad']:.2f} ms (+{t['img grad'] - t['plain']:.2f} ms)", flush=True)
    model.eval()
    x1 = img[:1]
    t = interleaved({"ig32": lambda: xvit.interpret.input_attributions(model, x1, steps=32)}, rounds=3)
    print(f"input_attributions(integrated_gradients, steps=32, batch_size=16) at B = 1: {t['ig32']:.1f} ms", flush=True)


if __name__ == "__main__":
    if os.environ.get("XVIT_PATCH_EMBED"):
        sys.exit("unset XVIT_PATCH_EMBED: this tool compares both paths itself")
    dgrad_case("configs1 B=8", 8, 2, (128, 128, 128), (16, 16, 16), 768)
    dgrad_case("configs1 B=126", 126, 2, (128, 128, 128), (16, 16, 16), 768)
    dgrad_case("mist B=8", 8, 3, (128, 128, 64), (16, 16, 8), 1024)
    dgrad_case("ucsf B=4", 4, 4, (240, 240, 240), (16, 16, 16), 768)
    step_case()
