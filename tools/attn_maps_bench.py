#!/usr/bin/env python3
"""Cost of the attention maps.  (1) xvit_attn_rollout_step against xvit_attn_fwd, and xvit_attn_relevance_step against the rollout step, at
the same (B, H, N), alternated in one process (HIP events, random data, median of 5 rounds); (2) xvit.interpret.attention_maps(model, img,
rollout=True) against a plain eval forward (torch.no_grad) of ModelCross at configs[1] (R.make_config("base")), B = 8, and
xvit.interpret.relevance_maps(model, img) against attention_maps(rollout=True), alternated the same way."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-attention-vit_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_cpu as R  # noqa: E402
import xvit  # noqa: E402
from xvit import ops  # noqa: E402


def timed(fn, n=20):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3      # us


def med(v):
    return sorted(v)[len(v) // 2]


def kernels():
    dev = torch.device("cuda:0")
    H, d, scale = 12, 768, 0.125
    for B, N in ((8, 513), (126, 513), (8, 4097)):
        qkv = torch.randn(B * N, 3 * d, device=dev).bfloat16()
        _, lse = ops.attn_fwd(qkv, B, N, H, scale)
        do = torch.randn(B * N, d, device=dev).bfloat16()
        r = torch.rand(B, N, device=dev)
        r /= r.sum(dim=1, keepdim=True)
        f, s, g = [], [], []
        for _ in range(5):
            f.append(timed(lambda: ops.attn_fwd(qkv, B, N, H, scale)))
            s.append(timed(lambda: ops.attn_rollout_step(qkv, lse, r, B, N, H, scale)))
            g.append(timed(lambda: ops.attn_relevance_step(qkv, lse, do, r, B, N, H, scale)))
        print(f"B={B:3d} H={H} N={N:5d}: attn_fwd {med(f):8.1f} us   rollout_step {med(s):8.1f} us   ratio {med(s) / med(f):.2f}   "
              f"(spread fwd {min(f):.1f}-{max(f):.1f}, step {min(s):.1f}-{max(s):.1f})", flush=True)
        print(f"B={B:3d} H={H} N={N:5d}: relevance_step {med(g):8.1f} us   vs rollout_step: ratio {med(g) / med(s):.2f}   "
              f"(spread {min(g):.1f}-{max(g):.1f})", flush=True)


def model_maps():
    dev = torch.device("cuda:0")
    cfg = R.make_config("base")
    model = xvit.ModelCross(cfg).to(dev)
    model.load_state_dict(R.make_state_dict(cfg, seed=0))
    model.eval()
    img, labels = R.make_inputs(cfg, 8, seed=0)
    img, labels = img.to(dev), labels.to(dev)

    def plain():
        with torch.no_grad():
            model(img, labels)

    p, m, g = [], [], []
    for _ in range(5):
        p.append(timed(plain, n=5))
        m.append(timed(lambda: xvit.interpret.attention_maps(model, img, rollout=True), n=5))
        g.append(timed(lambda: xvit.interpret.relevance_maps(model, img), n=5))
    print(f"configs[1] B=8: eval forward {med(p) / 1e3:7.2f} ms   attention_maps(rollout=True) {med(m) / 1e3:7.2f} ms   ratio {med(m) / med(p):.2f}   "
          f"(spread {min(p) / 1e3:.2f}-{max(p) / 1e3:.2f} / {min(m) / 1e3:.2f}-{max(m) / 1e3:.2f} ms)", flush=True)
    print(f"configs[1] B=8: relevance_maps {med(g) / 1e3:7.2f} ms   vs attention_maps(rollout=True): ratio {med(g) / med(m):.2f}   "
          f"(spread {min(g) / 1e3:.2f}-{max(g) / 1e3:.2f} ms)", flush=True)


if __name__ == "__main__":
    kernels()
    model_maps()
