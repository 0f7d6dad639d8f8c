#!/usr/bin/env python3
"""What the optimizer step costs at configs[1] (ModelCross d = 768, 2 x 128^3, 16^3 patches; ~93 M parameters), host and GPU, and what
fused clipping and the in-graph optimizer change.  One process per mode, variants interleaved in rounds (A, B, A, B, ...) so that
clock and host drift hit both; one JSON line per variant.  Run each mode under its own time limit:

    python tools/optim_bench.py step  [iters] [rounds]   # FusedAdam.step(): host wall time of the call and GPU time
    python tools/optim_bench.py clip  [iters] [rounds]   # clip_grad_norm_ + FusedAdam.step()  vs  FusedAdam(max_grad_norm=...)
    python tools/optim_bench.py graph [iters] [rounds]   # batch 8: GraphedStep + eager opt.step()  vs  GraphedStep(optimizer=opt)
    python tools/optim_bench.py adamw [iters] [rounds]   # FusedAdamW without an average  vs  FusedAdam at equal settings (eager and capturable)
    python tools/optim_bench.py ema   [iters] [rounds]   # FusedAdamW(ema_decay=...)  vs  FusedAdam.step() + torch._foreach_lerp_ over the same tensors
    python tools/optim_bench.py layers [iters] [rounds]  # batch 8, GraphedStep on layer_decay_groups: FusedAdamW (one launch set)  vs  FusedAdam (one per group)

host_ms: time.perf_counter around the call(s), no synchronisation inside (what the Python thread pays per step);
gpu_ms: device events around the same calls;  wall_ms: a block of iterations ending in a synchronise, per iteration."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cross-attention-vit_amd"))
sys.path.insert(0, ROOT)
import xvit  # noqa: E402
from bench import base_config  # noqa: E402
from xvit.graph import GraphedStep  # noqa: E402
from xvit.optim import FusedAdam, FusedAdamW, layer_decay_groups  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "step"
nums = [int(a) for a in sys.argv[2:] if a.isdigit()]
iters = nums[0] if nums else 20
rounds = nums[1] if len(nums) > 1 else 5
B = 8
dev = torch.device("cuda:0")
assert torch.cuda.is_available(), "optim_bench needs a GPU"
cfg = base_config()


def make_model(seed=0):
    torch.manual_seed(seed)
    m = xvit.ModelCross(cfg).to(dev)
    m.train()
    return m


torch.manual_seed(1)
img = torch.randn(B, cfg.num_modalities, 1, *cfg.img_size).to(dev, torch.bfloat16)
labels = torch.randint(0, 2, (B,)).to(dev)


def backward(model):
    _, loss = model(img, labels)
    loss.backward()


def measure(variants, extra=None):
    """variants: {name: callable}; extra: {name: dict} merged into the variant's JSON line.  Rounds of `iters` calls each, interleaved; per call host time and event time, per block wall time."""
    res = {k: {"host": [], "gpu": [], "wall": []} for k in variants}
    for fn in variants.values():                          # warm-up: every variant, every shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in variants.items():
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
            torch.cuda.synchronize()
            t_block = time.perf_counter()
            for a, b in evs:
                a.record()
                t0 = time.perf_counter()
                fn()
                res[name]["host"].append((time.perf_counter() - t0) * 1e3)
                b.record()
            torch.cuda.synchronize()
            res[name]["wall"].append((time.perf_counter() - t_block) / iters * 1e3)
            res[name]["gpu"].extend(a.elapsed_time(b) for a, b in evs)
    n_params = sum(p.numel() for p in model.parameters())
    for name, r in res.items():
        print(json.dumps({"tool": "optim_bench", "mode": mode, "variant": name, "params_M": round(n_params / 1e6, 1), "batch": B,
                          "iters": iters, "rounds": rounds,
                          "host_ms_median": round(statistics.median(r["host"]), 4), "gpu_ms_median": round(statistics.median(r["gpu"]), 4),
                          "wall_ms_per_iter_median": round(statistics.median(r["wall"]), 4),
                          "wall_ms_per_iter_min_max": [round(min(r["wall"]), 4), round(max(r["wall"]), 4)],
                          "gpu_ms_round_medians": [round(statistics.median(r["gpu"][i * iters:(i + 1) * iters]), 4) for i in range(rounds)],
                          **((extra or {}).get(name, {}))}), flush=True)


model = make_model()
if mode == "step":
    backward(model)
    opt = FusedAdam(model.parameters(), lr=1e-5)
    cap = FusedAdam(model.parameters(), lr=1e-5, capturable=True)       # same parameters and gradients: only the timing matters here
    measure({"FusedAdam.step() [host tables per step]": opt.step, "FusedAdam(capturable=True).step() [eager]": cap.step})
elif mode == "clip":
    backward(model)
    params = list(model.parameters())
    plain = FusedAdam(params, lr=1e-5)
    fused = FusedAdam(params, lr=1e-5, max_grad_norm=1.0)
    fused_cap = FusedAdam(params, lr=1e-5, max_grad_norm=1.0, capturable=True)

    def torch_clip_then_step():
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        plain.step()

    measure({"clip_grad_norm_ + FusedAdam.step()": torch_clip_then_step, "FusedAdam(max_grad_norm=1).step()": fused.step,
             "FusedAdam(max_grad_norm=1, capturable=True).step()": fused_cap.step})
elif mode == "graph":
    model_b, model_c = make_model(), make_model()
    opt_a = FusedAdam(model.parameters(), lr=1e-5)
    step_a = GraphedStep(model, img, labels)
    opt_b = FusedAdam(model_b.parameters(), lr=1e-5, capturable=True)
    step_b = GraphedStep(model_b, img, labels, optimizer=opt_b)
    opt_c = FusedAdam(model_c.parameters(), lr=1e-5, max_grad_norm=1.0, capturable=True)
    step_c = GraphedStep(model_c, img, labels, optimizer=opt_c)

    def graph_then_eager_step():
        step_a(img, labels)
        opt_a.step()

    measure({"GraphedStep + eager FusedAdam.step()": graph_then_eager_step, "GraphedStep(optimizer=FusedAdam(capturable))": lambda: step_b(img, labels),
             "GraphedStep(optimizer=FusedAdam(capturable, max_grad_norm=1))": lambda: step_c(img, labels)})
elif mode == "adamw":
    backward(model)
    params = list(model.parameters())
    n = sum(p.numel() for p in params)
    kw = dict(lr=1e-5, weight_decay=0.05)
    adam, adamw = FusedAdam(params, **kw), FusedAdamW(params, **kw)
    adam_c, adamw_c = FusedAdam(params, capturable=True, **kw), FusedAdamW(params, capturable=True, **kw)
    measure({"FusedAdam.step()": adam.step, "FusedAdamW.step()": adamw.step, "FusedAdam(capturable=True).step()": adam_c.step,
             "FusedAdamW(capturable=True).step()": adamw_c.step}, {k: {"bytes_per_step_GB": round(26 * n / 1e9, 3)} for k in ("FusedAdam(capturable=True).step()", "FusedAdamW(capturable=True).step()")})
elif mode == "ema":
    backward(model)
    params = list(model.parameters())
    n = sum(p.numel() for p in params)
    kw = dict(lr=1e-5, weight_decay=0.05)
    adam, adam_c = FusedAdam(params, **kw), FusedAdam(params, capturable=True, **kw)
    fused, fused_c = FusedAdamW(params, ema_decay=0.9999, **kw), FusedAdamW(params, ema_decay=0.9999, capturable=True, **kw)
    shadow = [p.detach().clone() for p in params]
    datas = [p.detach() for p in params]

    def adam_then_lerp(opt):
        def fn():
            opt.step()
            torch._foreach_lerp_(shadow, datas, 1.0 - 0.9999)
        return fn

    measure({"FusedAdam.step() + _foreach_lerp_": adam_then_lerp(adam), "FusedAdamW(ema_decay).step()": fused.step,
             "FusedAdam(capturable=True).step() + _foreach_lerp_": adam_then_lerp(adam_c), "FusedAdamW(ema_decay, capturable=True).step()": fused_c.step},
            {"FusedAdam.step() + _foreach_lerp_": {"bytes_per_step_GB": round(38 * n / 1e9, 3)}, "FusedAdamW(ema_decay).step()": {"bytes_per_step_GB": round(34 * n / 1e9, 3)},
             "FusedAdam(capturable=True).step() + _foreach_lerp_": {"bytes_per_step_GB": round(38 * n / 1e9, 3)},
             "FusedAdamW(ema_decay, capturable=True).step()": {"bytes_per_step_GB": round(34 * n / 1e9, 3)}})
elif mode == "layers":
    model_b = make_model()
    opt_a = FusedAdamW(layer_decay_groups(model, 0.75, 0.05), lr=1e-5, capturable=True)
    step_a = GraphedStep(model, img, labels, optimizer=opt_a)
    opt_b = FusedAdam(layer_decay_groups(model_b, 0.75, 0.05), lr=1e-5, capturable=True)      # ignores lr_scale: only the launch structure is compared
    step_b = GraphedStep(model_b, img, labels, optimizer=opt_b)
    measure({"GraphedStep(optimizer=FusedAdamW(layer_decay_groups))": lambda: step_a(img, labels),
             "GraphedStep(optimizer=FusedAdam(layer_decay_groups))": lambda: step_b(img, labels)},
            {"GraphedStep(optimizer=FusedAdamW(layer_decay_groups))": {"groups": len(opt_a.param_groups), "optimizer_launches": 2 * len(opt_a._entries)},
             "GraphedStep(optimizer=FusedAdam(layer_decay_groups))": {"groups": len(opt_b.param_groups), "optimizer_launches": 2 * len(opt_b._entries)}})
else:
    raise SystemExit(f"unknown mode {mode!r}: step | clip | graph | adamw | ema | layers")
