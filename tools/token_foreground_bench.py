"""Time foreground-ranked token selection at configs[1] (128^3 volumes, 16^3 patches, M = 2, bf16), B = 126 and B = 8.

    python tools/token_foreground_bench.py [--reps 20] [--inner 10] [--model-reps 10] [--batches 126 8] [--out FILE]

Volumes are synthetic skull-stripped "brains" as in tools/augment_bench.py --mode crop: an ellipsoid of positive values that fills about
half of its box, over an exactly-zero background; the threshold is 0.  Per batch size, four groups, the arms of a group interleaved inside
every repeat of one process (device-event times, median over the repeats):

  1. xvit_patch_occupancy beside xvit_volume_bbox (boxes only; the same compare per voxel, a harder reduction, two launches) on the same
     tensor, twice each, and beside the torch composition ((img > a) reshaped to the patch grid and summed).  The yardstick is the
     bytes/s xvit_volume_bbox reaches in this run; the line under the group says whether the occupancy kernel reaches it, and by how much not.
  2. xvit_token_select_ranked in both modes beside xvit_token_select_draw.
  3. The eager training step (zero-grad, operand re-cast, forward, backward) at patch_dropout 0.5 with patch_select "random" and "foreground".
  4. The eval() forward under no_grad at eval_patch_dropout 0 / 0.25 / 0.5 / 0.75.

Bytes are what the algorithm needs, computed from shapes: every voxel once plus the counts for the occupancy arms, the volumes once for
the bounding box, the int32 tables read and written for the draws.  Nothing is asserted of a time: the file is a record."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cross-attention-vit_amd"))

M, VOL, PATCH = 2, (128, 128, 128), (16, 16, 16)
P, PD = 512, 4096


def config(**over):
    base = dict(hidden_dim=768, mlp_dim=3072, num_heads=12, num_multi_blocks=2, num_self_blocks=2, img_size=VOL, patch_size=PATCH, num_modalities=M,
                attn_order={"0": "1", "1": "0"}, num_classes=2, dropout=0.0, lr=1e-4, weight_decay=0.0, optim_params={"T_max": 1, "eta_min": 0.0}, label_smoothing=0.0)
    base.update(over)
    return SimpleNamespace(**base)


def interleaved(arms, reps, inner):
    """Device-event microseconds per call of every arm, the arms interleaved inside every repeat -> {name: [reps values]}."""
    for _, fn in arms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for _ in range(reps):
        for name, fn in arms:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(inner):
                fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / inner)
    return times


def brain_volumes(B, dev):
    """bf16 [B, M, 1, 128, 128, 128]: per sample an ellipsoid with semi-axes (62, 58, 60) around a centre that moves a little with the
    sample, positive noise inside, exactly zero outside: pi / 6 = 52 % of a box that nearly fills the grid."""
    g = torch.Generator().manual_seed(0)
    img = torch.empty(B, M, 1, *VOL, dtype=torch.bfloat16, device=dev)
    z, y, x = (torch.arange(n, device=dev, dtype=torch.float32) for n in VOL)
    for b in range(B):
        c = (63.5 + b % 3 - 1, 63.5 - b % 2, 63.5 + b % 5 - 2)
        inside = ((z[:, None, None] - c[0]) / 62.0) ** 2 + ((y[None, :, None] - c[1]) / 58.0) ** 2 + ((x[None, None, :] - c[2]) / 60.0) ** 2 <= 1.0
        noise = (torch.randn(M, *VOL, generator=g).abs() + 0.1).to(dev)
        img[b, :, 0] = (noise * inside).to(torch.bfloat16)
    return img


def report(lines, arms, times, nbytes, rate_of=()):
    med = {}
    for name, _ in arms:
        t = times[name]
        med[name] = statistics.median(t)
        nb = nbytes.get(name)
        size = f"  {nb / 1e6:10.2f} MB" if nb else ""
        rate = f"  {nb / med[name] / 1e3:8.1f} GB/s" if nb and name in rate_of else ""
        lines.append(f"  {name:46s} median {med[name]:10.2f} us  (min {min(t):10.2f}, max {max(t):10.2f}){size}{rate}")
    return med


def one_batch(B, a, dev, lines):
    import xvit
    from xvit import _lib, ops
    from xvit.augment import _crop_tables, crop_config

    img = brain_volumes(B, dev)
    S = M * B
    vol_bytes = img.numel() * 2
    lines.append(f"B = {B}: {S} volumes, {vol_bytes / 1e6:.1f} MB of bf16 voxels, {S * P * 4 / 1e6:.3f} MB of counts")

    # ---- 1. occupancy, bounding box, torch -----------------------------------------------------------------------------------------------
    occ = torch.empty(S, P, dtype=torch.int32, device=dev)
    box_cfg = crop_config(None, 0, False, 0.0)
    boxes, crop_t, _ = _crop_tables(B, M, dev)
    box_ws = ops.volume_bbox_workspace(S, VOL[0] * VOL[1] * VOL[2], dev)
    src5 = img.view(B, M, *VOL)

    def torch_counts():
        fg = (img > 0.0).view(B, M, 8, 16, 8, 16, 8, 16)
        return fg.sum(dim=(3, 5, 7), dtype=torch.int32).permute(1, 0, 3, 4, 2).reshape(S, P)

    ops.patch_occupancy(img, PATCH, 0.0, out=occ)
    assert torch.equal(occ, torch_counts())
    ops.volume_bbox(src5, box_cfg, VOL, boxes, crop_t, box_ws)
    assert int(boxes[..., 6].sum()) == int(occ.sum())                          # the same voxels counted by both
    fraction = float(occ.sum()) / img.numel()
    fg_patches = float((occ >= 205).sum()) / occ.numel()
    lines.append(f"  {100 * fraction:.1f} % of the voxels foreground; {100 * fg_patches:.1f} % of the patches hold at least 5 % foreground (205 voxels)")
    f_occ = lambda: ops.patch_occupancy(img, PATCH, 0.0, out=occ)             # noqa: E731
    f_box = lambda: ops.volume_bbox(src5, box_cfg, VOL, boxes, crop_t, box_ws)   # noqa: E731
    arms = [("xvit_patch_occupancy", f_occ), ("xvit_volume_bbox (boxes only, 2 launches)", f_box), ("torch: (img > a) on the patch grid, summed", torch_counts),
            ("xvit_patch_occupancy (again)", f_occ), ("xvit_volume_bbox (again)", f_box)]
    nbytes = {n: vol_bytes + S * P * 4 for n, _ in arms if "occupancy" in n or n.startswith("torch")}
    nbytes.update({n: vol_bytes for n, _ in arms if "bbox" in n})
    times = interleaved(arms, a.reps, a.inner)
    med = report(lines, arms, times, nbytes, rate_of=[n for n, _ in arms])
    t_occ = min(med["xvit_patch_occupancy"], med["xvit_patch_occupancy (again)"])
    t_box = min(med["xvit_volume_bbox (boxes only, 2 launches)"], med["xvit_volume_bbox (again)"])
    r_occ, r_box = (vol_bytes + S * P * 4) / t_occ / 1e3, vol_bytes / t_box / 1e3
    spread = max(max(times[n]) - min(times[n]) for n in ("xvit_volume_bbox (boxes only, 2 launches)", "xvit_volume_bbox (again)"))
    verdict = "reaches it" if r_occ >= r_box else f"MISSES it by {100 * (1 - r_occ / r_box):.1f} %"
    lines.append(f"  yardstick: xvit_volume_bbox reaches {r_box:.1f} GB/s in this run (spread of its repeats {spread:.2f} us); xvit_patch_occupancy {r_occ:.1f} GB/s -> {verdict}; "
                 f"{t_occ / (vol_bytes / 6.3e12 * 1e6):.2f} x the time of reading the voxels once at the 6.3 TB/s a copy reaches; torch takes "
                 f"{med['torch: (img > a) on the patch grid, summed'] / t_occ:.1f} x as long")

    # ---- 2. the draws ---------------------------------------------------------------------------------------------------------------------
    K = 256
    keep, slot, n_fg = (torch.empty(S, n, dtype=torch.int32, device=dev) for n in (K, P, 1))
    n_fg = n_fg.view(S)
    arms = [("xvit_token_select_draw", lambda: ops.token_select_draw(keep, slot, B, False, 1)),
            ("xvit_token_select_ranked, RANDOM", lambda: ops.token_select_ranked(occ, keep, slot, B, False, _lib.TOKEN_RANK_RANDOM, 205, 1, n_fg)),
            ("xvit_token_select_ranked, TOP", lambda: ops.token_select_ranked(occ, keep, slot, B, False, _lib.TOKEN_RANK_TOP, 205, 1, n_fg)),
            ("xvit_token_select_ranked, RANDOM, shared", lambda: ops.token_select_ranked(occ, keep, slot, B, True, _lib.TOKEN_RANK_RANDOM, 410, 1, n_fg))]
    nbytes = {n: S * ((P + K) + (0 if n.endswith("draw") else (M if "shared" in n else 1) * P + 1)) * 4 for n, _ in arms}
    report(lines, arms, interleaved(arms, a.reps, a.inner), nbytes)

    # ---- 3. the eager training step, 4. the eval() forward ---------------------------------------------------------------------------------
    labels = torch.randint(0, 2, (B,), generator=torch.Generator().manual_seed(1)).to(dev)
    torch.manual_seed(0)
    models = {sel: xvit.ModelCross(config(patch_dropout=0.5, patch_select=sel, eval_patch_dropout=0.0)).to(dev).train() for sel in ("random", "foreground")}

    def step(model):
        for p in model.parameters():
            p.grad = None
        xvit.invalidate_shadows()
        model(img, labels)[1].backward()

    arms = [(f"training step, patch_dropout 0.5, {sel}", lambda m=m: step(m)) for sel, m in models.items()]
    times = interleaved(arms, a.model_reps, 1)
    med = report(lines, arms, times, {})
    d = med["training step, patch_dropout 0.5, foreground"] - med["training step, patch_dropout 0.5, random"]
    lines.append(f"  foreground - random: {d:+.2f} us per step ({100 * d / med['training step, patch_dropout 0.5, random']:+.2f} %); the two new launches alone, from "
                 f"the groups above: occupancy {t_occ:.2f} us + ranked draw - plain draw")
    del models["random"]
    model = models["foreground"].eval()
    for p in model.parameters():
        p.grad = None

    def forward(rate):
        model.eval_patch_dropout = rate
        with torch.no_grad():
            model(img, labels)

    arms = [(f"eval() forward, eval_patch_dropout {r}", lambda r=r: forward(r)) for r in (0.0, 0.25, 0.5, 0.75)]
    med = report(lines, arms, interleaved(arms, a.model_reps, 1), {})
    full = med["eval() forward, eval_patch_dropout 0.0"]
    lines.append("  against the full grid: " + ", ".join(f"{r}: {med[f'eval() forward, eval_patch_dropout {r}'] / full:.3f} x ({xvit.functional.patch_keep_count(P, r)} tokens kept)"
                                                       for r in (0.25, 0.5, 0.75)))
    del model, models, img
    torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--model-reps", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[126, 8])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("token_foreground_bench: needs a GPU; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    lines = [f"token_foreground_bench: configs[1] {VOL} / {PATCH}, M = {M}, bf16, P = {P}, ellipsoid brains over a zero background, threshold 0; {a.reps} repeats x {a.inner} calls "
             f"per kernel arm, {a.model_reps} repeats x 1 call per model arm, the arms of a group interleaved; device-event microseconds per call"]
    for B in a.batches:
        one_batch(B, a, dev, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
