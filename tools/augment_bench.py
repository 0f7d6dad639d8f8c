"""Time the augmenting input stage at the reference's input shape: B = 8, M = 2, 240 x 240 x 155 int16 -> 128^3 bf16.

    python tools/augment_bench.py [--reps 20] [--inner 10] [--out FILE] [--mode stage|elastic|crop|components]

--mode elastic times elastic deformation against the general path of the same run (see `elastic` below; profiles/elastic_measured.txt).
--mode crop times the foreground bounding-box pair against the statistics pair of the same run, and the whole stage with and without
crop_foreground (see `crop` below; profiles/crop_measured.txt).
--mode components times the connected-component pipeline at connectivity 6 and 26 against the bounding-box pair of the same run, and the
whole stage with crop_component None / "largest" (see `components` below; profiles/components_measured.txt).

Arms, interleaved inside every repeat (so that drift hits them alike): xvit_resize_pad_crop_i16 (twice: two identical arms), the exact
path as identity, the exact path with all three flips, the general path (every random transform on), the draw kernel, the statistics pair
of xvit_volume_stats alone (histogram + scan, 0.5 % / 99.5 % percentiles, no fold) and the whole stage (every random transform on) without
and with normalize="zscore" (two and four launches).  Times are
device-event times per launch (median over the repeats); GB/s counts the source bytes the destination maps to, read once, plus the
destination bytes.  The identity arm is held against xvit_resize_pad_crop_i16: it may be slower by no more than the spread, which is the
largest max - min over the repeats of the two identical arms.  Exit status 1 when it is.  The other arms are reported, not gated: the
statistics pair against the time of reading every raw volume once at the achievable HBM rate (6.3 TB/s) and against the apply launches of
the same run."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cross-attention-vit_amd"))

B, M, SRC, DST = 8, 2, (240, 240, 155), (128, 128, 128)


def interleaved(arms, reps, inner):
    """Device-event microseconds per launch of every arm, the arms interleaved inside every repeat -> {name: [reps values]}."""
    for _, fn in arms:          # warm-up: code objects, allocator
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


def elastic(a) -> int:
    """--mode elastic: xvit_augment_apply on general-path records against xvit_augment_apply_elastic on the same records (every flag 1,
    every flag 0), the elastic draw, and the whole stage with and without elastic_prob = 1.  Reported, not gated: nothing is asserted of a
    time.  7^3 control points, max_displacement 7.5, locked_borders 2 (the defaults of VolumeAugment)."""
    from xvit import ops
    from xvit.augment import ElasticField, VolumeAugment

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 3000, (B, M) + SRC, generator=g, dtype=torch.int16).to(dev)
    on = dict(flip_prob=(1, 1, 1), rotate_prob=1, zoom_prob=1, translate_prob=1, scale_intensity_prob=1, shift_intensity_prob=1, noise_prob=0, intensity_scale=1e-3)
    plain, deform = VolumeAugment(DST, **on), VolumeAugment(DST, elastic_prob=1.0, **on)
    t_full = plain.draw(B, M, SRC, dev)
    assert not bool(t_full.exact.any())
    el_on = deform.draw_elastic(B, M, dev)
    assert bool((el_on.active == 1).all())
    el_off = ElasticField(el_on.field.clone(), torch.zeros_like(el_on.record))
    zero = ElasticField.zeros(B, deform.elastic_grid, dev)
    zero.active[:] = 1.0
    want = plain.apply(src, t_full).view(torch.int16)
    assert torch.equal(plain.apply(src, t_full, elastic=el_off).view(torch.int16), want)       # flags 0: xvit_augment_apply
    assert torch.equal(plain.apply(src, t_full, elastic=zero).view(torch.int16), want)         # a zero field: the same bits
    assert not torch.equal(plain.apply(src, t_full, elastic=el_on).view(torch.int16), want)
    scratch = el_on.clone()

    arms = [
        ("xvit_augment_apply, general path", lambda: plain.apply(src, t_full)),
        ("elastic apply, every flag 1", lambda: plain.apply(src, t_full, elastic=el_on)),
        ("elastic apply, every flag 0", lambda: plain.apply(src, t_full, elastic=el_off)),
        ("elastic draw", lambda: ops.elastic_draw(deform.elastic_config, scratch.field, scratch.record, 1)),
        ("stage, elastic_prob=0", lambda: plain(src)),
        ("stage, elastic_prob=1", lambda: deform(src)),
        ("xvit_augment_apply, general path (again)", lambda: plain.apply(src, t_full)),
    ]
    times = interleaved(arms, a.reps, a.inner)
    med = {name: statistics.median(t) for name, t in times.items()}
    same = ("xvit_augment_apply, general path", "xvit_augment_apply, general path (again)")
    spread = max(max(times[n]) - min(times[n]) for n in same)
    ref = min(med[n] for n in same)
    lines = [f"augment_bench --mode elastic: B={B} M={M} {SRC} int16 -> {DST} bf16, control grid {deform.elastic_grid}, max_displacement "
             f"{tuple(deform.elastic_config.max_displacement)}, {a.reps} repeats x {a.inner} launches per arm, interleaved; device-event microseconds per launch"]
    for name, _ in arms:
        t = times[name]
        lines.append(f"  {name:42s} median {med[name]:8.2f} us  (min {min(t):8.2f}, max {max(t):8.2f})")
    lines.append(f"  yardstick: xvit_augment_apply's general path in this run, {ref:.2f} us; spread between its two identical arms' repeats {spread:.2f} us, "
                 f"their medians differ by {abs(med[same[0]] - med[same[1]]):.2f} us")
    d0 = med["elastic apply, every flag 0"] - ref
    lines.append(f"  every flag 0 against the yardstick: {d0:+.2f} us ({med['elastic apply, every flag 0'] / ref:.3f} x) -> "
                 f"{'within' if abs(d0) <= spread else 'OUTSIDE'} the spread")
    lines.append(f"  every flag 1 against the yardstick: {med['elastic apply, every flag 1'] - ref:+.2f} us ({med['elastic apply, every flag 1'] / ref:.3f} x)")
    lines.append(f"  stage with elastic_prob=1 - stage without: {med['stage, elastic_prob=1'] - med['stage, elastic_prob=0']:+.2f} us "
                 f"(elastic draw alone {med['elastic draw']:.2f} us)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


def brain_volumes(dev):
    """A synthetic skull-stripped "brain" per volume: an off-centre ellipsoid of about 172 x 140 x 136 voxels (of 240 x 240 x 155) of
    positive int16 values over an exactly-zero background, a little different per sample."""
    g = torch.Generator().manual_seed(0)
    src = torch.randint(1, 3000, (B, M) + SRC, generator=g, dtype=torch.int16).to(dev)
    z, y, x = (torch.arange(n, device=dev, dtype=torch.float32) for n in SRC)
    for b in range(B):
        c = (125.0 + b, 112.0 - 2 * b, 80.0 + b)
        inside = ((z[:, None, None] - c[0]) / 86.0) ** 2 + ((y[None, :, None] - c[1]) / 70.0) ** 2 + ((x[None, None, :] - c[2]) / 68.0) ** 2 <= 1.0
        src[b] *= inside.to(torch.int16)
    return src


def crop(a) -> int:
    """--mode crop: the xvit_volume_bbox pair (boxes only, twice: two identical arms) against the xvit_volume_stats pair on the same brains,
    and the whole stage (every random transform on) with crop_foreground None / "center" / "fit", each without and with
    normalize="zscore".  Reported, not gated: nothing is asserted of a time."""
    from xvit import ops
    from xvit.augment import NSTAT, VolumeAugment, _crop_tables, crop_config, norm_config

    dev = torch.device("cuda:0")
    src = brain_volumes(dev)
    nvox = SRC[0] * SRC[1] * SRC[2]
    on = dict(flip_prob=(1, 1, 1), rotate_prob=1, zoom_prob=1, translate_prob=1, scale_intensity_prob=1, shift_intensity_prob=1, noise_prob=0)
    stages = {(c, n): VolumeAugment(DST, crop_foreground=c, normalize=n, **(on if n else dict(on, intensity_scale=1e-3)))
              for c in (None, "center", "fit") for n in (None, "zscore")}
    box_cfg = crop_config(None, 0, False, 0.0)
    boxes, crop_t, _ = _crop_tables(B, M, dev)
    box_ws = ops.volume_bbox_workspace(B * M, nvox, dev)
    stats_cfg = norm_config(None, 0.0, (0.005, 0.995))
    stats = torch.empty(B, M, NSTAT, dtype=torch.float64, device=dev)
    stats_ws = ops.volume_stats_workspace(B * M, dev)
    ops.volume_bbox(src, box_cfg, DST, boxes, crop_t, box_ws)
    lo, hi = crop_t[:, 0:6:2].cpu(), crop_t[:, 1:6:2].cpu()
    extent = (hi - lo + 1).float().mean(0).tolist()
    fraction = float(boxes[..., 6].sum()) / (B * M * nvox)

    bbox = lambda: ops.volume_bbox(src, box_cfg, DST, boxes, crop_t, box_ws)      # noqa: E731
    arms = [("bounding-box pair", bbox), ("statistics pair", lambda: ops.volume_stats(src, stats_cfg, stats, stats_ws))]
    arms += [(f"stage, crop={c}, normalize={n}", lambda st=st: st(src)) for (c, n), st in stages.items()]
    arms += [("bounding-box pair (again)", bbox)]
    times = interleaved(arms, a.reps, a.inner)
    med = {name: statistics.median(t) for name, t in times.items()}
    raw_bytes = src.numel() * 2
    lines = [f"augment_bench --mode crop: B={B} M={M} {SRC} int16 -> {DST} bf16; ellipsoid brains, mean box {extent[0]:.0f} x {extent[1]:.0f} x {extent[2]:.0f} voxels, "
             f"{100 * fraction:.1f} % of the voxels foreground; {a.reps} repeats x {a.inner} calls per arm, interleaved; device-event microseconds per call"]
    for name, _ in arms:
        t = times[name]
        rate = f"  {raw_bytes / med[name] / 1e3:8.1f} GB/s" if "pair" in name else ""
        lines.append(f"  {name:40s} median {med[name]:8.2f} us  (min {min(t):8.2f}, max {max(t):8.2f}){rate}")
    same = ("bounding-box pair", "bounding-box pair (again)")
    spread = max(max(times[n]) - min(times[n]) for n in same)
    pair, stat = min(med[n] for n in same), med["statistics pair"]
    lines.append(f"  bounding-box pair: reads {raw_bytes / 1e6:.1f} MB of raw volumes once (GB/s above counts these); at the 8.0 TB/s HBM peak that is "
                 f"{raw_bytes / 8.0e12 * 1e6:.1f} us: {pair / (raw_bytes / 8.0e12 * 1e6):.2f} x that ({pair / (raw_bytes / 6.3e12 * 1e6):.2f} x the time at the 6.3 TB/s a copy "
                 f"reaches); spread between the two identical arms' repeats {spread:.2f} us")
    lines.append(f"  bounding-box pair against the statistics pair of this run: {pair / stat:.3f} x ({pair - stat:+.2f} us) -> "
                 f"{'not slower' if pair <= stat else 'SLOWER than the statistics pair'}")
    base = med["stage, crop=None, normalize=None"]
    for c in ("center", "fit"):
        lines.append(f"  stage with crop={c} - stage without: {med[f'stage, crop={c}, normalize=None'] - base:+.2f} us; with normalize=zscore on both: "
                     f"{med[f'stage, crop={c}, normalize=zscore'] - med['stage, crop=None, normalize=zscore']:+.2f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


def components(a) -> int:
    """--mode components: xvit_volume_components and xvit_volume_bbox_components at connectivity 6 and 26 against the xvit_volume_bbox pair
    (twice: two identical arms) on the brains of --mode crop plus 300 isolated bright voxels per volume, and the whole stage (every random
    transform on) with crop_foreground "center" / "fit", each with crop_component None and "largest".  Reported, not gated: nothing is
    asserted of a time.  The kernels of one call are told apart by a kernel trace of this run, not by this tool."""
    from xvit import ops
    from xvit.augment import VolumeAugment, _component_tables, _crop_tables, component_config, crop_config

    dev = torch.device("cuda:0")
    src = brain_volumes(dev)
    nvox = SRC[0] * SRC[1] * SRC[2]
    g = torch.Generator().manual_seed(1)
    flat = src.view(B * M, nvox)
    for v in range(B * M):
        flat[v, torch.randint(0, nvox, (300,), generator=g).to(dev)] = 3000
    on = dict(flip_prob=(1, 1, 1), rotate_prob=1, zoom_prob=1, translate_prob=1, scale_intensity_prob=1, shift_intensity_prob=1, noise_prob=0, intensity_scale=1e-3)
    stages = {(c, k): VolumeAugment(DST, crop_foreground=c, crop_component=k, **on) for c in ("center", "fit") for k in (None, "largest")}
    box_cfg = crop_config(None, 0, False, 0.0)
    boxes, crop_t, _ = _crop_tables(B, M, dev)
    box_ws = ops.volume_bbox_workspace(B * M, nvox, dev)
    labels, comps, ws = _component_tables(src)
    cfgs = {c: component_config("largest", c, 0.0) for c in (6, 26)}
    ops.volume_bbox(src, box_cfg, DST, boxes, crop_t, box_ws)
    plain_extent = (crop_t[:, 1:6:2] - crop_t[:, 0:6:2] + 1).float().mean(0).tolist()
    ops.volume_bbox_components(src, box_cfg, cfgs[6], DST, boxes, crop_t, labels, comps, ws)
    kept_extent = (crop_t[:, 1:6:2] - crop_t[:, 0:6:2] + 1).float().mean(0).tolist()
    assert int(comps[..., 5].abs().sum()) == 0, "status"
    ncomp, kept_frac = comps[..., 0].float().mean().item(), float(comps[..., 4].sum()) / (B * M * nvox)

    bbox = lambda: ops.volume_bbox(src, box_cfg, DST, boxes, crop_t, box_ws)      # noqa: E731
    arms = [("bounding-box pair", bbox)]
    for c in (6, 26):
        arms += [(f"components alone, connectivity {c}", lambda c=c: ops.volume_components(src, cfgs[c], labels, comps, ws)),
                 (f"components + boxes + finish, connectivity {c}", lambda c=c: ops.volume_bbox_components(src, box_cfg, cfgs[c], DST, boxes, crop_t, labels, comps, ws))]
    arms += [(f"stage, crop={c}, component={k}", lambda st=st: st(src)) for (c, k), st in stages.items()]
    arms += [("bounding-box pair (again)", bbox)]
    times = interleaved(arms, a.reps, a.inner)
    med = {name: statistics.median(t) for name, t in times.items()}
    raw_bytes, label_bytes = src.numel() * 2, src.numel() * 4
    least = raw_bytes + 2 * label_bytes                  # the source read once, the labels written once and read once
    lines = [f"augment_bench --mode components: B={B} M={M} {SRC} int16 -> {DST} bf16; ellipsoid brains plus 300 bright voxels per volume: {ncomp:.0f} components per "
             f"volume at connectivity 6, {100 * kept_frac:.1f} % of the voxels in the largest; mean crop {plain_extent[0]:.0f} x {plain_extent[1]:.0f} x {plain_extent[2]:.0f} "
             f"voxels unfiltered, {kept_extent[0]:.0f} x {kept_extent[1]:.0f} x {kept_extent[2]:.0f} over the largest component; labels {label_bytes / 1e6:.0f} MB, workspace "
             f"{ws.numel() / 1e6:.0f} MB; {a.reps} repeats x {a.inner} calls per arm, interleaved; device-event microseconds per call"]
    for name, _ in arms:
        t = times[name]
        rate = f"  {raw_bytes / med[name] / 1e3:8.1f} GB/s of source" if "pair" in name else f"  {least / med[name] / 1e3:8.1f} GB/s of least traffic" if "components" in name else ""
        lines.append(f"  {name:48s} median {med[name]:9.2f} us  (min {min(t):9.2f}, max {max(t):9.2f}){rate}")
    same = ("bounding-box pair", "bounding-box pair (again)")
    spread = max(max(times[n]) - min(times[n]) for n in same)
    pair = min(med[n] for n in same)
    lines.append(f"  least traffic of the component pipeline: {least / 1e6:.0f} MB (source once, labels written once and read once); at the 6.3 TB/s a copy reaches that is "
                 f"{least / 6.3e12 * 1e6:.0f} us; spread between the two identical bounding-box arms' repeats {spread:.2f} us")
    for c in (6, 26):
        full = med[f"components + boxes + finish, connectivity {c}"]
        lines.append(f"  connectivity {c}: components + boxes + finish is {full / pair:.1f} x the bounding-box pair of this run ({full - pair:+.2f} us), "
                     f"{full / (least / 6.3e12 * 1e6):.1f} x its least traffic at 6.3 TB/s")
    for c in ("center", "fit"):
        lines.append(f"  stage with crop={c}, component=largest - stage with component=None: "
                     f"{med[f'stage, crop={c}, component=largest'] - med[f'stage, crop={c}, component=None']:+.2f} us "
                     f"({med[f'stage, crop={c}, component=largest'] / med[f'stage, crop={c}, component=None']:.2f} x)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode", choices=("stage", "elastic", "crop", "components"), default="stage")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: needs a GPU; a CPU run measures nothing")
    if a.mode == "elastic":
        return elastic(a)
    if a.mode == "crop":
        return crop(a)
    if a.mode == "components":
        return components(a)
    from xvit import ops
    from xvit.augment import NSTAT, AugmentParams, VolumeAugment, norm_config

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 3000, (B, M) + SRC, generator=g, dtype=torch.int16).to(dev)
    off = dict(flip_prob=(0, 0, 0), rotate_prob=0, zoom_prob=0, translate_prob=0, scale_intensity_prob=0, shift_intensity_prob=0, noise_prob=0)
    ident = VolumeAugment(DST, **off)
    t_ident = ident.draw(B, M, SRC, dev)
    t_flip = VolumeAugment(DST, **dict(off, flip_prob=(1, 1, 1))).draw(B, M, SRC, dev)
    full = VolumeAugment(DST, flip_prob=(1, 1, 1), rotate_prob=1, zoom_prob=1, translate_prob=1, scale_intensity_prob=1, shift_intensity_prob=1, noise_prob=0,
                         intensity_scale=1e-3)
    t_full = full.draw(B, M, SRC, dev)
    assert bool(t_ident.exact.all()) and bool(t_flip.exact.all()) and not bool(t_full.exact.any())
    assert torch.equal(ident.apply(src, t_ident).view(torch.int16), ops.resize_pad_crop_i16(src, DST, -1.0).view(torch.int16))
    table = AugmentParams(torch.empty(B, M, 32, dtype=torch.float32, device=dev))
    on = dict(flip_prob=(1, 1, 1), rotate_prob=1, zoom_prob=1, translate_prob=1, scale_intensity_prob=1, shift_intensity_prob=1, noise_prob=0)
    stage_plain = VolumeAugment(DST, intensity_scale=1e-3, **on)
    stage_norm = VolumeAugment(DST, normalize="zscore", **on)
    stats_cfg = norm_config(None, 0.0, (0.005, 0.995))
    stats = torch.empty(B, M, NSTAT, dtype=torch.float64, device=dev)
    workspace = ops.volume_stats_workspace(B * M, dev)

    arms = [
        ("xvit_resize_pad_crop_i16", lambda: ops.resize_pad_crop_i16(src, DST, -1.0)),
        ("exact path, identity", lambda: ident.apply(src, t_ident)),
        ("exact path, three flips", lambda: ident.apply(src, t_flip)),
        ("general path", lambda: ident.apply(src, t_full)),
        ("draw kernel", lambda: ops.augment_draw(full.config, table.table, SRC, DST, 1)),
        ("statistics pair", lambda: ops.volume_stats(src, stats_cfg, stats, workspace)),
        ("stage, normalize=None", lambda: stage_plain(src)),
        ("stage, normalize=zscore", lambda: stage_norm(src)),
        ("xvit_resize_pad_crop_i16 (again)", lambda: ops.resize_pad_crop_i16(src, DST, -1.0)),
    ]
    times = interleaved(arms, a.reps, a.inner)      # us per launch
    nvol = B * M
    src_elems = nvol * min(SRC[0], DST[0]) * min(SRC[1], DST[1]) * min(SRC[2], DST[2])
    nbytes = src_elems * 2 + nvol * DST[0] * DST[1] * DST[2] * 2
    raw_bytes = src.numel() * 2
    lines = [f"augment_bench: B={B} M={M} {SRC} int16 -> {DST} bf16, {a.reps} repeats x {a.inner} launches per arm, interleaved; "
             f"{nbytes / 1e6:.1f} MB per launch (source region read once + destination)"]
    med = {}
    for name, _ in arms:
        t = times[name]
        med[name] = statistics.median(t)
        rate = "" if name == "draw kernel" or name.startswith("stage") else f"  {(raw_bytes if name == 'statistics pair' else nbytes) / med[name] / 1e3:8.1f} GB/s"
        lines.append(f"  {name:34s} median {med[name]:8.2f} us  (min {min(t):8.2f}, max {max(t):8.2f}){rate}")
    same = ("xvit_resize_pad_crop_i16", "xvit_resize_pad_crop_i16 (again)")
    spread = max(max(times[n]) - min(times[n]) for n in same)
    ref = min(med[n] for n in same)
    delta = med["exact path, identity"] - ref
    ok = delta <= spread
    lines.append(f"  identity vs xvit_resize_pad_crop_i16: {delta:+.2f} us ({med['exact path, identity'] / ref:.3f} x); spread between the identical arms' repeats "
                 f"{spread:.2f} us; the two identical arms' medians differ by {abs(med[same[0]] - med[same[1]]):.2f} us -> {'OK' if ok else 'SLOWER THAN THE SPREAD ALLOWS'}")
    pair, floor = med["statistics pair"], raw_bytes / 6.3e12 * 1e6
    lines.append(f"  statistics pair: reads {raw_bytes / 1e6:.1f} MB of raw volumes (GB/s above counts these); once at 6.3 TB/s is {floor:.1f} us: {pair / floor:.2f} x that; "
                 f"{pair / med['general path']:.2f} x the general-path apply, {pair / med['exact path, identity']:.2f} x the identity apply")
    lines.append(f"  stage with normalize=zscore - stage without: {med['stage, normalize=zscore'] - med['stage, normalize=None']:+.2f} us "
                 f"(statistics pair alone {pair:.2f} us)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
