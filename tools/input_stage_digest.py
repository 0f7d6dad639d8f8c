#!/usr/bin/env python3
"""One sha256 per case of the raw bytes the device input stage writes: the three draws, xvit_augment_apply, xvit_augment_apply_elastic,
xvit_contrast_apply and xvit_volume_bbox (boxes, crop and the folded table; these cases come last, so that a build without them prints
the same lines up to there), on small fixed inputs.  Two builds of the library compute the same thing exactly when their printouts are equal:

    XVIT_LIB=/path/to/other/libxvit_hip.so python tools/input_stage_digest.py > other.txt
    python tools/input_stage_digest.py > this.txt && cmp other.txt this.txt

Every input comes from one fixed-seed generator; the records of the apply cases are written here, not drawn, so that a difference in a
draw does not hide one in an apply.  The library in use is named on stderr only."""
import hashlib
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cross-attention-vit_amd"))
from xvit import _lib, augment as A, ops  # noqa: E402

DEV = torch.device("cuda:0")
GEN = torch.Generator().manual_seed(20240317)
PAIRS = [(s, d) for s in (torch.int16, torch.bfloat16, torch.float32) for d in (torch.bfloat16, torch.float32)]


def say(name, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
    print(f"{name:<72s} {h.hexdigest()}")


def short(dt):
    return str(dt).split(".")[1]


def volumes(shape, dtype, lo, hi):
    v = torch.rand(shape, generator=GEN) * (hi - lo) + lo
    return (v.round().to(torch.int16) if dtype == torch.int16 else v.to(dtype)).to(DEV)


def draws():
    B, M = 3, 2
    aug = A.VolumeAugment((5, 6, 20), intensity_scale=1e-3)
    con = A.ContrastAugment(blur_prob=.6, bias_prob=.6, gamma_prob=.6)
    for seed in (0, 0x9E3779B97F4A7C15):
        for start in (None, 0, 5):
            tag = f"seed {seed:#x} counter {start}"

            def drawn(name, draw, *out):
                """draw(counter, advance) on a counter of its own at `start`, advanced and hashed behind what was drawn; or without one."""
                counter = None if start is None else torch.full((1,), start, dtype=torch.int64, device=DEV)
                draw(counter, counter is not None)
                say(f"{name} {tag}", *out, *(() if counter is None else (counter,)))

            table = torch.empty(B, M, A.NPARAM, device=DEV)
            drawn("augment_draw", lambda *at: ops.augment_draw(aug.config, table, (7, 8, 22), aug.img_size, seed, *at), table)
            ctable = torch.empty(B, M, A.CON_NPARAM, device=DEV)
            drawn("contrast_draw", lambda *at: ops.contrast_draw(con.config, ctable, seed, *at), ctable)
            for grid in ((4, 5, 7), (7, 7, 7)):
                for locked in (0, 2):
                    cfg = A.VolumeAugment((5, 6, 20), elastic_prob=.7, elastic_control_points=grid, elastic_max_displacement=1.5, elastic_locked_borders=locked,
                                          elastic_allow_folding=True).elastic_config
                    el = A.ElasticField.zeros(B, grid, DEV)
                    drawn(f"elastic_draw grid {grid} locked {locked}", lambda *at: ops.elastic_draw(cfg, el.field, el.record, seed, *at), el.field, el.record)


def augment_records(src_shape, dst_shape):
    """[2, 2, 32]: an exact record with an x flip; rotation about z plus zoom; the same clamped; the same with noise."""
    ctr = [0.5 * (n - 1) for n in dst_shape]
    off = [A.pad_crop_offset(s, d) for s, d in zip(src_shape, dst_shape)]

    def record(L):
        r = torch.zeros(A.NPARAM, dtype=torch.float64)
        for i in range(3):
            r[A.MATRIX + 4 * i:A.MATRIX + 4 * i + 3] = torch.tensor(L[i], dtype=torch.float64)
            r[A.MATRIX + 4 * i + 3] = ctr[i] + off[i] - sum(L[i][j] * ctr[j] for j in range(3))
        r[A.SCALE], r[A.SHIFT] = 1e-3, 0.25
        return r.to(torch.float32)

    c, s = math.cos(0.3), math.sin(0.3)
    flip, general = record([[1, 0, 0], [0, 1, 0], [0, 0, -1]]), record([[1 / 1.1, 0, 0], [0, c / 0.95, -s / 1.05], [0, s / 0.95, c / 1.05]])
    flip[A.FLAGS] = A.FLAG_EXACT
    clamped, noisy = general.clone(), general.clone()
    clamped[A.FLAGS], clamped[A.CLAMP_LO], clamped[A.CLAMP_HI] = A.FLAG_CLAMP, 200.0, 1800.0
    noisy[A.SIGMA] = 0.05
    noisy.view(torch.int32)[A.NOISE_SEED] = 0x5EED1234
    return torch.stack([flip, general, clamped, noisy]).reshape(2, 2, A.NPARAM).to(DEV)


def augment_applies():
    grid = (4, 5, 7)
    for dst_shape in ((5, 6, 20), (4, 5, 40), (4, 4, 72)):           # the three brick widths, each with a ragged last run
        for grow in (2, -2):
            src_shape = tuple(n + grow for n in dst_shape)
            table = augment_records(src_shape, dst_shape)
            field = ((torch.rand((2, 3) + grid, generator=GEN) * 3.0) - 1.5).to(DEV)
            for sdt, ddt in PAIRS:
                src = volumes((2, 2) + src_shape, sdt, -200.0, 3000.0)
                tag = f"{short(sdt)} -> {short(ddt)} {src_shape} -> {dst_shape}"
                say(f"augment_apply {tag}", ops.augment_apply(src, table, dst_shape, -1.0, ddt))
                outs = []
                for flags in ((1.0, 0.0), (0.0, 1.0)):                  # mixed over the samples, each sample deformed once
                    erec = torch.zeros(2, A.ELASTIC_NREC, device=DEV)
                    erec[:, A.ELASTIC_FLAG] = torch.tensor(flags, device=DEV)
                    outs.append(ops.augment_apply_elastic(src, table, field, erec, dst_shape, -1.0, ddt))
                say(f"augment_apply_elastic {tag}", *outs)


def contrast_records():
    """[5, 1, 32]: copy, bias only, gamma only, blur only (three different radii), all three."""
    t = A.ContrastParams.identity(5, 1)
    sigma = torch.tensor([0.4, 0.9, 1.7])
    bias = torch.tensor([0.2, -0.15, 0.1, -0.05, 0.12, -0.2, 0.07, -0.11, 0.16])
    for row, (blur, biased, gamma) in enumerate(((0, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 0), (1, 1, 1))):
        t.flags[row] = blur * A.CON_FLAG_BLUR + biased * A.CON_FLAG_BIAS + gamma * A.CON_FLAG_GAMMA
        if blur:
            t.sigma[row] = sigma
            t.radius[row] = torch.clamp(torch.ceil(3 * sigma), max=A.CON_MAX_RADIUS)
        if biased:
            t.bias[row] = bias
        if gamma:
            t.gamma[row] = 1.3
    return t.table.to(DEV)


def contrast_applies():
    table = contrast_records()
    for shape in ((5, 18, 70), (6, 16, 64)):                           # a ragged and a whole 64 x 16 tile
        for sdt in (torch.bfloat16, torch.float32):
            src = volumes((5, 1, 1) + shape, sdt, -0.1, 1.1)
            for ddt in (torch.bfloat16, torch.float32):
                say(f"contrast_apply {short(sdt)} -> {short(ddt)} {shape}", ops.contrast_apply(src, table, ddt))


def crops():
    """xvit_volume_bbox on sparse volumes (about one voxel in six above 0, so the boxes do not fill the volume): boxes only, and both folds
    into the records of augment_records, with and without a margin."""
    for src_shape, dst_shape in (((9, 10, 37), (5, 6, 20)), ((9, 31, 31), (4, 5, 40))):      # the second: two chunks per volume
        for sdt in (torch.int16, torch.bfloat16, torch.float32):
            src = volumes((2, 2) + src_shape, sdt, -2500.0, 500.0)
            src[:, :, :2], src[:, :, :, -3:], src[1, 1] = 0, 0, 0                            # empty faces; sample 1 has an empty modality
            workspace = ops.volume_bbox_workspace(4, src[0, 0].numel(), DEV)
            for mode, margin, up in ((None, 0, False), ("center", 0, False), ("center", (1, 0, 2), False), ("fit", 0, False), ("fit", (0, 2, 1), True)):
                table = augment_records(src_shape, dst_shape)
                boxes, crop = torch.empty(2, 2, A.BBOX_NREC, dtype=torch.int32, device=DEV), torch.empty(2, A.BBOX_NREC, dtype=torch.int32, device=DEV)
                ops.volume_bbox(src, A.crop_config(mode, margin, up, 0.0), dst_shape, boxes, crop, workspace, table)
                say(f"volume_bbox {short(sdt)} {src_shape} -> {dst_shape} {mode} margin {margin} upscale {up}", boxes, crop, table)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("input_stage_digest: needs a GPU")
    print(f"input_stage_digest: {_lib.LIB_PATH}, library version {_lib.load().xvit_version()}", file=sys.stderr)
    draws()
    augment_applies()
    contrast_applies()
    crops()
    torch.cuda.synchronize()
