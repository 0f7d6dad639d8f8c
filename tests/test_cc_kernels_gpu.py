"""GPU: xvit_volume_components and xvit_volume_bbox_components (csrc/volume_components.hip) against the NumPy restatement of
tests/_cc_check.py, bit for bit: labels, comps and boxes with assert_array_equal, sentinels around every output, status 0, and every call
made twice with the bytes compared.

Shapes (tests/_cc_check.py, SHAPES): (1, 1, 1), (1, 1, 9), (3, 5, 7); T - 1, T, T + 1 and 2 T + 1 along each axis of the (8, 8, 32) tile;
(40, 36, 70); one 64^3 case of four volumes.  Several have an odd voxel count, so later volumes are only element-aligned.  Every shape
carries all patterns of `masks` as the volumes of one call (M = 2: the first sample pairs a full with an empty modality), at connectivity 6
and 26, as int16, bf16 and fp32 (the float backgrounds hold NaN, -0.0 and -inf; the specks hold the largest values)."""
import functools

import numpy as np
import pytest
import torch

import _crop_check as X
import _cc_check as CC
from _util import dev

pytestmark = pytest.mark.gpu

GUARD = 64                                        # sentinel elements on either side of an output
SENTINEL = {torch.int32: -0x5A5A5A5B, torch.float32: float("nan")}
TORCH = {"int16": torch.int16, "bf16": torch.bfloat16, "fp32": torch.float32}
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)     # noqa: E731


def guarded(shape, dtype=torch.int32):
    """(buffer, view): a contiguous 16-byte aligned view of `shape` with GUARD sentinel elements on either side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=dev())
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf, what):
    edge = torch.cat([buf[:GUARD], buf[-GUARD:]]).view(torch.int32)
    want = torch.full((1,), SENTINEL[buf.dtype], dtype=buf.dtype).view(torch.int32).item()
    assert bool((edge == want).all()), f"{what}: written outside the output"


@functools.lru_cache(maxsize=None)
def source(shape, conn, dtype_name):
    """Computed once and shared.  -> (src on the device [B, 2, Ds, Hs, Ws], its foreground equals CC.case(shape, conn)'s)."""
    names, fg, labels = CC.case(shape, conn)
    v = CC.values(fg, dtype_name, CC.specks_of(names, labels))
    assert np.array_equal(CC.foreground(v, 0.0), fg)
    t = torch.from_numpy(v).to(dev())
    t = t.to(torch.bfloat16) if dtype_name == "bf16" else t
    assert np.array_equal(CC.foreground(t.float().cpu().numpy(), 0.0), fg), "the cast keeps the foreground"
    return t.reshape((fg.shape[0] // 2, 2) + tuple(shape)).contiguous()


def config(conn, keep, n, above=0.0):
    from xvit import _lib
    c = _lib.ComponentConfig()
    c.connectivity, c.keep, c.min_voxels, c.foreground_above = conn, keep, n, above
    return c


def run(src, conn, keep, n, margin=(0, 0, 0), mode=None, img_size=(1, 1, 1), table=None, boxes_too=True):
    """One call with sentinels around labels, comps, boxes and crop -> numpy (labels, comps, boxes, crop)."""
    from xvit import ops
    from xvit.augment import crop_config
    B, M = src.shape[:2]
    ws = ops.volume_components_workspace(B * M, src[0, 0].numel(), dev())
    ws.fill_(0xA5)                                  # its contents must not matter
    lb, labels = guarded(tuple(src.shape))
    cb, comps = guarded((B, M, 8))
    if not boxes_too:
        ops.volume_components(src, config(conn, keep, n), labels, comps, ws)
        outs = [(lb, labels), (cb, comps)]
    else:
        bb, boxes = guarded((B, M, 8))
        rb, crop = guarded((B, 8))
        ops.volume_bbox_components(src, crop_config(mode, margin, False, 0.0), config(conn, keep, n), img_size, boxes, crop, labels, comps, ws, table)
        outs = [(lb, labels), (cb, comps), (bb, boxes), (rb, crop)]
    torch.cuda.synchronize()
    for buf, _ in outs:
        guards_intact(buf, f"output of {tuple(buf.shape)}")
    return [view.cpu().numpy().reshape((B * M,) + tuple(view.shape[2:])) if view.dim() > 2 else view.cpu().numpy() for _, view in outs]


def check(name, got, labels, keep, n, M, margin, shape):
    comps, boxes = CC.tables_ref(labels, keep, n)
    np.testing.assert_array_equal(got[0], labels, err_msg=f"{name}: labels")
    assert (got[1][:, CC.STATUS] == 0).all(), f"{name}: status {got[1][:, CC.STATUS]}"
    np.testing.assert_array_equal(got[1], comps, err_msg=f"{name}: comps")
    if len(got) > 2:
        np.testing.assert_array_equal(got[2], boxes, err_msg=f"{name}: boxes")
        np.testing.assert_array_equal(got[3], X.crop_ref(boxes, M, margin, shape), err_msg=f"{name}: crop")


@pytest.mark.parametrize("dtype_name", ["int16", "bf16", "fp32"])
@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("shape", CC.SHAPES, ids=ids)
def test_every_pattern_bit_for_bit(shape, conn, dtype_name):
    names, fg, labels = CC.case(shape, conn)
    src = source(shape, conn, dtype_name)
    nvox = int(np.prod(shape))
    name = f"{ids(shape)} connectivity {conn} {dtype_name}"
    first = run(src, conn, CC.LARGEST, 1, margin=(2, 2, 2))
    check(name + " largest", first, labels, CC.LARGEST, 1, 2, (2, 2, 2), shape)
    again = run(src, conn, CC.LARGEST, 1, margin=(2, 2, 2))
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes(), f"{name}: two runs differ"
    alone = run(src, conn, CC.LARGEST, 1, boxes_too=False)
    assert alone[0].tobytes() == first[0].tobytes() and alone[1].tobytes() == first[1].tobytes(), f"{name}: the components alone differ"
    n2 = max(CC.second_size(labels[names.index("brain-specks")]), 1)      # at a component's size, at one more, above every size
    for n in (n2, n2 + 1, nvox + 1):
        check(f"{name} min_voxels {n}", run(src, conn, CC.MIN_VOXELS, n, margin=(1, 0, 2)), labels, CC.MIN_VOXELS, n, 2, (1, 0, 2), shape)


@pytest.mark.parametrize("dtype_name", ["int16", "bf16"])
@pytest.mark.parametrize("conn", [6, 26])
def test_four_volumes_of_64_cubed(conn, dtype_name):
    names, fg, labels = CC.case(CC.CUBE, conn)
    assert len(names) == 4
    src = source(CC.CUBE, conn, dtype_name)
    first = run(src, conn, CC.MIN_VOXELS, 5, margin=(1, 1, 1))
    check(f"64^3 connectivity {conn} {dtype_name}", first, labels, CC.MIN_VOXELS, 5, 2, (1, 1, 1), CC.CUBE)
    again = run(src, conn, CC.MIN_VOXELS, 5, margin=(1, 1, 1))
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes(), "two runs differ"


@pytest.mark.parametrize("conn", [6, 26])
def test_a_threshold_other_than_zero(conn):
    from xvit.augment import foreground_components
    rng = np.random.default_rng(5)
    v = rng.integers(-40, 40, (2, 1, 9, 10, 37)).astype(np.int16)
    got = foreground_components(torch.from_numpy(v).to(dev()), foreground_above=12.0, connectivity=conn)
    labels, comps, _ = CC.reference(CC.foreground(v.reshape(2, 9, 10, 37), 12.0), conn)
    np.testing.assert_array_equal(got.labels.cpu().numpy().reshape(labels.shape), labels)
    np.testing.assert_array_equal(got.table.cpu().numpy().reshape(comps.shape), comps)
    assert got.count.tolist() == comps[:, :1].tolist() and got.status.tolist() == [[0], [0]]


@pytest.mark.parametrize("mode", ["center", "fit"])
def test_the_crop_and_the_fold_are_those_of_volume_bbox_on_the_kept_voxels(mode):
    """The finish is shared: boxes, crop and the folded table equal xvit_volume_bbox's on a source whose dropped components are zeroed."""
    from xvit import ops
    from xvit.augment import crop_config
    shape, conn, img = (17, 9, 33), 6, (8, 8, 16)
    names, fg, labels = CC.case(shape, conn)
    src = source(shape, conn, "int16")
    B, M = src.shape[:2]
    for keep, n in ((CC.LARGEST, 1), (CC.MIN_VOXELS, 4)):
        kept = np.stack([np.isin(lab, CC.comps_ref(lab, keep, n)[1]) & (lab >= 0) for lab in labels])
        clean = torch.from_numpy(np.where(kept, src.cpu().numpy().reshape(kept.shape), 0).astype(np.int16)).to(dev()).reshape(src.shape)
        before = X.tables(B * M, M, shape, img, "general", np.random.default_rng(3))
        t_cc, t_plain = (torch.from_numpy(before.copy()).to(dev()).reshape(B, M, 32) for _ in range(2))
        got = run(src, conn, keep, n, margin=(1, 0, 2), mode=mode, img_size=img, table=t_cc)
        boxes, crop = torch.empty(B, M, 8, dtype=torch.int32, device=dev()), torch.empty(B, 8, dtype=torch.int32, device=dev())
        ops.volume_bbox(clean, crop_config(mode, (1, 0, 2), False, 0.0), img, boxes, crop, ops.volume_bbox_workspace(B * M, int(np.prod(shape)), dev()), t_plain)
        np.testing.assert_array_equal(got[2], boxes.cpu().numpy().reshape(B * M, 8))
        np.testing.assert_array_equal(got[3], crop.cpu().numpy())
        assert torch.equal(t_cc.view(torch.int32), t_plain.view(torch.int32)), "the folded tables differ"
        assert not np.array_equal(t_cc.cpu().numpy().reshape(B * M, 32).view(np.uint32), before.view(np.uint32)), "nothing was folded"
        X.check_tables(f"{mode} keep {keep}", got[2], got[3], t_cc.cpu().numpy().reshape(B * M, 32), before, clean.cpu().numpy().reshape(kept.shape), M, 0.0,
                       (1, 0, 2), mode, False, img)
