"""GPU: xvit_volume_bbox (csrc/volume_bbox.hip) against the NumPy restatement of tests/_crop_check.py, under its gate: boxes, crop, the
crop scale, FLAGS and the matrix bit for bit, the offsets bit for bit at kf == 1 and within 2^-23 otherwise, every other slot untouched.

Shapes (tests/_crop_check.py `volume_sets`): 5 x 6 x 7, 4 x 3 x 3 and 6 x 5 x 1, where a 16-byte run spans two and three rows and every row;
9 x 10 x 37, an odd voxel count, with nvol = 3, M = 3 and nvol = 4, M = 2, so that later volumes start 2-byte aligned; 9 x 31 x 31, the
smallest shape the chunk rule splits (two chunks per volume), with single voxels on the first and last voxel of each chunk, of its scalar
head, of its 16-byte runs and of its scalar tail.  A voxel at each corner, empty and full volumes, an empty modality beside a non-empty
one, values equal to the threshold, -0.0, NaN and the infinities, a negative threshold.  Sentinels frame boxes, crop, the table and the
workspace's claimed size."""
import numpy as np
import pytest
import torch

import _crop_check as X
from _util import dev

pytestmark = pytest.mark.gpu

DTYPES = ("int16", "bf16", "fp32")
SENT_I, SENT_F, SENT_B = -777777, -12345.678, 0xA5
SET_NAMES = {d: sorted(X.volume_sets(d)) for d in DTYPES}


def on_gpu(src, dtype_name, M):
    t = torch.from_numpy(np.ascontiguousarray(src))
    t = t.to(torch.bfloat16) if dtype_name == "bf16" else t
    if dtype_name != "int16":
        assert torch.equal(t.float().nan_to_num(nan=7.0), torch.from_numpy(src).nan_to_num(nan=7.0)), "the values are exact in the source dtype"
    return t.to(dev()).reshape((src.shape[0] // M, M) + src.shape[1:])


def run(src_np, dtype_name, M, above, margin, mode, up, img, table_np):
    """One call of the pair into sentinel-framed outputs -> (boxes, crop, table or None) as NumPy, and the workspace bytes it left."""
    from xvit import _lib, ops
    from xvit.augment import crop_config
    src = on_gpu(src_np, dtype_name, M)
    nvol, B = src_np.shape[0], src_np.shape[0] // M
    need = _lib.load().xvit_volume_bbox_workspace_bytes(nvol, int(np.prod(src_np.shape[1:])))
    assert need == X.workspace_bytes(nvol, int(np.prod(src_np.shape[1:])))
    fb = torch.full((nvol * 8 + 32,), SENT_I, dtype=torch.int32, device=dev())
    fc = torch.full((B * 8 + 32,), SENT_I, dtype=torch.int32, device=dev())
    fw = torch.full((need + 64,), SENT_B, dtype=torch.uint8, device=dev())
    fp = torch.full((nvol * 32 + 32,), SENT_F, dtype=torch.float32, device=dev())
    boxes, crop, ws = fb[16:16 + nvol * 8].view(B, M, 8), fc[16:16 + B * 8].view(B, 8), fw[32:32 + need]
    params = None
    if table_np is not None:
        params = fp[16:16 + nvol * 32].view(B, M, 32)
        params.view(torch.int32).copy_(torch.from_numpy(table_np.view(np.int32)).view(B, M, 32))          # bit patterns: NaN payloads survive
    ops.volume_bbox(src, crop_config(mode, margin, up, above), img, boxes, crop, ws, params)
    torch.cuda.synchronize()
    for name, frame, n, sent in (("boxes", fb, nvol * 8, SENT_I), ("crop", fc, B * 8, SENT_I), ("params", fp, nvol * 32, np.float32(SENT_F))):
        f = frame.cpu().numpy()
        assert np.all(f[:16] == sent) and np.all(f[16 + n:] == sent), f"a write outside {name}"
    w = fw.cpu().numpy()
    assert np.all(w[:32] == SENT_B) and np.all(w[32 + need:] == SENT_B), "a write outside the workspace's claimed size"
    if table_np is None:
        assert np.all(fp.cpu().numpy() == np.float32(SENT_F))
    table = None if table_np is None else params.view(torch.int32).cpu().numpy().view(np.float32).reshape(nvol, 32).copy()
    return boxes.cpu().numpy().reshape(nvol, 8), crop.cpu().numpy(), table, w[32:32 + need].copy()


@pytest.mark.parametrize("dtype_name,name", [(d, n) for d in DTYPES for n in SET_NAMES[d]])
def test_boxes_and_crops_match_np_nonzero(dtype_name, name):
    src, M, above = X.volume_sets(dtype_name)[name]
    shape = src.shape[1:]
    rng = np.random.default_rng(11)
    for margin in ((0, 0, 0), (1, 0, 2)):
        boxes, crop, table, _ = run(src, dtype_name, M, above, margin, "fit", False, (4, 4, 4), None)              # params = NULL: no fold
        X.check_tables(f"{dtype_name} {name} margin {margin}", boxes, crop, None, None, src, M, above, margin, None, False, (4, 4, 4))
    before = X.tables(src.shape[0], M, shape, (4, 4, 4), "general", rng)
    boxes, crop, table, _ = run(src, dtype_name, M, above, (1, 1, 1), None, False, (4, 4, 4), before)                # mode 0: the table is left alone
    X.check_tables(f"{dtype_name} {name} mode 0", boxes, crop, table, before, src, M, above, (1, 1, 1), None, False, (4, 4, 4))


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("case", X.FOLD_CASES, ids=lambda c: "-".join(str(v).replace(" ", "") for v in c))
def test_the_fold_matches_the_float64_restatement(case, dtype_name):
    name, img, mode, margin, up, kind = case
    src, M, above = X.volume_sets(dtype_name)[name]
    before = X.tables(src.shape[0], M, src.shape[1:], img, kind, np.random.default_rng(3))
    boxes, crop, table, ws = run(src, dtype_name, M, above, margin, mode, up, img, before)
    X.check_tables(f"{dtype_name} {case}", boxes, crop, table, before, src, M, above, margin, mode, up, img)
    again = run(src, dtype_name, M, above, margin, mode, up, img, before)                                            # fresh outputs: identical bytes
    assert np.array_equal(again[0], boxes) and np.array_equal(again[1], crop) and np.array_equal(again[3], ws)
    assert np.array_equal(again[2].view(np.uint32), table.view(np.uint32))


def test_samples_of_a_batch_do_not_mix():
    """Every sample is folded from its own crop: shuffling the samples of a batch shuffles the records."""
    src, M, above = X.volume_sets("int16")["brain-9x10x37-m2"]
    img = (4, 8, 16)
    before = X.tables(4, M, src.shape[1:], img, "general", np.random.default_rng(5))
    _, crop, table, _ = run(src, "int16", M, above, (0, 0, 0), "fit", False, img, before)
    swap = [2, 3, 0, 1]
    _, crop2, table2, _ = run(src[swap], "int16", M, above, (0, 0, 0), "fit", False, img, before[swap])
    assert np.array_equal(crop2, crop[[1, 0]]) and np.array_equal(table2.view(np.uint32), table[swap].view(np.uint32))
    assert not np.array_equal(crop[0], crop[1])
