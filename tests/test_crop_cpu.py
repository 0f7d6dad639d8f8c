"""CPU: the foreground crop without a GPU.  The two entry points are exported and bound; every argument error of xvit_volume_bbox is refused
on the host before any launch, with its message (dummy aligned addresses that are never dereferenced); the struct, the enums and the record
constants are the same in include/xvit.h, xvit._lib, xvit.augment and tests/_crop_check.py; the workspace size follows the documented chunk
rule; VolumeAugment and foreground_boxes refuse bad arguments; the default stage has no crop."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import _crop_check as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "xvit.h")).read()
P = 4096   # any non-null, 16-byte aligned "address"


def _lib():
    from xvit import _lib
    return _lib, _lib.load()


def _config(mode=2, margin=(0, 0, 0), allow_upscale=0, foreground_above=0.0):
    from xvit import _lib
    c = _lib.CropConfig()
    c.mode, c.margin[:], c.allow_upscale, c.foreground_above = mode, margin, allow_upscale, foreground_above
    return c


def test_new_symbols_are_exported_and_bound():
    mod, lib = _lib()
    for name in ("xvit_volume_bbox", "xvit_volume_bbox_workspace_bytes"):
        assert name in mod.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b(int|int64_t) " + name + r"\(", HEADER)
    assert "xvit_volume_bbox" in mod.SIGNATURES and len(mod.SIGNATURES["xvit_volume_bbox"]) == 17
    assert lib.xvit_version() >= 318
    src = open(os.path.join(ROOT, "cross-attention-vit_amd", "build.py")).read()
    assert '"volume_bbox.hip"' in src


def test_config_struct_and_constants_match_the_header():
    from xvit import _lib, augment
    body = re.search(r"typedef struct xvit_crop_config \{(.*?)\} xvit_crop_config;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, decl in re.findall(r"(float|int)\s+([^;]+);", body):
        for item in decl.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            fields.append((m.group(1), int(m.group(2) or 1), ctype))
    kind = lambda t: "int" if (t._type_ if hasattr(t, "_length_") else t) is C.c_int32 else "float"   # noqa: E731
    assert [(n, getattr(t, "_length_", 1), kind(t)) for n, t in _lib.CropConfig._fields_] == fields
    assert fields == [("mode", 1, "int"), ("margin", 3, "int"), ("allow_upscale", 1, "int"), ("foreground_above", 1, "float")]
    assert C.sizeof(_lib.CropConfig) == 24 and _lib.CropConfig.foreground_above.offset == 20
    assert int(re.search(r"#define XVIT_BBOX_NREC (\d+)", HEADER).group(1)) == _lib.BBOX_NREC == augment.BBOX_NREC == X.NREC == 8
    assert int(re.search(r"#define XVIT_AUG_CROP_SCALE (\d+)", HEADER).group(1)) == _lib.AUG_CROP_SCALE == augment.CROP_SCALE == X.CROP_SCALE == 31
    enum = dict((k, int(v)) for k, v in re.findall(r"XVIT_BBOX_([A-Z0-9]+) = (\d+)", HEADER))
    assert enum == dict(Z0=0, Z1=1, Y0=2, Y1=3, X0=4, X1=5, COUNT=6)
    assert [getattr(_lib, "BBOX_" + k) for k in ("Z0", "Z1", "Y0", "Y1", "X0", "X1", "COUNT")] == list(range(7))
    modes = dict((k, int(v)) for k, v in re.findall(r"XVIT_CROP_([A-Z_]+) = (\d+)", HEADER))
    assert modes == dict(BOXES_ONLY=0, CENTER=1, FIT=2) == dict(BOXES_ONLY=_lib.CROP_BOXES_ONLY, CENTER=_lib.CROP_CENTER, FIT=_lib.CROP_FIT)
    assert X.MODES == {None: 0, "center": 1, "fit": 2} == augment._CROP_MODES


def test_workspace_bytes_follow_the_documented_chunk_rule():
    mod, lib = _lib()
    src = open(os.path.join(ROOT, "cross-attention-vit_amd", "csrc", "volume_bbox.hip")).read()
    assert int(re.search(r"kBoxMinChunk = (\d+);", src).group(1)) == X.MIN_CHUNK and int(re.search(r"kBoxMaxGroups = (\d+);", src).group(1)) == X.MAX_GROUPS
    assert "2048 / nvol" in HEADER and "nvox / 8192" in HEADER
    for nvol in (1, 2, 3, 12, 16, 100, 2047, 2048, 2049, 5000):
        for nvox in (1, 7, 8, 8191, 8192, 8193, 8649, 16384, 16385, 210 * 1000, 240 * 240 * 155, 2 ** 31 - 1):
            assert lib.xvit_volume_bbox_workspace_bytes(nvol, nvox) == X.workspace_bytes(nvol, nvox), (nvol, nvox)
            parts, chunk = X.chunk_rule(nvol, nvox)
            assert chunk % 8 == 0 and (parts - 1) * chunk < nvox <= parts * chunk and nvol * parts <= max(nvol, X.MAX_GROUPS)
            assert lib.xvit_volume_bbox_workspace_bytes(nvol, nvox) <= lib.xvit_volume_bbox_workspace_bytes(nvol, 2 ** 31 - 1)
    assert X.chunk_rule(16, 240 * 240 * 155) == (128, 69752)
    assert lib.xvit_volume_bbox_workspace_bytes(0, 100) == 0 and lib.xvit_volume_bbox_workspace_bytes(4, 0) == 0


def test_argument_errors_do_not_launch():
    mod, lib = _lib()
    err = lib.xvit_last_error_string
    need = lib.xvit_volume_bbox_workspace_bytes(4, 9 * 10 * 37)

    def bbox(src=P, sdt=2, nvol=4, M=2, vs=(9, 10, 37), d=(8, 8, 16), cfg=None, boxes=2 * P, crop=3 * P, params=4 * P, ws=5 * P, wsb=None, null_cfg=False):
        cfg = cfg if cfg is not None else _config()
        return lib.xvit_volume_bbox(src, sdt, nvol, M, *vs, *d, None if null_cfg else C.byref(cfg), boxes, crop, params, ws, need if wsb is None else wsb, None)

    for kw in (dict(src=None), dict(null_cfg=True), dict(boxes=None), dict(crop=None), dict(ws=None)):
        assert bbox(**kw) < 0 and b"xvit_volume_bbox" in err() and b"null" in err(), kw
    for sdt in (3, -1):
        assert bbox(sdt=sdt) < 0 and b"unknown source dtype" in err()
    for mode in (3, -1):
        assert bbox(cfg=_config(mode=mode)) < 0 and b"unknown mode" in err()
    for nvol, M in ((0, 1), (-2, 1), (4, 0), (4, -1), (4, 3), (2, 4)):
        assert bbox(nvol=nvol, M=M) < 0 and b"multiple of M" in err(), (nvol, M)
    for vs, d in (((0, 10, 37), (8, 8, 16)), ((9, -1, 37), (8, 8, 16)), ((9, 10, 0), (8, 8, 16)), ((9, 10, 37), (0, 8, 16)), ((9, 10, 37), (8, -4, 16)),
                  ((9, 10, 37), (8, 8, 0))):
        assert bbox(vs=vs, d=d) < 0 and b"must be positive" in err(), (vs, d)
    assert bbox(vs=(2048, 1024, 1024)) < 0 and b"2^31" in err()                      # exactly 2^31 voxels
    for margin in ((-1, 0, 0), (0, -1, 0), (0, 0, -5)):
        assert bbox(cfg=_config(margin=margin)) < 0 and b"margin" in err()
    assert bbox(cfg=_config(foreground_above=math.nan)) < 0 and b"NaN" in err()
    assert bbox(src=P + 1) < 0 and b"element size" in err()
    assert bbox(src=P + 2, sdt=1) < 0 and b"element size" in err()                   # fp32 at a 2-byte boundary
    for kw in (dict(boxes=2 * P + 8), dict(crop=3 * P + 4), dict(params=4 * P + 4), dict(ws=5 * P + 8)):
        assert bbox(**kw) < 0 and b"16-byte aligned" in err(), kw
    assert bbox(wsb=need - 1) < 0 and b"workspace of" in err() and str(need).encode() in err()
    assert bbox(wsb=0) < 0 and b"workspace of" in err()


def test_the_python_side_refuses_bad_arguments():
    from xvit.augment import AugmentParams, ForegroundBoxes, VolumeAugment, crop_config, foreground_boxes
    for kw in (dict(crop_foreground="centre"), dict(crop_foreground="box"), dict(crop_foreground=1), dict(crop_foreground="fit", crop_margin=-1),
               dict(crop_foreground="fit", crop_margin=1.5), dict(crop_foreground="fit", crop_margin=(1, 2)), dict(crop_foreground="fit", crop_margin=(1, 2, -3)),
               dict(crop_foreground="fit", crop_margin=(1, 2, 3.0)), dict(crop_foreground="center", crop_margin=True), dict(crop_foreground="center", crop_margin="4"),
               dict(crop_foreground="center", crop_above=math.nan), dict(crop_margin=-2), dict(crop_foreground="fit", crop_margin=2 ** 31)):
        with pytest.raises(ValueError, match="VolumeAugment: crop_"):
            VolumeAugment((8, 8, 8), **kw)
    aug = VolumeAugment((8, 8, 8), crop_foreground="fit", crop_margin=(1, 2, 3), crop_upscale=True, foreground_above=2.5)
    c = aug.crop_config
    assert (c.mode, tuple(c.margin), c.allow_upscale, c.foreground_above) == (2, (1, 2, 3), 1, 2.5) and aug.last_crop is None     # crop_above: foreground_above
    c = VolumeAugment((8, 8, 8), crop_foreground="center", crop_margin=4, crop_above=-1.0, foreground_above=2.5).crop_config
    assert (c.mode, tuple(c.margin), c.allow_upscale, c.foreground_above) == (1, (4, 4, 4), 0, -1.0)
    default = VolumeAugment((8, 8, 8))
    assert default.crop_foreground is None and default.crop_config.mode == 0 and default.last_crop is None
    with pytest.raises(ValueError, match="crop_margin"):
        crop_config("fit", margin=[1, 2])
    with pytest.raises(RuntimeError, match="GPU"):
        foreground_boxes(torch.zeros(2, 2, 4, 4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        aug(torch.zeros(2, 2, 4, 4, 4, dtype=torch.int16))

    class FakeCuda(torch.Tensor):
        is_cuda = True

    with pytest.raises(ValueError, match="need"):
        foreground_boxes(torch.zeros(2, 4, 4, 4).as_subclass(FakeCuda))
    with pytest.raises(TypeError, match="not supported"):
        foreground_boxes(torch.zeros(2, 2, 4, 4, 4, dtype=torch.float64).as_subclass(FakeCuda))
    with pytest.raises(ValueError, match="contiguous"):
        foreground_boxes(torch.zeros(2, 2, 4, 4, 8)[..., ::2].as_subclass(FakeCuda))
    with pytest.raises(ValueError, match="crop_margin"):
        foreground_boxes(torch.zeros(2, 2, 4, 4, 4).as_subclass(FakeCuda), margin=-1)
    with pytest.raises(ValueError, match="NaN"):
        foreground_boxes(torch.zeros(2, 2, 4, 4, 4).as_subclass(FakeCuda), foreground_above=math.nan)

    boxes, crop = torch.arange(2 * 3 * 8, dtype=torch.int32).reshape(2, 3, 8), torch.arange(100, 116, dtype=torch.int32).reshape(2, 8)
    fb = ForegroundBoxes(boxes, crop)
    assert fb.lo.tolist() == [[100, 102, 104], [108, 110, 112]] and fb.hi.tolist() == [[101, 103, 105], [109, 111, 113]]
    assert fb.nonempty.tolist() == [106, 114] and fb.count.tolist() == [[6, 14, 22], [30, 38, 46]]
    assert fb.volume_lo[1, 2].tolist() == [40, 42, 44] and fb.volume_hi[1, 2].tolist() == [41, 43, 45]
    assert fb.clone().boxes is not boxes and torch.equal(fb.clone().crop, crop)
    for bad in ((boxes.float(), crop), (boxes, crop[:1]), (boxes[..., :7], crop), (boxes, crop.long())):
        with pytest.raises(ValueError, match="ForegroundBoxes"):
            ForegroundBoxes(*bad)
    t = torch.arange(64, dtype=torch.float32).reshape(1, 2, 32)
    assert AugmentParams(t).crop_scale.tolist() == [[31.0, 63.0]]
    AugmentParams(t).crop_scale[0, 1] = 2.0                                            # a view
    assert t[0, 1, 31] == 2.0


def test_a_capturable_stage_allocates_its_box_tables_outside_a_capture(monkeypatch):
    from xvit.augment import VolumeAugment
    aug = VolumeAugment((8, 8, 8), crop_foreground="fit", capturable=True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="call the stage once on this batch shape before capturing it"):
        aug._table(2, 2, torch.device("cpu"))
    assert not aug._tables and not aug._crops
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    aug._table(2, 2, torch.device("cpu"))                                              # outside a capture: everything at once
    boxes, crop, workspace = aug._crops[(2, 2, torch.device("cpu"))]
    assert tuple(boxes.shape) == (2, 2, 8) and tuple(crop.shape) == (2, 8) and boxes.dtype == crop.dtype == torch.int32
    assert workspace.numel() == X.workspace_bytes(4, 2 ** 31 - 1) == 4 * 512 * 32
    plain = VolumeAugment((8, 8, 8), capturable=True)
    plain._table(2, 2, torch.device("cpu"))
    assert not plain._crops                                                            # no crop: nothing new is allocated
