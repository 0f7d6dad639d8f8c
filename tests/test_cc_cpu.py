"""CPU: the connected foreground components without a GPU.  The three entry points are exported and bound; every argument error of
xvit_volume_components and xvit_volume_bbox_components is refused on the host before any launch, with its message (dummy aligned
addresses that are never dereferenced); the struct, the enums and the record constants are the same in include/xvit.h, xvit._lib,
xvit.augment and tests/_cc_check.py; the workspace size is the documented sum; VolumeAugment, foreground_components and foreground_boxes
refuse bad arguments; without crop_component the stage holds nothing of it."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import _cc_check as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "xvit.h")).read()
P = 4096   # any non-null, 16-byte aligned "address"


def _lib():
    from xvit import _lib
    return _lib, _lib.load()


def _comp(connectivity=6, keep=0, min_voxels=1, foreground_above=0.0):
    from xvit import _lib
    c = _lib.ComponentConfig()
    c.connectivity, c.keep, c.min_voxels, c.foreground_above = connectivity, keep, min_voxels, foreground_above
    return c


def _crop(mode=2, margin=(0, 0, 0), allow_upscale=0, foreground_above=0.0):
    from xvit import _lib
    c = _lib.CropConfig()
    c.mode, c.margin[:], c.allow_upscale, c.foreground_above = mode, margin, allow_upscale, foreground_above
    return c


def test_new_symbols_are_exported_and_bound():
    mod, lib = _lib()
    for name in ("xvit_volume_components", "xvit_volume_bbox_components", "xvit_volume_components_workspace_bytes"):
        assert name in mod.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b(int|int64_t) " + name + r"\(", HEADER)
    assert len(mod.SIGNATURES["xvit_volume_components"]) == 12 and len(mod.SIGNATURES["xvit_volume_bbox_components"]) == 20
    assert lib.xvit_version() >= 322
    src = open(os.path.join(ROOT, "cross-attention-vit_amd", "build.py")).read()
    assert '"volume_components.hip"' in src


def test_config_struct_and_constants_match_the_header():
    from xvit import _lib, augment
    body = re.search(r"typedef struct xvit_component_config \{(.*?)\} xvit_component_config;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(name, ctype) for ctype, name in re.findall(r"(float|int)\s+(\w+);", body)]
    assert fields == [("connectivity", "int"), ("keep", "int"), ("min_voxels", "int"), ("foreground_above", "float")]
    assert [(n, "int" if t is C.c_int32 else "float") for n, t in _lib.ComponentConfig._fields_] == fields
    assert C.sizeof(_lib.ComponentConfig) == 16 and _lib.ComponentConfig.foreground_above.offset == 12
    assert C.sizeof(_lib.CropConfig) == 24, "the crop config keeps its layout: the new options have their own struct"
    assert int(re.search(r"#define XVIT_CC_NREC (\d+)", HEADER).group(1)) == _lib.CC_NREC == augment.CC_NREC == CC.NREC == 8
    slots = dict((k, int(v)) for k, v in re.findall(r"XVIT_CC_(COUNT|LARGEST_ROOT|LARGEST_SIZE|KEPT|KEPT_VOXELS|STATUS) = (\d+)", HEADER))
    assert slots == dict(COUNT=0, LARGEST_ROOT=1, LARGEST_SIZE=2, KEPT=3, KEPT_VOXELS=4, STATUS=5)
    assert [getattr(_lib, "CC_" + k) for k in slots] == list(range(6)) == [CC.COUNT, CC.LARGEST_ROOT, CC.LARGEST_SIZE, CC.KEPT, CC.KEPT_VOXELS, CC.STATUS]
    keep = dict((k, int(v)) for k, v in re.findall(r"XVIT_CC_(LARGEST|MIN_VOXELS) = (\d+)", HEADER))
    assert keep == dict(LARGEST=0, MIN_VOXELS=1) == dict(LARGEST=_lib.CC_LARGEST, MIN_VOXELS=_lib.CC_MIN_VOXELS) == dict(LARGEST=CC.LARGEST, MIN_VOXELS=CC.MIN_VOXELS)
    src = open(os.path.join(ROOT, "cross-attention-vit_amd", "csrc", "volume_components.hip")).read()
    assert tuple(int(v) for v in re.search(r"kCcTZ = (\d+), kCcTY = (\d+), kCcTX = (\d+);", src).groups()) == CC.TILE


def test_workspace_bytes_are_the_documented_sum():
    mod, lib = _lib()
    for nvol in (1, 2, 3, 16, 2049):
        for nvox in (1, 7, 105, 2673, 8192, 240 * 240 * 155, 2 ** 31 - 1):
            want = 32 * nvol + (4 * nvol * nvox + 15) // 16 * 16 + lib.xvit_volume_bbox_workspace_bytes(nvol, nvox)
            assert lib.xvit_volume_components_workspace_bytes(nvol, nvox) == want, (nvol, nvox)
            assert want % 16 == 0
    assert lib.xvit_volume_components_workspace_bytes(0, 100) == 0 and lib.xvit_volume_components_workspace_bytes(4, 0) == 0
    assert lib.xvit_volume_components_workspace_bytes(16, 240 * 240 * 155) == 512 + 571392000 + 65536


def test_argument_errors_do_not_launch():
    mod, lib = _lib()
    err = lib.xvit_last_error_string
    need = lib.xvit_volume_components_workspace_bytes(4, 9 * 10 * 37)

    def comps(src=P, sdt=2, nvol=4, vs=(9, 10, 37), cfg=None, labels=2 * P, table=3 * P, ws=5 * P, wsb=None, null_cfg=False):
        cfg = cfg if cfg is not None else _comp()
        return lib.xvit_volume_components(src, sdt, nvol, *vs, None if null_cfg else C.byref(cfg), labels, table, ws, need if wsb is None else wsb, None)

    def boxes(src=P, sdt=2, nvol=4, M=2, vs=(9, 10, 37), d=(8, 8, 16), crop_cfg=None, cfg=None, boxes=6 * P, crop=7 * P, params=8 * P, labels=2 * P, table=3 * P,
              ws=5 * P, wsb=None, null_cfg=False, null_crop_cfg=False):
        cfg = cfg if cfg is not None else _comp()
        crop_cfg = crop_cfg if crop_cfg is not None else _crop()
        return lib.xvit_volume_bbox_components(src, sdt, nvol, M, *vs, *d, None if null_crop_cfg else C.byref(crop_cfg), None if null_cfg else C.byref(cfg), boxes,
                                               crop, params, labels, table, ws, need if wsb is None else wsb, None)

    for fn, who in ((comps, b"xvit_volume_components"), (boxes, b"xvit_volume_bbox_components")):
        for kw in (dict(src=None), dict(null_cfg=True), dict(labels=None), dict(table=None), dict(ws=None)):
            assert fn(**kw) < 0 and who + b":" in err() and b"null" in err(), kw
        for sdt in (3, -1):
            assert fn(sdt=sdt) < 0 and b"unknown source dtype" in err()
        for conn in (18, 0, 4, 8, 27, -6):
            assert fn(cfg=_comp(connectivity=conn)) < 0 and b"must be 6 or 26" in err(), conn
        for keep in (2, -1):
            assert fn(cfg=_comp(keep=keep)) < 0 and b"unknown keep mode" in err()
        for n in (0, -3):
            for keep in (0, 1):
                assert fn(cfg=_comp(keep=keep, min_voxels=n)) < 0 and b"min_voxels" in err()
        assert fn(cfg=_comp(foreground_above=math.nan)) < 0 and b"NaN" in err()
        for nvol, vs in ((0, (9, 10, 37)), (-2, (9, 10, 37)), (4, (0, 10, 37)), (4, (9, -1, 37)), (4, (9, 10, 0))):
            assert fn(nvol=nvol, vs=vs) < 0 and b"must be positive" in err(), (nvol, vs)
        assert fn(vs=(2048, 1024, 1024)) < 0 and b"2^31" in err()                      # exactly 2^31 voxels
        assert fn(src=P + 1) < 0 and b"element size" in err()
        assert fn(src=P + 2, sdt=1) < 0 and b"element size" in err()                   # fp32 at a 2-byte boundary
        for kw in (dict(labels=2 * P + 8), dict(table=3 * P + 4), dict(ws=5 * P + 8)):
            assert fn(**kw) < 0 and b"16-byte aligned" in err(), kw
        assert fn(wsb=need - 1) < 0 and b"workspace of" in err() and str(need).encode() in err()
        assert fn(wsb=0) < 0 and b"workspace of" in err()
    # what xvit_volume_bbox refuses
    for kw in (dict(null_crop_cfg=True), dict(boxes=None), dict(crop=None)):
        assert boxes(**kw) < 0 and b"xvit_volume_bbox_components" in err() and b"null" in err(), kw
    for mode in (3, -1):
        assert boxes(crop_cfg=_crop(mode=mode)) < 0 and b"unknown mode" in err()
    for nvol, M in ((4, 0), (4, -1), (4, 3), (2, 4)):
        assert boxes(nvol=nvol, M=M) < 0 and b"multiple of M" in err(), (nvol, M)
    for d in ((0, 8, 16), (8, -4, 16), (8, 8, 0)):
        assert boxes(d=d) < 0 and b"must be positive" in err(), d
    for margin in ((-1, 0, 0), (0, -1, 0), (0, 0, -5)):
        assert boxes(crop_cfg=_crop(margin=margin)) < 0 and b"margin" in err()
    assert boxes(crop_cfg=_crop(foreground_above=1.0)) < 0 and b"same foreground_above" in err()
    assert boxes(crop_cfg=_crop(foreground_above=math.nan), cfg=_comp(foreground_above=math.nan)) < 0 and b"NaN" in err()
    for kw in (dict(boxes=6 * P + 8), dict(crop=7 * P + 4), dict(params=8 * P + 4)):
        assert boxes(**kw) < 0 and b"16-byte aligned" in err(), kw


def test_the_python_side_refuses_bad_arguments():
    from xvit.augment import ForegroundBoxes, ForegroundComponents, VolumeAugment, component_config, foreground_boxes, foreground_components
    with pytest.raises(ValueError, match="crop_component needs crop_foreground"):
        VolumeAugment((8, 8, 8), crop_component="largest")
    with pytest.raises(ValueError, match="crop_component needs crop_foreground"):
        VolumeAugment((8, 8, 8), crop_component=10, crop_connectivity=26)
    for kw in (dict(crop_component="biggest"), dict(crop_component=0), dict(crop_component=-4), dict(crop_component=2.0), dict(crop_component=True),
               dict(crop_component=2 ** 31), dict(crop_component=("largest",)), dict(crop_component="largest", crop_connectivity=18),
               dict(crop_component=5, crop_connectivity=4), dict(crop_connectivity=18), dict(crop_component="largest", crop_connectivity="6"),
               dict(crop_component="largest", crop_connectivity=True)):
        with pytest.raises(ValueError, match="VolumeAugment: crop_(component|connectivity)"):
            VolumeAugment((8, 8, 8), crop_foreground="fit", **kw)
    aug = VolumeAugment((8, 8, 8), crop_foreground="fit", crop_component="largest", foreground_above=2.5)
    c = aug.component_config
    assert (c.connectivity, c.keep, c.min_voxels, c.foreground_above) == (6, 0, 1, 2.5) == (6, CC.LARGEST, 1, aug.crop_config.foreground_above)
    c = VolumeAugment((8, 8, 8), crop_foreground="center", crop_component=40, crop_connectivity=26, crop_above=-1.0, foreground_above=2.5).component_config
    assert (c.connectivity, c.keep, c.min_voxels, c.foreground_above) == (26, CC.MIN_VOXELS, 40, -1.0)
    with pytest.raises(ValueError, match="NaN"):
        component_config("largest", 6, math.nan)
    for call in (lambda: foreground_components(torch.zeros(2, 2, 4, 4, 4)), lambda: foreground_boxes(torch.zeros(2, 2, 4, 4, 4), component="largest"),
                 lambda: aug(torch.zeros(2, 2, 4, 4, 4, dtype=torch.int16))):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="ForegroundComponents"):
        ForegroundComponents(torch.zeros(2, 2, 4, 4, 4), torch.zeros(2, 2, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="ForegroundComponents"):
        ForegroundComponents(torch.zeros(2, 2, 4, 4, 4, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int32))
    table = torch.arange(32, dtype=torch.int32).reshape(2, 2, 8)
    fc = ForegroundComponents(torch.zeros(2, 2, 4, 4, 4, dtype=torch.int32), table)
    assert [getattr(fc, n)[1, 0].item() for n in ("count", "largest_root", "largest_size", "kept", "kept_voxels", "status")] == list(range(16, 22))
    fb = ForegroundBoxes(torch.zeros(2, 2, 8, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int32))
    assert fb.components is None and fb.clone().components is None
    fb = ForegroundBoxes(torch.zeros(2, 2, 8, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int32), fc)
    assert fb.clone().components.table is not table and torch.equal(fb.clone().components.table, table)


def test_without_the_option_the_stage_holds_nothing_of_it():
    from xvit.augment import VolumeAugment
    for kw in (dict(), dict(crop_foreground="fit"), dict(crop_foreground="center", crop_connectivity=26)):
        aug = VolumeAugment((8, 8, 8), **kw)
        assert aug.crop_component is None and aug.component_config is None and not aug._components
