"""CPU: the augmenting input stage without a GPU.  The two entry points are exported and bound; every argument error is refused on the
host before any launch, with its message (dummy aligned addresses that are never dereferenced); VolumeAugment refuses CPU tensors, bad
ranks and probabilities or ranges out of order; the AugmentParams views index the record as include/xvit.h lays it out."""
import ctypes as C
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "xvit.h")).read()
P = 256   # any non-null, 16-byte aligned "address"


def _lib():
    from xvit import _lib
    return _lib, _lib.load()


def _config(**kw):
    from xvit import _lib
    c = _lib.AugmentConfig()
    c.zoom_range[:] = (0.9, 1.1)
    c.scale_range[:] = (0.9, 1.1)
    c.shift_range[:] = (-0.1, 0.1)
    c.intensity_scale = 1.0
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(c, k)[:] = v
        else:
            setattr(c, k, v)
    return c


def test_new_symbols_are_exported_and_bound():
    mod, lib = _lib()
    for name in ("xvit_augment_draw", "xvit_augment_apply"):
        assert name in mod.EXPORTS and name in mod.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(", HEADER)
    assert lib.xvit_version() >= 309


def test_config_struct_and_record_constants_match_the_header():
    from xvit import _lib, augment
    body = re.search(r"typedef struct xvit_augment_config \{(.*?)\} xvit_augment_config;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in re.findall(r"float\s+([^;]+);", body):
        for item in decl.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            fields.append((m.group(1), int(m.group(2) or 1)))
    assert [(n, getattr(t, "_length_", 1)) for n, t in _lib.AugmentConfig._fields_] == fields
    assert C.sizeof(_lib.AugmentConfig) == 4 * sum(n for _, n in fields)
    enum = dict((k, int(v)) for k, v in re.findall(r"XVIT_AUG_([A-Z_]+) = (\d+)", HEADER))
    assert int(re.search(r"#define XVIT_AUG_NPARAM (\d+)", HEADER).group(1)) == augment.NPARAM == _lib.AUG_NPARAM == 32
    for name in ("MATRIX", "SCALE", "SHIFT", "SIGMA", "NOISE_SEED", "FLAGS", "FLIPS", "ANGLES", "ZOOMS", "TRANSLATION"):
        assert getattr(augment, name) == enum[name], name
    assert augment.FLAG_EXACT == enum["FLAG_EXACT"] == 1
    assert re.search(r"XVIT_I16 = 2\b", HEADER)
    from xvit import ops
    assert ops.I16 == 2


def test_params_views_index_the_record_as_the_header_says():
    from xvit.augment import AugmentParams
    t = torch.arange(2 * 3 * 32, dtype=torch.float32).reshape(2, 3, 32)
    p = AugmentParams(t)
    row = t[1, 2]
    assert p.matrix.shape == (2, 3, 3, 4) and torch.equal(p.matrix[1, 2], row[0:12].reshape(3, 4))
    assert p.scale[1, 2] == row[12] and p.shift[1, 2] == row[13] and p.sigma[1, 2] == row[14] and p.flags[1, 2] == row[16]
    assert torch.equal(p.flips[1, 2], row[17:20]) and torch.equal(p.angles[1, 2], row[20:23])
    assert torch.equal(p.zooms[1, 2], row[23:26]) and torch.equal(p.translation[1, 2], row[26:29])
    p.matrix[0, 0, 2, 3] = -7.0          # views: writing through them edits the table
    p.scale[0, 1] = 2.5
    assert t[0, 0, 11] == -7.0 and t[0, 1, 12] == 2.5
    t.view(torch.int32)[1, 0, 15] = -2   # a uint32 bit pattern in slot 15
    assert int(p.noise_seed[1, 0]) == 0xFFFFFFFE
    t[..., 16] = torch.tensor([[1.0, 0.0, 3.0], [2.0, 1.0, 0.0]])
    assert p.exact.tolist() == [[True, False, True], [False, True, False]]
    ident = AugmentParams.identity(2, 2, (9, 10, 11), (8, 8, 16))
    assert torch.equal(ident.matrix[1, 1], torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 1.0], [0, 0, 1.0, -2.0]]))    # crop 9 -> 8: 4 - 4; 10 -> 8: 5 - 4; pad 11 -> 16: -(5 // 2)
    assert ident.exact.all() and (ident.scale == 1).all() and (ident.shift == 0).all() and (ident.sigma == 0).all()
    with pytest.raises(ValueError):
        AugmentParams(torch.zeros(2, 2, 31))
    with pytest.raises(ValueError):
        AugmentParams(torch.zeros(2, 2, 32, dtype=torch.float64))


def test_draw_argument_errors_do_not_launch():
    mod, lib = _lib()
    err = lib.xvit_last_error_string

    def draw(cfg=None, params=P, B=2, M=2, src=(9, 10, 11), dst=(8, 8, 16), counter=None, advance=0, null_cfg=False):
        cfg = cfg if cfg is not None else _config()
        return lib.xvit_augment_draw(None if null_cfg else C.byref(cfg), params, B, M, *src, *dst, 0, counter, advance, None)

    assert draw(null_cfg=True) < 0 and b"xvit_augment_draw" in err() and b"null" in err()
    assert draw(params=None) < 0 and b"null" in err()
    assert draw(B=0) < 0 and b"B=0" in err()
    assert draw(M=-1) < 0 and b"M=-1" in err()
    assert draw(src=(9, 0, 11)) < 0 and b"non-positive size" in err()
    assert draw(dst=(8, 8, -16)) < 0 and b"non-positive size" in err()
    assert draw(params=P + 4) < 0 and b"16-byte aligned" in err()
    assert draw(counter=P + 4) < 0 and b"8-byte aligned" in err()
    assert draw(advance=1) < 0 and b"advance needs a counter" in err()
    for field in ("rotate_prob", "zoom_prob", "translate_prob", "scale_prob", "shift_prob", "noise_prob"):
        for bad in (-0.1, 1.5, math.nan):
            assert draw(_config(**{field: bad})) < 0 and b"probability" in err(), (field, bad)
    assert draw(_config(flip_prob=(0.5, 1.01, 0.5))) < 0 and b"probability" in err()
    assert draw(_config(zoom_range=(1.1, 0.9))) < 0 and b"zoom_range" in err() and b"reversed" in err()
    assert draw(_config(zoom_range=(0.0, 0.9))) < 0 and b"zoom_range" in err()
    assert draw(_config(scale_range=(1.1, 0.9))) < 0 and b"scale_range" in err() and b"reversed" in err()
    assert draw(_config(shift_range=(0.1, -0.1))) < 0 and b"shift_range" in err() and b"reversed" in err()
    assert draw(_config(rotate_range=(0.1, -0.1, 0.1))) < 0 and b"half-widths" in err()
    assert draw(_config(translate_range=(8.0, 8.0, -1.0))) < 0 and b"half-widths" in err()
    assert draw(_config(noise_std=-0.05)) < 0 and b"noise_std" in err()


def test_apply_argument_errors_do_not_launch():
    mod, lib = _lib()
    err = lib.xvit_last_error_string

    def apply(src=P, sdt=2, dst=P, ddt=0, params=P, nvol=4, s=(9, 10, 11), d=(8, 8, 16)):
        return lib.xvit_augment_apply(src, sdt, dst, ddt, params, nvol, *s, *d, -1.0, None)

    assert apply(src=None) < 0 and b"xvit_augment_apply" in err() and b"null" in err()
    assert apply(dst=None) < 0 and b"null" in err()
    assert apply(params=None) < 0 and b"null" in err()
    assert apply(sdt=3) < 0 and b"unknown source dtype 3" in err()
    assert apply(sdt=-1) < 0 and b"unknown source dtype" in err()
    assert apply(ddt=2) < 0 and b"unknown destination dtype 2" in err()      # int16 is a source dtype only
    assert apply(nvol=0) < 0 and b"non-positive size" in err()
    assert apply(s=(9, 10, 0)) < 0 and b"non-positive size" in err()
    assert apply(d=(0, 8, 16)) < 0 and b"non-positive size" in err()
    assert apply(s=(2048, 1024, 1024)) < 0 and b"2^31" in err()              # exactly 2^31 source voxels
    assert apply(d=(1 << 11, 1 << 10, 1 << 10)) < 0 and b"2^31" in err()
    assert apply(params=P + 8) < 0 and b"16-byte aligned" in err()
    assert apply(src=P + 1) < 0 and b"element size" in err()
    assert apply(sdt=1, src=P + 2) < 0 and b"element size" in err()
    assert apply(ddt=1, dst=P + 2) < 0 and b"element size" in err()


def test_volume_augment_refuses_bad_arguments():
    from xvit.augment import AugmentParams, VolumeAugment
    for kw in (dict(rotate_prob=1.5), dict(flip_prob=(0.5, -0.1, 0.5)), dict(noise_prob=math.nan), dict(zoom_prob=-1),
               dict(zoom_range=(1.1, 0.9)), dict(zoom_range=(0.0, 1.0)), dict(scale_intensity_range=(1.1, 0.9)),
               dict(shift_intensity_range=(0.1, -0.1)), dict(rotate_range=(0.1, -0.2, 0.1)), dict(translate_range=(8, 8)),
               dict(noise_std=-1.0), dict(out_dtype=torch.float16), dict(flip_prob=(0.5, 0.5))):
        with pytest.raises(ValueError):
            VolumeAugment((8, 8, 16), **kw)
    with pytest.raises(ValueError):
        VolumeAugment((8, 8))
    with pytest.raises(ValueError):
        VolumeAugment((8, 0, 16))
    aug = VolumeAugment((8, 8, 16))
    assert aug.training and aug.calls == 0 and aug.last_params is None and aug.call_index == 0
    with pytest.raises(RuntimeError, match="GPU"):
        aug(torch.zeros(2, 2, 9, 10, 11, dtype=torch.int16))                     # a CPU tensor
    with pytest.raises(RuntimeError, match="GPU"):
        aug.apply(torch.zeros(2, 2, 9, 10, 11), AugmentParams.identity(2, 2, (9, 10, 11), (8, 8, 16)))
    assert aug.calls == 0                                                        # nothing was drawn

    class FakeCuda(torch.Tensor):
        is_cuda = True

    for shape in ((2, 9, 10, 11), (2, 2, 2, 9, 10, 11), (9, 10, 11)):            # rank 4, a channel dimension of 2, rank 3
        with pytest.raises(ValueError, match="need"):
            aug(torch.zeros(shape).as_subclass(FakeCuda))
    with pytest.raises(TypeError, match="not supported"):
        aug(torch.zeros(2, 2, 9, 10, 11, dtype=torch.float64).as_subclass(FakeCuda))
    with pytest.raises(ValueError, match="contiguous"):
        aug(torch.zeros(2, 2, 9, 10, 22)[..., ::2].as_subclass(FakeCuda))
