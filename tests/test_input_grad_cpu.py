"""CPU: host-side refusals of xvit_patch_embed_dgrad / xvit_unpatchify (no launch: callable without a GPU), the geometries the fused
input gradient accepts, and the refusals of xvit.interpret.input_attributions that come before any GPU work."""
import ctypes as C

import pytest
import torch

import ref_cpu as R


def _geom(B=2, M=2, vol=(128, 128, 128), patch=(16, 16, 16), cls_rows=1):
    from xvit import _lib
    g = _lib.PatchGeom()
    g.B, g.M, (g.D, g.H, g.W), (g.dp, g.hp, g.wp), g.cls_rows = B, M, vol, patch, cls_rows
    return g


def _dgrad(lib, dx=64, lddx=768, w=64, ldw=4096, g=None, d=768, out=64, dtype=1):
    return lib.xvit_patch_embed_dgrad(dx, lddx, w, ldw, C.byref(g if g is not None else _geom()), d, out, dtype, None)


def test_dgrad_argument_errors_do_not_launch():
    """Dummy non-null addresses (never dereferenced): each call is refused on the host, with its reason."""
    from xvit import _lib
    lib = _lib.load()
    err = lambda: lib.xvit_last_error_string()   # noqa: E731
    for arg in ("dx", "w", "out"):
        assert _dgrad(lib, **{arg: None}) < 0 and b"null pointer" in err(), (arg, err())
    assert _dgrad(lib, dtype=7) < 0 and b"bad output dtype" in err(), err()
    assert _dgrad(lib, lddx=760) < 0 and b"leading dimension" in err(), err()          # < d
    assert _dgrad(lib, lddx=772) < 0 and b"leading dimension" in err(), err()          # not a multiple of 8
    assert _dgrad(lib, ldw=4092) < 0 and b"leading dimension" in err(), err()
    assert _dgrad(lib, dx=72) < 0 and b"16-byte aligned" in err(), err()
    assert _dgrad(lib, out=72) < 0 and b"16-byte aligned" in err(), err()
    for bad in (dict(g=_geom(patch=(16, 16, 4))), dict(g=_geom(B=1, M=1)), dict(d=96), dict(g=_geom(vol=(128, 128, 120)))):
        assert _dgrad(lib, **bad) < 0 and b"not supported" in err(), (bad, err())


def test_unpatchify_argument_errors_do_not_launch():
    from xvit import _lib
    lib = _lib.load()
    err = lambda: lib.xvit_last_error_string()   # noqa: E731

    def call(p=64, img=64, dt=1, B=2, M=2, D=32, H=32, W=16, dp=8, hp=8, wp=8, sb=65, sm=130, off=1):
        return lib.xvit_unpatchify(p, img, dt, B, M, D, H, W, dp, hp, wp, sb, sm, off, None)
    assert call(p=None) < 0 and b"null pointer" in err()
    assert call(img=None) < 0 and b"null pointer" in err()
    assert call(dt=5) < 0 and b"bad dtype" in err()
    assert call(B=0) < 0 and b"bad sizes" in err()
    assert call(wp=0) < 0 and b"bad sizes" in err()
    assert call(W=20) < 0 and b"divisible" in err()
    assert call(sb=0) < 0 and b"placement" in err()
    assert call(off=-1) < 0 and b"placement" in err()


GEOMS = [(2, 2, (128, 128, 128), (16, 16, 16), 768), (1, 4, (240, 240, 240), (16, 16, 16), 768), (2, 3, (128, 128, 64), (16, 16, 8), 1024),
         (126, 2, (128, 128, 128), (16, 16, 16), 768), (1, 1, (128, 128, 128), (8, 8, 8), 256), (3, 2, (128, 64, 128), (16, 8, 16), 512),
         (20, 1, (80, 48, 112), (16, 16, 16), 256), (2, 3, (96, 160, 48), (8, 16, 16), 512), (2, 2, (32, 32, 2), (8, 8, 2), 192),
         (4, 1, (64, 64, 64), (4, 4, 4), 256), (8, 2, (128, 128, 128), (16, 16, 16), 768)]


def test_dgrad_accepts_every_forward_geometry():
    """xvit_patch_embed_dgrad_supported is a superset of xvit_patch_embed_supported; configs[1] (B = 8 and 126), configs[2] and mist
    take the fused input gradient."""
    from xvit import _lib
    lib = _lib.load()
    for B, M, vol, patch, d in GEOMS:
        g = _geom(B, M, vol, patch)
        fwd, dg = lib.xvit_patch_embed_supported(C.byref(g), d), lib.xvit_patch_embed_dgrad_supported(C.byref(g), d)
        assert dg >= fwd, (B, M, vol, patch, d)
    for B, M, vol, patch, d in GEOMS[:4] + GEOMS[-1:]:
        assert lib.xvit_patch_embed_dgrad_supported(C.byref(_geom(B, M, vol, patch)), d) == 1
    assert lib.xvit_patch_embed_dgrad_supported(C.byref(_geom(2, 2, (32, 32, 2), (8, 8, 2))), 192) == 0      # runs of 2 voxels
    assert lib.xvit_patch_embed_dgrad_supported(None, 768) == 0


def test_ctypes_rows():
    from xvit import _lib
    lib = _lib.load()
    assert len(lib.xvit_patch_embed_dgrad.argtypes) == 9 and len(lib.xvit_unpatchify.argtypes) == 15
    assert lib.xvit_patch_embed_dgrad_supported.restype is C.c_int


def _restored():
    import xvit.functional as XF
    from xvit.cross_vit import STREAM_MODE
    return XF.GRAD_SINK is None and XF.ATTN_RECORDER.get() is None and STREAM_MODE.get() is None


def test_input_attributions_refusals(monkeypatch):
    import xvit
    cfg = R.make_config("tiny")
    model = xvit.ModelCross(cfg).eval()
    img, _ = R.make_inputs(cfg, 2, seed=0)
    ia = xvit.interpret.input_attributions
    with pytest.raises(RuntimeError, match="input_attributions: model and img must be on the GPU"):
        ia(model, img)
    with pytest.raises(TypeError, match="need a ModelCross or a ModelVIT"):
        ia(torch.nn.Linear(2, 2), img)
    with pytest.raises(ValueError, match="target must be an int or an int64 tensor"):
        ia(model, img, target=torch.tensor([0, 1, 1]))
    for bad in (torch.tensor([0.0, 1.7]), 1.5, torch.tensor([True, False])):
        with pytest.raises(ValueError, match="integer tensor"):
            ia(model, img, target=bad)
    for bad in (-1, torch.tensor([0, -4])):
        with pytest.raises(ValueError, match="negative class"):
            ia(model, img, target=bad)
    with pytest.raises(ValueError, match="baseline must be"):
        ia(model, img, baseline=torch.zeros(3, *img.shape[1:]))
    with pytest.raises(ValueError, match="baseline must be"):
        ia(model, img, baseline=torch.zeros(1, 1, 1, *img.shape[3:]))
    for steps in (0, -2):
        with pytest.raises(ValueError, match="steps and batch_size must be >= 1"):
            ia(model, img, steps=steps)
    with pytest.raises(ValueError, match="steps and batch_size must be >= 1"):
        ia(model, img, batch_size=0)
    with pytest.raises(ValueError, match="method must be one of"):
        ia(model, img, method="smoothgrad")
    with pytest.raises(ValueError, match="img must be"):
        ia(model, img[:, :, 0])
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        ia(model, img)
    model.eval()
    monkeypatch.setenv("XVIT_ATTN_FP8", "1")
    with pytest.raises(RuntimeError, match="XVIT_ATTN_FP8"):
        ia(model, img)
    assert _restored()
