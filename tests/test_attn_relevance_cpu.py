"""CPU: host-side refusals of xvit_attn_relevance_step (no launch: callable without a GPU), and those of xvit.interpret.relevance_maps
that come before any GPU work."""
import pytest
import torch

import ref_cpu as R


def _step(lib, q=64, k=64, v=64, sb=3 * 768 * 513, sn=3 * 768, lse=64, do=64, sbo=768 * 513, sno=768, r_in=4096, r_out=1 << 20,
          B=2, H=12, N=513, dh=64):
    return lib.xvit_attn_relevance_step(q, k, v, sb, sn, lse, do, sbo, sno, r_in, r_out, B, H, N, dh, 0.125, None)


def test_relevance_step_argument_errors_do_not_launch():
    """Dummy non-null addresses (never dereferenced): each call is refused on the host, with its reason."""
    from xvit import _lib
    lib = _lib.load()
    err = lambda: lib.xvit_last_error_string()   # noqa: E731
    for dh in (32, 128):
        assert _step(lib, dh=dh) < 0
        assert b"xvit_attn_relevance_step" in err() and b"head dim %d unsupported (only 64)" % dh in err(), err()
    for arg in ("q", "k", "v", "lse", "do", "r_in", "r_out"):
        assert _step(lib, **{arg: None}) < 0 and b"null pointer" in err(), (arg, err())
    assert _step(lib, r_in=4096, r_out=4096) < 0 and b"alias" in err(), err()
    assert _step(lib, r_in=4096, r_out=4096 + 4 * 513) < 0 and b"alias" in err(), err()     # overlapping [B, N] ranges
    for bad in (dict(sn=3 * 768 + 4), dict(sb=3 * 768 * 513 + 2), dict(sno=768 + 4), dict(sbo=768 * 513 + 2)):
        assert _step(lib, **bad) < 0 and b"multiples of 8" in err(), (bad, err())
    for bad in (dict(B=0), dict(H=0), dict(N=0), dict(B=-1)):
        assert _step(lib, **bad) < 0 and b"bad B/H/N" in err(), (bad, err())


def test_relevance_maps_refuses_cpu_tensors_and_other_models():
    import xvit
    import xvit.functional as XF
    from xvit.cross_vit import STREAM_MODE
    cfg = R.make_config("tiny")
    model = xvit.ModelCross(cfg).eval()
    img, _ = R.make_inputs(cfg, 2, seed=0)
    with pytest.raises(RuntimeError, match="relevance_maps: model and img must be on the GPU"):
        xvit.interpret.relevance_maps(model, img)
    with pytest.raises(TypeError, match="relevance_maps: need a ModelCross or a ModelVIT"):
        xvit.interpret.relevance_maps(torch.nn.Linear(2, 2), img)
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        xvit.interpret.relevance_maps(model, img)
    assert XF.GRAD_SINK is None and XF.ATTN_RECORDER.get() is None and STREAM_MODE.get() is None
