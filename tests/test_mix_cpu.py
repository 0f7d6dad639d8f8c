"""CPU: the host side of Mixup / CutMix — the argument refusals of the C entry points (nothing is launched), the record layout, and the
model's attributes at the config's defaults."""
import re

import pytest
import torch

import ref_cpu as R
import _mix_check as K


def test_record_layout_matches_the_header():
    import os
    from xvit import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xvit.h")).read()
    macro = lambda n: int(re.search(rf"#define XVIT_MIX_{n} (\d+)", header).group(1))   # noqa: E731
    names = ("NPARAM", "MODE", "PARTNER", "LAM", "OML", "BOX", "LAM0", "MODE_MIXUP", "MODE_CUTMIX", "DRAW_STRIDE")
    assert [macro(n) for n in names] == [16, 0, 1, 2, 3, 4, 10, 1, 2, 256]
    assert [getattr(_lib, "MIX_" + n) for n in names] == [macro(n) for n in names]
    assert (K.NPARAM, K.MODE, K.PARTNER, K.LAM, K.OML, K.BOX, K.LAM0, K.MIXUP, K.CUTMIX, K.STRIDE) == tuple(macro(n) for n in names)
    assert [f[0] for f in _lib.MixConfig._fields_] == ["mixup_alpha", "cutmix_alpha", "prob", "switch_prob", "per_sample"]
    import ctypes
    assert ctypes.sizeof(_lib.MixConfig) == 20
    rec = K.record(K.CUTMIX, 3, 0.75, box=(1, 2, 3, 4, 5, 6), lam0=0.4)
    assert rec.tolist() == [2, 3, 0.75, 0.25, 1, 2, 3, 4, 5, 6, pytest.approx(0.4), 0, 0, 0, 0, 0]


def test_argument_refusals_do_not_launch():
    """Dummy non-null, aligned addresses; nothing is dereferenced because nothing is launched."""
    import ctypes as C
    from xvit import _lib
    lib = _lib.load()
    A = 4096
    err = lib.xvit_last_error_string
    cfg = lambda *v: C.byref(_lib.MixConfig(*v))   # noqa: E731
    draw = lambda c, table=A, B=4, vol=(8, 8, 8): lib.xvit_mix_draw(c, table, B, *vol, 1, None)   # noqa: E731
    assert draw(cfg(-0.1, 1.0, 1.0, 0.5, 0)) < 0 and b"xvit_mix_draw" in err() and b"alpha" in err()
    assert draw(cfg(1.0, float("nan"), 1.0, 0.5, 0)) < 0 and draw(cfg(float("inf"), 0.0, 1.0, 0.5, 0)) < 0
    assert draw(cfg(1.0, 1.0, 1.5, 0.5, 0)) < 0 and b"[0, 1]" in err()
    assert draw(cfg(1.0, 1.0, 1.0, -0.5, 0)) < 0 and draw(cfg(1.0, 1.0, float("nan"), 0.5, 0)) < 0
    assert draw(None) < 0 and draw(cfg(1.0, 1.0, 1.0, 0.5, 0), table=None) < 0 and b"null" in err()
    assert draw(cfg(1.0, 1.0, 1.0, 0.5, 0), table=A + 4) < 0 and b"aligned" in err()
    assert draw(cfg(1.0, 1.0, 1.0, 0.5, 0), B=0) < 0 and draw(cfg(1.0, 1.0, 1.0, 0.5, 0), vol=(0, 8, 8)) < 0
    assert draw(cfg(1.0, 1.0, 1.0, 0.5, 0), vol=(2048, 1024, 1024)) < 0 and b"2^31" in err()

    n = 8 * 8 * 8
    apply = lambda src, dst, dtype=0, B=2, M=2, sb=2 * n, sm=n, table=A: lib.xvit_mix_apply(src, dst, dtype, table, B, M, 8, 8, 8, sb, sm, None)   # noqa: E731
    big = 1 << 20
    assert apply(big, big) < 0 and b"xvit_mix_apply" in err() and b"aliases" in err()          # in place
    assert apply(big, big + 2 * (4 * n - 1)) < 0 and b"aliases" in err()                       # dst starts inside the last source voxel's element
    assert apply(big + 2 * (4 * n - 1), big) < 0 and b"aliases" in err()                       # src starts inside dst
    assert apply(big, big + 64, sb=8 * n) < 0 and b"aliases" in err()                          # dst inside the gap of a batch-strided source still overlaps its range
    assert apply(None, big) < 0 and apply(big, None) < 0 and apply(big, 2 * big, table=None) < 0 and b"null" in err()
    assert apply(big, 2 * big, dtype=2) < 0 and b"dtype" in err()
    assert apply(big, 2 * big, B=0) < 0 and apply(big, 2 * big, sb=0) < 0 and apply(big, 2 * big, sm=-1) < 0
    assert apply(big + 1, 2 * big) < 0 and b"aligned" in err()

    ce = lambda table: lib.xvit_mean_ce_mix(A, A, table, 0.1, A, A, A, 2, 4, 3, None)   # noqa: E731
    assert ce(None) < 0 and b"xvit_mean_ce_mix" in err() and b"null record table" in err()
    assert lib.xvit_mean_ce_mix(None, A, A, 0.1, A, A, A, 2, 4, 3, None) < 0 and lib.xvit_mean_ce_mix(A, A, A, 0.1, A, A, A, 2, 0, 3, None) < 0


def test_wrappers_refuse_before_the_library():
    """The tensor-level checks of xvit.ops / xvit.functional that need no GPU: a wrong table, an aliasing `out`, a volume that requires grad."""
    from xvit import ops
    import xvit.functional as XF
    img = torch.zeros(2, 2, 1, 4, 4, 8)
    with pytest.raises(RuntimeError, match="record table"):
        ops.mix_apply(img, torch.zeros(2, 8))
    with pytest.raises(RuntimeError, match="record table"):
        ops.mix_apply(img, torch.zeros(3, 16))
    with pytest.raises(RuntimeError, match="record table"):
        ops.mean_ce_mix(torch.zeros(2, 2, 3), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 16, dtype=torch.float64), 0.0)
    with pytest.raises(RuntimeError, match="record table is required"):
        ops.mean_ce_mix(torch.zeros(2, 2, 3), torch.zeros(2, dtype=torch.int64), None, 0.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.mix_apply(img.transpose(4, 5), torch.zeros(2, 16))
    with pytest.raises(RuntimeError, match="not on the GPU"):          # no CPU fallback behind the checks
        ops.mix_apply(img, torch.zeros(2, 16))
    with pytest.raises(RuntimeError, match="mixing"):
        XF.mix_volumes(img.clone().requires_grad_(), torch.zeros(2, 16))


def test_model_attributes():
    """A config without the new fields constructs as before and holds no table; bad fields are refused; a positive alpha switches the
    captured step's device epoch on."""
    import xvit
    from xvit.graph import _has_dropout
    cfg = R.make_config("tiny")
    assert not hasattr(cfg, "mixup_alpha")
    plain = xvit.ModelCross(cfg)
    assert (plain.mixup_alpha, plain.cutmix_alpha, plain.mix_prob, plain.mix_switch_prob, plain.mix_per_sample) == (0.0, 0.0, 1.0, 0.5, False)
    assert plain.last_mix is None and not _has_dropout(plain)
    model = xvit.ModelCross(R.make_config("tiny", mixup_alpha=0.8, cutmix_alpha=1.0, mix_prob=0.9, mix_switch_prob=0.25, mix_per_sample=True))
    assert (model.mixup_alpha, model.cutmix_alpha, model.mix_prob, model.mix_switch_prob, model.mix_per_sample) == (0.8, 1.0, 0.9, 0.25, True)
    assert model.last_mix is None and set(model.state_dict()) == set(plain.state_dict())
    assert _has_dropout(model) and _has_dropout(xvit.ModelCross(R.make_config("tiny", cutmix_alpha=1.0)))
    for bad in (dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1.0), dict(mixup_alpha=float("nan")), dict(cutmix_alpha=float("inf")), dict(mixup_alpha=1.0, mix_prob=1.5),
                dict(mixup_alpha=1.0, mix_switch_prob=-0.1), dict(mix_prob=float("nan"))):
        with pytest.raises(ValueError):
            xvit.ModelCross(R.make_config("tiny", **bad))
