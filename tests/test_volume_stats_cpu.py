"""CPU: per-volume intensity statistics without a GPU.  The entry points are exported and bound, the config struct and the constants match
include/xvit.h, every argument error is refused on the host before any launch, with its message (dummy aligned addresses that are never
dereferenced), and xvit.augment validates its normalisation arguments."""
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


def _config(mode=1, clip=1, fg=0.0, q=(0.005, 0.995)):
    from xvit import _lib
    c = _lib.NormConfig()
    c.mode, c.clip, c.foreground_above, (c.q_lo, c.q_hi) = mode, clip, fg, q
    return c


def test_new_symbols_are_exported_and_bound():
    mod, lib = _lib()
    for name in ("xvit_volume_stats", "xvit_volume_stats_workspace_bytes"):
        assert name in mod.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b(int|int64_t) " + name + r"\(", HEADER)
    assert "xvit_volume_stats" in mod.SIGNATURES and len(mod.SIGNATURES["xvit_volume_stats"]) == 10
    assert lib.xvit_version() >= 310
    from xvit import ops
    assert callable(ops.volume_stats) and callable(ops.volume_stats_workspace)


def test_config_struct_and_constants_match_the_header():
    from xvit import _lib, augment
    body = re.search(r"typedef struct xvit_norm_config \{(.*?)\} xvit_norm_config;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, decl in re.findall(r"(int|float)\s+([^;]+);", body):
        fields += [(name.strip(), ctype) for name in decl.split(",")]
    assert [(n, "int" if t is C.c_int32 else "float") for n, t in _lib.NormConfig._fields_] == fields
    assert C.sizeof(_lib.NormConfig) == 4 * len(fields) == 20
    enum = dict((k, int(v)) for k, v in re.findall(r"XVIT_(AUG_[A-Z_]+|STATS_[A-Z_]+|NORM_[A-Z_]+) = (\d+)", HEADER))
    assert enum["AUG_CLAMP_LO"] == augment.CLAMP_LO == 29 and enum["AUG_CLAMP_HI"] == augment.CLAMP_HI == 30
    assert enum["AUG_FLAG_CLAMP"] == augment.FLAG_CLAMP == 2 and enum["AUG_FLAG_EXACT"] == augment.FLAG_EXACT == 1
    assert (enum["STATS_WINDOW_LO"], enum["STATS_WINDOW_BINS"]) == (_lib.STATS_WINDOW_LO, _lib.STATS_WINDOW_BINS)
    assert 0 <= _lib.STATS_WINDOW_LO and _lib.STATS_WINDOW_LO + _lib.STATS_WINDOW_BINS <= 65536
    assert (enum["NORM_STATS_ONLY"], enum["NORM_ZSCORE"], enum["NORM_WINDOW"]) == (_lib.NORM_STATS_ONLY, _lib.NORM_ZSCORE, _lib.NORM_WINDOW) == (0, 1, 2)
    assert int(re.search(r"#define XVIT_STATS_NSTAT (\d+)", HEADER).group(1)) == _lib.STATS_NSTAT == augment.NSTAT == 8
    assert "reads slots 0..16 only" not in HEADER


def test_workspace_size():
    _, lib = _lib()
    ws = lib.xvit_volume_stats_workspace_bytes
    assert ws(1) == 65536 * 4 and ws(16) == 16 * 65536 * 4 and ws(0) == 0 and ws(-3) == 0
    assert ws(1 << 14) == (1 << 14) * 65536 * 4 > 1 << 31                       # 64-bit


def test_argument_errors_do_not_launch():
    _, lib = _lib()
    err = lib.xvit_last_error_string
    need = lib.xvit_volume_stats_workspace_bytes(4)

    def stats(src=P, sdt=2, nvol=4, nvox=1000, cfg=None, out=P, params=None, ws=P, ws_bytes=need, null_cfg=False):
        cfg = cfg if cfg is not None else _config()
        return lib.xvit_volume_stats(src, sdt, nvol, nvox, None if null_cfg else C.byref(cfg), out, params, ws, ws_bytes, None)

    assert stats(src=None) < 0 and b"xvit_volume_stats" in err() and b"null" in err()
    assert stats(null_cfg=True) < 0 and b"null" in err()
    assert stats(out=None) < 0 and b"null" in err()
    assert stats(ws=None) < 0 and b"null" in err()
    assert stats(sdt=1) < 0 and b"fp32 sources are not supported" in err() and b"cast to bf16 or normalise beforehand" in err()
    assert stats(sdt=3) < 0 and b"unknown source dtype 3" in err()
    assert stats(nvol=0) < 0 and b"nvol=0" in err()
    assert stats(nvol=-2) < 0 and b"nvol=-2" in err()
    assert stats(nvox=0) < 0 and b"nvox=0" in err()
    assert stats(nvox=1 << 31) < 0 and b"2^31" in err()
    assert stats(cfg=_config(mode=3)) < 0 and b"unknown mode 3" in err()
    assert stats(cfg=_config(fg=math.nan)) < 0 and b"NaN" in err()
    assert stats(cfg=_config(q=(0.9, 0.1))) < 0 and b"percentiles" in err()      # q_lo > q_hi
    assert stats(cfg=_config(q=(0.5, 1.5))) < 0 and b"percentiles" in err()      # q > 1
    assert stats(cfg=_config(q=(math.nan, 0.5))) < 0 and b"percentiles" in err()
    assert stats(cfg=_config(q=(0.5, math.nan))) < 0 and b"percentiles" in err()
    assert stats(ws_bytes=need - 1) < 0 and b"workspace" in err() and str(need).encode() in err()
    assert stats(out=P + 4) < 0 and b"stats must be 8-byte aligned" in err()
    assert stats(src=P + 1) < 0 and b"element size" in err()
    assert stats(params=P + 8) < 0 and b"16-byte aligned" in err()
    assert stats(ws=P + 8) < 0 and b"workspace must be 16-byte aligned" in err()


def test_python_argument_validation():
    from xvit.augment import VolumeAugment, VolumeStats, norm_config, volume_stats
    for kw in (dict(normalize="minmax"), dict(normalize="zscore", percentiles=(0.9, 0.1)), dict(normalize="window", percentiles=(0.1, 1.5)),
               dict(normalize="window", percentiles=(-0.1, 0.5)), dict(normalize="zscore", percentiles=(0.5,)), dict(normalize="zscore", foreground_above=math.nan)):
        with pytest.raises(ValueError, match="VolumeAugment"):
            VolumeAugment((8, 8, 16), **kw)
    aug = VolumeAugment((8, 8, 16))
    assert aug.normalize is None and aug.last_stats is None and aug.norm_config.mode == 0
    aug = VolumeAugment((8, 8, 16), normalize="window", foreground_above=-math.inf, percentiles=None, clip=False)
    c = aug.norm_config
    assert (c.mode, c.clip, c.foreground_above, c.q_lo < 0) == (2, 0, -math.inf, True)
    c = VolumeAugment((8, 8, 16), normalize="zscore").norm_config
    assert (c.mode, c.clip, c.foreground_above) == (1, 1, 0.0) and (c.q_lo, c.q_hi) == (C.c_float(0.005).value, C.c_float(0.995).value)
    assert norm_config().mode == 0 and norm_config().q_lo < 0
    with pytest.raises(RuntimeError, match="GPU"):
        volume_stats(torch.zeros(2, 2, 4, 4, 4, dtype=torch.int16))                        # a CPU tensor
    with pytest.raises(RuntimeError, match="GPU"):
        VolumeAugment((8, 8, 16), normalize="zscore")(torch.zeros(2, 2, 9, 10, 11, dtype=torch.int16))

    class FakeCuda(torch.Tensor):
        is_cuda = True

    with pytest.raises(ValueError, match="need"):
        volume_stats(torch.zeros(4, 4, dtype=torch.int16).as_subclass(FakeCuda))
    with pytest.raises(ValueError, match="contiguous"):
        volume_stats(torch.zeros(2, 2, 4, 8, dtype=torch.int16)[..., ::2].as_subclass(FakeCuda))
    with pytest.raises(ValueError, match="percentiles"):
        volume_stats(torch.zeros(2, 2, 4, dtype=torch.int16).as_subclass(FakeCuda), percentiles=(0.6, 0.4))
    t = torch.arange(2 * 3 * 8, dtype=torch.float64).reshape(2, 3, 8)
    s = VolumeStats(t)
    row = t[1, 2]
    assert [float(v[1, 2]) for v in (s.n, s.n_w, s.mean, s.std, s.lo, s.hi, s.min, s.max)] == row.tolist()
    with pytest.raises(ValueError):
        VolumeStats(torch.zeros(2, 3, 8))
    with pytest.raises(ValueError):
        VolumeStats(torch.zeros(2, 3, 7, dtype=torch.float64))


def test_capturable_stage_allocates_nothing_inside_a_capture(monkeypatch):
    """The statistics buffers are allocated in the same pre-capture call as the table and the counter, and a first call inside a capture
    is refused with the same error."""
    from xvit.augment import VolumeAugment
    aug = VolumeAugment((8, 8, 16), normalize="zscore", capturable=True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before capturing"):
        aug._table(2, 2, torch.device("cpu"))
    assert not aug._tables and not aug._stats and not aug._workspaces and aug._counter is None
