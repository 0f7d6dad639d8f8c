"""CPU: the contrast stage without a GPU.  The two entry points are exported and bound; every argument error is refused on the host
before any launch, with its message (dummy aligned addresses that are never dereferenced); ContrastAugment refuses bad constructor
arguments, CPU tensors, other dtypes, non-contiguous input, wrong ranks and tables of the wrong shape, dtype or device; eval() hands its
input back; the record layout is the same in include/xvit.h, xvit.augment, xvit._lib and tests/_contrast_check.py."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import _contrast_check as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "xvit.h")).read()
P = 256   # any non-null, 16-byte aligned "address"


def _lib():
    from xvit import _lib
    return _lib, _lib.load()


def _config(**kw):
    from xvit import _lib
    c = _lib.ContrastConfig()
    c.blur_prob, c.bias_prob, c.gamma_prob, c.bias_coeff = 0.2, 0.2, 0.3, 0.3
    c.blur_sigma_range[:] = (0.5, 1.5)
    c.log_gamma_range[:] = (-0.3, 0.3)
    c.gamma_window[:] = (0.0, 1.0)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(c, k)[:] = v
        else:
            setattr(c, k, v)
    return c


def test_new_symbols_are_exported_and_bound():
    mod, lib = _lib()
    for name in ("xvit_contrast_draw", "xvit_contrast_apply"):
        assert name in mod.EXPORTS and name in mod.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(", HEADER)
    assert lib.xvit_version() >= 316


def test_config_struct_and_record_constants_match_the_header():
    from xvit import _lib, augment
    body = re.search(r"typedef struct xvit_contrast_config \{(.*?)\} xvit_contrast_config;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, decl in re.findall(r"(float|int)\s+([^;]+);", body):
        for item in decl.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            fields.append((m.group(1), int(m.group(2) or 1), ctype))
    kind = lambda t: "int" if (t._type_ if hasattr(t, "_length_") else t) is C.c_int32 else "float"   # noqa: E731
    got = [(n, getattr(t, "_length_", 1), kind(t)) for n, t in _lib.ContrastConfig._fields_]
    assert got == fields
    assert C.sizeof(_lib.ContrastConfig) == 4 * sum(n for _, n, _ in fields)
    enum = dict((k, int(v)) for k, v in re.findall(r"XVIT_CON_([A-Z_]+) = (\d+)", HEADER))
    assert int(re.search(r"#define XVIT_CON_NPARAM (\d+)", HEADER).group(1)) == augment.CON_NPARAM == _lib.CON_NPARAM == K.NPARAM == 32
    assert int(re.search(r"#define XVIT_CON_MAX_RADIUS (\d+)", HEADER).group(1)) == augment.CON_MAX_RADIUS == _lib.CON_MAX_RADIUS == K.MAX_RADIUS == 6
    for name in ("FLAGS", "SIGMA", "RADIUS", "GAMMA", "WINDOW_LO", "WINDOW_HI", "BIAS", "U_BLUR", "U_BIAS", "U_GAMMA", "BETA"):
        assert getattr(augment, "CON_" + name) == enum[name] == getattr(K, name), name
    for name, bit in (("FLAG_BLUR", 1), ("FLAG_BIAS", 2), ("FLAG_GAMMA", 4)):
        assert getattr(augment, "CON_" + name) == enum[name] == getattr(K, name) == bit
    assert augment.CON_BIAS_TERMS == ("z", "y", "x", "zz", "yy", "xx", "zy", "zx", "yx")
    src = open(os.path.join(ROOT, "cross-attention-vit_amd", "csrc", "contrast.hip")).read()
    assert re.search(r"constexpr int TX = (\d+), TY = (\d+);", src).groups() == (str(K.TX), str(K.TY))
    assert re.search(r"constexpr uint64_t kConSalt = 0x([0-9A-F]+)ull", src).group(1) == "%X" % K.SALT and "%X" % K.SALT in HEADER


def test_params_views_index_the_record_as_the_header_says():
    from xvit.augment import ContrastParams
    t = torch.arange(2 * 3 * 32, dtype=torch.float32).reshape(2, 3, 32)
    p = ContrastParams(t)
    row = t[1, 2]
    assert p.flags[1, 2] == row[0] and torch.equal(p.sigma[1, 2], row[1:4]) and torch.equal(p.radius[1, 2], row[4:7])
    assert p.gamma[1, 2] == row[7] and torch.equal(p.window[1, 2], row[8:10]) and torch.equal(p.bias[1, 2], row[10:19])
    assert torch.equal(p.draws[1, 2], row[19:22]) and p.beta[1, 2] == row[22]
    p.bias[0, 0, 8] = -7.0                # views: writing through them edits the table
    p.gamma[0, 1] = 2.5
    assert t[0, 0, 18] == -7.0 and t[0, 1, 7] == 2.5
    t[..., 0] = torch.tensor([[1.0, 0.0, 3.0], [2.0, 4.0, 7.0]])
    assert p.blurred.tolist() == [[True, False, True], [False, False, True]]
    assert p.biased.tolist() == [[False, False, True], [True, False, True]]
    assert p.gamma_on.tolist() == [[False, False, False], [False, True, True]]
    ident = ContrastParams.identity(2, 2, window=(-1.0, 3.0))
    assert (ident.flags == 0).all() and (ident.gamma == 1).all() and ident.window[1, 1].tolist() == [-1.0, 3.0] and (ident.table[..., 10:] == 0).all()
    assert p.clone().table is not t and torch.equal(p.clone().table, t)
    with pytest.raises(ValueError):
        ContrastParams(torch.zeros(2, 2, 31))
    with pytest.raises(ValueError):
        ContrastParams(torch.zeros(2, 2, 32, dtype=torch.float64))


def test_draw_argument_errors_do_not_launch():
    mod, lib = _lib()
    err = lib.xvit_last_error_string

    def draw(cfg=None, params=P, nvol=4, counter=None, advance=0, null_cfg=False):
        cfg = cfg if cfg is not None else _config()
        return lib.xvit_contrast_draw(None if null_cfg else C.byref(cfg), params, nvol, 0, counter, advance, None)

    assert draw(null_cfg=True) < 0 and b"xvit_contrast_draw" in err() and b"null" in err()
    assert draw(params=None) < 0 and b"null" in err()
    assert draw(nvol=0) < 0 and b"nvol=0" in err()
    assert draw(nvol=-3) < 0 and b"nvol=-3" in err()
    assert draw(params=P + 4) < 0 and b"16-byte aligned" in err()
    assert draw(counter=P + 4) < 0 and b"8-byte aligned" in err()
    assert draw(advance=1) < 0 and b"advance needs a counter" in err()
    for field in ("blur_prob", "bias_prob", "gamma_prob"):
        for bad in (-0.1, 1.5, math.nan):
            assert draw(_config(**{field: bad})) < 0 and b"probability" in err(), (field, bad)
    for bad in ((1.5, 0.5), (0.0, 1.0), (-0.5, 1.0), (0.5, 2.5), (math.nan, 1.0), (0.5, math.nan), (0.5, math.inf)):
        assert draw(_config(blur_sigma_range=bad)) < 0 and b"blur_sigma_range" in err(), bad
    for bad in (-0.1, math.nan, math.inf):
        assert draw(_config(bias_coeff=bad)) < 0 and b"bias_coeff" in err(), bad
    for bad in ((0.3, -0.3), (math.nan, 0.3), (-0.3, math.inf)):
        assert draw(_config(log_gamma_range=bad)) < 0 and b"log_gamma_range" in err(), bad
    for bad in ((1.0, 0.0), (0.5, 0.5), (math.nan, 1.0), (0.0, math.inf)):
        assert draw(_config(gamma_window=bad)) < 0 and b"gamma_window" in err(), bad


def test_apply_argument_errors_do_not_launch():
    mod, lib = _lib()
    err = lib.xvit_last_error_string

    def apply(src=P, dst=2 * P, sdt=0, ddt=0, params=P, nvol=4, d=(8, 8, 16)):
        return lib.xvit_contrast_apply(src, dst, sdt, ddt, params, nvol, *d, None)

    assert apply(src=None) < 0 and b"xvit_contrast_apply" in err() and b"null" in err()
    assert apply(dst=None) < 0 and b"null" in err()
    assert apply(params=None) < 0 and b"null" in err()
    assert apply(sdt=2) < 0 and b"unknown source dtype 2" in err()              # int16 volumes belong to the stage in front
    assert apply(sdt=-1) < 0 and b"unknown source dtype" in err()
    assert apply(ddt=3) < 0 and b"unknown destination dtype 3" in err()
    assert apply(nvol=0) < 0 and b"non-positive size" in err()
    for d in ((0, 8, 16), (8, -1, 16), (8, 8, 0)):
        assert apply(d=d) < 0 and b"non-positive size" in err(), d
    assert apply(d=(2048, 1024, 1024)) < 0 and b"2^31" in err()                  # exactly 2^31 voxels
    assert apply(src=P + 8) < 0 and b"16-byte aligned" in err()
    assert apply(dst=2 * P + 2) < 0 and b"16-byte aligned" in err()
    assert apply(params=P + 4) < 0 and b"16-byte aligned" in err()
    assert apply(dst=P) < 0 and b"out of place" in err()


def test_contrast_augment_refuses_bad_arguments():
    from xvit.augment import ContrastAugment, ContrastParams
    for kw in (dict(blur_prob=1.5), dict(bias_prob=-0.1), dict(gamma_prob=math.nan), dict(blur_sigma_range=(1.5, 0.5)), dict(blur_sigma_range=(0.0, 1.0)),
               dict(blur_sigma_range=(0.5, 2.01)), dict(blur_sigma_range=(0.5,)), dict(bias_coeff=-0.3), dict(bias_coeff=math.inf), dict(bias_coeff=math.nan),
               dict(gamma_window=(1.0, 0.0)), dict(gamma_window=(0.5, 0.5)), dict(gamma_window=(0.0, math.inf)), dict(gamma_window=(math.nan, 1.0)),
               dict(log_gamma_range=(0.3, -0.3)), dict(log_gamma_range=(-math.inf, 0.3)), dict(log_gamma_range=(math.nan, 0.3)),
               dict(out_dtype=torch.float16)):
        with pytest.raises(ValueError, match="ContrastAugment"):
            ContrastAugment(**kw)
    ContrastAugment(blur_sigma_range=(2.0, 2.0), bias_coeff=0.0, log_gamma_range=(0.0, 0.0), blur_prob=0, gamma_prob=1)    # the edges are legal
    con = ContrastAugment()
    assert isinstance(con, torch.nn.Module) and con.training and con.calls == 0 and con.call_index == 0 and con.last_params is None
    assert abs(con.config.blur_prob - 0.2) < 1e-7 and con.config.blur_isotropic == 0 and tuple(con.config.gamma_window) == (0.0, 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        con(torch.zeros(2, 2, 8, 8, 16))                                         # a CPU tensor
    with pytest.raises(RuntimeError, match="GPU"):
        con.apply(torch.zeros(2, 2, 8, 8, 16), ContrastParams.identity(2, 2))

    class FakeCuda(torch.Tensor):
        is_cuda = True

    fake = lambda *shape, **kw: torch.zeros(*shape, **kw).as_subclass(FakeCuda)   # noqa: E731
    for shape in ((2, 8, 8, 16), (2, 2, 2, 8, 8, 16), (8, 8, 16), (2, 2, 1, 1, 8, 8, 16)):   # rank 4, a channel dimension of 2, rank 3, rank 7
        with pytest.raises(ValueError, match="need"):
            con(fake(*shape))
    for dt in (torch.int16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="not supported"):
            con(fake(2, 2, 8, 8, 16, dtype=dt))
    with pytest.raises(ValueError, match="contiguous"):
        con(torch.zeros(2, 2, 8, 8, 32)[..., ::2].as_subclass(FakeCuda))
    with pytest.raises(RuntimeError, match="no backward"):
        con(torch.zeros(2, 2, 8, 8, 16, requires_grad=True).as_subclass(FakeCuda))
    for bad in (torch.zeros(2, 2, 31), torch.zeros(2, 3, 32), torch.zeros(4, 32), torch.zeros(2, 2, 32, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="table"):
            con.apply(fake(2, 2, 8, 8, 16), bad)
    with pytest.raises(ValueError, match="table is on"):
        con.apply(fake(2, 2, 8, 8, 16), torch.zeros(2, 2, 32, device="meta"))
    assert con.calls == 0 and con.last_params is None                            # nothing was drawn


def test_eval_returns_its_input():
    from xvit.augment import ContrastAugment
    con = ContrastAugment(seed=3).eval()
    x = torch.zeros(2, 2, 1, 4, 4, 8)                                            # even a CPU tensor: nothing is looked at, nothing is launched
    assert con(x) is x and con.calls == 0 and con.call_index == 0 and con.last_params is None
    seq = torch.nn.Sequential(torch.nn.Identity(), con).eval()
    assert seq(x) is x


def test_capturable_stage_allocates_nothing_inside_a_capture(monkeypatch):
    """A first call inside a capture is refused with VolumeAugment's message: the table and the counter must exist before the graph."""
    from xvit.augment import ContrastAugment
    con = ContrastAugment(capturable=True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="call the stage once on this batch shape before capturing it"):
        con._table(2, 2, torch.device("cpu"))
    assert not con._tables and con._counter is None
