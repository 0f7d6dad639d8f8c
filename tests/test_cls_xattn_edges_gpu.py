"""GPU: xvit_cls_xattn_fwd and xvit_cls_xattn_bwd (csrc/cls_xattn.hip) element by element, through the C entry points with every stride free, under
the gate of tests/_xattn_check.py: bit for bit where the arithmetic is exact, against float64 under derived bounds where it is not, sentinels around
every destination (between the halves of dk | dv, behind row N - 1, behind column 2 d, in front of and behind p and coef) and NaN behind every input.
The shapes are the smallest that reach each edge of the launch geometry (see _xattn_check's docstring); tests/test_xattn_gate_cpu.py shows on the
CPU that the gate names planted faults.  The rel-L2 tests of the same kernels (tests/test_cls_xattn_gpu.py, tests/test_kernels_gpu.py,
tests/test_dropout_gpu.py) stay as they are."""
import pytest
import torch

import _xattn_check as X
from _cls_check import SENT, check_all_sentinel, device_keep

pytestmark = pytest.mark.gpu

RANDOM_DROP = (0.25, 7)         # the float64 tier's dropout: 1 / (1 - p) is no power of two


def _both_tiers(c, kind2=None, exact=True):
    for on in (False, True):
        if exact:
            p, seed = X.DROP if on else (0.0, 0)
            e = X.with_(c, p=p, seed=seed, tier="exact")
            X.fwd_run(e, X.exact_operands_fwd(e))
            ob = X.exact_operands_bwd(e)
            X.bwd_run(e, ob, ob["p"])
        p, seed = RANDOM_DROP if on else (0.0, 0)
        for kind in ("random",) + ((kind2,) if kind2 else ()):
            r = X.with_(c, p=p, seed=seed, tier="random", kind=kind)
            o, log = X.random_operands(r), f"xattn:{kind}:drop{p:g}"
            saved = X.fwd_run(r, o, log=log)
            X.fwd_run(r, o, qsel="bf16", variants=False, log=log + ":bf16q")
            X.bwd_run(r, o, saved, log=log)                          # on the forward's own p, as the fusion runs it


@pytest.mark.parametrize("N", X.NS)
def test_cls_xattn_every_sequence_length(N):
    """Fewer rows than slices, one pass, one pass plus a row, the 256 block of the softmax loops and both sides of it, two full softmax passes, a long
    row; layouts, batch sizes and a second content (x 15, equal, dominant) rotate."""
    _both_tiers(*X.n_cases(N))


@pytest.mark.parametrize("k", range(len(X.layout_cases())), ids=lambda k: "{0.layout}-N{0.N}-H{0.H}".format(X.layout_cases()[k]))
def test_cls_xattn_every_layout(k):
    """(a) fusion, (b) the interpret path's qkv thirds, (c) every stride padded, (d) k and v in separate buffers; below and above 16 heads."""
    _both_tiers(X.layout_cases()[k])


@pytest.mark.parametrize("k", range(len(X.HS)), ids=lambda k: f"H{X.HS[k]}")
def test_cls_xattn_every_head_count(k):
    _both_tiers(X.h_cases()[k])


def test_cls_xattn_raised_lds_limit():
    """N = 16385: 72 KiB of dynamic LDS, above what a kernel may ask for without opting in."""
    assert X.xa_lds(14332) <= 64 * 1024 < X.xa_lds(14333) <= X.xa_lds(16385)
    _both_tiers(X.lds_case(), exact=False)


def test_hash_keep_is_the_kernels_mask():
    c = X.with_(X.case(2, 3, 65), p=0.25, seed=7)
    assert torch.equal(X.keep_mask(c), device_keep(c.B * c.H, c.N, c.p, c.seed).reshape(c.B, c.H, c.N))


def _sentinel_windows(w):
    for v in w.values():
        for t in v if isinstance(v, list) else [v]:
            t.fill_(SENT)
    return w


def _all_sentinel(name, w):
    for k, v in w.items():
        for t in v if isinstance(v, list) else [v]:
            check_all_sentinel(f"{name}: {k}", t.reshape(1, -1) if t.dim() == 1 else t)


def test_cls_xattn_refusals():
    """Every argument error is answered on the host, with the entry point's name, and nothing is written."""
    assert X.xa_lds(X.XA_MAX_N) <= 160 * 1024 < X.xa_lds(X.XA_MAX_N + 1) and X.XA_MAX_N == 38908     # N = 38908 itself runs in tests/test_cls_xattn_gpu.py
    c = X.case(2, 1, 8, "a")
    o = X.random_operands(c)
    st = X.stage(c, o, torch.full((c.B, c.H, c.N), 1.0 / c.N))
    common = [("dh = 32", {"dh": 32}), ("dh = 128", {"dh": 128}), ("sb not a multiple of 8", {"sb": c.sb + 4}), ("sn not a multiple of 8", {"sn": c.sn + 4}),
              ("B = 65536", {"B": 65536}), ("N = 38909", {"N": 38909}), ("dropout 1", {"drop_p": 1.0}), ("dropout < 0", {"drop_p": -0.25})]
    fwd = common + [("ldq not a multiple of 8", {"ldq": c.ld + 4}), ("q and q_f32 null", {"q": None, "qf": None}), ("o and o_f32 null", {"o": None, "of": None})]
    bwd = common + [("ldq not a multiple of 8", {"ldq": c.ld + 4}), ("lddo not a multiple of 8", {"lddo": c.ld + 4}), ("dk without dv", {"dv": None, "coef": None}),
                    ("dk without dv, with coef", {"dv": None}), ("dv without dk", {"dk": None}), ("none of dk, dv, coef", {"dk": None, "dv": None, "coef": None})]
    for name, cases, windows, args, call in (("xvit_cls_xattn_fwd", fwd, lambda: X.fwd_windows(c), lambda wd: X.fwd_args(c, st, wd, "bf16"), X.fwd_call),
                                             ("xvit_cls_xattn_bwd", bwd, lambda: X.bwd_windows(c), lambda wd: X.bwd_args(c, st, wd), X.bwd_call)):
        for what, change in cases:
            wd = X._to_dev(_sentinel_windows(windows()))
            a = args(wd)
            a.update(change)
            rc = call(a)
            msg = X.last_error()
            assert rc < 0, f"{name}: {what} was not refused (rc {rc})"
            assert name in msg, f"{name}: {what}: the message does not name the entry point: {msg!r}"
            _all_sentinel(f"{name}: {what}", X._to_cpu(wd))
