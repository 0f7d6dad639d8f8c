"""GPU: xvit_dropout against an independent statement of its mask (tests/_optim_check.py: hash32 / draw24 / Dropout(p, seed) in numpy
integers), bit for bit, guards included.  Every other dropout test of the suite takes its mask from xvit_dropout itself; this one ties
the hash, the truncated threshold, the `>=` and the epoch seed mixing to the formulas of csrc/xvit_common.h.

Sizes 1 .. 2 * 2^20 + 3: the last two go round the grid that grid_for caps at 4096 blocks of 256 threads.  x is random with +-0 planted
(kept zeros keep their sign, dropped elements are +0), so the scaled value fl(x inv) and, in bf16, its rounding are checked too.
_optim_check.THRESHOLD_SEED = 8 draws exactly thr = 2^22 at element 1752363 for p = 0.25: the one element on which `>` and `>=` differ.
Element indices at or above 2^32 are out of reach of a test of a few seconds; the mirror's 64-bit arithmetic is checked on the CPU
(tests/test_optim_gate_cpu.py)."""
import functools
import math

import pytest
import torch

import _optim_check as X

pytestmark = pytest.mark.gpu

NS = (1, 255, 256, 257, 2 ** 20 - 1, 2 ** 20 + 1, 2 * 2 ** 20 + 3)
NMAX = NS[-1]
PS = (0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.9)
SEEDS = (0, 1234, 2 ** 32 + 12345, 2 ** 64 - 1, X.THRESHOLD_SEED, X.THIRD_SEED)
DTYPES = {"f32": (torch.float32, 1), "bf16": (torch.bfloat16, 0)}      # XVIT_F32 = 1, XVIT_BF16 = 0


@functools.lru_cache(maxsize=None)
def _x(dtype_name):
    """-> (CPU tensor of NMAX values, its device copy): random, with -0 and +0 planted."""
    x = torch.randn(NMAX, generator=torch.Generator().manual_seed(101)) * 1.7
    x[::97] = -0.0
    x[1::101] = 0.0
    x[X.THRESHOLD_INDEX] = 1.2345678
    x[X.THIRD_INDEX] = -2.3456789
    x = x.to(DTYPES[dtype_name][0])
    return x, x.to(X._dev())


@functools.lru_cache(maxsize=4)
def _draw(seed):
    return X.draw24_np(seed, NMAX)


def _run(dtype_name, n, p, seed, draw, epoch=None):
    from xvit import _lib
    dt, code = DTYPES[dtype_name]
    x, xd = _x(dtype_name)
    src = torch.cat([xd[:n], torch.full((X.GUARD,), math.nan, dtype=dt, device=X._dev())])
    y = torch.full((n + X.GUARD,), X.SENT, dtype=dt, device=X._dev())
    rc = _lib.load().xvit_dropout(src.data_ptr(), y.data_ptr(), code, n, p, seed, X._stream())
    assert rc == 0, X.last_error()
    got = y.cpu()
    name = f"xvit_dropout {dtype_name} n = {n} p = {p:g} seed = {seed:#x}" + (f" epoch {epoch:#x}" if epoch is not None else "")
    X.check_tail_guard(name, got, n)
    want = X.dropout_expected(x[:n], p, seed, epoch, draw=draw)
    X.assert_bits(name, got[:n], want, X.where_drop)
    return got[:n]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_dropout_equals_the_integer_mirror_bit_for_bit(dtype_name, seed):
    draw = _draw(seed)
    for n in NS:
        for p in PS:
            got = _run(dtype_name, n, p, seed, draw)
            if p == 0.0:
                X.assert_bits(f"p = 0 is the identity (n = {n})", got, _x(dtype_name)[0][:n], X.where_drop)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_the_element_that_draws_exactly_the_threshold_is_kept(dtype_name):
    """draw24(8, 1752363) == thr(0.25) == 2^22: `>=` keeps it, `>` would drop it (the mirror is checked on the CPU; this is the device)."""
    i, thr = X.THRESHOLD_INDEX, X.drop_params(0.25)[0]
    assert X.hash32_int(X.THRESHOLD_SEED, i) & 0xFFFFFF == thr == 1 << 22
    got = _run(dtype_name, NMAX, 0.25, X.THRESHOLD_SEED, _draw(X.THRESHOLD_SEED))
    x = _x(dtype_name)[0]
    assert float(x[i]) != 0.0 and float(got[i]) != 0.0, f"element {i} draws exactly the threshold and was dropped"
    # p = 1/3: float32(p) 2^24 = 5592405.5; element 421518 of seed 13 draws 5592405 = the truncated threshold (kept), below a rounded one (dropped)
    i, thr = X.THIRD_INDEX, X.drop_params(1.0 / 3.0)[0]
    assert X.hash32_int(X.THIRD_SEED, i) & 0xFFFFFF == thr == 5592405
    got = _run(dtype_name, NMAX, 1.0 / 3.0, X.THIRD_SEED, _draw(X.THIRD_SEED))
    assert float(x[i]) != 0.0 and float(got[i]) != 0.0, f"element {i} draws exactly the truncated threshold and was dropped"


@pytest.mark.parametrize("epoch", [0, 1, 2 ** 40 + 5])
def test_a_registered_epoch_counter_is_mixed_into_the_seed(epoch):
    from xvit import ops
    counter = torch.tensor([epoch], dtype=torch.int64, device=X._dev())
    try:
        ops.set_dropout_epoch(counter)
        for seed in (1234, 2 ** 64 - 1):
            draw = X.draw24_np(X.epoch_seed(seed, epoch), NS[-2])
            for dtype_name in DTYPES:
                for n in (257, NS[-2]):
                    for p in (0.25, 1.0 / 3.0):
                        _run(dtype_name, n, p, seed, draw, epoch=epoch)
                    got = _run(dtype_name, n, 0.0, seed, None)                       # p = 0: the counter changes nothing
                    X.assert_bits("p = 0 with a counter", got, _x(dtype_name)[0][:n], X.where_drop)
        if epoch:
            assert X.epoch_seed(1234, epoch) != 1234
    finally:
        ops.set_dropout_epoch(None)
    _run("f32", 257, 0.25, 1234, None)                                               # and switched off again: the plain seed
