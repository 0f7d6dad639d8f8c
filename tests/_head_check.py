"""Oracle, launchers and gate for the kernels of the cross-attention fusion's low-rank form: xvit_head_rows, xvit_head_cols, xvit_head_wgrad,
xvit_head_bias_grad, xvit_cls_softmax_fwd, xvit_cls_softmax_bwd (csrc/head_linear.hip) and xvit_xattn_kv_dgrad (csrc/cls_xattn.hip).

Launchers.  They go through the C entry points (_lib.load()) with every stride free.  A destination is a window (_cls_check.window, or
`swindow` for the three-index layouts [b, h, c]): the sentinel everywhere, NaN where the kernel must write; after the launch every
element outside the destination (padding columns, gaps between heads and samples, the other half of the [2 H, B, d] slab, row B of every
head, fp32 and bf16, padding heads included: a strided window is allocated for B + 1 samples of which B are the destination, as `window` has its
guard row) is compared with the sentinel bit for bit.  The padding of every INPUT is NaN: the columns behind d / H of
x, W, row_scale, bias_scale, the scores and dp; rows B .. 31 of the last 32-row tile behind x, t and the scales (the kernels clamp their
row index for the loads: a lane that did not would read NaN); head rows H .. 15 of the [B, 16, d] operand t; the floats behind coef and R.

Mirror of the launch geometry (plain Python; picks the cases and names where a wrong element sits).
  32x32 tile      element (row, col) of a tile: lane col + 32 hl, accumulator i with row = (i & 3) + 8 (i >> 2) + 4 hl      (`tile_slot`)
  head_cols       four waves, wave w contracts K in [w kq, (w + 1) kq), kq = d / 4 (two 8-deep steps at H = 1)                (`cols_kq`)
  softmax         thread tid owns column tid & 15 of rows (tid >> 4) + 64 k: row n is pass n / 64, wave (n % 64) / 4          (`sm_owner`)
  kv_dgrad        xkv_slices / rows_per_block, XKV_ROWS = 64 rows per staging pass, J2 = 2 H rounded up to 8                  (`xkv_geometry`)
The mirror shows what the sizes reach: at B <= 3 every slice has at most 32 rows (N = 130 is five slices of 26, the short last slice comes at
N = 63 (32 + 31) and N = 65 (22 + 22 + 21)), so the second staging pass of a block needs ceil(1024 / B) * 64 < N: B = 130, N = 600 (8 slices of 75 = 64 + 11).

Exact tier (no tolerance).  Operands in {-3..3} 2^-s (_util.exact_operands), row scales / bias / bias scale / dp small integers times a power
of two (_util.exact_grid), rz a power of two, scale = 0.125, dropout p = 0 or 0.5 (1 / (1 - p) = 2).  Every partial sum stays below 2^24
units of its grid, so the fp32 result is the same in any order and with or without multiply-add contraction, and each oracle asserts that its
float64 result is an fp32 number.  head_rows, head_cols (fmaf(v, rs, bias * bias_scale) included), head_wgrad ((x * rs) included),
head_bias_grad and both halves of cls_softmax_bwd's coef must match bit for bit; every bf16 copy (out_bf16, ds_bf16, dhn) is the
round-to-nearest-even of the exact value.

Exact facts of the softmax forward, on any input, from the device's own e: the padding columns H .. lde - 1 of e and e_masked are +0; e at
each column's arg-max row is 1.0; e_masked = where(keep, e, 0) bit for bit with keep = hash_keep at index (b H + h) N + n; with dropout on,
e and stat[0] are bit-equal to the p = 0 launch.

Float64 tier (random operands).  Each bound is the worst case of the number of fp32 operations on the path, in any order, times 2^-24, times
the sum of the absolute terms, times SLACK = 1 + 2^-20 (second-order terms).  Derived, not measured:
  head_rows       (64 + 2) 2^-24 sum_e |x W|                                   64 products into the accumulator, store
  head_cols       (d + 3 + 3) 2^-24 (|rs| sum_c |t W| + |bias bias_scale|)     d products, 3 merges of the K-quarters, fma + bias product + store
  head_wgrad      (B + 2) 2^-24 sum_b |x rs t|                                 B products, the x * rs product
  head_bias_grad  (B + 1) 2^-24 sum_b |x w|
  kv_dgrad        (2 H + 1) 2^-24 sum_j |coef R|, then the stored bf16 inside [bf16(ref - bound), bf16(ref + bound)]
  every bf16 copy of an fp32 output: bit-equal to the round-to-nearest-even of the fp32 value the same launch stored.
  cls_softmax_bwd float64 on the very inputs (bf16 e, fp32 rz and dp; m = keep / (1 - p) with the fp32 quotient):
                  |ds - ref| <= scale |p| (|m dp| + sum_n |p m dp|) (ceil(N / 64) + 24) 2^-24       a thread's ceil(N / 64) fma, 2 shuffles, 15 waves,
                  |p' - ref| <= 3 2^-24 |p'|                                                       p, m dp, the difference, scale p, the product, ...
  cls_softmax_fwd rz and stat against float64 sums of the device's own e / e_masked (no exp enters; all terms positive, so the bound is
                  relative): (ceil(N / 64) + 2 + 15 + c_div) 2^-24 for rz = stat[0], 2 more for stat[1] = rz / (1 - p) (the difference, the
                  quotient), 3 more for stat[2] = stat[1] * tm (those 2 and the product), tm the masked sum.  tm is summed by the same threads in the
                  same order as the full sum, so its worst case is a second chain of ceil(N / 64) + 17 operations.  That chain is NOT granted:
                  stat[2] is held to the count of stat[1] plus one product, a bound tighter than its worst case by less than a factor 2.  Errors
                  of positive sums only reach their worst case when every rounding goes the same way, and a kernel that sums tm in a longer or
                  another chain than the full sum should be looked at, which is what exceeding this bound would say.  c_div = 1: build.py
                  compiles with -O3 -ffp-contract=fast and no fast-math flag, and HIP's default keeps fp32 division correctly rounded, so
                  1.0f / t is one rounding.
  cls_softmax_fwd e against float64 exp(scale (s - max)):  |e - ref| <= ref (C_exp + 3 ln 2 |a|) 2^-24,  a = the base-2 argument
                  scale log2(e) (s - max): three roundings on the argument (the difference, the constant scale * log2 e, their product), each
                  worth ln 2 |a| 2^-24 of e.  The stored bf16 must lie inside [bf16(ref - bound), bf16(ref + bound)]; a reference below the
                  fp32 range (the dominant content: 2^-180; +-640: 2^-231) rounds to 0 there, which is what the kernel must store, and no
                  content puts a reference between 2^-149 and 2^-126, where v_exp_f32 might flush.

C_exp.  The one constant nobody can derive here (the error of v_exp_f32).  Fixed from the reference side as in _cls_check.py / _ln_check.py:
`sm_mirror` is the kernel's formula in float32 on the CPU (torch.exp2 on the fp32 argument, torch sums); tests/test_head_gate_cpu.py runs it
over the GPU tests' own scores and asserts C_exp = the smallest power of two at or above 4 x the mirror's largest need (the 4 for the
hardware exp against torch's).  The device's need is logged (XVIT_MEASURE_LOG, profiles/head_linear_gate_measured.txt) and sets nothing.

  float32 CPU mirror, the largest need of C_exp over N in {1, 15, 63, 64, 65, 513, 1025, 4097} x H in {1, 3, 12, 16}
  content     need
  random x 4  0.46
  equal       0.00
  dominant    0.00   (every other row underflows to 0, the fp32 rounding of its reference)
  +-640       0.50
  largest 0.499, 4 x need = 2.0 (1.997), C_exp = 2
  MI355X (profiles/head_linear_gate_measured.txt, sets nothing): e exists only in bf16, so the device's need is read off a ladder of constants;
  it is 0 in every launch (hidden below the bf16 store: the argument term of the bound alone covers it).
"""
import functools
import math
import re
import types

import torch

from _cls_check import EPS32, SENT, SLACK, check_bf16_only, check_bound, check_window, drop_inv, f32, hash_keep, padded, window
from _util import assert_exact, exact_grid, exact_operands, note

C_EXP = 2.0                           # see the table above
C_DIV = 1                             # IEEE division (build.py: no fast-math flag)
GUARD = 64
XKV_ROWS, XKV_TARGET = 64, 1024
LOG2E = 1.4426950408889634
LADDER = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0)


class Case(types.SimpleNamespace):
    def __repr__(self):
        return self.kernel + "[" + ", ".join(f"{k}={v}" for k, v in vars(self).items() if k != "kernel" and not k.startswith("_")) + "]"


# ---------------------------------------------------------------------------------------------------------------- launch geometry
def tile_slot(r):
    """Row r (0 .. 31) of a 32x32 fp32 MFMA tile -> (accumulator index i, lane half hl): r = (i & 3) + 8 (i >> 2) + 4 hl."""
    for i in range(16):
        for hl in range(2):
            if (i & 3) + 8 * (i >> 2) + 4 * hl == r % 32:
                return i, hl
    raise AssertionError(r)


def cols_kq(d):
    """head_cols_kernel's K-quarter: ((d / 8 + 3) / 4) * 8, which is d / 4 at d = 64 H."""
    kq = ((d >> 3) + 3) >> 2 << 3
    assert kq * 4 == d and kq % 16 == 0, (d, kq)
    return kq


def sm_owner(n, h):
    """Row n, column h of the softmax kernels -> (thread, wave, pass)."""
    tid = (n % 64) * 16 + h
    return tid, tid >> 6, n // 64


def xkv_geometry(B, N, H):
    """-> (slices, rows_per_block, J2) of xvit_xattn_kv_dgrad."""
    s = min((XKV_TARGET + B - 1) // B, (N + 31) // 32)
    s = max(s, 1)
    return s, (N + s - 1) // s, (2 * H + 7) // 8 * 8


def where_rows(c):
    def w(row, col):
        h, cc = divmod(col, c.d)
        i, hl = tile_slot(row)
        return f"head_rows_kernel: sample {row}, head {h}, column {cc}: 32x32 tile ({row // 32}, {cc // 32}) of head {h}, lane {cc % 32 + 32 * hl}, accumulator {i}"
    return w


def where_cols(c):
    def w(row, col):
        i, hl = tile_slot(row)
        return (f"head_cols_kernel: sample {row}, head {col // 64}, 32x32 tile ({row // 32}, {(col % 64) // 32}), lane {col % 32 + 32 * hl}, accumulator {i}, "
                f"four K-quarters of {cols_kq(c.d)} (wave w holds [w kq, (w + 1) kq))")
    return w


def where_wgrad(c):
    def w(row, col):
        i, hl = tile_slot(row % 64)
        return (f"head_wgrad_kernel: head {row // 64}, 32x32 tile ({(row % 64) // 32}, {col // 32}), lane {col % 32 + 32 * hl}, accumulator {i}, "
                f"{(c.B + 31) // 32} batch steps of 32, {-c.B % 32} padded lanes in the last")
    return w


def where_bias(c):
    return lambda row, col: f"head_bias_grad_kernel: column {col}: block {col // 256}, thread {col % 256}, head {col // 64}"


def where_sm(c, what="e"):
    def w(row, col):
        b, n = divmod(row, c.N)
        tid, wave, k = sm_owner(n, col % 16)
        return f"cls_softmax {what}: sample {b}, row {n}, column {col}: thread {tid}, wave {wave}, pass {k} of {(c.N + 63) // 64}"
    return w


def where_stat(c):
    return lambda row, col: f"cls_softmax stat[{row // c.B}]: sample {row % c.B}, head {col}: thread {col} of block {row % c.B}"


def where_coef(c):
    def w(row, col):
        b, n = divmod(row, c.N)
        half, h = divmod(col, c.H)
        tid, wave, k = sm_owner(n, h)
        return f"cls_softmax_bwd coef {'ds' if half == 0 else 'p-prime'} half: sample {b}, row {n}, head {h}: thread {tid}, wave {wave}, pass {k} of {(c.N + 63) // 64}"
    return w


def where_kv(c):
    def w(row, col):
        b, n = divmod(row, c.N)
        s, rpb, j2 = xkv_geometry(c.B, c.N, c.H)
        return (f"xattn_kv_dgrad_kernel<{j2}>: sample {b}, row {n}, column {col}: slice {n // rpb} of {s} ({rpb} rows), staging pass {(n % rpb) // XKV_ROWS}, "
                f"thread {col // 4}, {2 * c.H} coefficients")
    return w


def _named(fn, where):
    try:
        return fn()
    except AssertionError as e:
        m = re.search(r"\(row (\d+), col (\d+)\)", str(e))
        raise AssertionError(str(e) + (" | " + where(int(m.group(1)), int(m.group(2))) if m else "")) from None


# ---------------------------------------------------------------------------------------------------------------- windows and inputs
def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def swindow(shape, strides, dtype=torch.float32, offset=0, fill=math.nan):
    """A flat buffer of SENT that holds the strided destination [b, h, c] = [shape] (NaN: must be written) at `offset`.  The buffer is that of
    shape[0] + 1 samples plus GUARD elements: row B of every head (what a lane that forgot `row < B` would store) lies inside it and holds the
    sentinel, wherever the sample stride puts it."""
    n = offset + shape[0] * strides[0] + sum((s - 1) * st for s, st in zip(shape[1:], strides[1:])) + 1 + GUARD
    buf = torch.full((n,), SENT, dtype=dtype)
    buf.as_strided(shape, strides, offset).fill_(fill)
    return buf


def sview(buf, shape, strides, offset=0):
    return buf.as_strided(shape, strides, offset)


def check_swindow(name, buf, shape, strides, offset=0):
    """Everything outside the strided destination must hold the sentinel, bit for bit."""
    buf = buf.detach().cpu()
    must = torch.zeros(buf.numel(), dtype=torch.bool)
    must.as_strided(shape, strides, offset).fill_(True)
    bad = (_bits(buf) != _bits(torch.full_like(buf, SENT))) & ~must
    if bool(bad.any()):
        flat = int(bad.nonzero()[0])
        last = offset + sum((s - 1) * st for s, st in zip(shape, strides))
        where = "in front of the destination" if flat < offset else "behind the last element" if flat > last else "in a gap the strides leave inside the destination"
        # [b, h, c]: which element of the layout, continued past row B - 1, is it (the nearest row, where the strides allow several readings)?
        hits = [divmod(flat - offset - h * strides[1], strides[0]) + (h,) for h in range(shape[1] if len(shape) == 3 else 0) if flat - offset - h * strides[1] >= 0]
        hits = sorted((b, h, cc) for b, cc, h in hits if cc < shape[2] and b >= shape[0])
        if hits:
            b, h, cc = hits[0]
            where += f" = (sample {b}, head {h}, column {cc}) of the layout: row {b} of a destination of {shape[0]} rows"
        raise AssertionError(f"{name}: {int(bad.sum())} sentinel elements were overwritten; first {where}, at flat offset {flat} "
                             f"(destination: offset {offset}, shape {tuple(shape)}, strides {tuple(strides)}): {float(buf[flat])!r}")


def up32(B):
    return (B + 31) // 32 * 32


def nan_rows(t, rows):
    """t [B, ...] inside [rows, ...] with NaN behind row B."""
    out = torch.full((rows,) + tuple(t.shape[1:]), math.nan, dtype=t.dtype)
    out[:t.shape[0]] = t
    return out


def nan_tail(t, n=XKV_ROWS * 32):
    """t flat with n NaN elements behind it."""
    return torch.cat((t.reshape(-1), torch.full((n,), math.nan, dtype=t.dtype)))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev():
    return torch.device("cuda:0")


def _ptr(t, offset=0):
    return t.data_ptr() + offset * t.element_size() if t is not None else None


def _lib():
    from xvit import _lib as L
    return L.load()


def _ok(rc, c):
    assert rc == 0, f"{c}: rc {rc}: {_lib().xvit_last_error_string().decode()}"
    torch.cuda.synchronize()


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _scales(shape, seed, kind):
    """Row / bias scales of the exact tier: small integers / 4 without a zero ("grid"), or signed powers of two 2^-2 .. 2^3 that differ by head
    and row ("pow2"); random tier: |randn| + 0.5."""
    if kind == "grid":
        t = exact_grid(shape, seed=seed, unit=0.25, span=6)
        return torch.where(t == 0, torch.full_like(t, 0.25), t)
    if kind == "pow2":
        g = torch.Generator().manual_seed(seed)
        b, h = torch.meshgrid(torch.arange(shape[0]), torch.arange(shape[1]), indexing="ij")
        k = (b * (shape[1] + 1) + h) % 6 - 2        # the next head's and the next row's exponent always differ (H + 1 is no multiple of 6 at H = 1, 3, 12, 16)
        return torch.ldexp(torch.where(torch.randint(0, 2, tuple(shape), generator=g) > 0, 1.0, -1.0), k)
    return _rand(shape, seed).abs() + 0.5


@functools.lru_cache(maxsize=None)
def _W(d, tier):
    return exact_operands((d, d), seed=3000 + d, s=3) if tier == "exact" else _rand((d, d), 3100 + d, d ** -0.5)


def _x(B, d, tier, seed):
    return exact_operands((B, d), seed=seed + B + 3 * d, s=2) if tier == "exact" else _rand((B, d), seed + 1 + B + 3 * d)


def _t16(B, H, d, tier, seed):
    """[B, 16, d]: heads H .. 15 NaN."""
    t = torch.full((B, 16, d), math.nan)
    t[:, :H] = exact_operands((B, H, d), seed=seed + B + 5 * d, s=2) if tier == "exact" else _rand((B, H, d), seed + 1 + B + 5 * d)
    return t


def _fp32_number(v, what):
    assert torch.equal(v.float().double(), v), f"{what}: the exact tier's result must be an fp32 number"


def _rne(t):
    return t.float().to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------- head_rows
def rows_case(B, H, layout="T", ob=0, wide=False, tier="exact"):
    """layout "T": out = the second half of a [2 H, B, d] slab, transposed to [b, h, c] (functional.py's R); "P": [B, H, d], with gaps between heads
    and samples when wide.  ob: head rows of the bf16 copy (0: absent, H, or 16 > H: the padding heads are zeroed)."""
    d = 64 * H
    c = Case(kernel="head_rows", B=B, H=H, d=d, layout=layout, ob=ob, wide=wide, tier=tier)
    c.ldx, c.ldw = (d + 8, d + 3) if wide else (d, d)
    if layout == "T":      # wide: a [2 H, B + 1, d] slab, so that row B of EVERY head is sentinel (packed: row B of head h is row 0 of head h + 1)
        rows = B + 1 if wide else B
        c._o = ((B, H, d), (d, rows * d, 1), H * rows * d)
    else:
        sh = d + 4 if wide else d
        c._o = ((B, H, d), (H * sh + (8 if wide else 0), sh, 1), 0)
    c._ob = ((B, ob, d), (ob * d + (8 if wide else 0), d, 1), 0) if ob else None
    return c


def rows_configs(B, H):
    return [rows_case(B, H, "T", ob=16), rows_case(B, H, "T", ob=16, wide=True), rows_case(B, H, "P", ob=H, wide=True), rows_case(B, H, "P", ob=0, wide=True),
            rows_case(B, H, "T", ob=16, wide=True, tier="random")]


def rows_operands(c):
    return {"x": _x(c.B, c.d, c.tier, 100), "W": _W(c.d, c.tier)}


def rows_oracle(c, o):
    x, W = o["x"].double().view(c.B, c.H, 64), o["W"].double().view(c.H, 64, c.d)
    ref, S = torch.einsum("bhe,hec->bhc", x, W), torch.einsum("bhe,hec->bhc", x.abs(), W.abs())
    if c.tier == "exact":
        _fp32_number(ref, c)
        return {"out": ref, "B": None}
    return {"out": ref, "B": (64 + 2) * EPS32 * S * SLACK}


def rows_windows(c):
    w = {"out": swindow(*c._o[:2], offset=c._o[2])}
    if c._ob:
        w["ob"] = swindow(*c._ob[:2], dtype=torch.bfloat16)
    return w


def rows_launch(c, o):
    dev = _dev()
    xd, Wd = padded(nan_rows(o["x"], up32(c.B)), c.ldx).to(dev), padded(o["W"], c.ldw).to(dev)
    wd = {k: t.to(dev) for k, t in rows_windows(c).items()}
    ob = c._ob
    _ok(_lib().xvit_head_rows(_ptr(xd), c.ldx, _ptr(Wd), c.ldw, _ptr(wd["out"], c._o[2]), c._o[1][0], c._o[1][1], _ptr(wd.get("ob")), ob[1][0] if ob else 0,
                              ob[1][1] if ob else 0, c.ob, c.B, c.H, c.d, _stream()), c)
    return {k: t.cpu() for k, t in wd.items()}


def rows_written(c, o):
    """The windows a correct launch leaves, from torch's fp32 einsum on the CPU (exact tier: the exact result)."""
    w = rows_windows(c)
    out = torch.einsum("bhe,hec->bhc", o["x"].view(c.B, c.H, 64), o["W"].view(c.H, 64, c.d))
    sview(w["out"], *c._o)[:] = out
    if c._ob:
        v = sview(w["ob"], *c._ob)
        v[:] = 0.0
        v[:, :c.H] = out.to(torch.bfloat16)
    return w


def rows_check(c, wins, ora, log=None):
    check_swindow(f"{c}: out", wins["out"], *c._o)
    out = sview(wins["out"], *c._o).reshape(c.B, c.H * c.d)
    ref = ora["out"].reshape(c.B, c.H * c.d)
    if ora["B"] is None:
        _named(lambda: assert_exact(out, ref.float(), f"{c}: out"), where_rows(c))
    else:
        _named(lambda: check_bound(f"{c}: out", out, ref, ora["B"].reshape(c.B, -1), log=log), where_rows(c))
    if c._ob:
        check_swindow(f"{c}: out_bf16", wins["ob"], *c._ob)
        ob = sview(wins["ob"], *c._ob)
        _named(lambda: assert_exact(ob[:, :c.H].reshape(c.B, -1), out, f"{c}: out_bf16 against the out the same launch stored"), where_rows(c))
        if ora["B"] is None:
            _named(lambda: assert_exact(ob[:, :c.H].reshape(c.B, -1), ref.float(), f"{c}: out_bf16"), where_rows(c))
        if c.ob > c.H:
            _named(lambda: assert_exact(ob[:, c.H:].reshape(c.B, -1), torch.zeros(c.B, (c.ob - c.H) * c.d), f"{c}: padding heads {c.H} .. {c.ob - 1} of out_bf16 (zeros)"),
                   lambda row, col: f"head_rows_kernel: sample {row}, padding head {c.H + col // c.d}, column {col % c.d}: block ({(row // 32) * (c.d // 32) + (col % c.d) // 32}, {c.H + col // c.d})")


# ---------------------------------------------------------------------------------------------------------------- head_cols
def cols_case(B, H, rs=None, bias=False, bsc=False, bf=False, wide=False, tier="exact"):
    d = 64 * H
    c = Case(kernel="head_cols", B=B, H=H, d=d, rs=rs, bias=bias, bsc=bsc, bf=bf, wide=wide, tier=tier)
    c.ldw, c.rs_ld, c.bsc_ld, c.ldo, c.ldob = (d + 4, H + 3, H + 5, d + 5, d + 3) if wide else (d, H, H, d, d)
    return c


def cols_configs(B, H):
    return [cols_case(B, H, bsc=True),                                                  # bias_scale without a bias: ignored
            cols_case(B, H, rs="grid", bias=True, bf=True, wide=True),
            cols_case(B, H, rs="pow2", bias=True, bsc=True, bf=True, wide=True),        # scales that differ by head and row
            cols_case(B, H, rs="pow2", bsc=True, wide=True),
            cols_case(B, H, rs="random", bias=True, bsc=True, bf=True, wide=True, tier="random")]


def cols_operands(c):
    ex = c.tier == "exact"
    o = {"t": _t16(c.B, c.H, c.d, c.tier, 200), "W": _W(c.d, c.tier), "rs": None, "bias": None, "bsc": None}
    if c.rs:
        o["rs"] = _scales((c.B, c.H), 210 + c.B + c.H, c.rs)
    if c.bias:
        o["bias"] = exact_grid((c.d,), seed=220 + c.d, unit=2.0 ** -5, span=64) if ex else _rand((c.d,), 221 + c.d)
    if c.bsc:
        o["bsc"] = _scales((c.B, c.H), 230 + c.B + c.H, "grid" if ex else "random")
    return o


def cols_oracle(c, o):
    t, W = o["t"][:, :c.H].double(), o["W"].double().view(c.H, 64, c.d)
    v, S = torch.einsum("bhc,hec->bhe", t, W), torch.einsum("bhc,hec->bhe", t.abs(), W.abs())
    if o["rs"] is not None:
        v, S = v * o["rs"].double()[:, :, None], S * o["rs"].double().abs()[:, :, None]
    if o["bias"] is not None:
        bb = o["bias"].double().view(1, c.H, 64) * (o["bsc"].double()[:, :, None] if o["bsc"] is not None else 1.0)
        v, S = v + bb, S + bb.abs()
    v, S = v.reshape(c.B, c.d), S.reshape(c.B, c.d)
    if c.tier == "exact":
        _fp32_number(v, c)
        assert float(S.max()) * 2.0 ** 7 < 2.0 ** 24
        return {"out": v, "B": None}
    return {"out": v, "B": (c.d + 3 + 3) * EPS32 * S * SLACK}


def cols_windows(c):
    w = {"out": window(c.B, c.d, c.ldo)}
    if c.bf:
        w["ob"] = window(c.B, c.d, c.ldob, torch.bfloat16)
    return w


def cols_launch(c, o):
    dev, Bp = _dev(), up32(c.B)
    td, Wd = nan_rows(o["t"], Bp).to(dev), padded(o["W"], c.ldw).to(dev)
    rs = padded(nan_rows(o["rs"], Bp), c.rs_ld).to(dev) if o["rs"] is not None else None
    bsc = padded(nan_rows(o["bsc"], Bp), c.bsc_ld).to(dev) if o["bsc"] is not None else None
    bias = o["bias"].to(dev) if o["bias"] is not None else None
    wd = {k: t.to(dev) for k, t in cols_windows(c).items()}
    _ok(_lib().xvit_head_cols(_ptr(td), 16 * c.d, c.d, _ptr(Wd), c.ldw, _ptr(rs), c.rs_ld if rs is not None else 0, _ptr(bias), _ptr(bsc),
                              c.bsc_ld if bsc is not None else 0, _ptr(wd["out"]), c.ldo, _ptr(wd.get("ob")), c.ldob if c.bf else 0, c.B, c.H, c.d, _stream()), c)
    return {k: t.cpu() for k, t in wd.items()}


def cols_mirror(c, o, fault=None):
    """head_cols in float32 on the CPU -> out [B, d].  fault: "quarter" (the last K-quarter missing), "neighbour_scale" (row 0 of head 0 scaled with
    head 1's row scale), "no_bias_scale"."""
    t, W = o["t"][:, :c.H], o["W"].view(c.H, 64, c.d)
    k = c.d - cols_kq(c.d) if fault == "quarter" else c.d
    v = torch.einsum("bhc,hec->bhe", t[:, :, :k], W[:, :, :k])
    if o["rs"] is not None:
        rs = o["rs"].clone()
        if fault == "neighbour_scale":
            rs[0, 0] = rs[0, 1]
        v = v * rs[:, :, None]
    if o["bias"] is not None:
        v = v + o["bias"].view(1, c.H, 64) * (o["bsc"][:, :, None] if o["bsc"] is not None and fault != "no_bias_scale" else 1.0)
    return v.reshape(c.B, c.d)


def cols_written(c, o, fault=None):
    w = cols_windows(c)
    out = cols_mirror(c, o, fault)
    w["out"][:c.B, :c.d] = out
    if c.bf:
        w["ob"][:c.B, :c.d] = out.to(torch.bfloat16)
    return w


def _check_2d(c, name, win, rows, cols, ref, bound, where, log=None):
    check_window(f"{c}: {name}", win, rows, cols)
    got = win[:rows, :cols]
    if bound is None:
        _named(lambda: assert_exact(got, ref.float(), f"{c}: {name}"), where)
    else:
        _named(lambda: check_bound(f"{c}: {name}", got, ref, bound, log=log), where)
    return got


def cols_check(c, wins, ora, log=None):
    out = _check_2d(c, "out", wins["out"], c.B, c.d, ora["out"], ora["B"], where_cols(c), log)
    if c.bf:
        check_window(f"{c}: out_bf16", wins["ob"], c.B, c.d)
        _named(lambda: assert_exact(wins["ob"][:c.B, :c.d], out, f"{c}: out_bf16 against the out the same launch stored"), where_cols(c))


# ---------------------------------------------------------------------------------------------------------------- head_wgrad
def wgrad_case(B, H, rs=None, wide=False, tier="exact"):
    d = 64 * H
    c = Case(kernel="head_wgrad", B=B, H=H, d=d, rs=rs, wide=wide, tier=tier)
    c.ldx, c.rs_ld, c.lddw = (d + 8, H + 3, d + 3) if wide else (d, H, d)
    return c


def wgrad_configs(B, H):
    return [wgrad_case(B, H), wgrad_case(B, H, rs="pow2", wide=True), wgrad_case(B, H, rs="random", wide=True, tier="random")]


def wgrad_operands(c):
    return {"x": _x(c.B, c.d, c.tier, 300), "t": _t16(c.B, c.H, c.d, c.tier, 310), "rs": _scales((c.B, c.H), 320 + c.B + c.H, c.rs) if c.rs else None}


def wgrad_oracle(c, o):
    x, t = o["x"].double().view(c.B, c.H, 64), o["t"][:, :c.H].double()
    rs = o["rs"].double() if o["rs"] is not None else torch.ones(c.B, c.H, dtype=torch.float64)
    ref = torch.einsum("bhe,bh,bhc->hec", x, rs, t).reshape(c.d, c.d)
    S = torch.einsum("bhe,bh,bhc->hec", x.abs(), rs.abs(), t.abs()).reshape(c.d, c.d)
    if c.tier == "exact":
        _fp32_number(ref, c)
        return {"dW": ref, "B": None}
    return {"dW": ref, "B": (c.B + 2) * EPS32 * S * SLACK}


def wgrad_launch(c, o):
    dev, Bp = _dev(), up32(c.B)
    xd, td = padded(nan_rows(o["x"], Bp), c.ldx).to(dev), nan_rows(o["t"], Bp).to(dev)
    rs = padded(nan_rows(o["rs"], Bp), c.rs_ld).to(dev) if o["rs"] is not None else None
    dW = window(c.d, c.d, c.lddw).to(dev)
    _ok(_lib().xvit_head_wgrad(_ptr(xd), c.ldx, _ptr(td), 16 * c.d, c.d, _ptr(rs), c.rs_ld if rs is not None else 0, _ptr(dW), c.lddw, c.B, c.H, c.d, _stream()), c)
    return {"dW": dW.cpu()}


def wgrad_written(c, o, fault=None):
    """fault "tail": the padded lanes of the last 32-deep batch step keep scale 1 (they re-read row 0)."""
    x, t = o["x"].view(c.B, c.H, 64), o["t"][:, :c.H]
    rs = o["rs"] if o["rs"] is not None else torch.ones(c.B, c.H)
    dW = torch.einsum("bhe,bhc->hec", x * rs[:, :, None], t)
    if fault == "tail":
        dW = dW + (-c.B % 32) * torch.einsum("he,hc->hec", x[0] * rs[0, :, None], t[0])
    w = window(c.d, c.d, c.lddw)
    w[:c.d, :c.d] = dW.reshape(c.d, c.d)
    return {"dW": w}


def wgrad_check(c, wins, ora, log=None):
    _check_2d(c, "dW", wins["dW"], c.d, c.d, ora["dW"], ora["B"], where_wgrad(c), log)


# ---------------------------------------------------------------------------------------------------------------- head_bias_grad
def bias_case(B, d, wide=True, tier="exact"):
    c = Case(kernel="head_bias_grad", B=B, H=d // 64, d=d, wide=wide, tier=tier)
    c.ldx, c.ldw = (d + 8, c.H + 3) if wide else (d, c.H)
    return c


def bias_operands(c):
    return {"x": _x(c.B, c.d, c.tier, 400), "w": _scales((c.B, c.H), 410 + c.B + c.H, "pow2" if c.tier == "exact" else "random")}


def bias_oracle(c, o):
    x, w = o["x"].double().view(c.B, c.H, 64), o["w"].double()[:, :, None]
    ref, S = (x * w).sum(0).reshape(1, c.d), (x * w).abs().sum(0).reshape(1, c.d)
    if c.tier == "exact":
        _fp32_number(ref, c)
        return {"out": ref, "B": None}
    return {"out": ref, "B": (c.B + 1) * EPS32 * S * SLACK}


def bias_launch(c, o):
    dev = _dev()
    xd, wd = padded(o["x"], c.ldx).to(dev), padded(o["w"], c.ldw).to(dev)
    out = window(1, c.d, c.d + GUARD).to(dev)
    _ok(_lib().xvit_head_bias_grad(_ptr(xd), c.ldx, _ptr(wd), c.ldw, _ptr(out), c.B, c.H, c.d, _stream()), c)
    return {"out": out.cpu()}


def bias_written(c, o):
    w = window(1, c.d, c.d + GUARD)
    w[0, :c.d] = (o["x"].view(c.B, c.H, 64) * o["w"][:, :, None]).sum(0).reshape(-1)
    return {"out": w}


def bias_check(c, wins, ora, log=None):
    _check_2d(c, "out", wins["out"], 1, c.d, ora["out"], ora["B"], where_bias(c), log)


# ---------------------------------------------------------------------------------------------------------------- cls_softmax_fwd
SM_N = (1, 15, 63, 64, 65, 513, 1025, 4097)
SM_H = (1, 3, 12, 16)
SM_KINDS = ("random", "equal", "dominant", "pm640")
SCALE = 0.125


def sm_case(B, H, N, kind="random", lds=16, lde=16, p=0.0, seed=0):
    return Case(kernel="cls_softmax_fwd", B=B, H=H, N=N, kind=kind, lds=lds, lde=lde, p=p, seed=seed, scale=SCALE)


def sm_lde(H, k):
    """The row strides of the bf16 outputs the cases walk through: H, 8 at H = 3, 16."""
    return ((H, 8, 16) if H == 3 else (H, 16))[k % (3 if H == 3 else 2)]


def sm_configs(N, H):
    """p = 0: the four contents, the strides rotating; dropout: p in {0.25, 0.5} x two seeds on the random content."""
    B = 3 if N <= 65 else 2
    cs = [sm_case(B, H, N, kind, lds=(16, 24)[k % 2], lde=sm_lde(H, k)) for k, kind in enumerate(SM_KINDS)]
    cs += [sm_case(B, H, N, "random", lds=(24, 16)[k % 2], lde=sm_lde(H, k + 1), p=p, seed=seed) for k, (p, seed) in enumerate(((0.25, 20240607), (0.25, 7), (0.5, 20240607), (0.5, 7)))]
    return cs


def sm_dominant_rows(N, H):
    """Where the dominant row of each head sits: even heads in the last pass (row N - 1), odd heads in the last wave's rows (n % 64 = 63) where one exists."""
    last_wave = max((n for n in range(N) if n % 64 == 63), default=N - 1)
    return [N - 1 if h % 2 == 0 else last_wave for h in range(H)]


def sm_scores(c):
    """-> s fp32 [B, N, H]."""
    B, N, H = c.B, c.N, c.H
    n = _rand((B, N, H), 500 + 7 * N + H)
    if c.kind == "random":
        return 4 * n
    if c.kind == "equal":
        return torch.full((B, N, H), 0.75)
    if c.kind == "dominant":                # ahead by 1000: the others are exp(-125) = 2^-180, 0 in fp32 and in bf16
        s = n.clone()
        for h, r in enumerate(sm_dominant_rows(N, H)):
            s[:, r, h] += 1000.0
        return s
    if c.kind == "pm640":                   # exp(0.125 * 1280) = e^160 overflows fp32: only the max subtraction keeps the exp finite
        return 640 * torch.where(_rand((B, N, H), 501 + N + H) > 0, 1.0, -1.0) + 0.01 * n
    raise ValueError(c.kind)


def sm_keep(c, heads=None):
    """keep [B, N, H] of the mask of xvit_dropout on a contiguous [B, H, N] tensor (heads: the H the index is built with; a fault when != H)."""
    Hh = c.H if heads is None else heads
    k = hash_keep(c.B * Hh, c.N, c.p, c.seed).reshape(c.B, Hh, c.N)
    return k[:, :c.H].permute(0, 2, 1).contiguous()


def sm_inv(p):
    """The kernel's 1 / (1 - p): the quotient goes through one fp32 difference."""
    return float(drop_inv(p))


def sm_windows(c):
    rows = c.B * c.N
    w = {"e": window(rows, c.lde, c.lde, torch.bfloat16), "stat": window(1, (3 if c.p > 0 else 1) * c.B * c.H, 3 * c.B * c.H + GUARD)}
    if c.p > 0:
        w["em"] = window(rows, c.lde, c.lde, torch.bfloat16)
    return w


def sm_launch(c, s):
    dev = _dev()
    sd = padded(s.reshape(c.B * c.N, c.H), c.lds).to(dev)
    wd = {k: t.to(dev) for k, t in sm_windows(c).items()}
    _ok(_lib().xvit_cls_softmax_fwd(_ptr(sd), c.lds, _ptr(wd["e"]), c.lde, _ptr(wd["stat"]), c.B, c.H, c.N, c.scale, _ptr(wd.get("em")), float(c.p), int(c.seed), _stream()), c)
    return {k: t.cpu() for k, t in wd.items()}


def sm_arg(c, s):
    """-> (mx [B, 1, H], the fp32 base-2 argument [B, N, H]) as the kernel forms them."""
    mx = s.amax(dim=1, keepdim=True)
    cc = torch.tensor(c.scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    return mx, (s - mx) * cc


def sm_mirror(c, s, keep=None, fault=None):
    """cls_softmax_kernel in float32 on the CPU (torch.exp2, torch sums) -> e32 (unrounded), e (bf16), em (bf16 | None), stat [k, B, H].
    fault "unrounded_rz": rz from the weights before their bf16 rounding."""
    _, a = sm_arg(c, s)
    e32 = torch.exp2(a)
    e = e32.to(torch.bfloat16)
    one = torch.tensor(1.0, dtype=torch.float32)
    z = one / (e32 if fault == "unrounded_rz" else e.float()).sum(1)
    if c.p <= 0:
        return e32, e, None, z[None]
    em = torch.where(keep, e, torch.zeros_like(e))
    zi = z / (one - torch.tensor(c.p, dtype=torch.float32))
    return e32, e, em, torch.stack((z, zi, zi * em.float().sum(1)))


def sm_written(c, s, keep=None, fault=None):
    _, e, em, stat = sm_mirror(c, s, keep, fault)
    w = sm_windows(c)
    w["e"][:c.B * c.N] = 0.0
    w["e"][:c.B * c.N, :c.H] = e.reshape(-1, c.H)
    if c.p > 0:
        w["em"][:c.B * c.N] = 0.0
        w["em"][:c.B * c.N, :c.H] = em.reshape(-1, c.H)
    w["stat"][0, :stat.numel()] = stat.reshape(-1)
    return w


def exp_ref(c, s):
    """-> float64 exp(scale (s - max)) and |a|, a = the base-2 argument."""
    s64 = s.double()
    x = f32(c.scale) * (s64 - s64.amax(dim=1, keepdim=True))
    return torch.exp(x), (x * LOG2E).abs()


def exp_bound(ref, a, cexp=None):
    return ref * ((C_EXP if cexp is None else cexp) + 3 * math.log(2) * a) * EPS32 * SLACK


def exp_need32(e32, ref, a):
    """The smallest C_exp with which the unrounded fp32 weights of the mirror pass exp_bound.  A reference below the fp32 range (2^-180 on the
    dominant content) has no fp32 neighbour but its rounding, 0: that result needs nothing, as in the interval check of the stored bf16."""
    err = (e32.double() - ref).abs()
    err = torch.where((ref < 2.0 ** -126) & (e32.double() == ref.float().double()), torch.zeros_like(err), err)
    need = (err / (ref * EPS32 * SLACK).clamp_min(1e-300) - 3 * math.log(2) * a).clamp_min(0)
    return float(torch.where(torch.isnan(need), torch.full_like(need, math.inf), need).max())


def exp_need_ladder(e, ref, a):
    """The device's e exists only in bf16: the smallest constant of LADDER whose interval holds every element (inf: none)."""
    g = e.double()
    for cexp in LADDER:
        B = exp_bound(ref, a, cexp)
        if bool(((g >= _rne(ref - B).double()) & (g <= _rne(ref + B).double())).all()):
            return cexp
    return math.inf


def sm_check(c, s, wins, keep=None, wins0=None, log=None):
    """The forward's windows against the exact facts and the float64 tier.  keep: [B, N, H] (p > 0); wins0: the windows of the p = 0 launch of
    the same scores and strides."""
    B, N, H, rows = c.B, c.N, c.H, c.B * c.N
    nstat = 3 if c.p > 0 else 1
    check_window(f"{c}: e", wins["e"], rows, c.lde)
    check_window(f"{c}: stat", wins["stat"], 1, nstat * B * H)
    e2 = wins["e"][:rows]
    names = [("e", e2)]
    if c.p > 0:
        check_window(f"{c}: e_masked", wins["em"], rows, c.lde)
        names.append(("e_masked", wins["em"][:rows]))
    for name, t in names:       # the padding columns: +0, bit for bit
        bad = _bits(t[:, H:]) != 0
        if bool(bad.any()):
            r, cc = (int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{c}: {name}: {int(bad.sum())} elements of the padding columns {H} .. {c.lde - 1} are not +0; first at (row {r}, col {H + cc}): {float(t[r, H + cc])!r}"
                                 f" | {where_sm(c, name)(r, H + cc)}")
    e = e2[:, :H].reshape(B, N, H)
    stat = wins["stat"][0, :nstat * B * H].reshape(nstat * B, H)
    # e at each column's arg-max row is exactly 1
    top = torch.gather(e.float(), 1, s.argmax(dim=1, keepdim=True))
    bad = top != 1.0
    if bool(bad.any()):
        b, _, h = (int(v) for v in bad.nonzero()[0])
        n = int(s[b, :, h].argmax())
        raise AssertionError(f"{c}: e at the arg-max row of a column must be 1.0; sample {b}, head {h}, (row {b * N + n}, col {h}): {float(top[b, 0, h])!r} | {where_sm(c)(b * N + n, h)}")
    # e against float64
    ref, a = exp_ref(c, s)
    if log is not None:
        note(f"{log}:need_exp_ladder", exp_need_ladder(e, ref, a))
    _named(lambda: check_bf16_only(f"{c}: e against float64 exp(scale (s - max))", e.reshape(rows, H), ref.reshape(rows, H), exp_bound(ref, a).reshape(rows, H)), where_sm(c))
    # rz / stat against float64 sums of the device's own weights
    chain = (N + 63) // 64 + 2 + 15 + C_DIV
    z = 1.0 / e.double().sum(1)
    refs, chains = [z], [chain]
    if c.p > 0:
        em = wins["em"][:rows, :H].reshape(B, N, H)
        _named(lambda: assert_exact(em.reshape(rows, H), torch.where(keep, e, torch.zeros_like(e)).float().reshape(rows, H), f"{c}: e_masked = where(keep, e, 0)"),
               where_sm(c, "e_masked"))
        zi = z / (1.0 - f32(c.p))
        refs, chains = [z, zi, zi * em.double().sum(1)], [chain, chain + 2, chain + 3]
    ref_stat = torch.cat(refs)
    bound = torch.cat([r * k * EPS32 * SLACK for r, k in zip(refs, chains)])
    _named(lambda: check_bound(f"{c}: rz / stat", stat, ref_stat, bound, log=f"{log}:stat" if log else None), where_stat(c))
    if c.kind == "equal":
        _named(lambda: assert_exact(e.reshape(rows, H), torch.ones(rows, H), f"{c}: e on equal scores"), where_sm(c))
        if N & (N - 1) == 0:
            _named(lambda: assert_exact(stat[:B], torch.full((B, H), 1.0 / N), f"{c}: rz = 1 / N on equal scores"), where_stat(c))
    if wins0 is not None:
        _named(lambda: assert_exact(e2, wins0["e"][:rows].float(), f"{c}: e with dropout against the p = 0 launch"), where_sm(c))
        _named(lambda: assert_exact(stat[:B], wins0["stat"][0, :B * H].reshape(B, H), f"{c}: stat[0] against the rz of the p = 0 launch"), where_stat(c))


# ---------------------------------------------------------------------------------------------------------------- cls_softmax_bwd
def bw_case(B, H, N, lde=16, ldp=16, ldb=16, p=0.0, seed=0, tier="exact"):
    return Case(kernel="cls_softmax_bwd", B=B, H=H, N=N, lde=lde, ldp=ldp, ldb=ldb, p=p, seed=seed, scale=SCALE, tier=tier)


def bw_configs(N, H):
    B = 3 if N <= 65 else 2
    cs = [bw_case(B, H, N, lde=sm_lde(H, 0), ldp=24, ldb=sm_lde(H, 1)), bw_case(B, H, N, lde=16, ldp=H, ldb=sm_lde(H, 0), p=0.5, seed=11),
          bw_case(B, H, N, lde=sm_lde(H, 1), ldp=16, ldb=16, p=0.5, seed=20240607)]
    if H == 3:      # the 8-column operand layout on all three
        cs.append(bw_case(B, H, N, lde=8, ldp=8, ldb=8, p=0.5, seed=3))
    return cs


def bw_exact_inputs(c):
    """Synthetic inputs on which the backward is exact: e in {0..7} / 8, rz in {1, 1/2, 1/4, 1/8}, dp in {-4..4} / 8."""
    g = torch.Generator().manual_seed(600 + 7 * c.N + c.H)
    e = (torch.randint(0, 8, (c.B, c.N, c.H), generator=g).float() / 8).to(torch.bfloat16)
    rz = torch.ldexp(torch.ones(c.B, c.H), -torch.randint(0, 4, (c.B, c.H), generator=g))
    return {"e": e, "rz": rz, "dp": exact_grid((c.B, c.N, c.H), seed=610 + c.N + c.H, unit=2.0 ** -3, span=4)}


def bw_random_dp(c):
    return _rand((c.B, c.N, c.H), 620 + c.N + c.H)


def bw_oracle(c, i, keep=None):
    """float64 on the very inputs -> ds, pp (p'), their bounds (None on the exact tier: bit-exact)."""
    e, rz, dp = i["e"].double(), i["rz"].double()[:, None, :], i["dp"].double()
    m = keep.double() * sm_inv(c.p) if c.p > 0 else torch.ones_like(e)
    p = e * rz
    dsum, S = (p * m * dp).sum(1, keepdim=True), (p * m * dp).abs().sum(1, keepdim=True)
    ds, pp = f32(c.scale) * p * (m * dp - dsum), p * m
    if c.tier == "exact":
        _fp32_number(ds, c)
        _fp32_number(pp, c)
        assert float(S.max()) * 2.0 ** 9 < 2.0 ** 24
        return {"ds": ds, "pp": pp, "Bds": None, "Bpp": None}
    chain = (c.N + 63) // 64 + 24
    return {"ds": ds, "pp": pp, "Bds": f32(c.scale) * p.abs() * ((m * dp).abs() + S) * chain * EPS32 * SLACK, "Bpp": 3 * EPS32 * pp.abs() * SLACK}


def bw_windows(c):
    rows = c.B * c.N
    return {"coef": window(1, rows * 2 * c.H, rows * 2 * c.H + GUARD), "dsb": window(rows, c.ldb, c.ldb, torch.bfloat16)}


def bw_launch(c, i, e_padding=math.nan):
    """e_padding: what the columns H .. lde - 1 of e hold (NaN; the forward leaves zeros there)."""
    dev, rows = _dev(), c.B * c.N
    ed = torch.full((rows, c.lde), e_padding, dtype=torch.bfloat16)
    ed[:, :c.H] = i["e"].reshape(rows, c.H)
    ed, rz, dp = ed.to(dev), i["rz"].contiguous().to(dev), padded(i["dp"].reshape(rows, c.H), c.ldp).to(dev)
    wd = {k: t.to(dev) for k, t in bw_windows(c).items()}
    _ok(_lib().xvit_cls_softmax_bwd(_ptr(ed), c.lde, _ptr(rz), _ptr(dp), c.ldp, _ptr(wd["coef"]), _ptr(wd["dsb"]), c.ldb, c.B, c.H, c.N, c.scale, float(c.p), int(c.seed),
                                    _stream()), c)
    return {k: t.cpu() for k, t in wd.items()}


def bw_mirror(c, i, keep=None, fault=None):
    """cls_softmax_bwd_kernel in float32 on the CPU -> coef [B, N, 2 H].  fault: "wave" (wave 5's partial missing from head 0's dsum),
    "no_inv" (p' without 1 / (1 - p)), "swapped" (the halves of coef exchanged)."""
    e, rz, dp = i["e"].float(), i["rz"][:, None, :], i["dp"]
    m = keep.float() * drop_inv(c.p) if c.p > 0 else torch.ones_like(e)
    p = e * rz
    term = p * (m * dp)
    if fault == "wave":
        n = torch.arange(c.N)
        term = term.clone()
        term[:, (n % 64) // 4 == 5, 0] = 0.0
    ds = torch.tensor(c.scale, dtype=torch.float32) * p * (m * dp - term.sum(1, keepdim=True))
    pp = p * (keep.float() if fault == "no_inv" else m)
    return torch.cat((pp, ds) if fault == "swapped" else (ds, pp), dim=2)


def bw_written(c, i, keep=None, fault=None):
    coef = bw_mirror(c, i, keep, fault)
    w, rows = bw_windows(c), c.B * c.N
    w["coef"][0, :rows * 2 * c.H] = coef.reshape(-1)
    w["dsb"][:rows] = 0.0
    w["dsb"][:rows, :c.H] = coef[:, :, :c.H].reshape(rows, c.H).to(torch.bfloat16)
    return w


def bw_check(c, wins, ora, log=None):
    rows, H = c.B * c.N, c.H
    check_window(f"{c}: coef", wins["coef"], 1, rows * 2 * H)
    check_window(f"{c}: ds_bf16", wins["dsb"], rows, c.ldb)
    coef = wins["coef"][0, :rows * 2 * H].reshape(rows, 2 * H)
    ref = torch.cat((ora["ds"], ora["pp"]), dim=2).reshape(rows, 2 * H)
    if ora["Bds"] is None:
        _named(lambda: assert_exact(coef, ref.float(), f"{c}: coef"), where_coef(c))
    else:
        _named(lambda: check_bound(f"{c}: coef", coef, ref, torch.cat((ora["Bds"], ora["Bpp"]), dim=2).reshape(rows, 2 * H), log=log), where_coef(c))
    dsb = wins["dsb"][:rows]
    _named(lambda: assert_exact(dsb[:, :H], coef[:, :H], f"{c}: ds_bf16 against the ds the same launch stored"), where_sm(c, "ds_bf16"))
    bad = _bits(dsb[:, H:]) != 0
    if bool(bad.any()):
        r, cc = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{c}: ds_bf16: {int(bad.sum())} elements of the padding columns {H} .. {c.ldb - 1} are not +0; first at (row {r}, col {H + cc}): {float(dsb[r, H + cc])!r}")


# ---------------------------------------------------------------------------------------------------------------- xattn_kv_dgrad
KV_H = (1, 4, 5, 8, 9, 12, 13, 16)
KV_N = (1, 31, 63, 64, 65, 130)


def kv_case(B, H, N, wide=False, tier="exact"):
    d = 64 * H
    return Case(kernel="xattn_kv_dgrad", B=B, H=H, N=N, d=d, lddh=d + 4 if wide else d, tier=tier)


def kv_configs(N, H):
    return [kv_case(1, H, N, wide=True), kv_case(3, H, N), kv_case(3, H, N, wide=True, tier="random")]


def kv_operands(c):
    if c.tier == "exact":
        return {"coef": exact_operands((c.B, c.N, 2 * c.H), seed=700 + c.B + c.N + c.H, s=2), "R": exact_operands((2 * c.H, c.B, c.d), seed=710 + c.B + c.H, s=3)}
    return {"coef": _rand((c.B, c.N, 2 * c.H), 720 + c.B + c.N + c.H), "R": _rand((2 * c.H, c.B, c.d), 730 + c.B + c.H)}


def kv_oracle(c, o):
    ref = torch.einsum("bnj,jbc->bnc", o["coef"].double(), o["R"].double()).reshape(c.B * c.N, c.d)
    if c.tier == "exact":
        _fp32_number(ref, c)
        return {"dhn": ref, "B": None}
    S = torch.einsum("bnj,jbc->bnc", o["coef"].double().abs(), o["R"].double().abs()).reshape(c.B * c.N, c.d)
    return {"dhn": ref, "B": (2 * c.H + 1) * EPS32 * S * SLACK}


def kv_launch(c, o):
    dev = _dev()
    coef, R = nan_tail(o["coef"]).to(dev), nan_tail(o["R"]).to(dev)
    dhn = window(c.B * c.N, c.d, c.lddh, torch.bfloat16).to(dev)
    _ok(_lib().xvit_xattn_kv_dgrad(_ptr(coef), _ptr(R), _ptr(dhn), c.lddh, c.B, c.H, c.N, c.d, _stream()), c)
    return {"dhn": dhn.cpu()}


def kv_written(c, o, fault=None):
    """fault "last_j": coefficient j = 2 H - 1 dropped."""
    coef = o["coef"]
    if fault == "last_j":
        coef = coef.clone()
        coef[:, :, -1] = 0.0
    w = window(c.B * c.N, c.d, c.lddh, torch.bfloat16)
    w[:c.B * c.N, :c.d] = torch.einsum("bnj,jbc->bnc", coef, o["R"]).reshape(c.B * c.N, c.d).to(torch.bfloat16)
    return {"dhn": w}


def kv_check(c, wins, ora):
    rows = c.B * c.N
    check_window(f"{c}: dhn", wins["dhn"], rows, c.d)
    got = wins["dhn"][:rows, :c.d]
    if ora["B"] is None:
        _named(lambda: assert_exact(got, ora["dhn"].float(), f"{c}: dhn"), where_kv(c))
    else:
        _named(lambda: check_bf16_only(f"{c}: dhn", got, ora["dhn"], ora["B"]), where_kv(c))


# ---------------------------------------------------------------------------------------------------------------- whole cases on the device
KERNELS = {"head_rows": (rows_operands, rows_oracle, rows_launch, rows_check), "head_cols": (cols_operands, cols_oracle, cols_launch, cols_check),
           "head_wgrad": (wgrad_operands, wgrad_oracle, wgrad_launch, wgrad_check), "head_bias_grad": (bias_operands, bias_oracle, bias_launch, bias_check)}


def run(c, log=None, twice=False):
    """Operands, oracle, launch, check of one case of the four head kernels.  twice: launch again and ask for bit-equal windows."""
    operands, oracle, launch, check = KERNELS[c.kernel]
    o = operands(c)
    ora = oracle(c, o)
    wins = launch(c, o)
    check(c, wins, ora, log=f"{log}:{c.kernel}" if log and ora["B"] is not None else None)
    if twice:
        again = launch(c, o)
        for k in wins:
            assert torch.equal(_bits(wins[k]), _bits(again[k])), f"{c}: {k} differs between two launches of the same inputs"
    return wins
