"""Oracle, launchers and gate for the CLS-query cross-attention kernels xvit_cls_xattn_fwd and xvit_cls_xattn_bwd (csrc/cls_xattn.hip).

Launchers.  They go through the C entry points (_lib.load()) with every stride free.  o, o_f32 and dq are windows (_cls_check.window: NaN where the
kernel must write, the sentinel in the padding columns and the guard row); p and coef are packed, so they sit between GUARD sentinel floats in front
and behind (`gwindow`).  dk and dv live in a buffer with the geometry of k and v (the same sb and sn) that is one sample longer than the operand: after
the launch every element outside rows [0, N) x columns [64 h, 64 h + 64) of each half is compared with the sentinel bit for bit (`check_dkv`): the
other third of a qkv row, the columns behind 2 d up to sn, the rows between N sn and sb, the guard sample B.  The padding of every INPUT is NaN: behind
d in q, q_f32 and dO, around the used columns of each kv row, the rows between samples, behind the saved p.

Layouts.   (a) fusion       k | v = the halves of [B N, 2 d]                        (b) interpret   k, v = columns d and 2 d of a qkv [B N, 3 d]
           (c) padded       sn = 2 d + 8, sb = (N + 3) sn, vector strides d + 8     (d) separate    k and v in two buffers, sn = d + 8, sb = (N + 1) sn

Mirror of the launch geometry (plain Python; names where a wrong element sits and picks the cases).
  PV / dp / dq loops   thread tid: part = tid & 7 (columns 8 part .. 8 part + 7 of the head), slice = tid >> 3; row n belongs to slice n % 32, pass n / 32;
                       wave (n % 32) / 8 holds that slice (the dsum partials are summed over the 4 waves in wave order)             (`pv_owner`)
  softmax loops        row n belongs to thread n % 256, wave (n % 256) / 64, pass n / 256                                          (`sm_owner`)
  output column c      of a head: summed over the 32 slices in slice order by thread c
  LDS                  ((N + 3) & ~3) + 4 + 32 * 64 floats: above 64 KiB from N = 14 333, refused above 160 KiB: N <= 38 908       (`xa_lds`)
`edge_rows(N)` are the rows on those edges: 0, N - 1, 31 | 32 (slice-pass boundary), N - 2, 255 | 256 (the first and last row of a 256 block),
63 | 64, 511 | 512, then fillers; at most 16.

Facts that need no tolerance, asserted in every launch of both tiers: o = bf16(o_f32) bit for bit; o the same with and without o_f32; q_f32 alone
= q and q_f32 together (the bf16 q is NaN then: q_f32 wins); dk = bf16(coef[.., h] q), dv = bf16(coef[.., H + h] dO) from the device's own coef (one
fp32 product on the CPU, one rounding); dq and coef the same for the three output selections; coef[.., H + h] = p m as an fp32 product (m = 1, or
hash_keep at index (b H + h) N + n times drop_inv(p)); the saved p the same with and without dropout; two launches the same; N = 1: p = 1, dq = dk = 0.

Exact tier (no tolerance).
  backward   q, k, v, dO in {-3..3} / 4 (_util.exact_operands), p zero but on edge_rows(N) where it is in {1/4, 1/2, 1}, scale = 0.125, dropout 0 or
             0.5 (m = 2).  Every partial sum of dp, dsum, dsn and dq stays below 2^24 units of its grid (`bwd_oracle` asserts it from the sums of the
             absolute terms, and that the float64 result is an fp32 number), so dq, coef, dk, dv must match bit for bit; a dead row is +0 or -0
             as the kernel's formula p (dp - dsum) scale gives it in float32: the bits are compared, not the values.
  forward    q on the grid without a zero, live keys 0 (score exactly 0: the row maximum), dead keys -512 q (score <= -256: exp = 2^-369, stored 0),
             the dead rows' v = +-2^60.  L = a power of two of live rows on edge_rows(N): p = 1 / L or +0, o_f32 = the exact mean of the live v rows
             (dropout 0.5: of the rows hash_keep keeps, doubled), o its bf16.  No reference lies between 2^-149 and 2^-126 (`fwd_oracle` asserts it).

Float64 tier (random operands; q fp32 and not bf16-representable, and the bf16 q path).  Each bound is the number of fp32 roundings on the path,
counted from csrc/cls_xattn.hip, times 2^-24, times the sum of the absolute terms, times SLACK = 1 + 2^-20.  Derived, not measured.
  o_f32      against the float64 sum of the device's own (p m) v:  (ceil(N / 32) + 32 + [dropout: 1]) 2^-24 sum_n |p m v|
             ceil(N / 32) fma of a thread, 32 adds over the slices, the product p * drop.inv
  p          against the float64 softmax:  p ((1 + E_n)(1 + max_m E_m)(1 + X_n)(1 + Z)(1 + C_DIV 2^-24)(1 + 2^-24) - 1) + 2^-125
             E = 12 2^-24 scale sum_e |q k|      the score: 8 fma, 3 shuffle adds, the product by scale; once for the element, once for the sum
                                                 (a softmax moves by at most the largest score error of its row)
             X = (C_exp + 3 ln 2 |a|) 2^-24      __expf(x) is lowered to v_exp_f32(x * 0x3fb8aa3b): the difference s - max, the constant log2 e and
                                                 the product are the three roundings on the base-2 argument a, each worth ln 2 |a| 2^-24 of e
             Z = (ceil(N / 256) + 6 + 3) 2^-24   a thread's adds, six wave levels, three adds over the waves, on a positive sum
             C_DIV = 1 (1.0f / sum is IEEE: v_div_scale / v_div_fmas / v_div_fixup), the product e * inv.
             2^-125: v_exp_f32 may flush a result below 2^-126 (the x 15 content reaches it), as in _cls_check.  NOT granted: the exp errors of the
             other rows inside the sum (a p-weighted mean of X_m: the row maximum itself is exp(0) = 1 exactly).
  coef[h]    dsn = p (dp - dsum) scale against float64 on the very inputs (the saved fp32 p, bf16 v and dO, m):
             |p| scale (err(dp) + err(dsum)) + 3 2^-24 |dsn|
             err(dp)   = 12 2^-24 m sum_e |dO v|                       8 fma, 3 shuffle adds, the product by m
             err(dsum) = (ceil(N / 32) + 6 + 3) 2^-24 sum_n |p dp|     a thread's fma, six wave levels, three adds; parts 1 .. 7 add exact zeros
             3: the difference, the product by p, the product by scale; + 2^-125: a dsn below the smallest normal fp32 number (p down to 2^-126 on the
             x 15 content) is rounded to 2^-149, or flushed.  NOT granted: the dp errors carried into dsum.
  dq         against the float64 sum of the device's own coef[h] k:  (ceil(N / 32) + 32) 2^-24 sum_n |dsn k|

C_exp.  The one constant nobody can derive here (the error of v_exp_f32).  Fixed from the reference side as in _head_check.py: `fwd_mirror` is the
forward in float32 on the CPU (torch.exp2 on the fp32 argument, torch sums); tests/test_xattn_gate_cpu.py runs it over the GPU file's own contents
and asserts C_exp = the smallest power of two at or above 4 x the mirror's largest need (the 4 for the hardware exp against torch's).  The device's need
is read off LADDER (the smallest constant with which every p of a launch passes) and logged (XVIT_MEASURE_LOG,
profiles/cls_xattn_gate_measured.txt); it sets nothing.

  float32 CPU mirror, the largest need of C_exp over every case of tests/test_cls_xattn_edges_gpu.py
  content     need
  random      0.48
  x 15        0.00   (the weights below the maximum have a large |a|: the argument term covers them)
  equal       0.50   (torch's einsum does not give identical rows bit-identical scores: weights just below 1)
  dominant    0.00   (every other row underflows to 0, the fp32 rounding of its reference)
  exact tier  0.00
  largest 0.50, 4 x need = 2.0, C_exp = 2

Planted faults (tests/test_xattn_gate_cpu.py asserts every row: the new check names the fault; the old gate is _util.rel on the same data against
TOL_F32 = 1e-3 (fp32 outputs) / TOL_BF16 = 3e-3 (dk, dv), or nothing where it never looks).
  fault                                                                 new check   old gate (same data)
  the last key row missing from the PV sum (N = 4097)                   caught      6.6e-3: seen
  slice 31's partial missing from o (N = 33)                            caught      0.34: seen
  wave 2's partial missing from dsum (N = 513)                          caught      1.5e-2 on coef's dsn half: seen
  inv from a sum without the last N mod 256 terms (N = 257)             caught      5.1e-3: seen
  p saved after dropout                                                 caught      0.65: seen
  the halves of coef swapped                                            caught      not seen (the old tests compare dk and dv, which this fault leaves alone, not coef)
  dk stored with the packed 2 d stride under layout (c)                 caught      not seen (it never ran a padded layout)
  one store into the gap behind column 2 d                              caught      not seen (it never looks there)
  a store to row N of the last sample                                   caught      not seen
  dv truncated to bf16, not rounded                                     caught      3.4e-3 on the 3e-3 gate: seen (RNE alone is 1.7e-3)
  one element of dq one ulp off                                         caught      5.6e-9: not seen
  the mask index built with 16 in place of H (H = 3, sample 1)          caught      0.58 on dv: seen
"""
import math
import re
import types

import torch

from _cls_check import EPS32, SENT, SLACK, UNDERFLOW, check_bound, check_window, drop_inv, f32, hash_keep, padded, window
from _util import assert_exact, exact_operands, note

C_EXP = 2.0                           # see the table above
C_DIV = 1                             # IEEE division (build.py: no fast-math flag)
K_ARG = 3                             # roundings on the base-2 argument of v_exp_f32
GUARD = 64
SCALE = 0.125
LOG2E = 1.4426950408889634
LADDER = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0)
KINDS = ("random", "x15", "equal", "dominant")
NS = (1, 2, 7, 8, 31, 32, 33, 63, 65, 255, 256, 257, 513, 4097)
HS = (1, 3, 12, 16, 20, 32)
XA_MAX_N = 38908


class Case(types.SimpleNamespace):
    def __repr__(self):
        return "cls_xattn[" + ", ".join(f"{k}={v}" for k, v in vars(self).items() if k in ("B", "H", "N", "layout", "p", "seed", "tier", "kind")) + "]"


def case(B, H, N, layout="a", p=0.0, seed=0, tier="random", kind="random"):
    d = 64 * H
    sn, sb, koff, voff, ld = {"a": (2 * d, N * 2 * d, 0, d, d), "b": (3 * d, N * 3 * d, d, 2 * d, d), "c": (2 * d + 8, (N + 3) * (2 * d + 8), 0, d, d + 8),
                              "d": (d + 8, (N + 1) * (d + 8), 0, 0, d)}[layout]
    return Case(B=B, H=H, N=N, d=d, layout=layout, p=p, seed=seed, tier=tier, kind=kind, sn=sn, sb=sb, koff=koff, voff=voff, ld=ld, sep=layout == "d", scale=SCALE)


def with_(c, **kw):
    a = {k: getattr(c, k) for k in ("B", "H", "N", "layout", "p", "seed", "tier", "kind")}
    a.update(kw)
    return case(**a)


# ---------------------------------------------------------------------------------------------------------------- the cases of the GPU file
DROP = (0.5, 20240607)


def n_cases(N):
    """Every N at one layout (rotating), B rotating over 1, 2, 3; a second content rotating over x 15, equal, dominant."""
    i = NS.index(N)
    return case((1, 2, 3)[i % 3] if N < 4097 else 1, 3, N, "abcd"[i % 4]), KINDS[1 + i % 3]


def layout_cases():
    return [case(2, H, N, layout) for layout in "abcd" for N in (33, 257) for H in (3, 20)]


def h_cases():
    return [case(2, H, 65, "abcd"[i % 4]) for i, H in enumerate(HS)]


def lds_case():
    return case(1, 1, 16385, "a")


def all_cases():
    """-> (case, second content | None) of every test of tests/test_cls_xattn_edges_gpu.py."""
    return [n_cases(N) for N in NS] + [(c, None) for c in layout_cases() + h_cases()]


# ---------------------------------------------------------------------------------------------------------------- launch geometry
def xa_lds(N):
    return (((N + 3) & ~3) + 4 + 32 * 64) * 4


def pv_owner(n):
    """Row n in the PV / dp / dq loops -> (slice, pass, wave)."""
    return n % 32, n // 32, (n % 32) // 8


def sm_owner(n):
    """Row n in the softmax loops -> (thread, wave, pass)."""
    return n % 256, (n % 256) // 64, n // 256


def edge_rows(N):
    cand = [0, N - 1, 31, 32, N - 2, 255, 256, 63, 64, 511, 512] + list(range(1, 17))
    rows = []
    for r in cand:
        if 0 <= r < N and r not in rows:
            rows.append(r)
    return rows[:16]


def _row(c, n):
    s, k, w = pv_owner(n)
    t, sw, sp = sm_owner(n)
    return f"key row {n} of {c.N}: slice {s}, pass {k} of {(c.N + 31) // 32}, wave {w}; softmax thread {t}, wave {sw}, pass {sp} of {(c.N + 255) // 256}"


def where_p(c):
    return lambda row, col: f"cls_xattn_fwd p: sample {row // c.H}, head {row % c.H}, {_row(c, col)}"


def where_vec(c, what):
    return lambda row, col: (f"{what}: sample {row}, head {col // 64}, column {col % 64}: thread {col % 64} sums the 32 slices in slice order; "
                             f"part {(col % 64) // 8} of each slice, {(c.N + 31) // 32} passes, {max(0, 32 - c.N)} empty slices")


def where_coef(c):
    return lambda row, col: f"cls_xattn_bwd coef {'dsn' if col < c.H else 'p-prime'} half: sample {row // c.N}, head {col % c.H}, {_row(c, row % c.N)}"


def where_dkv(c, what):
    return lambda row, col: f"cls_xattn_bwd {what}: sample {row // c.N}, head {col // 64}, column {col % 64} (part {(col % 64) // 8}), {_row(c, row % c.N)}"


def _named(fn, where):
    try:
        return fn()
    except AssertionError as e:
        m = re.search(r"\(row (\d+), col (\d+)\)", str(e))
        raise AssertionError(str(e) + (" | " + where(int(m.group(1)), int(m.group(2))) if m else "")) from None


# ---------------------------------------------------------------------------------------------------------------- windows
def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def assert_bits(got, ref, what):
    """Values (NaN fails) and then the bits: a zero must carry the reference's sign."""
    assert_exact(got, ref, what)
    g, r = got.detach().cpu(), ref.to(got.dtype)
    bad = _bits(g) != _bits(r)
    if bool(bad.any()):
        row, col = (int(v) for v in bad.reshape(-1, bad.shape[-1]).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits (the sign of a zero); first at (row {row}, col {col}): "
                             f"{float(g.reshape(-1, g.shape[-1])[row, col])!r} != {float(r.reshape(-1, r.shape[-1])[row, col])!r}")


def gwindow(n, fill=math.nan):
    """GUARD sentinels, n floats the kernel must write, GUARD sentinels."""
    b = torch.full((n + 2 * GUARD,), SENT)
    b[GUARD:GUARD + n] = fill
    return b


def gview(buf):
    return buf[GUARD:buf.numel() - GUARD]


def check_gwindow(name, buf):
    buf = buf.detach().cpu()
    bad = _bits(buf) != _bits(torch.full_like(buf, SENT))
    bad[GUARD:buf.numel() - GUARD] = False
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        where = f"{GUARD - i} floats in front of the tensor" if i < GUARD else f"{i - (buf.numel() - GUARD)} floats behind its last element"
        raise AssertionError(f"{name}: {int(bad.sum())} sentinel floats around the packed tensor were overwritten; first {where}: {float(buf[i])!r}")


def kv_shape(c):
    return (c.B, c.N, c.d), (c.sb, c.sn, 1)


def kv_inputs(c, k, v):
    """k, v [B, N, d] -> the operand buffers (one, or two under layout (d)): NaN but where the kernel may read."""
    bufs = [torch.full((c.B * c.sb + GUARD,), math.nan, dtype=torch.bfloat16) for _ in range(2 if c.sep else 1)]
    bufs[0].as_strided(*kv_shape(c), c.koff).copy_(k)
    bufs[-1].as_strided(*kv_shape(c), c.voff).copy_(v)
    return bufs


def dkv_windows(c):
    """The gradient buffers, with the geometry of the operand and one guard sample more: the sentinel, NaN where dk and dv must be written."""
    bufs = [torch.full(((c.B + 1) * c.sb + GUARD,), SENT, dtype=torch.bfloat16) for _ in range(2 if c.sep else 1)]
    bufs[0].as_strided(*kv_shape(c), c.koff).fill_(math.nan)
    bufs[-1].as_strided(*kv_shape(c), c.voff).fill_(math.nan)
    return bufs


def dkv_views(c, bufs):
    return bufs[0].as_strided(*kv_shape(c), c.koff), bufs[-1].as_strided(*kv_shape(c), c.voff)


def check_dkv(c, bufs):
    """Everything outside rows [0, N) x the d columns of each half must hold the sentinel, bit for bit."""
    for i, buf in enumerate(bufs):
        buf = buf.detach().cpu()
        must = torch.zeros(buf.numel(), dtype=torch.bool)
        for j, off in enumerate((c.koff, c.voff)):
            if not c.sep or i == j:
                must.as_strided(*kv_shape(c), off).fill_(True)
        bad = (_bits(buf) != _bits(torch.full_like(buf, SENT))) & ~must
        if bool(bad.any()):
            flat = int(bad.nonzero()[0])
            b, rem = divmod(flat, c.sb)
            n, col = divmod(rem, c.sn)
            used = ((c.koff, "dk"), (c.voff, "dv")) if not c.sep else ((0, ("dk", "dv")[i]),)
            half = next((f"column {col - off} of the {nm} half" for off, nm in used if off <= col < off + c.d), None)
            half = half or (f"column {col}: the gap behind column {max(off for off, _ in used) + c.d} up to the row stride {c.sn}" if col >= max(off for off, _ in used) + c.d
                            else f"column {col}: in front of the halves (the q third of a qkv row)")
            if b >= c.B:
                last = (flat - (c.B - 1) * c.sb) // c.sn
                where = f"behind the last sample: row {last} of sample {c.B - 1}, which has {c.N} (the guard sample {b}, row {n})"
            elif n >= c.N:
                where = f"row {n} of sample {b}, which has {c.N}: between its rows and the sample stride ({c.sb // c.sn} rows)"
            else:
                where = f"sample {b}, row {n}"
            name = "dk | dv buffer" if not c.sep else ("dk", "dv")[i] + " buffer"
            raise AssertionError(f"{c}: {name}: {int(bad.sum())} sentinel elements were overwritten; first at flat offset {flat}: {where}, {half} "
                                 f"(sb {c.sb}, sn {c.sn}, halves at columns {c.koff} and {c.voff}): {float(buf[flat])!r}")


def nan_tail(t, n=GUARD):
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


def last_error():
    return _lib().xvit_last_error_string().decode()


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rt(t):
    return t.to(torch.bfloat16).float()


def _rne(t):
    return t.float().to(torch.bfloat16)


def _fp32_number(v, what):
    assert torch.equal(v.float().double(), v), f"{what}: the exact tier's result must be an fp32 number"


# ---------------------------------------------------------------------------------------------------------------- masks and operands
def keep_mask(c, heads=None):
    """keep [B, H, N] of the mask of xvit_dropout on a contiguous [B, H, N] tensor (heads: the H the index is built with; a fault when != H)."""
    Hh = c.H if heads is None else heads
    return hash_keep(c.B * Hh, c.N, c.p, c.seed).reshape(c.B, Hh, c.N)[:, :c.H].contiguous()


def mask32(c, keep):
    """m fp32 [B, H, N]: 1, or keep * (1 / (1 - p)) with the kernel's fp32 quotient."""
    return keep.float() * drop_inv(c.p) if c.p > 0 else torch.ones(c.B, c.H, c.N)


def dominant_rows(N, H):
    """Even heads: the last row; odd heads: the last row of the first 256 block's last wave where there is one."""
    return [N - 1 if h % 2 == 0 else min(N - 1, 255) for h in range(H)]


def random_operands(c):
    """-> q (fp32, not bf16-representable), qb (its bf16), k, v [B, N, d], dO [B, d] (bf16-exact fp32)."""
    B, H, N, d = c.B, c.H, c.N, c.d
    seed = 9000 + 131 * N + 7 * H + B + KINDS.index(c.kind)
    q = _rand((B, d), seed, 15.0 if c.kind == "x15" else 1.0)
    k, v, dO = _rt(_rand((B, N, d), seed + 1)), _rt(_rand((B, N, d), seed + 2)), _rt(_rand((B, d), seed + 3))
    if c.kind == "equal":
        k = k[:, :1].expand(B, N, d).contiguous()
    if c.kind == "dominant":                 # the score of that row is 4 |q|^2 ~ 256: every other row is below 2^-149 and must be stored as 0
        for h, r in enumerate(dominant_rows(N, H)):
            k[:, r, 64 * h:64 * h + 64] = _rt(32 * q[:, 64 * h:64 * h + 64])
    return {"q": q, "qb": _rt(q), "k": k, "v": v, "dO": dO}


def exact_operands_bwd(c):
    """The backward's exact content: operands in {-3..3} / 4, p in {1/4, 1/2, 1} on edge_rows(N) and 0 elsewhere (p is an input: it need not sum to 1)."""
    B, H, N, d = c.B, c.H, c.N, c.d
    seed = 7000 + 131 * N + 7 * H + B
    q = exact_operands((B, d), seed=seed, s=2)
    g = torch.Generator().manual_seed(seed + 4)
    p = torch.zeros(B, H, N)
    rows = edge_rows(N)
    p[:, :, rows] = torch.ldexp(torch.ones(B, H, len(rows)), -torch.randint(0, 3, (B, H, len(rows)), generator=g))
    return {"q": q, "qb": q, "k": exact_operands((B, N, d), seed=seed + 1, s=2), "v": exact_operands((B, N, d), seed=seed + 2, s=2),
            "dO": exact_operands((B, d), seed=seed + 3, s=2), "p": p}


def live_rows(N):
    rows = edge_rows(N)
    return rows[:1 << (len(rows).bit_length() - 1)]


def exact_operands_fwd(c):
    """The forward's exact content: see the docstring."""
    B, H, N, d = c.B, c.H, c.N, c.d
    seed = 8000 + 131 * N + 7 * H + B
    q = exact_operands((B, d), seed=seed, s=2)
    q = torch.where(q == 0, torch.full_like(q, 0.25), q)
    live = torch.zeros(N, dtype=torch.bool)
    live[live_rows(N)] = True
    k = torch.where(live[None, :, None], torch.zeros(B, N, d), (-512.0 * q)[:, None, :].expand(B, N, d))
    big = exact_operands((B, N, d), seed=seed + 5, s=0) * 2.0 ** 58 + 2.0 ** 60          # {1..7} 2^58: never 0, exact in bf16
    v = torch.where(live[None, :, None], exact_operands((B, N, d), seed=seed + 2, s=2), big)
    return {"q": q, "qb": q, "k": k.contiguous(), "v": v, "dO": exact_operands((B, d), seed=seed + 3, s=2)}


def _h4(c, t):
    return t.view(c.B, c.N, c.H, 64)


# ---------------------------------------------------------------------------------------------------------------- forward: mirror, oracle
def fwd_mirror(c, q, o, keep=None, fault=None):
    """cls_xattn_fwd_kernel in float32 on the CPU (torch sums, torch.exp2 on the fp32 argument) -> dict s, e, p (saved), of [B, d].
    fault: "last_row" (row N - 1 missing from the PV sum), "slice31" (slice 31's partial missing from o), "inv_tail" (inv from a sum without the last
    N mod 256 terms), "p_after_dropout"."""
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    s = torch.einsum("bhe,bnhe->bhn", q.view(c.B, c.H, 64), _h4(c, o["k"])) * t(c.scale)
    e = torch.exp2((s - s.amax(-1, keepdim=True)) * t(LOG2E))
    terms = e[..., :c.N - c.N % 256] if fault == "inv_tail" else e
    p = e * (t(1.0) / terms.sum(-1, keepdim=True))
    w = p * mask32(c, keep)
    saved = w if fault == "p_after_dropout" else p
    if fault in ("last_row", "slice31"):
        w = w.clone()
        w[..., torch.arange(c.N) % 32 == 31 if fault == "slice31" else c.N - 1] = 0.0
    of = torch.einsum("bhn,bnhe->bhe", w, _h4(c, o["v"])).reshape(c.B, c.d) + 0.0
    return {"s": s, "e": e, "p": saved, "of": of}


def fwd_windows(c, osel="both"):
    w = {"p": gwindow(c.B * c.H * c.N)}
    if osel in ("both", "o"):
        w["o"] = window(c.B, c.d, c.ld, torch.bfloat16)
    if osel in ("both", "of"):
        w["of"] = window(c.B, c.d, c.ld)
    return w


def fwd_written(c, q, o, keep=None, fault=None):
    """The windows a launch leaves, from the float32 mirror."""
    m, w = fwd_mirror(c, q, o, keep, fault), fwd_windows(c)
    gview(w["p"])[:] = m["p"].reshape(-1)
    w["of"][:c.B, :c.d] = m["of"]
    w["o"][:c.B, :c.d] = m["of"].to(torch.bfloat16)
    return w


def exp_need32(m):
    """The smallest C_exp with which the mirror's e passes (C_exp + K_ARG ln 2 |a|) 2^-24 against float64 exp of ITS OWN fp32 scores (the score
    error is another term of the bound).  A reference below the fp32 range has no fp32 neighbour but its rounding: that result needs nothing."""
    x = m["s"].double() - m["s"].double().amax(-1, keepdim=True)
    ref, a = torch.exp(x), (x * LOG2E).abs()
    err = (m["e"].double() - ref).abs()
    err = torch.where((ref < 2.0 ** -126) & (m["e"].double() == ref.float().double()), torch.zeros_like(err), err)
    need = (err / (ref * EPS32 * SLACK).clamp_min(1e-300) - K_ARG * math.log(2) * a).clamp_min(0)
    return float(torch.where(torch.isnan(need), torch.full_like(need, math.inf), need).max())


def fwd_oracle(c, q, o, keep=None):
    """-> dict: exact tier p, of (fp32, THE result); float64 tier P, the terms of its bound, m."""
    B, H, N = c.B, c.H, c.N
    q64, k64 = q.double().view(B, H, 64), _h4(c, o["k"]).double()
    sc = f32(c.scale)
    s = sc * torch.einsum("bhe,bnhe->bhn", q64, k64)
    x = s - s.amax(-1, keepdim=True)
    m = mask32(c, keep)
    if c.tier == "exact":
        ref = torch.exp(x)
        assert not bool(((ref > 2.0 ** -149) & (ref < 2.0 ** -126)).any()), f"{c}: an exact-tier reference between 2^-149 and 2^-126"
        assert bool(((x == 0) | (x <= -256)).all())
        live = x == 0
        L = live.sum(-1, keepdim=True)
        assert bool((L & (L - 1) == 0).all()) and bool((L > 0).all())
        p = torch.where(live, 1.0 / L.double(), torch.zeros_like(x))
        w = p * m.double()
        vl = torch.where(_h4(c, o["v"]).abs() < 2.0 ** 50, _h4(c, o["v"]), torch.zeros(())).double()        # a dead row's weight is +0: its v never counts
        of, S = torch.einsum("bhn,bnhe->bhe", w, vl).reshape(B, c.d), torch.einsum("bhn,bnhe->bhe", w, vl.abs())
        _fp32_number(p, c)
        _fp32_number(of, c)
        assert float(S.max()) * 2.0 ** 2 * float(L.max()) < 2.0 ** 24
        return {"p": p.float(), "of": of.float() + 0.0, "m": m}
    E = 12 * EPS32 * sc * torch.einsum("bhe,bnhe->bhn", q64.abs(), k64.abs())
    return {"P": torch.softmax(s, -1), "E": E, "Emax": E.amax(-1, keepdim=True), "a": (x * LOG2E).abs(), "m": m}


def p_bound(c, ora, cexp=None):
    cexp = C_EXP if cexp is None else cexp
    a = ora["a"] + (ora["E"] + ora["Emax"]) * LOG2E
    rel = ((1 + ora["E"]) * (1 + ora["Emax"]) * (1 + (cexp + K_ARG * math.log(2) * a) * EPS32) * (1 + ((c.N + 255) // 256 + 9) * EPS32)
           * (1 + C_DIV * EPS32) * (1 + EPS32) - 1)
    return ora["P"] * rel * SLACK + UNDERFLOW


def p_need_ladder(c, p, ora):
    g = p.double()
    for cexp in LADDER:
        if bool(((g - ora["P"]).abs() <= p_bound(c, ora, cexp)).all()):
            return cexp
    return math.inf


def fwd_check(c, o, wins, ora, wins0=None, log=None):
    """The forward's windows against the exact facts and the tier's reference.  wins0: the windows of the p = 0 launch of the same operands."""
    B, H, N, d = c.B, c.H, c.N, c.d
    check_gwindow(f"{c}: p", wins["p"])
    p = gview(wins["p"]).reshape(B * H, N)
    for k in ("o", "of"):
        if k in wins:
            check_window(f"{c}: {k}", wins[k], B, d)
    if "o" in wins and "of" in wins:
        _named(lambda: assert_bits(wins["o"][:B, :d], wins["of"][:B, :d], f"{c}: o against the bf16 rounding of the o_f32 the same launch stored"), where_vec(c, "cls_xattn_fwd o"))
    if N == 1:
        _named(lambda: assert_bits(p, torch.ones(B * H, 1), f"{c}: p = 1 at N = 1"), where_p(c))
    if wins0 is not None:
        _named(lambda: assert_bits(p, gview(wins0["p"]).reshape(B * H, N), f"{c}: the saved p with dropout against the p = 0 launch (it is saved before dropout)"), where_p(c))
    if c.tier == "exact":
        _named(lambda: assert_bits(p, ora["p"].reshape(B * H, N), f"{c}: p"), where_p(c))
        if "of" in wins:
            _named(lambda: assert_bits(wins["of"][:B, :d], ora["of"], f"{c}: o_f32"), where_vec(c, "cls_xattn_fwd o_f32"))
        if "o" in wins:
            _named(lambda: assert_bits(wins["o"][:B, :d], ora["of"], f"{c}: o"), where_vec(c, "cls_xattn_fwd o"))
        return
    if log is not None:
        note(f"{log}:need_exp_ladder", p_need_ladder(c, p.reshape(B, H, N), ora))
    _named(lambda: check_bound(f"{c}: p against the float64 softmax", p, ora["P"].reshape(B * H, N), p_bound(c, ora).reshape(B * H, N), log=f"{log}:p" if log else None), where_p(c))
    if "of" in wins:       # against the float64 sum of the device's own p m v
        w = p.reshape(B, H, N).double() * ora["m"].double()
        v64 = _h4(c, o["v"]).double()
        ref, S = torch.einsum("bhn,bnhe->bhe", w, v64).reshape(B, d), torch.einsum("bhn,bnhe->bhe", w, v64.abs()).reshape(B, d)
        chain = (N + 31) // 32 + 32 + (1 if c.p > 0 else 0)
        _named(lambda: check_bound(f"{c}: o_f32 against the float64 sum of the stored p m v", wins["of"][:B, :d], ref, chain * EPS32 * S * SLACK, log=f"{log}:o_f32" if log else None),
               where_vec(c, "cls_xattn_fwd o_f32"))


# ---------------------------------------------------------------------------------------------------------------- backward: mirror, oracle
def bwd_mirror(c, o, p, keep=None, fault=None):
    """cls_xattn_bwd_kernel in float32 on the CPU, in the kernel's order of operations -> dq [B, d], coef [B, N, 2 H], dk, dv [B, N, d] (bf16).
    fault: "wave" (wave 2's partial missing from head 0's dsum), "swapped" (the halves of coef exchanged)."""
    B, H, N, d = c.B, c.H, c.N, c.d
    m = mask32(c, keep)
    dO, qb = o["dO"].view(B, H, 64), o["qb"].view(B, H, 64)
    dp = torch.einsum("bhe,bnhe->bhn", dO, _h4(c, o["v"])) * m
    term = p * dp
    if fault == "wave":
        term = term.clone()
        term[:, 0, (torch.arange(N) % 32) // 8 == 2] = 0.0
    dsum = term.sum(-1, keepdim=True) + 0.0                    # the device's sum starts from +0 and never is -0
    dsn = p * (dp - dsum) * torch.tensor(c.scale, dtype=torch.float32)
    pr = p * m
    dq = torch.einsum("bhn,bnhe->bhe", dsn, _h4(c, o["k"])).reshape(B, d) + 0.0
    halves = (pr, dsn) if fault == "swapped" else (dsn, pr)
    return {"dq": dq, "coef": torch.cat([t.permute(0, 2, 1) for t in halves], dim=2).contiguous(), "dk": dkv_from(c, dsn.permute(0, 2, 1), qb), "dv": dkv_from(c, pr.permute(0, 2, 1), dO)}


def dkv_from(c, coef_half, vec):
    """bf16(coef[b, n, h] * vec[b, h, e]) -> [B, N, d]: one fp32 product, one rounding."""
    return (coef_half.float()[..., None] * vec.float().reshape(c.B, 1, c.H, 64)).to(torch.bfloat16).reshape(c.B, c.N, c.d)


def bwd_windows(c, sel="both"):
    w = {"dq": window(c.B, c.d, c.ld)}
    if sel in ("both", "dkv"):
        w["dkv"] = dkv_windows(c)
    if sel in ("both", "coef"):
        w["coef"] = gwindow(c.B * c.N * 2 * c.H)
    return w


def bwd_written(c, o, p, keep=None, fault=None):
    m, w = bwd_mirror(c, o, p, keep, fault), bwd_windows(c)
    w["dq"][:c.B, :c.d] = m["dq"]
    gview(w["coef"])[:] = m["coef"].reshape(-1)
    for view, t in zip(dkv_views(c, w["dkv"]), (m["dk"], m["dv"])):
        view.copy_(t)
    return w


def bwd_oracle(c, o, p, keep=None):
    """float64 on the very inputs -> dsn, pr (fp32 product), the bound of dsn (None: bit-exact, and then dsn, dq are the float32 evaluation)."""
    B, H, N = c.B, c.H, c.N
    m = mask32(c, keep)
    v64, dO64, p64, sc = _h4(c, o["v"]).double(), o["dO"].double().view(B, H, 64), p.double(), f32(c.scale)
    dp, Sdp = torch.einsum("bhe,bnhe->bhn", dO64, v64) * m.double(), torch.einsum("bhe,bnhe->bhn", dO64.abs(), v64.abs()) * m.double()
    dsum, Sds = (p64 * dp).sum(-1, keepdim=True), (p64 * dp).abs().sum(-1, keepdim=True)
    dsn = p64 * (dp - dsum) * sc
    out = {"pr": p * m, "m": m, "p": p}
    if c.tier == "exact":
        mir = bwd_mirror(c, o, p, keep)
        dq = torch.einsum("bhn,bnhe->bhe", dsn, _h4(c, o["k"]).double()).reshape(B, c.d)
        Sdq = torch.einsum("bhn,bnhe->bhe", dsn.abs(), _h4(c, o["k"]).double().abs())
        # units: dp 2^-4 (x m <= 2), p dp 2^-6, dsn 2^-11, dsn k 2^-13
        assert float(Sdp.max()) * 2.0 ** 4 < 2.0 ** 24 and float(Sds.max()) * 2.0 ** 6 < 2.0 ** 24 and float((p64 * (dp.abs() + Sds)).max()) * 2.0 ** 8 < 2.0 ** 24
        assert float(Sdq.max()) * 2.0 ** 13 < 2.0 ** 24
        for k, v in (("dsn", dsn), ("dq", dq)):
            _fp32_number(v, c)
        assert torch.equal(mir["coef"][:, :, :H].double(), dsn.permute(0, 2, 1)) and torch.equal(mir["dq"].double(), dq), f"{c}: the float32 evaluation is not the float64 one"
        out.update(dsn=mir["coef"][:, :, :H], dq=mir["dq"], dk=mir["dk"], dv=mir["dv"], Bdsn=None)
        return out
    err_dp, err_dsum = 12 * EPS32 * Sdp, ((N + 31) // 32 + 9) * EPS32 * Sds
    out.update(dsn=dsn.permute(0, 2, 1), Bdsn=((p64.abs() * sc * (err_dp + err_dsum) + 3 * EPS32 * dsn.abs()) * SLACK + UNDERFLOW).permute(0, 2, 1))
    return out


def bwd_check(c, o, wins, ora, coef=None, log=None):
    """The backward's windows.  coef: the [B N, 2 H] coefficients of another launch of the same inputs, where this one stored none."""
    B, H, N, d = c.B, c.H, c.N, c.d
    check_window(f"{c}: dq", wins["dq"], B, d)
    dq = wins["dq"][:B, :d]
    if "coef" in wins:
        check_gwindow(f"{c}: coef", wins["coef"])
        coef = gview(wins["coef"]).reshape(B * N, 2 * H)
        _named(lambda: assert_bits(coef[:, H:], ora["pr"].permute(0, 2, 1).reshape(B * N, H), f"{c}: coef[.., H + h] = p m"), lambda r, cc: where_coef(c)(r, cc + H))
        if ora["Bdsn"] is None:
            _named(lambda: assert_bits(coef[:, :H], ora["dsn"].reshape(B * N, H), f"{c}: coef[.., h] = dsn"), where_coef(c))
        else:
            _named(lambda: check_bound(f"{c}: coef[.., h] = dsn", coef[:, :H], ora["dsn"].reshape(B * N, H), ora["Bdsn"].reshape(B * N, H), log=f"{log}:dsn" if log else None), where_coef(c))
    assert coef is not None
    if ora["Bdsn"] is None:
        _named(lambda: assert_bits(dq, ora["dq"], f"{c}: dq"), where_vec(c, "cls_xattn_bwd dq"))
    else:
        dsn64, k64 = coef[:, :H].reshape(B, N, H).double(), _h4(c, o["k"]).double()
        ref, S = torch.einsum("bnh,bnhe->bhe", dsn64, k64).reshape(B, d), torch.einsum("bnh,bnhe->bhe", dsn64.abs(), k64.abs()).reshape(B, d)
        _named(lambda: check_bound(f"{c}: dq against the float64 sum of the stored dsn k", dq, ref, ((N + 31) // 32 + 32) * EPS32 * S * SLACK, log=f"{log}:dq" if log else None),
               where_vec(c, "cls_xattn_bwd dq"))
    one = N == 1 and bool((ora["p"] == 1).all())             # the forward's p at N = 1 (the exact tier's p is an input and need not be 1)
    if one:
        _named(lambda: assert_exact(dq, torch.zeros(B, d), f"{c}: dq = 0 at N = 1"), where_vec(c, "cls_xattn_bwd dq"))
    if "dkv" in wins:
        check_dkv(c, wins["dkv"])
        dk, dv = (t.reshape(B * N, d) for t in dkv_views(c, wins["dkv"]))
        c3 = coef.reshape(B, N, 2 * H)
        _named(lambda: assert_bits(dk, dkv_from(c, c3[:, :, :H], o["qb"]).reshape(B * N, d), f"{c}: dk = bf16(coef[.., h] q)"), where_dkv(c, "dk"))
        _named(lambda: assert_bits(dv, dkv_from(c, c3[:, :, H:], o["dO"]).reshape(B * N, d), f"{c}: dv = bf16(coef[.., H + h] dO)"), where_dkv(c, "dv"))
        if one:
            _named(lambda: assert_exact(dk, torch.zeros(B, d), f"{c}: dk = 0 at N = 1"), where_dkv(c, "dk"))
    return coef


# ---------------------------------------------------------------------------------------------------------------- launches on the device
def stage(c, o, p=None):
    """The inputs on the device, NaN in every padding -> dict."""
    dev = _dev()
    st = {"qf": padded(o["q"], c.ld).to(dev), "qb": padded(o["qb"].to(torch.bfloat16), c.ld).to(dev), "qnan": torch.full((c.B, c.ld), math.nan, dtype=torch.bfloat16).to(dev),
          "kv": [t.to(dev) for t in kv_inputs(c, o["k"], o["v"])], "dO": padded(o["dO"].to(torch.bfloat16), c.ld).to(dev)}
    if p is not None:
        st["p"] = nan_tail(p).to(dev)
    return st


def fwd_args(c, st, wd, qsel="f32", drop=None):
    """qsel: "f32" (q_f32 alone), "bf16" (q alone), "both" (q_f32 wins: the bf16 q is NaN)."""
    p, seed = (c.p, c.seed) if drop is None else drop
    return {"q": _ptr(st["qb"] if qsel == "bf16" else st["qnan"]) if qsel != "f32" else None, "ldq": c.ld if qsel != "f32" else 0,
            "qf": _ptr(st["qf"]) if qsel != "bf16" else None, "ldqf": c.ld if qsel != "bf16" else 0,
            "k": _ptr(st["kv"][0], c.koff), "v": _ptr(st["kv"][-1], c.voff), "sb": c.sb, "sn": c.sn, "o": _ptr(wd.get("o")), "ldo": c.ld, "of": _ptr(wd.get("of")), "ldof": c.ld,
            "p": _ptr(wd["p"], GUARD), "B": c.B, "H": c.H, "N": c.N, "dh": 64, "scale": c.scale, "drop_p": float(p), "seed": int(seed)}


def fwd_call(a):
    rc = _lib().xvit_cls_xattn_fwd(a["q"], a["ldq"], a["qf"], a["ldqf"], a["k"], a["v"], a["sb"], a["sn"], a["o"], a["ldo"], a["of"], a["ldof"], a["p"], a["B"], a["H"], a["N"], a["dh"],
                                   a["scale"], a["drop_p"], a["seed"], _stream())
    torch.cuda.synchronize()
    return rc


def fwd_launch(c, st, qsel="f32", osel="both", drop=None):
    wd = {k: t.to(_dev()) for k, t in fwd_windows(c, osel).items()}
    rc = fwd_call(fwd_args(c, st, wd, qsel, drop))
    assert rc == 0, f"{c}: xvit_cls_xattn_fwd rc {rc}: {last_error()}"
    return {k: t.cpu() for k, t in wd.items()}


def bwd_args(c, st, wd):
    dkv = wd.get("dkv")
    return {"q": _ptr(st["qb"]), "ldq": c.ld, "k": _ptr(st["kv"][0], c.koff), "v": _ptr(st["kv"][-1], c.voff), "sb": c.sb, "sn": c.sn, "p": _ptr(st["p"]), "dO": _ptr(st["dO"]), "lddo": c.ld,
            "dq": _ptr(wd["dq"]), "lddq": c.ld, "dk": _ptr(dkv[0], c.koff) if dkv else None, "dv": _ptr(dkv[-1], c.voff) if dkv else None,
            "coef": _ptr(wd["coef"], GUARD) if "coef" in wd else None, "B": c.B, "H": c.H, "N": c.N, "dh": 64, "scale": c.scale, "drop_p": float(c.p), "seed": int(c.seed)}


def bwd_call(a):
    rc = _lib().xvit_cls_xattn_bwd(a["q"], a["ldq"], a["k"], a["v"], a["sb"], a["sn"], a["p"], a["dO"], a["lddo"], a["dq"], a["lddq"], a["dk"], a["dv"], a["coef"], a["B"], a["H"], a["N"],
                                   a["dh"], a["scale"], a["drop_p"], a["seed"], _stream())
    torch.cuda.synchronize()
    return rc


def _to_dev(w):
    return {k: [t.to(_dev()) for t in v] if isinstance(v, list) else v.to(_dev()) for k, v in w.items()}


def _to_cpu(w):
    return {k: [t.cpu() for t in v] if isinstance(v, list) else v.cpu() for k, v in w.items()}


def bwd_launch(c, st, sel="both"):
    wd = _to_dev(bwd_windows(c, sel))
    rc = bwd_call(bwd_args(c, st, wd))
    assert rc == 0, f"{c}: xvit_cls_xattn_bwd rc {rc}: {last_error()}"
    return _to_cpu(wd)


def same(c, what, a, b):
    for k in a:
        if k in b:
            for x, y in zip(*((a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]]))):
                assert torch.equal(_bits(x), _bits(y)), f"{c}: {k} differs in its bits between {what}"


def fwd_run(c, o, qsel="f32", variants=True, log=None):
    """One forward case on the device: the main launch (both outputs) checked against the tier's reference, then the launches that must give the same
    bits.  -> the saved p [B, H, N]."""
    keep = keep_mask(c) if c.p > 0 else None
    q = o["qb"] if qsel == "bf16" else o["q"]
    ora = fwd_oracle(c, q, o, keep)
    st = stage(c, o)
    wins0 = fwd_launch(c, st, qsel, drop=(0.0, 0)) if c.p > 0 else None
    wins = fwd_launch(c, st, qsel)
    fwd_check(c, o, wins, ora, wins0, log)
    if variants:
        same(c, "two launches", wins, fwd_launch(c, st, qsel))
        for osel in ("o", "of"):
            w = fwd_launch(c, st, qsel, osel)
            fwd_check(c, o, w, ora, wins0)
            same(c, f"the launch with both outputs and the one with {osel} only", wins, w)
        if qsel == "f32":
            same(c, "q_f32 alone and q together with q_f32", wins, fwd_launch(c, st, "both"))
    return gview(wins["p"]).reshape(c.B, c.H, c.N).clone()


def bwd_run(c, o, p, log=None):
    """One backward case on the device: dk, dv and coef together, each alone, and the first again."""
    keep = keep_mask(c) if c.p > 0 else None
    ora = bwd_oracle(c, o, p, keep)
    st = stage(c, o, p)
    wins = bwd_launch(c, st)
    coef = bwd_check(c, o, wins, ora, log=log)
    same(c, "two launches", wins, bwd_launch(c, st))
    for sel in ("dkv", "coef"):
        w = bwd_launch(c, st, sel)
        bwd_check(c, o, w, ora, coef=coef)
        same(c, f"the launch with dk, dv and coef and the one with {sel} only", wins, w)
    return wins
