"""Oracle, launchers and gate for the fp32 kernels of the single-token CLS path: xvit_linear_f32 (csrc/linear_f32.hip) and, in
csrc/misc.hip, xvit_small_linear_fwd / _bwd, xvit_mean_ce, xvit_cls_row_fwd and xvit_embed_bwd.

Launchers.  They go through the C entry points (_lib.load()) with every stride free.  A destination is a `window`: [rows + 1, ld]
of a fixed sentinel, NaN where the kernel must write; the padding columns and the guard row behind the last one are compared with
the sentinel bit for bit afterwards (`check_window`).  The padding of every INPUT is NaN, so a read past K or N poisons the result.
The split-K workspace is NaN, exactly xvit_linear_f32_workspace_bytes long, with sentinels behind it.

Mirror of the launch geometry.  `f32_split` / `k_per_split` repeat linear_f32.hip; every launch asserts that the library's workspace
query equals split * M * N * 4 of the mirror (0 at split 1), so the mirror cannot drift, and the test cases are picked by it
(`live_splits`: K = 400 at one tile gives six splits of 80 of which the last starts at K).

Exact tier (no tolerance).  Operands from _util.exact_operands / exact_grid: values in {-3..3} 2^-s, bias / residual / prefills on the
product grid; every partial sum stays below 2^24 units, so the fp32 sum is exact in any order and the float64 product, which
`lin_oracle` asserts to be representable in fp32, is THE result: y, z_bf16 (round-to-nearest-even of bias + product), y_bf16 (of the
stored y), small_linear_fwd, small_linear_bwd's dx (bf16 RNE) / dW / db, embed_bwd's sums, cls_row_fwd's single add.  Dropout keeps
the single fp32 product v * float32(1 / (1 - p)); with a residual behind it only p = 0.5 is exact whether or not the compiler
contracts the multiply-add (the scale 2 is exact), which `lin_oracle` enforces.

Float64 tier.
  random operands   |got - ref| <= (K + split_k + 4) 2^-24 S, S = m (sum_k |x w| + |bias|) + |residual| (m = the dropout factor of the
                    element, 0 or 1 / (1 - p)): the worst case of that many fp32 additions in any order (K products, the slab sum, bias,
                    scale, residual, store).  Derived, not measured; test_cls_gate_cpu.py checks that torch's own fp32 matmul stays
                    inside it on the inputs used.
  GELU  y           against float64 erf-GELU of the pre-activation v: m |v| (1.5e-7 / 2 + C_gelu 2^-24) + 2^-24 (m |gelu| + |y|):
                    the 1.5e-7 of the rational erf (xvit_common.h gelu_parts, Abramowitz-Stegun 7.1.26) halved by cdf = (1 + erf) / 2,
                    C_gelu for its fp32 evaluation, one rounding each for the dropout scale and the residual add.  With a
                    pre-activation that is itself only known to B_v (random operands): + m 1.13 B_v (max |gelu'| = 1.129) and
                    |v| + B_v in place of |v|.
  GELU' dx          small_linear_bwd with z: |acc| (1 + |z| pdf(z)) (1.5e-7 / 2 + C_dgelu 2^-24), acc = sum_n dy W exact on this
                    tier; dx exists only in bf16, so it must lie inside [bf16(ref - B), bf16(ref + B)].
  mean_ce           float64 on the fp32 inputs (label smoothing as the float32 that crosses the C ABI):
                      logits     S = mean_m |logits_m|
                      loss       S = mean_b sum_c tgt (|logit| + |lz|)               lz = log sum exp
                      dlogits_m  S = (p (1 + |logit| + |lz|) + tgt) / (B M)          expf's relative error grows with its argument's
                    each with its own constant: |got - ref| <= C 2^-24 S; dlogits_m + 2^-125 on top: a probability below the smallest
                    normal fp32 number 2^-126 (logits of +-80: e^-160) may be flushed to 0, and so may its quotient by B M.
  Every bound is multiplied by 1 + 2^-20 for the second-order terms of the first-order analysis.

Constants.  From the reference side, as in _ln_check.py: a float32 CPU mirror of the formulas (`gelu_parts_mirror`: gelu_parts with
an exact division and torch.exp; `ce_mirror`: the kernel's CE in float32 with torch sums) runs over the tests' own inputs
(tests/test_cls_gate_cpu.py); C is the smallest power of two at or above 4 x the mirror's largest need (the 4 for v_rcp_f32 / __expf
against the exact division / exp, and for the order of the sums).  The device's needs are logged (XVIT_MEASURE_LOG,
profiles/cls_path_gate_measured.txt) and set nothing.

  float32 CPU mirror, the largest need over the inputs named
  kind       inputs                                                                          need   4 x need     C
  gelu       v on the exact grid of the GELU cases of test_cls_path_gpu.py + the randn sites  4.46      17.8    32
  dgelu      z = bf16(1.5 randn), every (M, K) of the small_linear cases                      3.07      12.3    16
  ce_logits  the four contents, M 1..3, B 1..600, C 2 / 3 / 7                                 2.00       8.0     8
  ce_loss    same (the largest on equal logits: lz = 0.75 + log C, rounded twice)             3.16      12.6    16
  ce_dl      same                                                                             2.18       8.7    16
  MI355X (profiles/cls_path_gate_measured.txt, sets nothing): gelu 1.59, dgelu 0 (hidden below the bf16 store), ce 2.00 / 2.06 / 2.72
  per content: usual 2.00 / 1.59 / 2.11, equal 0.00 / 3.16 / 0.81, +-80 1.60 / 1.10 / 1.36, dominant 2.00 / 2.07 / 2.18
"""
import functools
import math

import torch

from _util import assert_exact, exact_grid, exact_operands, note

EPS32 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
ERF_ABS = 1.5e-7                      # |error| of the rational erf (xvit_common.h)
DGELU_MAX = 1.13                      # max |gelu'| = 1.1289
UNDERFLOW = 2.0 ** -125               # twice the smallest normal fp32 number
C = {"gelu": 32.0, "dgelu": 16.0, "ce_logits": 8.0, "ce_loss": 16.0, "ce_dl": 16.0}   # see the table above
SENT = -123456.0                      # exact in fp32 and bf16; nothing a kernel here computes
ACT_NONE, ACT_GELU = 0, 1
WS_GUARD = 64


def pow2_at_or_above(v):
    return 2.0 ** math.ceil(math.log2(v))


def f32(v):
    """The float32 nearest to v, as a Python float (what a `float` argument of the C ABI carries)."""
    return float(torch.tensor(v, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------- launch geometry
def f32_split(M, N, K):
    """linear_f32.hip's f32_split: ~1024 waves, at least 64 of K per wave, at most 32 splits."""
    tiles = ((M + 31) // 32) * ((N + 31) // 32)
    split = min(1024 // max(tiles, 1), K // 64, 32)
    return max(split, 1)


def k_per_split(K, split):
    return (((K + 15) // 16 + split - 1) // split) * 16


def live_splits(K, split):
    """How many of the splits start before K (the others write zero tiles to the slab)."""
    kps = k_per_split(K, split)
    return sum(1 for s in range(split) if s * kps < K)


def workspace_bytes(M, N, K):
    s = f32_split(M, N, K)
    return s * M * N * 4 if s > 1 else 0


def where32(M, N, K, row, col):
    """Where element (row, col) of y sits in linear_f32_kernel."""
    r, t = row % 32, None
    for i in range(16):
        for h in range(2):
            if (i & 3) + 8 * (i >> 2) + 4 * h == r:
                t = (i, h)
    return (f"32x32 tile ({row // 32}, {col // 32}) of ({(M + 31) // 32}, {(N + 31) // 32}), lane {col % 32 + 32 * t[1]}, accumulator {t[0]}, "
            f"split_k {f32_split(M, N, K)} x {k_per_split(K, f32_split(M, N, K))}")


# ---------------------------------------------------------------------------------------------------------------- windows
def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def window(rows, cols, ld, dtype=torch.float32, fill=math.nan):
    """[rows + 1, ld] of SENT with [:rows, :cols] = fill (NaN: must be written; a tensor: an accumulator's prefill)."""
    b = torch.full((rows + 1, ld), SENT, dtype=dtype)
    b[:rows, :cols] = fill
    return b


def check_window(name, buf, rows, cols):
    """buf: a window after the launch (CPU).  Padding columns and guard row must hold the sentinel, bit for bit."""
    buf = buf.detach().cpu()
    bad = _bits(buf) != _bits(torch.full_like(buf, SENT))
    bad[:rows, :cols] = False
    if bool(bad.any()):
        r, c = (int(v) for v in bad.nonzero()[0])
        where = f"the guard row behind the last one (row {rows})" if r == rows else f"the padding between column {cols} and the row stride {buf.shape[1]}"
        raise AssertionError(f"{name}: {int(bad.sum())} sentinel elements were overwritten; first in {where}, at (row {r}, column {c}): {float(buf[r, c])!r}")


def check_all_sentinel(name, buf):
    check_window(name, buf, 0, 0)


def padded(t, ld, dtype=None):
    """An input [rows, cols] inside a [rows, ld] buffer whose padding is NaN."""
    b = torch.full((t.shape[0], ld), math.nan, dtype=dtype or t.dtype)
    b[:, :t.shape[1]] = t
    return b


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- dropout mask
def hash_keep(M, N, p, seed, row_stride=None):
    """xvit_common.h hash32 + the threshold of xvit_dropout, in uint64 arithmetic on the CPU: keep[r, c] for element index
    r * row_stride + c (row_stride = N: the mask of xvit_dropout on a contiguous [M, N] tensor; no dropout epoch registered)."""
    import numpy as np
    rs = N if row_stride is None else row_stride
    idx = (np.arange(M, dtype=np.uint64)[:, None] * np.uint64(rs) + np.arange(N, dtype=np.uint64)[None, :])
    with np.errstate(over="ignore"):
        z = idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        h = ((z ^ (z >> np.uint64(31))) >> np.uint64(16)) & np.uint64(0xFFFFFFFF)
    thr = int(f32(f32(p) * 16777216.0))
    return torch.from_numpy(((h & np.uint64(0xFFFFFF)) >= np.uint64(thr)))


def device_keep(M, N, p, seed):
    """The mask of ops.dropout on a contiguous [M, N] tensor with this seed (what xvit_linear_f32 promises to reproduce)."""
    from xvit import ops
    return (ops.dropout(torch.ones(M, N, dtype=torch.float32, device=_dev()), p, seed) != 0).cpu()


def drop_inv(p):
    return torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------- GELU
def gelu64(v):
    v = v.double()
    return 0.5 * v * (1 + torch.erf(v / math.sqrt(2)))


def pdf64(v):
    v = v.double()
    return torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)


def dgelu64(v):
    v = v.double()
    return 0.5 * (1 + torch.erf(v / math.sqrt(2))) + v * pdf64(v)


def gelu_parts_mirror(x):
    """xvit_common.h gelu_parts in float32 on the CPU, with an exact division and torch.exp -> (cdf, pdf)."""
    x = x.float()
    one = torch.tensor(1.0, dtype=torch.float32)
    u = x.abs() * torch.tensor(0.70710678118654752, dtype=torch.float32)
    t = one / (torch.tensor(0.3275911, dtype=torch.float32) * u + one)
    e = torch.exp(-u * u)
    poly = torch.tensor(1.061405429, dtype=torch.float32) * t + torch.tensor(-1.453152027, dtype=torch.float32)
    for c in (1.421413741, -0.284496736, 0.254829592):
        poly = poly * t + torch.tensor(c, dtype=torch.float32)
    erf_abs = -poly * t * e + one
    cdf = torch.tensor(0.5, dtype=torch.float32) * (one + torch.copysign(erf_abs, x))
    return cdf, torch.tensor(0.39894228040143268, dtype=torch.float32) * e


def gelu_mirror(x):
    cdf, _ = gelu_parts_mirror(x)
    return x.float() * cdf


def dgelu_mirror(x):
    cdf, pdf = gelu_parts_mirror(x)
    return x.float() * pdf + cdf


def gelu_bound(v, c=None):
    """|gelu_f(v) - gelu(v)| for an fp32 v: |v| (ERF_ABS / 2 + C_gelu 2^-24)."""
    return v.double().abs() * (ERF_ABS / 2 + (C["gelu"] if c is None else c) * EPS32)


def gelu_need(got, v):
    """The smallest C_gelu with which got = gelu(v) passes gelu_bound everywhere."""
    err = (got.double() - gelu64(v)).abs() - v.double().abs() * ERF_ABS / 2
    need = err.clamp_min(0) / (EPS32 * v.double().abs()).clamp_min(1e-300)
    return float(torch.where(torch.isnan(need), torch.full_like(need, math.inf), need).max())


def dgelu_scale(z):
    return 1 + z.double().abs() * pdf64(z)


def dgelu_bound(acc, z, c=None):
    """|acc dgelu_f(z) - acc gelu'(z)|: |acc| (1 + |z| pdf(z)) (ERF_ABS / 2 + C_dgelu 2^-24)."""
    return acc.double().abs() * dgelu_scale(z) * (ERF_ABS / 2 + (C["dgelu"] if c is None else c) * EPS32)


def dgelu_need(got, z):
    """The smallest C_dgelu for got = gelu'(z) (acc = 1)."""
    err = (got.double() - dgelu64(z)).abs() - dgelu_scale(z) * ERF_ABS / 2
    need = err.clamp_min(0) / (EPS32 * dgelu_scale(z))
    return float(torch.where(torch.isnan(need), torch.full_like(need, math.inf), need).max())


def _rne_bf16(t64):
    return t64.float().to(torch.bfloat16).double()      # float64 -> fp32 -> bf16, both monotone


def check_bf16_only(name, got, ref, B):
    """A bf16 output without an fp32 twin: inside [bf16(ref - B), bf16(ref + B)] (rounding is monotone).  NaN fails."""
    g, r = got.detach().cpu().double(), ref.double()
    assert g.shape == r.shape, f"{name}: shape {tuple(g.shape)} != {tuple(r.shape)}"
    lo, hi = _rne_bf16(r - B), _rne_bf16(r + B)
    bad = ~((g >= lo) & (g <= hi))
    if bool(bad.any()):
        flat = int(bad.reshape(-1).nonzero()[0])
        row, col = divmod(flat, g.shape[-1])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} bf16 elements outside [bf16(ref - B), bf16(ref + B)]; first at (row {row}, col {col}): "
                             f"got {float(g.reshape(-1)[flat])!r}, float64 reference {float(r.reshape(-1)[flat])!r}, "
                             f"interval [{float(lo.reshape(-1)[flat])!r}, {float(hi.reshape(-1)[flat])!r}]")


def check_bound(name, got, ref, B, log=None):
    """|got - ref| <= B element-wise (NaN fails) -> the worst share of its bound any element used."""
    g, r = got.detach().cpu().double(), ref.double()
    assert g.shape == r.shape, f"{name}: shape {tuple(g.shape)} != {tuple(r.shape)}"
    err = (g - r).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / B.double().clamp_min(1e-300))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if log is not None:
        note(f"{log}:max_err_over_bound", worst)
    if worst > 1.0:
        flat = int(ratio.reshape(-1).argmax())
        row, col = divmod(flat, g.shape[-1]) if g.dim() >= 1 and g.shape[-1] else (0, 0)
        raise AssertionError(f"{name}: {int((ratio > 1).sum())} of {ratio.numel()} elements out of bound, worst {worst:.3g}x its bound at (row {row}, col {col}): "
                             f"got {float(g.reshape(-1)[flat])!r}, float64 reference {float(r.reshape(-1)[flat])!r}, bound {float(B.double().reshape(-1)[flat]):.3g}")
    return worst


# ---------------------------------------------------------------------------------------------------------------- xvit_linear_f32
class LinCase:
    """One launch of xvit_linear_f32.  tier "exact": operands on the exact grid; "random": randn operands (float64 tier)."""

    def __init__(self, M, N, K, *, bias=False, res=False, act=ACT_NONE, z=False, yb=False, p=0.0, seed=0, wide=False, tier="exact", name=""):
        self.M, self.N, self.K, self.bias, self.res, self.act, self.z, self.yb, self.p, self.seed, self.wide, self.tier = M, N, K, bias, res, act, z, yb, p, seed, wide, tier
        self.name = name or f"linear_f32 {M}x{N}x{K}"
        self.split = f32_split(M, N, K)

    def __repr__(self):
        epi = "+".join(n for n, on in (("bias", self.bias), ("gelu", self.act == ACT_GELU), ("z", self.z), (f"drop{self.p:g}", self.p > 0), ("res", self.res), ("bf16", self.yb)) if on)
        return f"{self.name} [{self.tier}, split {self.split} ({live_splits(self.K, self.split)} live), {epi or 'plain'}, {'wide strides + CLS-row view' if self.wide else 'packed'}]"

    def strides(self):
        M, N, K = self.M, self.N, self.K
        if self.wide:   # all different, x = the CLS rows of a [M, 3, K] tensor
            return {"ldx": 3 * K, "ldw": K + 8, "ldy": N + 3, "ldz": N + 5, "ldyb": N + 1, "ldr": N + 2}
        return {"ldx": K, "ldw": K, "ldy": N, "ldz": N, "ldyb": N, "ldr": N}


@functools.lru_cache(maxsize=None)
def _exact_w(N, K):
    return exact_operands((N, K), seed=1000 + 7 * N + K, s=3)


@functools.lru_cache(maxsize=None)
def _random_w(N, K):
    g = torch.Generator().manual_seed(2000 + 7 * N + K)
    return torch.randn(N, K, generator=g) * K ** -0.5


def lin_operands(c):
    """-> x [M, K], W [N, K], bias [N] | None, residual [M, N] | None (fp32, CPU)."""
    M, N, K = c.M, c.N, c.K
    if c.tier == "exact":   # x in {-3..3}/4, W in {-3..3}/8: products on the grid of 2^-5, |sum| <= 9 K units < 2^24
        x, W = exact_operands((M, K), seed=11 + M + 3 * K, s=2), _exact_w(N, K)
        b = exact_grid((N,), seed=12 + N, unit=2.0 ** -5, span=64) if c.bias else None
        r = exact_grid((M, N), seed=13 + M + N, unit=2.0 ** -5, span=200) if c.res else None
    else:
        g = torch.Generator().manual_seed(21 + M + 3 * K)
        x, W = torch.randn(M, K, generator=g), _random_w(N, K)
        b = torch.randn(N, generator=g) if c.bias else None
        r = torch.randn(M, N, generator=g) if c.res else None
    return x, W, b, r


def lin_oracle(c, x, W, b, r, keep):
    """-> dict: v (pre-activation, float64), Bv (its bound; 0 on the exact tier), y (float64), By (None: bit-exact), z (float64 | None).
    keep: bool [M, N] (p > 0) or None."""
    v = x.double() @ W.double().T
    S = x.double().abs() @ W.double().abs().T
    if b is not None:
        v, S = v + b.double(), S + b.double().abs()
    exact = c.tier == "exact"
    if exact:
        assert torch.equal(v.float().double(), v) and float(S.max()) * 2.0 ** 5 < 2.0 ** 24, "the exact tier's sums must be fp32 numbers"
    chain = (c.K + c.split + 4) * EPS32
    Bv = torch.zeros_like(v) if exact else chain * S * SLACK
    m = torch.ones_like(v)
    if c.p > 0:
        m = keep.double() * float(drop_inv(c.p))
    out = {"v": v, "Bv": Bv, "z": v if c.z else None, "m": m}
    if c.act == ACT_GELU:
        y = m * gelu64(v)
        By = m * (DGELU_MAX * Bv + gelu_bound(v.abs() + Bv)) + EPS32 * (m * gelu64(v).abs() + y.abs())
        if r is not None:
            y = y + r.double()
            By = By + EPS32 * r.double().abs()
        out["y"], out["By"] = y, By * SLACK
    elif exact:
        assert not (c.p > 0 and r is not None and c.p != 0.5), "dropout + residual is bit-exact only at p = 0.5"
        y = v.float()
        if c.p > 0:
            y = torch.where(keep, y * drop_inv(c.p), torch.zeros_like(y))     # one fp32 product
        if r is not None:
            y = y + r                                                        # exact: both on the grid (p = 0.5 doubles, exactly)
        out["y"], out["By"] = y.double(), None
    else:
        y = m * v + (r.double() if r is not None else 0.0)
        out["y"], out["By"] = y, chain * (m * S + (r.double().abs() if r is not None else 0.0)) * SLACK
    return out


def lin_windows(c):
    """The destinations before the launch -> dict name -> window."""
    s = c.strides()
    w = {"y": window(c.M, c.N, s["ldy"])}
    if c.z:
        w["z"] = window(c.M, c.N, s["ldz"], torch.bfloat16)
    if c.yb:
        w["yb"] = window(c.M, c.N, s["ldyb"], torch.bfloat16)
    n = workspace_bytes(c.M, c.N, c.K) // 4
    if n:
        w["ws"] = window(1, n, n + WS_GUARD)
    return w


def lin_launch(c, x, W, b, r, change=None):
    """Run the case on the device -> (rc, dict name -> window after the launch (CPU)).  change(args): edits the argument dict just
    before the call (the refusal tests)."""
    from xvit import _lib
    lib, dev, s = _lib.load(), _dev(), c.strides()
    M, N, K = c.M, c.N, c.K
    need = lib.xvit_linear_f32_workspace_bytes(M, N, K)
    assert need == workspace_bytes(M, N, K), f"{c}: the library wants {need} bytes of workspace, the mirror of f32_split says {workspace_bytes(M, N, K)}"
    if c.wide:
        tok = torch.full((M, 3, K), math.nan)
        tok[:, 0] = x
        xd = tok.to(dev)[:, 0]                 # the CLS-row view: row stride 3 K
    else:
        xd = x.contiguous().to(dev)
    assert xd.stride(0) == s["ldx"]
    Wd = padded(W, s["ldw"]).to(dev)
    bd = b.to(dev) if b is not None else None
    rd = padded(r, s["ldr"]).to(dev) if r is not None else None
    wd = {k: t.to(dev) for k, t in lin_windows(c).items()}
    ptr = lambda t: t.data_ptr() if t is not None else None
    a = {"x": ptr(xd), "ldx": s["ldx"], "W": ptr(Wd), "ldw": s["ldw"], "bias": ptr(bd), "y": ptr(wd["y"]), "ldy": s["ldy"], "M": M, "N": N, "K": K,
         "act": c.act, "z": ptr(wd.get("z")), "ldz": s["ldz"] if c.z else 0, "res": ptr(rd), "ldr": s["ldr"] if r is not None else 0,
         "yb": ptr(wd.get("yb")), "ldyb": s["ldyb"] if c.yb else 0, "p": float(c.p), "seed": int(c.seed), "ws": ptr(wd.get("ws")), "ws_bytes": need}
    if change is not None:
        change(a)
    rc = lib.xvit_linear_f32(a["x"], a["ldx"], a["W"], a["ldw"], a["bias"], a["y"], a["ldy"], a["M"], a["N"], a["K"], a["act"], a["z"], a["ldz"],
                             a["res"], a["ldr"], a["yb"], a["ldyb"], a["p"], a["seed"], a["ws"], a["ws_bytes"], _stream())
    torch.cuda.synchronize()
    return rc, {k: t.cpu() for k, t in wd.items()}


def lin_check(c, wins, ora, log=None):
    """The windows after a launch against the oracle: every element, every sentinel.  -> the worst share of a bound used (0: all exact)."""
    M, N = c.M, c.N
    worst = 0.0
    for k, t in wins.items():
        check_window(f"{c}: {k}", t, 1 if k == "ws" else M, t.shape[1] - WS_GUARD if k == "ws" else N)
    y = wins["y"][:M, :N]
    try:
        if ora["By"] is None:
            assert_exact(y, ora["y"].float(), f"{c}: y")
        else:
            worst = check_bound(f"{c}: y", y, ora["y"], ora["By"], log=f"{log}:y" if log else None)
        if c.z:
            if c.tier == "exact":
                assert_exact(wins["z"][:M, :N], ora["z"].float(), f"{c}: z_bf16")
            else:
                check_bf16_only(f"{c}: z_bf16", wins["z"][:M, :N], ora["z"], ora["Bv"])
        if c.yb:
            assert_exact(wins["yb"][:M, :N], y, f"{c}: y_bf16 against the y the same launch stored")
            if ora["By"] is None:
                assert_exact(wins["yb"][:M, :N], ora["y"].float(), f"{c}: y_bf16")
    except AssertionError as e:
        import re
        m = re.search(r"\(row (\d+), col (\d+)\)", str(e))
        raise AssertionError(str(e) + (f" | in linear_f32_kernel: {where32(M, N, c.K, int(m.group(1)), int(m.group(2)))}" if m else "")) from None
    if "ws" in wins:   # every live and every empty split's tile was written: no NaN left in the slab
        assert not bool(torch.isnan(wins["ws"][0, :wins["ws"].shape[1] - WS_GUARD]).any()), f"{c}: part of the split-K slab was never written"
    return worst


def lin_written(c, ora, keep=None):
    """The windows as a correct launch leaves them, built on the CPU from the oracle (the gate's own test plants faults in these).
    GELU cases: y from the float32 mirror of gelu_parts."""
    w = lin_windows(c)
    M, N = c.M, c.N
    if c.act == ACT_GELU:
        y = gelu_mirror(ora["v"].float())
        if c.p > 0:
            y = torch.where(keep, y * drop_inv(c.p), torch.zeros_like(y))
    else:
        y = ora["y"].float()
    w["y"][:M, :N] = y
    if c.z:
        w["z"][:M, :N] = ora["z"].float().to(torch.bfloat16)
    if c.yb:
        w["yb"][:M, :N] = y.to(torch.bfloat16)
    if "ws" in w:
        w["ws"][0, :w["ws"].shape[1] - WS_GUARD] = 0.0
    return w


def lin_run(c, log=None):
    """Operands, mask, launch, check: the whole case on the device.  -> (windows, oracle)."""
    x, W, b, r = lin_operands(c)
    keep = device_keep(c.M, c.N, c.p, c.seed) if c.p > 0 else None
    ora = lin_oracle(c, x, W, b, r, keep)
    rc, wins = lin_launch(c, x, W, b, r)
    assert rc == 0, f"{c}: rc {rc}: {last_error()}"
    lin_check(c, wins, ora, log=log)
    return wins, ora


def last_error():
    from xvit import _lib
    return _lib.load().xvit_last_error_string().decode()


# ---------------------------------------------------------------------------------------------------------------- small_linear
def small_operands(M, N, K, bias=True, with_z=False, tier="exact"):
    """-> dict x (bf16 [M, K]), W, b, dy (fp32), z (bf16 | None)."""
    if tier == "exact":
        x = exact_operands((M, K), seed=31 + M + K, s=2).to(torch.bfloat16)
        W = exact_operands((N, K), seed=32 + N + K, s=3)
        b = exact_grid((N,), seed=33 + N, unit=2.0 ** -5, span=64) if bias else None
        dy = exact_operands((M, N), seed=34 + M + N, s=2)
    else:
        g = torch.Generator().manual_seed(35 + M + N + K)
        x, W = torch.randn(M, K, generator=g).to(torch.bfloat16), torch.randn(N, K, generator=g) * K ** -0.5
        b = torch.randn(N, generator=g) if bias else None
        dy = torch.randn(M, N, generator=g)
    z = None
    if with_z:
        g = torch.Generator().manual_seed(36 + M + K)
        z = (1.5 * torch.randn(M, K, generator=g)).to(torch.bfloat16)
    return {"x": x, "W": W, "b": b, "dy": dy, "z": z}


def small_oracle(o):
    """float64 results of the forward and the backward (exact on the exact tier) and the magnitudes behind them."""
    x, W, dy = o["x"].double(), o["W"].double(), o["dy"].double()
    y = x @ W.T + (o["b"].double() if o["b"] is not None else 0.0)
    acc = dy @ W
    out = {"y": y, "S_y": x.abs() @ W.abs().T + (o["b"].double().abs() if o["b"] is not None else 0.0), "acc": acc, "S_acc": dy.abs() @ W.abs(),
           "dW": dy.T @ x, "S_dW": dy.abs().T @ x.abs(), "db": dy.sum(0), "S_db": dy.abs().sum(0)}
    out["dx"] = acc * dgelu64(o["z"].float()) if o["z"] is not None else acc
    return out


def small_windows(M, N, K, with_z):
    return {"y": window(1, M * N, M * N + WS_GUARD), "dx": window(M, K, K + 3, torch.bfloat16),
            "dW": window(1, N * K, N * K + WS_GUARD, fill=0.0), "db": window(1, N, N + WS_GUARD, fill=0.0)}


def small_launch(o, deterministic, change=None):
    """xvit_small_linear_fwd and _bwd on the device: x a strided view (ldx = K + 8), z with ldz = K + 2, dx with lddx = K + 3; dW / db
    zero-filled, as the contract says.  -> (rc_fwd, rc_bwd, windows after)."""
    from xvit import _lib
    lib, dev = _lib.load(), _dev()
    M, K = o["x"].shape
    N = o["W"].shape[0]
    xd = padded(o["x"], K + 8).to(dev)
    zd = padded(o["z"], K + 2).to(dev) if o["z"] is not None else None
    Wd, dyd = o["W"].contiguous().to(dev), o["dy"].contiguous().to(dev)
    bd = o["b"].to(dev) if o["b"] is not None else None
    wd = {k: t.to(dev) for k, t in small_windows(M, N, K, o["z"] is not None).items()}
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc_f = lib.xvit_small_linear_fwd(ptr(xd), K + 8, ptr(Wd), ptr(bd), ptr(wd["y"]), M, N, K, _stream())
    rc_b = lib.xvit_small_linear_bwd(ptr(dyd), ptr(xd), K + 8, ptr(Wd), ptr(zd), K + 2 if zd is not None else 0, ptr(wd["dx"]), K + 3, ptr(wd["dW"]), ptr(wd["db"]),
                                     M, N, K, int(deterministic), _stream())
    torch.cuda.synchronize()
    return rc_f, rc_b, {k: t.cpu() for k, t in wd.items()}


def small_check(name, o, wins, ora, tier="exact", log=None):
    M, K = o["x"].shape
    N = o["W"].shape[0]
    check_window(f"{name}: y", wins["y"], 1, M * N)
    check_window(f"{name}: dx", wins["dx"], M, K)
    check_window(f"{name}: dW", wins["dW"], 1, N * K)
    check_window(f"{name}: db", wins["db"], 1, N)
    y, dx = wins["y"][0, :M * N].reshape(M, N), wins["dx"][:M, :K]
    dW, db = wins["dW"][0, :N * K].reshape(N, K), wins["db"][0, :N]
    if tier == "exact":
        assert_exact(y, ora["y"].float(), f"{name}: y")
        assert_exact(dW, ora["dW"].float(), f"{name}: dW")
        assert_exact(db, ora["db"].float(), f"{name}: db")
        if o["z"] is None:
            assert_exact(dx, ora["dx"].float(), f"{name}: dx")
        else:
            check_bf16_only(f"{name}: dx = acc gelu'(z)", dx, ora["dx"], dgelu_bound(ora["acc"], o["z"].float()) * SLACK)
            if log is not None:   # dx exists only in bf16: the device's need is the smallest constant of this ladder whose interval holds every element
                note(f"{log}:need_dgelu_ladder", next(c for c in (0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0) if _dx_inside(dx, ora, o, c)))
    else:   # random operands: chains of K / 64 + 7 (a lane's fma chain, six butterfly steps, bias), N and M + 1 additions
        check_bound(f"{name}: y", y, ora["y"], (K // 64 + 8) * EPS32 * ora["S_y"] * SLACK, log=f"{log}:y" if log else None)
        check_bound(f"{name}: dW", dW, ora["dW"], (M + 2) * EPS32 * ora["S_dW"] * SLACK, log=f"{log}:dW" if log else None)
        check_bound(f"{name}: db", db, ora["db"], (M + 2) * EPS32 * ora["S_db"] * SLACK, log=f"{log}:db" if log else None)
        Bacc = (N + 1) * EPS32 * ora["S_acc"] * SLACK
        B = Bacc if o["z"] is None else Bacc * DGELU_MAX + dgelu_bound(ora["acc"].abs() + Bacc, o["z"].float()) * SLACK
        check_bf16_only(f"{name}: dx", dx, ora["dx"], B)


def _dx_inside(dx, ora, o, c):
    try:
        check_bf16_only("dx", dx, ora["dx"], dgelu_bound(ora["acc"], o["z"].float(), c) * SLACK)
        return True
    except AssertionError:
        return False


def small_written(o, ora):
    """The windows of a correct launch, from the oracle (exact tier; dx with z from the float32 mirror)."""
    M, K = o["x"].shape
    N = o["W"].shape[0]
    w = small_windows(M, N, K, o["z"] is not None)
    w["y"][0, :M * N] = ora["y"].float().reshape(-1)
    dx = ora["acc"].float() * dgelu_mirror(o["z"].float()) if o["z"] is not None else ora["dx"].float()
    w["dx"][:M, :K] = dx.to(torch.bfloat16)
    w["dW"][0, :N * K] = ora["dW"].float().reshape(-1)
    w["db"][0, :N] = ora["db"].float()
    return w


# ---------------------------------------------------------------------------------------------------------------- mean_ce
CE_CONTENT = ("usual", "equal", "pm80", "dominant")


def ce_inputs(kind, M, B, Cn, seed=0):
    """-> logits_m fp32 [M, B, C], labels int64 [B]."""
    g = torch.Generator().manual_seed(41 + seed + 100 * M + 10 * B + Cn)
    n = torch.randn(M, B, Cn, generator=g)
    labels = torch.randint(0, Cn, (B,), generator=g)
    if kind == "usual":
        lm = 2 * n
    elif kind == "equal":                  # softmax exactly uniform
        lm = torch.full((M, B, Cn), 0.75)
    elif kind == "pm80":                   # exp(80) = 5.5e34, exp(160) overflows: only the max subtraction keeps expf finite
        sign = torch.where(torch.randn(1, B, Cn, generator=g) > 0, 1.0, -1.0)
        lm = 80 * sign + 0.01 * n
    elif kind == "dominant":               # one class ahead by 30: the others' probabilities are 1e-13
        lm = n.clone()
        lm[:, torch.arange(B), torch.randint(0, Cn, (B,), generator=g)] += 30.0
    else:
        raise ValueError(kind)
    return lm.contiguous(), labels


def ce_ref(lm, labels, eps):
    """float64 on the fp32 inputs; eps: the float32 value the kernel gets -> dict of values and magnitudes."""
    M, B, Cn = lm.shape
    l64 = lm.double()
    logits = l64.mean(0)
    lz = torch.logsumexp(logits, -1, keepdim=True)
    logp = logits - lz
    tgt = torch.nn.functional.one_hot(labels, Cn).double() * (1.0 - eps) + eps / Cn
    loss = -(tgt * logp).sum(-1).mean()
    p = torch.exp(logp)
    dl = ((p - tgt) / (B * M)).expand(M, B, Cn)
    mag = logits.abs() + lz.abs()
    return {"logits": logits, "S_logits": l64.abs().mean(0), "loss": loss, "S_loss": (tgt * mag).sum(-1).mean(), "dl": dl,
            "S_dl": ((p * (1 + mag) + tgt) / (B * M)).expand(M, B, Cn)}


def ce_mirror(lm, labels, eps, fault=None):
    """mean_ce_kernel's formulas in float32 on the CPU (torch sums) -> logits, loss, dlogits_m."""
    M, B, Cn = lm.shape
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    logits = lm.float().sum(0) / t(float(M))
    mx = logits.max(-1, keepdim=True).values
    lz = mx + torch.log(torch.exp(logits - mx).sum(-1, keepdim=True))
    logp = logits - lz
    tgt = torch.nn.functional.one_hot(labels, Cn).float() * (t(1.0) - t(eps)) + t(eps) / t(float(Cn))
    loss = (-(tgt * logp).sum(-1)).sum() / t(float(B * M if fault == "loss_over_BM" else B))
    dl = ((torch.exp(logp) - tgt) / t(float(B * M))).expand(M, B, Cn).contiguous()
    return logits, loss, dl


def ce_needs(logits, loss, dl, ref):
    def need(got, r, S, under=0.0):
        err = ((got.double() - r).abs() - under).clamp_min(0)
        n = torch.where(err == 0, torch.zeros_like(err), err / (EPS32 * S).clamp_min(1e-300))
        return float(torch.where(torch.isnan(n), torch.full_like(n, math.inf), n).max())
    return {"ce_logits": need(logits, ref["logits"], ref["S_logits"]), "ce_loss": need(loss.reshape(()), ref["loss"], ref["S_loss"]),
            "ce_dl": need(dl, ref["dl"], ref["S_dl"], UNDERFLOW)}


def ce_windows(M, B, Cn):
    return {"logits": window(1, B * Cn, B * Cn + WS_GUARD), "loss": window(1, 1, 1 + WS_GUARD), "dl": window(1, M * B * Cn, M * B * Cn + WS_GUARD)}


def ce_launch(lm, labels, eps):
    from xvit import _lib
    lib, dev = _lib.load(), _dev()
    M, B, Cn = lm.shape
    lmd, lab = lm.to(dev), labels.to(dev)
    wd = {k: t.to(dev) for k, t in ce_windows(M, B, Cn).items()}
    rc = lib.xvit_mean_ce(lmd.data_ptr(), lab.data_ptr(), eps, wd["logits"].data_ptr(), wd["loss"].data_ptr(), wd["dl"].data_ptr(), M, B, Cn, _stream())
    torch.cuda.synchronize()
    return rc, {k: t.cpu() for k, t in wd.items()}


def ce_check(name, wins, ref, M, B, Cn, log=None):
    check_window(f"{name}: logits", wins["logits"], 1, B * Cn)
    check_window(f"{name}: loss", wins["loss"], 1, 1)
    check_window(f"{name}: dlogits_m", wins["dl"], 1, M * B * Cn)
    logits, loss, dl = wins["logits"][0, :B * Cn].reshape(B, Cn), wins["loss"][0, 0], wins["dl"][0, :M * B * Cn].reshape(M, B, Cn)
    if log is not None:
        for k, v in ce_needs(logits, loss, dl, ref).items():
            note(f"{log}:need_{k}", v)
    w = check_bound(f"{name}: logits", logits, ref["logits"], C["ce_logits"] * EPS32 * ref["S_logits"] * SLACK)
    w = max(w, check_bound(f"{name}: loss", loss.reshape(1), ref["loss"].reshape(1), (C["ce_loss"] * EPS32 * ref["S_loss"] * SLACK).reshape(1)))
    w = max(w, check_bound(f"{name}: dlogits_m", dl.reshape(M * B, Cn), ref["dl"].reshape(M * B, Cn), (C["ce_dl"] * EPS32 * ref["S_dl"] * SLACK + UNDERFLOW).reshape(M * B, Cn)))
    for m in range(1, M):
        bad = _bits(dl[m]) != _bits(dl[0])
        if bool(bad.any()):
            b, c = (int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{name}: dlogits_m copy {m} differs from copy 0 in {int(bad.sum())} elements; first at (sample {b}, class {c}): "
                                 f"{float(dl[m, b, c])!r} != {float(dl[0, b, c])!r}")
    return w


def ce_written(lm, labels, eps, fault=None):
    M, B, Cn = lm.shape
    logits, loss, dl = ce_mirror(lm, labels, eps, fault=fault)
    w = ce_windows(M, B, Cn)
    w["logits"][0, :B * Cn] = logits.reshape(-1)
    w["loss"][0, 0] = loss
    w["dl"][0, :M * B * Cn] = dl.reshape(-1)
    return w


# ---------------------------------------------------------------------------------------------------------------- cls_row / embed_bwd
def embed_inputs(MB, N, d):
    """cls, pos (random fp32: cls_row_fwd is one fp32 add), two dx tensors and the dpos / dcls prefills on the exact grid."""
    g = torch.Generator().manual_seed(51 + MB + N + d)
    return {"cls": torch.randn(d, generator=g), "pos": torch.randn(N, d, generator=g),
            "dx": [exact_grid((MB, N, d), seed=52 + k + MB + N + d, unit=2.0 ** -6, span=300) for k in range(2)],
            "dpos0": exact_grid((N, d), seed=54 + N + d, unit=2.0 ** -6, span=500), "dcls0": exact_grid((1, d), seed=55 + d, unit=2.0 ** -6, span=500)}


def embed_oracle(e):
    dx = e["dx"][0].double() + e["dx"][1].double()
    return {"x0": e["cls"] + e["pos"][0], "dpos": (e["dpos0"].double() + dx.sum(0)).float(), "dcls": (e["dcls0"].double() + dx[:, 0].sum(0, keepdim=True)).float()}


def embed_windows(e, MB, N, d):
    x = window(MB, N * d, N * d)                     # [MB + 1, N d]: row 0 of every sample NaN, rows 1.. sentinel
    x[:MB, d:] = SENT
    return {"x": x, "dpos": window(N, d, d, fill=e["dpos0"]), "dcls": window(1, d, d, fill=e["dcls0"])}


def embed_launch(e, MB, N, d):
    from xvit import _lib
    lib, dev = _lib.load(), _dev()
    wd = {k: t.to(dev) for k, t in embed_windows(e, MB, N, d).items()}
    cls, pos = e["cls"].to(dev), e["pos"].to(dev)
    rc = [lib.xvit_cls_row_fwd(cls.data_ptr(), pos.data_ptr(), wd["x"].data_ptr(), MB, N, d, _stream())]
    for dx in e["dx"]:                               # twice into the same dpos / dcls, as PatchEmbedFn's per-modality backward does
        dxd = dx.contiguous().to(dev)
        rc.append(lib.xvit_embed_bwd(dxd.data_ptr(), wd["dpos"].data_ptr(), wd["dcls"].data_ptr(), MB, N, d, _stream()))
        torch.cuda.synchronize()
    return rc, {k: t.cpu() for k, t in wd.items()}


def embed_check(name, wins, ora, MB, N, d):
    check_window(f"{name}: x (rows 1.. of every sample and the guard row)", wins["x"], MB, d)
    check_window(f"{name}: dpos", wins["dpos"], N, d)
    check_window(f"{name}: dcls", wins["dcls"], 1, d)
    assert_exact(wins["x"][:MB, :d], ora["x0"].expand(MB, d), f"{name}: CLS rows = cls + pos[0]")
    assert_exact(wins["dpos"][:N], ora["dpos"], f"{name}: dpos")
    assert_exact(wins["dcls"][:1], ora["dcls"], f"{name}: dcls")
