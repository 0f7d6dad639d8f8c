"""Element-wise gate for LayerNorm (csrc/layernorm.hip) and the column sums (xvit_colsum, csrc/misc.hip): a float64 reference and a
per-element bound without a free tolerance.

The reference (`ln_ref`, `ln_bwd_ref`, `colsum_ref`) works in float64 on exactly the operands the device gets: the fp32 rows the kernel
reads (row k * seq_len from x_alt[k] when given), dy as the bf16 values, eps as the float32 that crosses the C ABI, and, for the backward,
the fp32 mean / rstd tensors that are HANDED to the kernel (it reads them, it does not recompute them; the tests feed it
float32(mu_ref), float32(rs_ref), so a forward error can neither hide in nor leak into the backward's verdict).  Next to every value
it returns the magnitude S that the value's fp32 round-off scales with:

  mean     S = mean_j |x_j|
  rstd     S = rs (1 + mean_j(|x_j - mu| (|x_j| + |mu|)) / (var + eps))       the variance sum's terms and mu's error carried into them
           + E = rs (C_mean 2^-24 S_mean)^2 / (2 (var + eps)), not multiplied by C_rstd: the square of mu's error in the variance
           (the term the float32 mirror itself needs on constant rows; |y - b| E / rs goes on top of y's bound in the same way)
  y        S = |g| rs (|x| + |mu| + S_mean) + |y - b| S_rstd / rs + |b|
  dx       S = rs32 (|a| + mean|a| + |h| mean|a h| + |m2| (|x| + |mu32|) rs32) + |dres|,   a = dy g, h = (x - mu32) rs32
           (the three terms cancel for constant dy g, where the exact dx is 0: hence the sum of magnitudes, not |dx|)
  column sums (dgamma, dbeta, dxsum, dressum, colsum)   S = |prefill| + sum over rows of |term|; a term of dxsum is the reference dx
           element and carries its own C_dx S_dx on top.

Gate.  fp32 outputs: |got - ref| <= C_k 2^-24 S with one constant per output kind, capped per element by the length of the summation
chain behind it (a row of V float4 per lane: 4 V + 6; a column: rows per wave + waves + blocks adding to the address).  bf16 outputs:
bit-equal to the round-to-nearest-even of the device's own fp32 tensor when the launch wrote both; inside [bf16(ref - B), bf16(ref + B)]
(B the fp32 bound; rounding is monotone) when only bf16 is written.  NaN / inf anywhere fails; the outputs are prefilled with NaN and
the padding between d and the row stride, and a guard row past the last one, must still be NaN afterwards.

Constants.  They come from the reference side, not from the kernel under test: the float32 CPU mirror below (the kernel's formulas in
float32: two-pass variance, plain torch sums, no device) runs over every content case at every width (tests/test_ln_gate_cpu.py,
257 rows each), its smallest passing constant per kind is the "mirror need", and C_k is the smallest power of two at or above 4 x the
largest mirror need (the 4 for summation order: the mirror adds pairwise, the kernel adds 4 V values per lane in sequence, then six
butterfly steps, and the column sums' atomics arrive in any order).  The device's needs (tests/test_layernorm_edges_gpu.py with
XVIT_MEASURE_LOG on an MI355X; profiles/ln_gate_measured.txt) are written next to them and set nothing.

Needs per case and output kind ("need" = the smallest constant that passes every element of every launch of the case; "worst" = the
largest error-to-bound ratio of any output of the case under the final constants; colsum = dgamma, dbeta, dressum, xvit_colsum):

  float32 CPU mirror, 257 rows, the largest over the 18 widths
  case                                 mean   rstd      y     dx colsum
  usual (mean 0.3, std 2)              1.64   1.56   1.57   2.56   1.13
  mean 100, std 0.5                    3.93   0.01   1.28   2.42   1.27
  mean -1000, std 1                    3.29   0.00   1.07   2.08   1.20
  std 1e-2                             1.70   1.40   1.52   2.68   1.21
  std 1e-3                             1.61   1.60   1.72   2.94   1.21
  constant rows                        7.80   1.05   2.60   2.70   0.95
  one row of 3e4 spikes                1.64   1.56   1.57   2.56   1.28
  colsum mirror (n 4 .. 3072, rows 1 .. 1026)                      2.31
  4 x the largest                      31.2   6.40   10.4   11.8   9.24
  C_k (power of two at or above)         32      8     16     16     16
  ceiling, 4 V + 6 (V = 3 / 4 / 16)      18 / 22 / 70 for the row kinds; rows per wave + waves + blocks + 1 for the column sums

  MI355X (tests/test_layernorm_edges_gpu.py; every line of the log in profiles/ln_gate_measured.txt)
  case                                 mean   rstd      y     dx colsum   worst
  widths, V = 3 (d <= 768)             1.79   1.08   1.03   2.02   1.40   0.13
  widths, V = 4 (d <= 1024)            0.67   1.10   1.34   1.92   1.19   0.14
  widths, V = 16 (d <= 4096)           0.66   1.09   1.40   2.25   1.37   0.14
  row counts 1 .. 16 393               0.80   1.19   1.41   2.46   3.40   0.42
  production, 64 638 x 768             0.85   1.16   1.29   2.60   0.25   0.16
  content: usual                       0.60   0.99   1.15   2.30   1.09   0.14
  content: mean 100                    2.40   0.01   0.80   1.80   0.89   0.13
  content: mean -1000                  2.11   0.00   0.70   1.75   0.92   0.12
  content: std 1e-2                    0.23   0.92   1.13   2.19   0.86   0.14
  content: std 1e-3                    0.27   1.38   1.43   2.51   0.84   0.17
  content: constant rows               1.99   0.92   0.66   2.02   0.73   0.13
  content: spikes                      0.60   0.99   1.15   2.30   1.26   0.14
  xvit_colsum (all n, rows, forms)        -      -      -      -   2.46   0.22

The device's largest needs are those of the mirror to within a factor of 1.5 (nothing was fitted to them); the largest ratio, 0.42,
is dgamma at 7 rows, where the chain caps the constant at 8 and the need is 3.40: the fp32 round-off of h = (x - mu) rs and of dy h,
which the mirror has too, plus the add to the prefilled value.  The rstd needs are those left after E; without E the mirror needs 48 on constant rows at eps = 1e-6.
"""
import math

import torch

from _util import note

EPS32 = 2.0 ** -24
C = {"mean": 32.0, "rstd": 8.0, "y": 16.0, "dx": 16.0, "colsum": 16.0}   # see the table above

LN_WAVES, LNB_WAVES = 8, 4          # layernorm.hip
WIDTHS = (4, 60, 192, 252, 256, 260, 764, 768, 772, 1020, 1024, 1028, 1536, 2048, 2052, 3072, 4092, 4096)
CONTENT = ("usual", "mean100", "mean-1000", "std1e-2", "std1e-3", "const", "spikes")


def pow2_at_or_above(v):
    return 2.0 ** math.ceil(math.log2(v))


def f32(v):
    """The float32 nearest to v, as a Python float (what a `float` argument of the C ABI carries)."""
    return float(torch.tensor(v, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------- the launch geometry
def v_of(d):
    """float4 per lane of the template instance that xvit_layernorm_fwd / _bwd dispatch d to."""
    return 3 if d <= 768 else (4 if d <= 1024 else 16)


def ln_fwd_grid(rows):
    return min(2048, (rows + LN_WAVES - 1) // LN_WAVES)


def ln_bwd_grid(rows):
    """layernorm.hip's ln_bwd_grid: at least 16 rows per block, at most 768 blocks."""
    return max(1, min(768, (rows + 4 * LNB_WAVES - 1) // (4 * LNB_WAVES)))


def colsum_rows_per_block(rows, n):
    """misc.hip's colsum_rows_per_block."""
    gx, rpb = (n // 4 + 63) // 64, 64
    while gx * ((rows + rpb - 1) // rpb) > 2048:
        rpb *= 2
    return rpb


def row_chain(d):
    return 4 * v_of(d) + 6


def ln_col_chain(rows):
    """Longest chain behind a dgamma / dbeta / dxsum / dressum element: the rows of one wave, the waves of a block, the blocks (and
    the value already in the vector)."""
    g = ln_bwd_grid(rows)
    return -(-rows // (g * LNB_WAVES)) + LNB_WAVES + g + 1


def colsum_chain(rows, n):
    """xvit_colsum: a thread adds every fourth row of its chunk into four accumulators (16-row main loop, 4-row tail), then the four
    accumulators, the four row groups, and the chunks (and the value already in the vector)."""
    rpb = colsum_rows_per_block(rows, n)
    return -(-min(rows, rpb) // 16) + 3 + 2 + 3 + -(-rows // rpb) + 1


# ---------------------------------------------------------------------------------------------------------------- inputs
def content(kind, rows, d, seed):
    """The row contents of the edge tests, fp32 [rows, d]."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(rows, d, generator=g)
    if kind == "usual":
        return n * 2 + 0.3
    if kind == "mean100":                # cancellation in the variance
        return n * 0.5 + 100.0
    if kind == "mean-1000":
        return n - 1000.0
    if kind == "std1e-2":                # variance at eps: eps decides the result
        return n * 1e-2
    if kind == "std1e-3":                # variance below eps
        return n * 1e-3
    if kind == "const":                  # variance exactly 0: rstd = eps^-1/2, dx from pure cancellation
        return (n[:, :1] * 2 + 0.3).expand(rows, d).contiguous()
    if kind == "spikes":                 # one row of 3e4-magnitude spikes among ordinary rows
        x = n * 2 + 0.3
        r = rows // 2
        x[r, ::37] = 3e4 * torch.sign(x[r, ::37])
        return x
    raise ValueError(kind)


def affine(d, seed):
    g = torch.Generator().manual_seed(seed)
    return 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)


def rows_read(x, x_alt=None, seq_len=0):
    """The rows the kernel reads: x, with row k * seq_len taken from x_alt[k] when x_alt is given."""
    r = x.clone()
    if x_alt is not None:
        idx = torch.arange(0, x.shape[0], seq_len)
        r[idx] = x_alt[:len(idx)].to(r.dtype)
    return r


# ---------------------------------------------------------------------------------------------------------------- reference
def ln_ref(x, x_alt, seq_len, gamma, beta, eps):
    """float64 LayerNorm of the rows the kernel reads -> dict of float64 tensors: rows, mu, var (biased), rs, y and the bound scales
    S_mean, S_rstd, S_y.  eps: the float32 value the kernel gets."""
    r = rows_read(x, x_alt, seq_len).double()
    g, b = gamma.double(), beta.double()
    mu = r.mean(-1)
    xc = r - mu[:, None]
    var = (xc * xc).mean(-1)
    rs = (var + eps) ** -0.5
    y = xc * rs[:, None] * g + b
    S_mean = r.abs().mean(-1)
    S_rstd = rs * (1 + (xc.abs() * (r.abs() + mu.abs()[:, None])).mean(-1) / (var + eps))
    S_y = g.abs() * rs[:, None] * (r.abs() + (mu.abs() + S_mean)[:, None]) + (y - b).abs() * (S_rstd / rs)[:, None] + b.abs()
    # second order, first seen in the float32 mirror on constant rows: with mu off by e every x - mu is off by e, the cross term
    # sum (x - mu) e vanishes and the variance grows by e^2 <= (C_mean 2^-24 S_mean)^2, i.e. rstd moves by rs e^2 / (2 (var + eps)):
    # nothing next to var + eps on ordinary rows, 40 x 2^-24 on a constant row of value 5 at eps = 1e-6.  In units of 2^-24:
    e = const_of("mean", row_chain(r.shape[1])) * S_mean
    E_rstd = rs * EPS32 * e * e / (2 * (var + eps))
    E_y = (y - b).abs() * (E_rstd / rs)[:, None]
    return {"rows": r, "mu": mu, "var": var, "rs": rs, "y": y, "S_mean": S_mean, "S_rstd": S_rstd, "S_y": S_y, "E_rstd": E_rstd, "E_y": E_y}


def ln_bwd_ref(dy, rows, mu32, rs32, gamma, dres=None):
    """float64 LayerNorm backward from the fp32 mean / rstd handed to the kernel.  dy: the bf16 values; rows: what the kernel reads
    (rows_read).  -> dx, dgamma, dbeta, dxsum, dressum (the sums WITHOUT any prefill) and their scales S_*; E_dxsum = sum of S_dx."""
    dy, r, g = dy.double(), rows.double(), gamma.double()
    mu, rs = mu32.double()[:, None], rs32.double()[:, None]
    a = dy * g
    h = (r - mu) * rs
    m1, m2 = a.mean(-1, keepdim=True), (a * h).mean(-1, keepdim=True)
    dx = rs * (a - m1 - h * m2)
    S_dx = rs * (a.abs() + a.abs().mean(-1, keepdim=True) + h.abs() * (a * h).abs().mean(-1, keepdim=True) + m2.abs() * (r.abs() + mu.abs()) * rs)
    out = {}
    if dres is not None:
        dr = dres.double()
        dx = dx + dr
        S_dx = S_dx + dr.abs()
        out["dressum"], out["S_dressum"] = dr.sum(0), dr.abs().sum(0)
    out.update({"dx": dx, "S_dx": S_dx, "dgamma": (dy * h).sum(0), "S_dgamma": (dy * h).abs().sum(0), "dbeta": dy.sum(0),
                "S_dbeta": dy.abs().sum(0), "dxsum": dx.sum(0), "S_dxsum": dx.abs().sum(0), "E_dxsum": S_dx.sum(0)})
    return out


def colsum_ref(x):
    x = x.double()
    return x.sum(0), x.abs().sum(0)


# ---------------------------------------------------------------------------------------------------------------- float32 CPU mirror
def ln_fwd_mirror(x, x_alt, seq_len, gamma, beta, eps, fault=None):
    """ln_fwd_kernel's formulas in float32 on the CPU (plain torch sums) -> (mean, rstd, y fp32).  fault: a planted defect."""
    if fault == "alt_ignored_seq1" and x_alt is not None:      # x_alt not used for the second sequence
        x_alt = x_alt.clone()
        x_alt[1] = x[seq_len]
    r = rows_read(x.float(), x_alt, seq_len)
    d = r.shape[1]
    inv_d = torch.tensor(1.0 / d, dtype=torch.float32)
    mu = r.sum(-1) * inv_d
    t = r - mu[:, None]
    ss = (t * t).sum(-1)
    if fault == "one_pass":
        var = (r * r).sum(-1) * inv_d - mu * mu
    elif fault == "var_dm1":
        var = ss * torch.tensor(1.0 / (d - 1), dtype=torch.float32)
    elif fault == "phantom":                                   # the zero columns of lanes past d counted as (0 - mu)^2
        var = (ss + (256 * v_of(d) - d) * mu * mu) * inv_d
    else:
        var = ss * inv_d
    e = {"no_eps": 0.0, "eps_1e-6": 1e-6}.get(fault, eps)
    rs = torch.rsqrt(var + torch.tensor(e, dtype=torch.float32))
    y = t * rs[:, None] * gamma.float() + beta.float()
    return mu, rs, y


def ln_bwd_mirror(dy, rows, mu32, rs32, gamma, dres=None, prefill=None, fault=None):
    """ln_bwd_kernel's formulas in float32 on the CPU -> dict dx, dgamma, dbeta, dxsum, dressum (added to prefill[name] when given)."""
    dy, r, g = dy.float(), rows.float(), gamma.float()
    mu, rs = mu32[:, None], rs32[:, None]
    d = r.shape[1]
    inv_d = torch.tensor(1.0 / d, dtype=torch.float32)
    a = dy * g
    h = (r - mu) * rs
    m1, m2 = a.sum(-1, keepdim=True) * inv_d, (a * h).sum(-1, keepdim=True) * inv_d
    if fault == "m2_dropped":
        m2 = torch.zeros_like(m2)
    dx = rs * (a - m1 - h * m2)
    out = {"dgamma": (dy * h).sum(0), "dbeta": dy.sum(0)}
    if dres is not None:
        dx = dx + dres.float()
        out["dressum"] = dres.float().sum(0)
    out["dx"] = dx
    out["dxsum"] = dx.sum(0) + (dres.float().sum(0) if fault == "dres_twice_in_dxsum" else 0.0)
    for name in ("dgamma", "dbeta", "dxsum", "dressum"):
        if prefill is not None and name in out and not (fault == "dgamma_stored" and name == "dgamma"):
            out[name] = out[name] + prefill[name]
    return out


def colsum_mirror(x, prefill=None, fault=None):
    x = x.float()
    if fault == "tail_rows_skipped":
        x = x[:x.shape[0] - x.shape[0] % 4]
    s = x.sum(0)
    return s + prefill if prefill is not None else s


def bf16_truncate(t):
    """fp32 -> bf16 by dropping the low 16 bits (the planted rounding fault)."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------- where
def where_row(row, col, d, rows, *, seq_len=0, bwd=False):
    """Where element (row, col) of a [rows, d] LayerNorm tensor sits in the kernels.  The block / wave / trip arithmetic repeats
    ln_grid / ln_bwd_grid and the row loops of layernorm.hip (forward: row = (block * 8 + wave) + trip * 8 grid; backward: row =
    (block * 4 + wave) + k * 4 grid, two rows k = 2 trip, 2 trip + 1 in flight per trip for d <= 1024, one for wider rows)."""
    c, nv, V = col // 4, d // 4, v_of(d)
    s = f"(row {row}, column {col})"
    if seq_len:
        s += ", a row from x_alt" if row % seq_len == 0 else ", a row from x"
    s += f": float4 {c} of nv = {nv} (lane {c % 64}, i = {c // 64} of V = {V}" + (", the last quad before nv)" if c == nv - 1 else ")")
    if bwd:
        g = ln_bwd_grid(rows)
        k, r = divmod(row, g * LNB_WAVES)
        trip = f"loop trip {k // 2}, {'second' if k % 2 else 'first'} row of its pair" if V <= 4 else f"loop trip {k}"
        return s + f"; backward block {r // LNB_WAVES} of {g}, wave {r % LNB_WAVES}, {trip}"
    g = ln_fwd_grid(rows)
    k, r = divmod(row, g * LN_WAVES)
    return s + f"; forward block {r // LN_WAVES} of {g}, wave {r % LN_WAVES}, grid-stride trip {k}"


def where_col(col, d):
    c, nv = col // 4, d // 4
    return (f"(column {col}): float4 {c} of nv = {nv} (lane {c % 64}, i = {c // 64}; colsum block x = {c // 64}, thread column {c % 64}"
            + (", the last quad before nv)" if c == nv - 1 else ")"))


class Loc:
    """Names an element of a [n, d] or per-row [n] tensor: row0 = the first row of a slab, rows = the launch's row count."""

    def __init__(self, rows, d, *, row0=0, seq_len=0, bwd=False):
        self.rows, self.d, self.row0, self.seq_len, self.bwd = rows, d, row0, seq_len, bwd

    def __call__(self, shape, flat):
        if len(shape) == 2:
            r, c = divmod(flat, shape[1])
            return where_row(self.row0 + r, c, self.d, self.rows, seq_len=self.seq_len, bwd=self.bwd)
        return where_row(self.row0 + flat, 0, self.d, self.rows, seq_len=self.seq_len, bwd=self.bwd).split(":")[0] + " (a per-row scalar)"


def col_loc(d):
    return lambda shape, flat: where_col(flat, d)


# ---------------------------------------------------------------------------------------------------------------- gate
def _ratio(err, bnd):
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp_min(1e-300))
    return torch.where(torch.isnan(ratio) | torch.isnan(err), torch.full_like(err, math.inf), ratio)


def const_of(kind, chain=None):
    return min(C[kind], float(chain)) if chain else C[kind]


def bound(kind, S, *, chain=None, extra=None):
    """The fp32 bound of an element: 2^-24 (C_kind S + extra), C_kind capped at the element's summation chain."""
    b = const_of(kind, chain) * S.double()
    if extra is not None:
        b = b + extra.double()
    return EPS32 * b


def ratio_of(kind, got, ref, S, *, chain=None, extra=None):
    """The worst error-to-bound ratio over all elements (inf where got is NaN), without failing."""
    g = got.detach().cpu().double()
    return float(_ratio((g - ref.double()).abs(), bound(kind, S, chain=chain, extra=extra)).max())


def need_of(got, ref, S, extra=None):
    """The smallest constant with which every element passes."""
    err = (got.detach().cpu().double() - ref.double()).abs()
    if extra is not None:
        err = (err - EPS32 * extra.double()).clamp_min(0)
    need = torch.where(err == 0, torch.zeros_like(err), err / (EPS32 * S.double()).clamp_min(1e-300))
    return float(torch.where(torch.isnan(need), torch.full_like(need, math.inf), need).max())


def check_f32(name, kind, got, ref, S, loc, *, chain=None, extra=None, log=None):
    """Fail when an element of the fp32 tensor `got` is NaN / inf or off `ref` by more than its bound; -> the worst ratio.
    log: a name under which the worst ratio and the constant the case needs go to XVIT_MEASURE_LOG."""
    g, r = got.detach().cpu().double(), ref.double()
    assert g.shape == r.shape, f"{name}: shape {tuple(g.shape)} != {tuple(r.shape)}"
    err = (g - r).abs()
    bnd = bound(kind, S, chain=chain, extra=extra)
    ratio = _ratio(err, bnd)
    worst = float(ratio.max())
    if log is not None:
        note(f"{log}:{name}:ratio", worst)
        note(f"{log}:{name}:need_{kind}", need_of(got, ref, S, extra))
    if worst > 1.0:
        bad = ratio > 1.0
        flat = int(ratio.reshape(-1).argmax())
        gv, rv, bv = float(g.reshape(-1)[flat]), float(r.reshape(-1)[flat]), float(bnd.reshape(-1)[flat])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements out of bound (C_{kind} = {const_of(kind, chain):g}), worst "
                             f"{worst:.3g}x its bound at {loc(tuple(g.shape), flat)}: got {gv!r}, float64 reference {rv!r}, bound {bv:.3g}")
    return worst


def check_bf16_copy(name, got, dev_f32, loc):
    """The bf16 tensor written next to an fp32 one by the same launch: bit-equal to that tensor's round-to-nearest-even."""
    g, f = got.detach().cpu(), dev_f32.detach().cpu()
    assert g.dtype == torch.bfloat16 and f.dtype == torch.float32 and g.shape == f.shape, f"{name}: dtype / shape"
    bad = (g.contiguous().view(torch.int16) != f.to(torch.bfloat16).contiguous().view(torch.int16)) | torch.isnan(g.float())
    if bool(bad.any()):
        flat = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} bf16 elements are not the round-to-nearest-even of the fp32 value the same "
                             f"launch wrote; first at {loc(tuple(g.shape), flat)}: bf16 {float(g.reshape(-1)[flat])!r}, fp32 {float(f.reshape(-1)[flat])!r}")


def _rne_bf16(t64):
    return t64.float().to(torch.bfloat16).double()      # float64 -> fp32 -> bf16, both monotone: the path a device fp32 value takes


def check_bf16_only(name, kind, got, ref, S, loc, *, chain=None, extra=None):
    """A bf16 output without an fp32 twin: inside [bf16(ref - B), bf16(ref + B)], B the fp32 bound."""
    g, r = got.detach().cpu().double(), ref.double()
    assert g.shape == r.shape, f"{name}: shape {tuple(g.shape)} != {tuple(r.shape)}"
    B = bound(kind, S, chain=chain, extra=extra)
    lo, hi = _rne_bf16(r - B), _rne_bf16(r + B)
    bad = ~((g >= lo) & (g <= hi))                       # NaN fails
    if bool(bad.any()):
        flat = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} bf16 elements outside [bf16(ref - B), bf16(ref + B)]; first at "
                             f"{loc(tuple(g.shape), flat)}: got {float(g.reshape(-1)[flat])!r}, float64 reference {float(r.reshape(-1)[flat])!r}, "
                             f"interval [{float(lo.reshape(-1)[flat])!r}, {float(hi.reshape(-1)[flat])!r}]")


def nan_buffer(rows, ld, dtype, device="cpu"):
    """[rows + 1, ld] of NaN: an output of `rows` rows with stride ld and a guard row behind it."""
    return torch.full((rows + 1, ld), math.nan, dtype=dtype, device=device)


def check_padding(name, buf, rows, d):
    """buf: the whole nan_buffer after the launch.  The columns past d of every row and the guard row must still be NaN."""
    b = buf.detach().cpu().float()
    pad = ~torch.isnan(b[:rows, d:])
    if bool(pad.any()):
        r, c = (int(v) for v in pad.nonzero()[0])
        raise AssertionError(f"{name}: {int(pad.sum())} elements of the padding between d = {d} and the row stride {b.shape[1]} were written; "
                             f"first at (row {r}, column {d + c}): {float(b[r, d + c])!r}")
    guard = ~torch.isnan(b[rows])
    assert not bool(guard.any()), f"{name}: {int(guard.sum())} elements of the row behind the last one (row {rows}) were written"


# ---------------------------------------------------------------------------------------------------------------- whole launches
def check_fwd(ref, d, rows, mean, rstd, yf=None, yb=None, *, row0=0, seq_len=0, log=None):
    """A forward launch (or the slab [row0, row0 + n) of one) against ln_ref's dict.  yf / yb: [n, d] views of the outputs."""
    loc = Loc(rows, d, row0=row0, seq_len=seq_len)
    ch = row_chain(d)
    w = check_f32("mean", "mean", mean, ref["mu"], ref["S_mean"], loc, chain=ch, log=log)
    w = max(w, check_f32("rstd", "rstd", rstd, ref["rs"], ref["S_rstd"], loc, chain=ch, extra=ref["E_rstd"], log=log))
    if yf is not None:
        w = max(w, check_f32("y_f32", "y", yf, ref["y"], ref["S_y"], loc, chain=ch, extra=ref["E_y"], log=log))
        if yb is not None:
            check_bf16_copy("y_bf16", yb, yf, loc)
    elif yb is not None:
        check_bf16_only("y_bf16", "y", yb, ref["y"], ref["S_y"], loc, chain=ch, extra=ref["E_y"])
    return w


def check_dx(ref, d, rows, dx, dxb=None, *, row0=0, seq_len=0, log=None):
    loc = Loc(rows, d, row0=row0, seq_len=seq_len, bwd=True)
    w = check_f32("dx", "dx", dx, ref["dx"], ref["S_dx"], loc, chain=row_chain(d), log=log)
    if dxb is not None:
        check_bf16_copy("dx_bf16", dxb, dx, loc)
    return w


def check_cols(ref, d, rows, got, prefill=None, *, log=None):
    """got: dict name -> fp32 [d] for any of dgamma, dbeta, dxsum, dressum; prefill: dict name -> what the vector held before."""
    w, ch = 0.0, ln_col_chain(rows)
    for name, t in got.items():
        p = prefill[name].double().cpu() if prefill is not None and name in prefill else torch.zeros(d, dtype=torch.float64)
        extra = const_of("dx", row_chain(d)) * ref["E_dxsum"] if name == "dxsum" else None
        w = max(w, check_f32(name, "colsum", t, ref[name] + p, ref["S_" + name] + p.abs(), col_loc(d), chain=ch, extra=extra, log=log))
    return w


def check_colsum(got, x, d, rows, prefill=None, *, log=None):
    """xvit_colsum's output against the float64 sum of x's values (+ what the vector held before when it accumulates)."""
    ref, S = colsum_ref(x)
    p = prefill.double().cpu() if prefill is not None else torch.zeros(d, dtype=torch.float64)
    return check_f32("colsum", "colsum", got, ref + p, S + p.abs(), col_loc(d), chain=colsum_chain(rows, d), log=log)
