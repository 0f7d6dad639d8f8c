"""Element-wise gate for the fused attention kernels (csrc/attention.hip): a float64 reference and a per-element bound.

The reference (`attn_ref`) works one (b, h) head at a time in float64 on the same bf16-rounded operands the device gets, so memory
stays at a few [N, N] float64 blocks (134 MB each at N = 4097).  For every output it also returns the scales of the per-element bound:

  T = sqrt(sum of the element's terms squared), e.g. T_o[i] = sqrt((P^2) @ (v^2))[i]: the kernels round P (forward, dV) and
      dS (dQ, dK) to bf16 before the second MFMA, an independent relative error of at most 2^-9 per term, and independent errors
      add like the root-sum-square of the terms, not like the sum of their magnitudes;
  S = sum of the magnitudes behind the element, carried through the same products: the fp32 round-off of the kernels' sums.
      dS = P (dP - delta) cancels (N = 1, constant V: the exact dq and dk are 0 and the kernel returns fp32 noise, because dP and
      delta are summed in different orders), so S of dS is P (|dO| |v| + |dO| . |o|); every P also carries the fp32 error of its
      exponent, relative 2^-24 E with E = 1 + scale |q| . |k| + |lse| (the magnitudes of the scores and of the max / lse subtracted).

`check_attn` fails an element when |got - ref| > a ulp_bf16(ref) + tau T + c 2^-24 S (lse, fp32: |got - ref| > c_lse 2^-24 (S + |lse| + 1)
with S = sum_j P E, an absolute-plus-relative fp32 bound), and names the worst element's (b, h, token, column), its 128-token
workgroup block and 32-row wave, its 64-row tile (tail or full) and, in the CLS-peel form, whether it is token 0 or a tiled token.

Calibration (tests/test_attn_edges_gpu.py on an MI355X with XVIT_MEASURE_LOG; "need" = the smallest constant that passes every
element of every case with the others held at their final values; "worst" = the largest error-to-bound ratio of any element):

  form                         need tau   need a   need c   need c_lse   worst
  grid (attn_peel 0 / 1)       7.68e-3    0.74     19.6     1.19         0.98
  grid, scale 4                3.78e-3    0.06     0.82     0.97         0.56
  grid, spikes (rescale)       6.74e-3    0.54     0.49     0.75         0.88
  grid, dropout                7.08e-3    0.32     0        0.87         0.91
  grid, dropout, scale 4       3.66e-3    0.06     0.12     0.79         0.52
  peel (attn_peel 2 / 1)       7.43e-3    0.40     16.0     1.15         0.95
  peel, scale 4                4.41e-3    0.16     0.82     1.00         0.63
  peel, spikes (rescale)       6.74e-3    0.36     0.32     0.73         0.88

So TAU = 2^-7 (7.81e-3: 1.02x the worst need, under the 2^-6 ceiling), C = 32 (1.6x), C_LSE = 2 (1.7x), and A = 1, the output's
own bf16 rounding (need 0.74).  The kernels' worst element is the bf16 rounding of P / dS at about 4 sigma of its root-sum-square
(2^-9 per term), as the model predicts; nothing needs more.
"""
import math

import torch

from _util import bf16_ulp, note, rt

A = 1.0              # bf16 ulps of the reference: the output's own rounding (half an ulp, an ulp across a binade edge)
TAU = 2.0 ** -7      # of T
C = 32.0             # of 2^-24 S (fp32 accumulation)
C_LSE = 2.0          # of 2^-24 (S_lse + |lse| + 1)
EPS32 = 2.0 ** -24

HEAD = 64


# ---------------------------------------------------------------------------------------------------------------- reference
def heads(t, B, N, H):
    """[B*N, H*64] (or [B, N, H*64]) -> [B, H, N, 64]."""
    return t.reshape(B, N, H, HEAD).permute(0, 2, 1, 3)


def unheads(t):
    """[B, H, N, 64] -> [B*N, H*64]."""
    B, H, N, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, H * HEAD)


def _head_ref(q, k, v, scale, mask, o_dev, dO):
    """One head in float64: q [Nq, 64], k / v [Nk, 64]; mask [Nq, Nk] (0 or 1/(1-p)) or None; o_dev / dO [Nq, 64] or None."""
    s = (q @ k.T) * scale
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    del s
    z = e.sum(-1, keepdim=True)
    lse = (m + torch.log(z)).squeeze(-1)
    P = e.div_(z)                                             # softmax (before dropout)
    E = (q.abs() @ k.abs().T).mul_(scale).add_(1.0).add_(lse.abs()[:, None])   # magnitude behind each exponent
    Pm = P * mask if mask is not None else P                  # the probabilities that reach P V
    r = {"lse": lse, "S_lse": (P * E).sum(-1)}
    PE = Pm * E
    r["o"] = Pm @ v
    r["T_o"] = ((Pm * Pm) @ (v * v)).sqrt()
    r["S_o"] = (Pm + PE) @ v.abs()
    if dO is None:
        return r
    dP = dO @ v.T
    if mask is not None:
        dP.mul_(mask)
    delta = (dO * o_dev).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    # S of dS: the fp32 sums dP and delta (magnitudes |dO| |v| and |dO| . |o|) and P's exponent error (relative 2^-24 E) times |dP - delta|
    absdp = dO.abs() @ v.abs().T
    if mask is not None:
        absdp.mul_(mask)
    SdS = P * (absdp + (dO.abs() * o_dev.abs()).sum(-1, keepdim=True) + (dP - delta).abs() * E)
    del absdp, dP
    dS2 = dS * dS
    r["dq"] = (dS @ k) * scale
    r["dk"] = (dS.T @ q) * scale
    r["dv"] = Pm.T @ dO
    r["T_dq"] = (dS2 @ (k * k)).sqrt() * scale
    r["T_dk"] = (dS2.T @ (q * q)).sqrt() * scale
    r["T_dv"] = ((Pm * Pm).T @ (dO * dO)).sqrt()
    r["S_dq"] = (SdS @ k.abs()) * scale
    r["S_dk"] = (SdS.T @ q.abs()) * scale
    r["S_dv"] = (Pm + PE).T @ dO.abs()
    return r


def attn_ref(q, k, v, scale, mask=None, o_dev=None, dO=None):
    """float64 attention and, given the DEVICE o (delta = rowsum(dO . o_dev), as the kernels compute it) and dO, its backward.
    q [B, H, Nq, 64], k / v [B, H, Nk, 64] (bf16-rounded values, any float dtype); mask [B, H, Nq, Nk] the exact dropout mask
    (0 or 1/(1-p)) or None.  Returns a dict of float64 CPU tensors: o, lse, T_o, S_o, S_lse and, with o_dev and dO, dq, dk, dv
    and their T_* / S_*.  One [N, N] head at a time; the forward and backward of a head share P."""
    B, H, Nq, _ = q.shape
    f = lambda t, b, h: None if t is None else t[b, h].detach().cpu().double()   # noqa: E731
    out = {}
    for b in range(B):
        for h in range(H):
            r = _head_ref(f(q, b, h), f(k, b, h), f(v, b, h), scale, f(mask, b, h), f(o_dev, b, h), f(dO, b, h))
            for name, t in r.items():
                if name not in out:
                    out[name] = torch.empty((B, H) + tuple(t.shape), dtype=torch.float64)
                out[name][b, h] = t
    return out


def attn_bwd_emulated(q, k, v, o_dev, do, lse, scale, mask=None):
    """The backward kernels' arithmetic on the CPU: P recomputed from the forward's lse, delta from the DEVICE o (bf16), and
    P / dS rounded to bf16 where they feed the second MFMA of their product (attention.hip: dV^T += dO^T P, dK^T += Q^T dS,
    dQ += dS K).  fp32 everywhere else.  mask: the dropout mask (0 or 1/(1-p)) on P V and on dP, or None."""
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.exp(s - lse[..., None])
    dp = do @ v.transpose(-1, -2)
    if mask is not None:
        dp = dp * mask
    delta = (do * o_dev).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dv = rt(p if mask is None else p * mask).transpose(-1, -2) @ do
    dk = rt(ds).transpose(-1, -2) @ q * scale
    dq = rt(ds) @ k * scale
    return dq, dk, dv


def online_softmax_emulated(q, k, v, scale, tile=64, skip_rescale=None, mask=None):
    """The forward kernel's arithmetic on the CPU in fp32: keys in 64-key tiles, P = exp(s - m_run) relative to the RUNNING max and
    rounded to bf16 before P V, l summed from the fp32 P, the accumulators rescaled whenever the max moves, o = acc / l.
    skip_rescale = (b, h, row, tile): a planted defect, that row's rescale skipped at that tile.  mask: the dropout mask, applied to P
    after the row sum.  -> (o fp32, lse fp32)."""
    q, k, v = q.float(), k.float(), v.float()
    Nk = k.shape[-2]
    shp = q.shape[:-1]
    m = torch.full(shp, -math.inf)
    l = torch.zeros(shp)
    acc = torch.zeros(q.shape)
    for t in range((Nk + tile - 1) // tile):
        s = (q @ k[..., t * tile:(t + 1) * tile, :].transpose(-1, -2)) * scale
        m_new = torch.maximum(m, s.amax(-1))
        alpha = torch.exp(m - m_new)
        if skip_rescale is not None and skip_rescale[3] == t:
            b, h, row = skip_rescale[:3]
            alpha[b, h, row] = 1.0
        m = m_new
        p = torch.exp(s - m[..., None])
        l = l * alpha + p.sum(-1)
        if mask is not None:
            p = p * mask[..., t * tile:(t + 1) * tile]
        acc = acc * alpha[..., None] + rt(p) @ v[..., t * tile:(t + 1) * tile, :]
    return acc / l[..., None], m + torch.log(l)


# ---------------------------------------------------------------------------------------------------------------- gate
def _where(shape, flat, layout):
    """(b, h, token, column) of element `flat` of a [B, H, N, 64] (or [B, H, N]) tensor and where it sits in the kernels' tiling.
    layout: "grid" (token 0 on the tile grid) or "peel" (the CLS-peel form: the tiles hold tokens 1 .. N-1)."""
    B, H, N = shape[:3]
    cols = shape[3] if len(shape) == 4 else 1
    b, rest = divmod(flat, H * N * cols)
    h, rest = divmod(rest, N * cols)
    n, col = divmod(rest, cols)
    s = f"(b {b}, h {h}, token {n}" + (f", column {col})" if len(shape) == 4 else ")")
    if layout == "peel" and n == 0:
        return s + ": token 0, off the tile grid in the peel form (initial state / post-loop block / merge kernel)"
    g = n - 1 if layout == "peel" else n
    ng = N - 1 if layout == "peel" else N
    tile, ntiles = g // 64, (ng + 63) // 64
    tail = ng % 64
    kind = f"the tail ({tail} rows)" if tile == ntiles - 1 and tail else "full"
    return (s + f": 128-token workgroup block {g // 128}, wave {(g % 128) // 32}, 64-row tile {tile} of {ntiles} ({kind})"
            + (", a tiled token of the peel form" if layout == "peel" else ""))


def bound(ref, T=None, S=None, *, a=A, tau=TAU, c=C, lse=False, c_lse=C_LSE):
    ref = ref.double()
    if lse:
        return c_lse * EPS32 * (S.double() + ref.abs() + 1.0)
    b = a * bf16_ulp(ref)
    if T is not None:
        b = b + tau * T.double()
    if S is not None:
        b = b + c * EPS32 * S.double()
    return b


def ratio_of(got, ref, T=None, S=None, **kw):
    """The worst ratio of |got - ref| to the bound over all elements (inf where got is NaN), without failing."""
    g, r = got.detach().cpu().double(), ref.double()
    err = (g - r).abs()
    ratio = err / bound(r, T, S, **kw).clamp_min(1e-300)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    return float(torch.where(torch.isnan(err), torch.full_like(err, math.inf), ratio).max())


def check_attn(name, got, ref, T=None, *, S=None, layout="grid", a=A, tau=TAU, c=C, lse=False, c_lse=C_LSE, log=None):
    """Fail when any element of `got` ([B, H, N, 64], or [B, H, N] for lse) is NaN or off `ref` by more than its bound (see the
    module docstring).  Returns the worst ratio of error to bound.  log: a name under which the worst ratio and the constants each
    case needs ("need_tau", "need_c", "need_a", "need_clse") go to XVIT_MEASURE_LOG."""
    g = got.detach().cpu().double()
    r = ref.double()
    assert g.shape == r.shape, f"{name}: shape {tuple(g.shape)} != {tuple(r.shape)}"
    err = (g - r).abs()
    bnd = bound(r, T, S, a=a, tau=tau, c=c, lse=lse, c_lse=c_lse)
    ratio = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err / bnd.clamp_min(1e-300))
    ratio = torch.where((err == 0), torch.zeros_like(ratio), ratio)
    worst = float(ratio.max())
    if log is not None:
        note(f"{log}:{name}:ratio", worst)
        if lse:
            note(f"{log}:{name}:need_clse", float((err / (EPS32 * (S.double() + r.abs() + 1.0))).max()))
        else:
            ulp = bf16_ulp(r)
            tT = tau * T.double() if T is not None else 0.0
            cS = c * EPS32 * S.double() if S is not None else 0.0
            if T is not None:
                need = ((err - a * ulp - cS).clamp_min(0) / T.double()).nan_to_num(0.0, posinf=0.0)
                note(f"{log}:{name}:need_tau", float(need.max()))
            if S is not None:
                need = ((err - a * ulp - tT).clamp_min(0) / (EPS32 * S.double())).nan_to_num(0.0, posinf=0.0)
                note(f"{log}:{name}:need_c", float(need.max()))
            need = ((err - tT - cS).clamp_min(0) / ulp).nan_to_num(0.0, posinf=0.0)
            note(f"{log}:{name}:need_a", float(need.max()))
    if worst > 1.0:
        bad = ratio > 1.0
        flat = int(ratio.reshape(-1).argmax())
        gv, rv, bv = float(g.reshape(-1)[flat]), float(r.reshape(-1)[flat]), float(bnd.reshape(-1)[flat])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements out of bound, worst {worst:.3g}x its bound at "
                             f"{_where(tuple(g.shape), flat, layout)}: got {gv!r}, float64 reference {rv!r}, bound {bv:.3g}")
    return worst


def check_fwd(ref, o, lse, *, layout="grid", log=None, **kw):
    """o [B, H, N, 64] and lse [B, H, N] of the device against attn_ref's dict; -> the worst ratio."""
    w = check_attn("o", o, ref["o"], ref["T_o"], S=ref["S_o"], layout=layout, log=log, **kw)
    return max(w, check_attn("lse", lse, ref["lse"], S=ref["S_lse"], lse=True, layout=layout, log=log, **kw))


def check_bwd(ref, dq, dk, dv, *, layout="grid", log=None, **kw):
    w = 0.0
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        w = max(w, check_attn(name, got, ref[name], ref["T_" + name], S=ref["S_" + name], layout=layout, log=log, **kw))
    return w
