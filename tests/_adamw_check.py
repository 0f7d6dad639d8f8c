"""Oracle, float32 mirror, launchers and gate for the AdamW kernels (csrc/misc.hip: adam_kernel<FROM_RECORD, ADAM_COUPLED | ADAM_DECOUPLED>, ema_swap_kernel;
xvit_adamw_step, xvit_adamw_step_dev, xvit_ema_swap), in the manner of _optim_check.py, whose arenas, sentinels, NaN guards behind g,
`where`, SIZES, operands and bounds are reused.

Arenas.  One more arena kind, `e` (the average), laid out like p / m / v with sentinel guards.  EMA modes: "none" (every extras row has
ema = NULL), "all", "alternate" (tensors 0, 2, 4, ... have one).  A tensor without an average still owns its slot of the `e` arena, which
then holds the sentinel throughout and is compared as a guard: an average written for the neighbour of a null-ema tensor shows there.
Placements: those of _optim_check with the average 16-byte aligned, and "ema 4 bytes off", which must select the scalar path (with an
average; without one the pointer is NULL and the 16-byte path stays).  `vec_ok` mirrors adam_vec_ok(t, ema) and every launch asserts it.

Per-tensor numbers.  Every tensor t has its own lr_scale s_t and weight decay wd_t (`HyperW.scales`, `.wds`, cycled over the tensors, 0
among both).  Uniform per tensor, formed in fp32: a = fl(L s_t), lr_t = fl(lr s_t) with L = lr / bc1 as the host computes it in double.

Exact tier.  _optim_check's exact operands, e on the same grid; s_t, wd_t, grad_scale powers of two (or 0), betas (0.5, 0.75), w in
{0.5, 0.25, 1}.  The oracle asserts in float64 that g s, wd p, g^, both products and the sum of each moment are fp32 numbers: m and v match
bit for bit.  e matches bit for bit wherever p' - e and w (p' - e) are fp32 numbers (p' the p the launch stored): the sum e + w d is then
rounded once, contracted or not.

Float64 tier (u = 2^-24, every bound times 1 + 2^-20).  _optim_check's B_g, B_m, B_v and T and the form of B_p are kept, with
  a = L s_t           one rounding more on upd: B_p has (C_u + 1) u |upd| in place of C_u u |upd|; the reference forms a in float64
  decay (decoupled)   p_d = p (1 - lr_t wd_t): lr_t = fl(lr s), x = fl(lr_t wd), F = fl(1 - x), fl(p F): with x the float64 product and
                      F = 1 - x,  B_d = |p| u (2 x + 2 |F|): two relative roundings on x, one on F, one on the product.  A contracted
                      1 - lr_t wd or p F only removes roundings.  The Adam part then starts from p_d: B_p = u |p'| + (C_u + 1) u |upd| + T + B_d.
  C_u is not counted but taken from the float32 CPU mirror (`adamw_mirror`) over the GPU tests' own inputs: the power of two at or above
  4 x the mirror's largest need of it, `C_UPD` (tests/test_adamw_gate_cpu.py re-derives it from the mirror and compares it with this
  table); the device's need is logged and sets nothing.

  float32 CPU mirror, largest need over every hyper-parameter set of `hypers`, both modes, every EMA mode
  kind        need          4 x need   C
  upd_exact   1.37 .. 1.46  below 8    8     (C_u.  The last digits of the need follow the host's libm and CPU: 1.37 and 1.46 were seen)
  upd_random  0.00          0.0        -     (T covers the mirror; C_u = 8 is used here too)
  ema         0.00          0.0        -     (the three counted roundings cover the mirror: no constant)

EMA.  Reference: float64 of e + w (p'_stored - e) with p'_stored the p the SAME launch stored.  Three roundings: the difference d, the
product w d, the sum: B_e = u (2 |w d| + |e'|).  By value w is exact.  From the record the kernel forms w = 1 - min(decay, (1 + t) / (10 + t))
in fp32: two sums, a quotient and a difference: the reference takes w in float64 from the fp32 decay and
B_e += |d| u (3 q + w), q the quotient.  Without warm-up w = fl(1 - decay): B_e += |d| u w.

Shadow.  Bit-exact round-to-nearest-even bf16 of the stored p on every tier and path, also after xvit_ema_swap."""
import bisect
import math

import numpy as np
import torch

import _optim_check as X
from _optim_check import CHUNK, EPS32, GUARD, SENT, SIZES, SLACK, _bits, f32
from _util import exact_grid, note

C_A = 1.0                              # the rounding of a = L s_t, counted
C_UPD = 8.0                            # C_u, see the table above
KEYS = ("p", "g", "m", "v", "sh", "e")
EXTRA = np.dtype([("ema", "<u8"), ("lr_scale", "<f4"), ("weight_decay", "<f4")])     # xvit_adamw_extra
assert EXTRA.itemsize == 16

PLACEMENTS = {k: dict(v, e=0) for k, v in X.PLACEMENTS.items()}
PLACEMENTS["ema 4 bytes off"] = dict(p=0, g=0, m=0, v=0, sh=0, e=1, vec=False)
EMA_MODES = ("none", "all", "alternate")


def vec_ok(p, g, m, v, sh, ema):
    """adam_vec_ok(t, ema) on byte addresses (sh / ema = 0: none)."""
    return X.vec_ok(p, g, m, v, sh) and (ema & 15) == 0


class HyperW:
    def __init__(self, base, decoupled, scales, wds, w=1.0, ema_decay=None, warmup=0):
        self.lr, self.b1, self.b2, self.eps, self.step, self.scale = base.lr, base.b1, base.b2, base.eps, base.step, base.scale
        self.decoupled, self.scales, self.wds, self.w, self.ema_decay, self.warmup = bool(decoupled), tuple(scales), tuple(wds), w, ema_decay, warmup

    def __repr__(self):
        return (f"{'decoupled' if self.decoupled else 'coupled'} lr {self.lr:g} betas ({self.b1:g}, {self.b2:g}) eps {self.eps:g} step {self.step} scale {self.scale:g} "
                f"lr_scale {self.scales} wd {self.wds} " + (f"w {self.w:g}" if self.ema_decay is None else f"ema_decay {self.ema_decay:g} warmup {self.warmup}"))

    def per_tensor(self, n):
        return [f32(self.scales[t % len(self.scales)]) for t in range(n)], [f32(self.wds[t % len(self.wds)]) for t in range(n)]

    def weight(self):
        """-> (w as the kernel's fp32 number or its float64 reference, allowance on w in units of u)."""
        if self.ema_decay is None:
            return f32(self.w), 0.0
        d = f32(self.ema_decay)
        if not self.warmup:
            return 1.0 - d, 1.0 - d
        q = (1.0 + self.step) / (10.0 + self.step)
        return (1.0 - min(d, q)), 3.0 * q + (1.0 - min(d, q))

    def weight32(self):
        """The kernel's own fp32 arithmetic for w (the mirror)."""
        if self.ema_decay is None:
            return np.float32(self.w)
        d = np.float32(self.ema_decay)
        if self.warmup:
            t = np.float32(self.step)
            d = min(d, (np.float32(1) + t) / (np.float32(10) + t))
        return np.float32(1) - d


SCALES_R, WDS_R = (1.0, 0.75, 0.31640625, 0.0, 1.5, 0.1), (0.05, 0.0, 0.01, 0.3)
SCALES_E, WDS_E = (1.0, 0.5, 0.25, 0.0, 2.0), (2.0 ** -4, 0.0, 2.0 ** -3)     # a smaller decay would push v' below the fp32 grid


def hypers(tier, decoupled):
    """_optim_check's HYPER_* sets extended by per-tensor scales and decays (all decays 0 where the base set has wd = 0) and a by-value w."""
    base, sc, wd, ws = (X.HYPER_EXACT, SCALES_E, WDS_E, (0.5, 0.25, 1.0)) if tier == "exact" else (X.HYPER_RANDOM, SCALES_R, WDS_R, (0.1, 1e-4, 1.0, 0.0))
    return [HyperW(b, decoupled, sc[i % 3:] + sc[:i % 3], wd if b.wd else (0.0,), w=ws[i % len(ws)]) for i, b in enumerate(base)]


# ---------------------------------------------------------------------------------------------------------------- the case
_E_OPERANDS = {}


def ema_operand(tier, sizes):
    key = (tier, tuple(sizes))
    if key not in _E_OPERANDS:
        N = sum(sizes)
        _E_OPERANDS[key] = exact_grid((N,), seed=76, unit=2.0 ** -6, span=64) if tier == "exact" else torch.randn(N, generator=torch.Generator().manual_seed(77))
    return _E_OPERANDS[key]


class Case(X.AdamCase):
    """One launch: X.AdamCase plus the `e` arena and the EMA mode."""

    def __init__(self, placement, tier, ema="all", sizes=SIZES, order="natural"):
        self.placement, self.tier, self.sizes, self.ema = placement, tier, tuple(sizes), ema
        pl = PLACEMENTS[placement]
        self.has_shadow = pl["sh"] is not None
        self.has_ema = [ema == "all" or (ema == "alternate" and t % 2 == 0) for t in range(len(self.sizes))]
        base_ok = X.vec_ok(*(4 * pl[k] for k in "pgmv"), 0 if pl["sh"] is None else 2 * pl["sh"])
        self.vec_t = [base_ok and (pl["e"] == 0 or not has) for has in self.has_ema]        # the path is chosen per tensor: a NULL average constrains nothing
        self.expect_vec = all(self.vec_t)
        self.offsets = [0]
        for n in self.sizes:
            self.offsets.append(self.offsets[-1] + n)
        self.N = self.offsets[-1]
        self.starts, self.total, self.pos = {}, {}, {}
        for k in KEYS:
            if k == "sh" and not self.has_shadow:
                continue
            self.starts[k], self.total[k] = X.layout(self.sizes, pl[k], 8 if k == "sh" else 4)
            self.pos[k] = torch.cat([torch.arange(s, s + n) for s, n in zip(self.starts[k], self.sizes)])
        allc = [(t, c) for t, n in enumerate(self.sizes) for c in range(X.n_chunks(n))]
        if order == "natural":
            self.chunks = allc
        elif order == "shuffled":
            self.chunks = [allc[i] for i in torch.randperm(len(allc), generator=torch.Generator().manual_seed(5)).tolist()]
        else:
            self.chunks = list(order)
        self.listed = torch.zeros(self.N, dtype=torch.bool)
        for t, c in self.chunks:
            self.listed[self.offsets[t] + c * CHUNK: self.offsets[t] + min((c + 1) * CHUNK, self.sizes[t])] = True
        self.with_e = torch.cat([torch.full((n,), h, dtype=torch.bool) for n, h in zip(self.sizes, self.has_ema)])
        self.vec = self.expect_vec

    def __repr__(self):
        return f"adamw [{self.placement}; ema {self.ema}; {self.tier} tier; {len(self.sizes)} tensors, {len(self.chunks)} chunks]"

    def locate(self, e):
        t = bisect.bisect_right(self.offsets, e) - 1
        return f"tensor {t} (n = {self.sizes[t]}), " + X.where(self.sizes[t], e - self.offsets[t], self.vec_t[t])

    def arenas(self):
        o = X.adam_operands(self.tier, self.sizes)
        a = {}
        for k in self.starts:
            if k == "sh":
                a[k] = torch.full((self.total[k],), SENT, dtype=torch.bfloat16)
                a[k][self.pos[k]] = o["p"].to(torch.bfloat16)
            elif k == "e":
                a[k] = torch.full((self.total[k],), SENT, dtype=torch.float32)
                a[k][self.pos[k][self.with_e]] = ema_operand(self.tier, self.sizes)[self.with_e]
            else:
                a[k] = torch.full((self.total[k],), math.nan if k == "g" else SENT, dtype=torch.float32)
                a[k][self.pos[k]] = o[k]
        return a

    def extras(self, base_e, h):
        sc, wd = h.per_tensor(len(self.sizes))
        x = np.zeros(len(self.sizes), dtype=EXTRA)
        x["ema"] = [base_e + 4 * self.starts["e"][t] if self.has_ema[t] else 0 for t in range(len(self.sizes))]
        x["lr_scale"], x["weight_decay"] = sc, wd
        return x

    def per_element(self, h):
        sc, wd = h.per_tensor(len(self.sizes))
        rep = torch.tensor(self.sizes)
        return torch.tensor(sc, dtype=torch.float64).repeat_interleave(rep), torch.tensor(wd, dtype=torch.float64).repeat_interleave(rep)


# ---------------------------------------------------------------------------------------------------------------- oracle and mirror
def oracle(case, h):
    """float64 on the fp32 operands -> dict m, v, p, upd and the bounds Bm, Bv, T, Bd."""
    o = X.adam_operands(case.tier, case.sizes)
    p, g, m, v = (o[k].double() for k in "pgmv")
    sc, wd = case.per_element(h)
    s, b1, b2, eps = f32(h.scale), f32(h.b1), f32(h.b2), f32(h.eps)
    omb1, omb2 = float(np.float32(1) - np.float32(h.b1)), float(np.float32(1) - np.float32(h.b2))
    L, I = X.host_numbers(h)
    gs = g * s
    if h.decoupled:
        x = f32(h.lr) * sc * wd
        F = 1.0 - x
        Bd = p.abs() * EPS32 * (2 * x + 2 * F.abs()) * SLACK
        p0, wp = p * F, torch.zeros_like(p)
    else:
        Bd, p0, wp = torch.zeros_like(p), p, wd * p
    gh = gs + wp
    m1 = b1 * m + omb1 * gh
    v1 = b2 * v + omb2 * gh * gh
    if case.tier == "exact":
        for name, t in (("g s", gs), ("wd p", wp), ("g^", gh), ("b1 m", b1 * m), ("(1 - b1) g^", omb1 * gh), ("m'", m1), ("b2 v", b2 * v),
                        ("(1 - b2) g^", omb2 * gh), ("(1 - b2) g^ g^", omb2 * gh * gh), ("v'", v1)):
            assert torch.equal(t.float().double(), t), f"exact tier: {name} is not an fp32 number ({h})"
        Bm = Bv = torch.zeros_like(m1)
    else:
        Bg = X.C["g"] * EPS32 * (gs.abs() + wp.abs())
        Bm = (X.C["m"] * EPS32 * ((b1 * m).abs() + (omb1 * gh).abs()) + omb1 * Bg) * SLACK
        Bv = (X.C["v"] * EPS32 * v1 + omb2 * (2 * gh.abs() * Bg + Bg * Bg)) * SLACK
    A = L * sc
    D = v1.sqrt() * I + eps
    Dlo, Dhi = (v1 - Bv).clamp_min(0).sqrt() * I + eps, (v1 + Bv).sqrt() * I + eps
    upd = A * m1 / D
    T = A * Bm / Dlo + A * m1.abs() * (Dhi - Dlo) / (D * Dlo)
    return {"m": m1, "v": v1, "p": p0 - upd, "upd": upd, "Bm": Bm, "Bv": Bv, "T": T, "Bd": Bd}


def p_bound(ora, c=None):
    return (EPS32 * ora["p"].abs() + ((C_UPD if c is None else c) + C_A) * EPS32 * ora["upd"].abs() + ora["T"]) * SLACK + ora["Bd"]


def upd_need(got_p, ora):
    """The smallest C_u with which got_p passes p_bound everywhere."""
    err = (((got_p.double() - ora["p"]).abs() - ora["Bd"]) / SLACK - EPS32 * ora["p"].abs() - ora["T"] - C_A * EPS32 * ora["upd"].abs()).clamp_min(0)
    need = torch.where(err == 0, torch.zeros_like(err), err / (EPS32 * ora["upd"].abs()).clamp_min(1e-300))
    return float(torch.where(torch.isnan(need), torch.full_like(need, math.inf), need).max()) if need.numel() else 0.0


def ema_ref(case, h, p_stored):
    """-> (float64 e', bound, exact: where p' - e and w (p' - e) are fp32 numbers) from the p the launch stored."""
    e = ema_operand(case.tier, case.sizes).double()
    w, dw = h.weight()
    d = p_stored.double() - e
    wd_ = w * d
    e1 = e + wd_
    B = (EPS32 * (2 * wd_.abs() + e1.abs()) + d.abs() * EPS32 * dw) * SLACK
    exact = (d.float().double() == d) & (wd_.float().double() == wd_)
    if h.ema_decay is not None and float(np.float32(w)) != w:
        exact &= False
    return e1, B, exact


FAULTS = ("decay applied after the update", "decay with lr / bc1", "lr_scale left out of the decay factor", "EMA of the old p", "w and 1 - w swapped",
          "warm-up using step - 1", "the coupled formula in decoupled mode")


def adamw_mirror(case, h, fault=None):
    """adam_kernel<., ADAM_COUPLED | ADAM_DECOUPLED> in float32 on the CPU (every product and sum rounded on its own) -> p', m', v', e' (fp32)."""
    o = X.adam_operands(case.tier, case.sizes)
    t = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
    p, g, m, v = o["p"], o["g"], o["m"], o["v"]
    sc, wd = (x.float() for x in case.per_element(h))
    b1, b2, one = t(h.b1), t(h.b2), t(1.0)
    L, I = (t(x) for x in X.host_numbers(h))
    a, lr_t = L * sc, t(h.lr) * sc
    if fault == "decay with lr / bc1":
        lr_t = a
    if fault == "lr_scale left out of the decay factor":
        lr_t = t(h.lr) * torch.ones_like(sc)
    coupled = not h.decoupled or fault == "the coupled formula in decoupled mode"
    p0 = p
    if not coupled and fault != "decay applied after the update":
        p0 = p * (one - lr_t * wd)
    gh = g * t(h.scale) + wd * p if coupled else g * t(h.scale)
    m1 = b1 * m + (one - b1) * gh
    v1 = b2 * v + (one - b2) * gh * gh
    p1 = p0 - a * m1 / (torch.sqrt(v1) * I + t(h.eps))
    if not coupled and fault == "decay applied after the update":
        p1 = p1 * (one - lr_t * wd)
    e = ema_operand(case.tier, case.sizes)
    w = h.weight32()
    if fault == "warm-up using step - 1":
        h2 = HyperW(h, h.decoupled, h.scales, h.wds, h.w, h.ema_decay, h.warmup)
        h2.step = h.step - 1
        w = h2.weight32()
    w = t(float(w))
    src = p if fault == "EMA of the old p" else p1
    e1 = e + (one - w) * (src - e) if fault == "w and 1 - w swapped" else e + w * (src - e)
    return p1, m1, v1, e1


def written(case, h, fault=None):
    """The arenas as a launch leaves them, built on the CPU from the float32 mirror; unlisted chunks and null-ema slots keep their values."""
    a = case.arenas()
    p1, m1, v1, e1 = adamw_mirror(case, h, fault)
    o = X.adam_operands(case.tier, case.sizes)
    L = case.listed
    new = {"p": torch.where(L, p1, o["p"]), "m": torch.where(L, m1, o["m"]), "v": torch.where(L, v1, o["v"])}
    for k in "pmv":
        a[k][case.pos[k]] = new[k]
    sel = L & case.with_e
    a["e"][case.pos["e"][sel]] = e1[sel]
    if case.has_shadow:
        a["sh"][case.pos["sh"]] = new["p"].to(torch.bfloat16)
    return a


# ---------------------------------------------------------------------------------------------------------------- the gate
def check_e_slots(case, after):
    """The slots of tensors without an average hold the sentinel, like a guard."""
    none = ~case.with_e
    if bool(none.any()):
        got = after["e"][case.pos["e"]]
        bad = (_bits(got) != _bits(torch.full_like(got, SENT))) & none
        if bool(bad.any()):
            X._fail(case, "an average was written for a tensor whose ema is NULL", bad, got, torch.full_like(got, SENT))


def check(case, h, after, log=None):
    """The arenas after an AdamW launch against the oracle: every element, every guard, g untouched -> shares of the bounds and needs."""
    before = case.arenas()
    X.check_guards(case, after, keys=("p", "m", "v", "sh", "e"))
    check_e_slots(case, after)
    bad = _bits(after["g"]) != _bits(before["g"])
    if bool(bad.any()):
        at = int(bad.nonzero()[0])
        inside = (case.pos["g"] == at).nonzero()
        raise AssertionError(f"{case}: g was overwritten in {int(bad.sum())} places; first at arena offset {at}: "
                             f"{case.locate(int(inside[0])) if inside.numel() else 'a guard element'}; holds {float(after['g'][at])!r}")
    ora = oracle(case, h)
    got = {k: after[k][case.pos[k]] for k in case.starts}
    old = {k: before[k][case.pos[k]] for k in case.starts}
    L = case.listed
    for k in ("p", "m", "v", "sh", "e"):
        if k in got and not bool(L.all()):
            bad = (_bits(got[k]) != _bits(old[k])) & ~L
            if bool(bad.any()):
                X._fail(case, f"`{k}` changed in a chunk the list does not name", bad, got[k], old[k])
    out = {}
    for k, B in (("m", ora["Bm"]), ("v", ora["Bv"])):
        if case.tier == "exact":
            bad = (_bits(got[k]) != _bits(ora[k].float())) & L
            if bool(bad.any()):
                X._fail(case, f"{k} ({h})", bad, got[k], ora[k], " (exact tier: bit for bit)")
            out[k] = 0.0
        else:
            out[k] = X._bound(case, f"{k} ({h})", got[k], ora[k], B, L)
    out["p"] = X._bound(case, f"p ({h})", got["p"], ora["p"], p_bound(ora), L)
    out["need_upd"] = upd_need(got["p"][L], {k: v[L] for k, v in ora.items()})
    sel = L & case.with_e
    if bool(sel.any()):
        e1, Be, exact = ema_ref(case, h, got["p"])
        out["e"] = X._bound(case, f"ema ({h})", got["e"], e1, Be, sel)
        if case.tier == "exact":
            bad = (_bits(got["e"]) != _bits(e1.float())) & sel & exact
            out["e_exact"] = int((sel & exact).sum())
            if bool(bad.any()):
                X._fail(case, f"ema ({h})", bad, got["e"], e1, " (exact tier: p' - e and w (p' - e) are fp32 numbers here: bit for bit)")
    if case.has_shadow:
        want = got["p"].to(torch.bfloat16)
        bad = (_bits(got["sh"]) != _bits(want)) & L
        if bool(bad.any()):
            X._fail(case, f"shadow != round-to-nearest-even bf16 of the stored p ({h})", bad, got["sh"].float(), want.float())
    if log is not None:
        for k, v in out.items():
            note(f"{log}:{k if k.startswith('need') or k == 'e_exact' else k + ':max_err_over_bound'}", float(v))
    return out


def swap_expected(case):
    """The arenas after xvit_ema_swap: p and e exchanged and the shadow bf16 of the new p where the tensor has an average and the chunk is listed."""
    a = case.arenas()
    sel = case.listed & case.with_e
    p, e = a["p"][case.pos["p"]].clone(), a["e"][case.pos["e"]].clone()
    a["p"][case.pos["p"][sel]] = e[sel]
    a["e"][case.pos["e"][sel]] = p[sel]
    if case.has_shadow:
        a["sh"][case.pos["sh"][sel]] = e[sel].to(torch.bfloat16)
    return a


# ---------------------------------------------------------------------------------------------------------------- device launches
def device_case(case, h):
    dev = X._dev()
    d = {k: t.to(dev) for k, t in case.arenas().items()}
    base = {k: t.data_ptr() for k, t in d.items()}
    assert all(b % 16 == 0 for b in base.values()), "arena bases must be 16-byte aligned"
    rows = case.table(base)
    ex = case.extras(base["e"], h)
    paths = [vec_ok(*r[:5], int(x["ema"])) for r, x in zip(rows, ex)]
    assert paths == case.vec_t, f"{case}: the mirror of adam_vec_ok(t, ema) picks {paths} (True: 16-byte path), the placement was built for {case.vec_t}"
    d["table"] = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev)
    d["extras"] = torch.from_numpy(ex.view(np.int64).reshape(-1, 2).copy()).to(dev)
    d["chunks"] = torch.from_numpy(np.asarray(case.chunks, dtype=np.int32).reshape(-1, 2)).to(dev)
    return d


def _download(case, d):
    torch.cuda.synchronize()
    return {k: d[k].cpu() for k in case.starts}


def launch(case, h, dev_record=False, skip=0):
    """xvit_adamw_step, or (dev_record) xvit_adamw_step_dev with a record the host wrote from the same fp32 numbers -> (rc, arenas after)."""
    from xvit import _lib
    lib, d = _lib.load(), device_case(case, h)
    args = (d["table"].data_ptr(), d["extras"].data_ptr(), d["chunks"].data_ptr(), len(case.chunks))
    if dev_record:
        L, I = X.host_numbers(h)
        rec = np.zeros((), dtype=X.REC)
        rec["step"], rec["lr"], rec["lr_over_bc1"], rec["inv_sqrt_bc2"], rec["clip_coef"], rec["skip"] = h.step, h.lr, L, I, h.scale, skip
        w = X.record_window(rec).to(X._dev())
        rc = lib.xvit_adamw_step_dev(*args, w.data_ptr() + 8 * X.REC_GUARD, h.b1, h.b2, h.eps, int(h.decoupled), h.ema_decay or 0.0, int(h.warmup), X._stream())
        after = _download(case, d)
        assert bytes(X.record_of(f"{case}: xvit_adamw_step_dev", w).tobytes()) == rec.tobytes(), f"{case}: xvit_adamw_step_dev changed the record it only reads"
        return rc, after
    rc = lib.xvit_adamw_step(*args, h.lr, h.b1, h.b2, h.eps, h.step, h.scale, int(h.decoupled), h.w, X._stream())
    return rc, _download(case, d)


def swap_launch(case, h, times=1):
    from xvit import _lib
    lib, d = _lib.load(), device_case(case, h)
    for _ in range(times):
        rc = lib.xvit_ema_swap(d["table"].data_ptr(), d["extras"].data_ptr(), d["chunks"].data_ptr(), len(case.chunks), X._stream())
        assert rc == 0, X.last_error()
    return _download(case, d)
