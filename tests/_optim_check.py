"""Oracle, launchers, launch-geometry mirror and gate for the fused Adam kernels, the gradient-norm partials and the step prologue
(csrc/misc.hip: adam_kernel<false|true, ADAM_PLAIN>, grad_sqnorm_kernel, adam_prologue_kernel), for the dropout mask (csrc/xvit_common.h hash32 /
draw24 / Dropout::keep, xvit_dropout) and for the casts and the row bookkeeping (xvit_cast_f32_bf16, xvit_add_cast_f32_bf16,
xvit_rows_combine).

Launchers.  They go through the C entry points (_lib.load()) with tables built here: rows p, g, m, v, shadow, n as int64 and a list of
(tensor, chunk) int32 pairs.  Every array kind (p, g, m, v, shadow) is ONE arena that holds all tensors of the launch; a tensor starts at
an element offset that sets its alignment (`PLACEMENTS`), with at least GUARD elements in front of it, between tensors and behind the last
one.  The guards of p, m, v and shadow hold a fixed sentinel and are compared with it bit for bit afterwards; the guards of g hold NaN
(a read past a chunk end poisons what it writes) and the whole g arena is compared bit for bit with what was uploaded.

Mirror of the path choice.  `vec_ok` repeats adam_vec_ok on the addresses of the launch: the 16-byte path needs p, g, m, v 16-byte
aligned and the shadow, when there is one, 8-byte aligned.  Every launch asserts that the path of its placement is the one the case was
built for, and `where` says where an element sits: chunk, path, and (16-byte path) iteration / thread / lane of the vector body or the
thread of the tail, (scalar path) iteration / thread.

Exact tier (no tolerance).  betas (0.5, 0.75), grad_scale and weight_decay powers of two (or 0), g in {-3..3} 2^-3, m and p integers
<= 64 times 2^-6, v = k 2^-6 (k in 0..32): g s, wd p, their sum g^, 0.5 m, 0.5 g^, 0.75 v, 0.25 g^, 0.25 g^ g^ and both sums are fp32
numbers, which `adam_oracle` asserts in float64 for every one of them, so m and v are THE result whether or not the compiler contracts a
multiply-add, and must match bit for bit.  Gradient partials: g in {-3..3} 2^-3, a chunk's sum of squares is at most 9 * 16384 units of
2^-6 < 2^24, exact in any order.  The shadow is the round-to-nearest-even bf16 of the p the SAME launch stored, on every tier and path.

Float64 tier (u = 2^-24; every bound times 1 + 2^-20 for the second-order terms).  Reference: float64 arithmetic on the fp32 inputs with
the fp32 hyper-parameters that cross the C ABI, 1 - beta as the fp32 difference the kernel forms, and lr_over_bc1 / inv_sqrt_bc2 as the
fp32 values the host computes in double (`host_numbers` mirrors xvit_adam_step).  Rounding counts read from the kernel's `upd`:
  g^ = g s + wd p              two products and a sum: B_g = 2 u (|g s| + |wd p|)
  m' = b1 m + (1 - b1) g^      two products and a sum: B_m = C_m u (|b1 m| + |(1 - b1) g^|) + (1 - b1) B_g,  C_m = 2
  v' = b2 v + (1 - b2) g^ g^   all terms non-negative; at most three roundings on a term: B_v = C_v u v' + (1 - b2) (2 |g^| B_g + B_g^2), C_v = 3
  upd = L m' / (sqrt(v') I + eps), p' = p - upd
      B_p = u |p'| + C_u u |upd| + T,  T = L B_m / D_lo + L |m'| (D_hi - D_lo) / (D D_lo): what B_m and B_v do to upd, with
      D = sqrt(v') I + eps, D_lo / D_hi the same at v' -+ B_v (v' - B_v clamped at 0).  This is |d upd / dm| B_m + |d upd / dv| B_v
      written as a difference, so that it stays finite and an upper bound where v' is small.
  Contraction (-ffp-contract=fast) only removes roundings.  On the exact tier B_m = B_v = T = 0: p has u |p'| + C_u u |upd| alone.
  C_u (root, product, sum, product, division: five roundings if root and division are correctly rounded) is not taken from that count
  but, like the constants of _cls_check.py, from the reference side: `adam_mirror`, the formula in float32 on the CPU, runs over the
  GPU tests' own inputs (tests/test_optim_gate_cpu.py); C_u is the smallest power of two at or above 4 x the mirror's largest need.
  The device's need is logged (XVIT_MEASURE_LOG, profiles/optim_gate_measured.txt) and sets nothing.

  float32 CPU mirror, the largest need over every hyper-parameter set of HYPER_RANDOM / HYPER_EXACT on the operands of `adam_operands`
  kind        need   4 x need     C
  upd_exact   2.17       8.7     16     (C_u, exact-tier operands, where B_m = B_v = T = 0 and the need is that of upd alone)
  upd_random  0.00       0.0      -     (random operands: T, what B_m and B_v do to upd, already covers the mirror; C_u = 16 is used here too)
  clip_coef   0.67       2.7      4     (C_div: max_norm / (norm + 1e-6f) over the prologue cases of tests/test_optim_edges_gpu.py)

Gradient-norm partials (random tier).  All terms g g are non-negative, so the relative error of a chunk's sum is at most
gamma(n) = n u / (1 - n u) with n the roundings on the longest path: scalar path 64 sequential fused multiply-adds per thread (the product
is not rounded on its own), 6 levels across the wave and 2 levels across the four waves ((w0 + w1) + (w2 + w3): three adds, two of them
on any path) = 72; 16-byte path 16 fused multiply-adds per accumulator, one more for a tail element, 2 levels to join the four
accumulators, 6 + 2 as before = 27.

Prologue.  Partials on a dyadic grid, so their double sum is exact in any order.  grad_norm = (float)sqrt(sum): exact where the sum is a
perfect square, within one fp32 ulp of float64 otherwise.  clip_coef from the record's own grad_norm: exactly 1 where the float64 quotient
max_norm / (fl32(norm + 1e-6f)) is >= 1, within C_div u of it otherwise.  lr_over_bc1 / inv_sqrt_bc2 within one fp32 ulp of the host's
double formula (host and device pow differ).

Dropout mask.  `hash32_np` / `draw24_np` are xvit_common.h:274-281 in numpy uint64 with wrapping multiplies; `drop_params` is the host-side
Dropout(p, seed): thr = int(float32(p) * float32(2^24)) truncated, inv = float32(1) / (float32(1) - float32(p)); element idx is kept iff
draw24 >= thr; a registered epoch counter turns the seed into seed + epoch * 0xD1B54A32D192ED03 mod 2^64.  xvit_dropout must equal
`dropout_expected` bit for bit: fp32 the single product fl(x inv), bf16 its round-to-nearest-even, dropped elements +0.
THRESHOLD_SEED / THRESHOLD_INDEX: a seed for which that element index draws exactly thr at p = 0.25 (found with the mirror), the one
element on which `>` and `>=` differ.  THIRD_SEED / THIRD_INDEX: the same for thr = 5592405 at p = 1/3, where float32(p) 2^24 = 5592405.5 and a
rounded threshold would be 5592406: the one element on which truncation and rounding of thr differ."""
import bisect
import math

import numpy as np
import torch

from _util import exact_grid, exact_operands, note

EPS32 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
SENT = -123456.0                      # exact in fp32 and bf16; nothing a kernel here computes
CHUNK = 16384                         # ADAM_CHUNK
GUARD = 8                             # sentinel / NaN elements in front of, between and behind the tensors of an arena
SIZES = (1, 3, 4, 5, 255, 1023, 1024, 1025, 1027, 16383, 16384, 16385, 16387, 2 * 16384 + 2)
C = {"m": 2.0, "v": 3.0, "g": 2.0, "upd": 16.0, "div": 4.0}   # m, v, g: rounding counts; upd, div: see the table above
NORM_ROUNDINGS = {"scalar": 64 + 6 + 2, "vec": 16 + 1 + 2 + 6 + 2}

# element offsets of a tensor's start inside its arena, modulo 4 floats (16 bytes); shadow: None (no shadow) or modulo 8 bf16 (16 bytes)
PLACEMENTS = {
    "aligned, no shadow": dict(p=0, g=0, m=0, v=0, sh=None, vec=True),
    "aligned, shadow 8-byte aligned": dict(p=0, g=0, m=0, v=0, sh=4, vec=True),
    "shadow 2 bytes off": dict(p=0, g=0, m=0, v=0, sh=1, vec=False),
    "p 4 bytes off": dict(p=1, g=0, m=0, v=0, sh=0, vec=False),
    "only g 4 bytes off": dict(p=0, g=1, m=0, v=0, sh=0, vec=False),
}


def f32(v):
    """The float32 nearest to v, as a Python float (what a `float` argument of the C ABI carries)."""
    return float(np.float32(v))


def pow2_at_or_above(v):
    return 2.0 ** math.ceil(math.log2(v))


def gamma(n):
    return n * EPS32 / (1.0 - n * EPS32)


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev():
    return torch.device("cuda:0")


def last_error():
    from xvit import _lib
    return _lib.load().xvit_last_error_string().decode()


# ---------------------------------------------------------------------------------------------------------------- hyper-parameters
class Hyper:
    def __init__(self, lr=3e-3, b1=0.9, b2=0.98, eps=1e-8, wd=0.0, step=1, scale=1.0):
        self.lr, self.b1, self.b2, self.eps, self.wd, self.step, self.scale = lr, b1, b2, eps, wd, step, scale

    def __repr__(self):
        return f"lr {self.lr:g} betas ({self.b1:g}, {self.b2:g}) eps {self.eps:g} wd {self.wd:g} step {self.step} scale {self.scale:g}"


HYPER_RANDOM = [Hyper(eps=e, wd=w, scale=s, step=t) for e in (1e-8, 1e-3) for w in (0.0, 0.05) for s in (1.0, 0.25, 1.0 / 3.0) for t in (1, 2, 1000)]
HYPER_EXACT = [Hyper(b1=0.5, b2=0.75, eps=e, wd=w, scale=s, step=t) for e in (1e-8, 1e-3) for w in (0.0, 2.0 ** -4) for s in (1.0, 0.25) for t in (1, 2)]


def host_numbers(h, step=None):
    """xvit_adam_step's double arithmetic -> (lr_over_bc1, inv_sqrt_bc2) as the fp32 numbers the kernel gets."""
    step = h.step if step is None else step
    bc1, bc2 = 1.0 - math.pow(f32(h.b1), step), 1.0 - math.pow(f32(h.b2), step)
    return f32(f32(h.lr) / bc1), f32(1.0 / math.sqrt(bc2))


# ---------------------------------------------------------------------------------------------------------------- launch geometry
def vec_ok(p, g, m, v, sh):
    """adam_vec_ok on byte addresses (sh = 0: no shadow)."""
    return ((p | g | m | v) & 15) == 0 and (sh == 0 or (sh & 7) == 0)


def n_chunks(n):
    return (n + CHUNK - 1) // CHUNK


def where(n, i, vec):
    """Where element i of an n-element tensor sits in adam_kernel / grad_sqnorm_kernel."""
    c = i // CHUNK
    begin, end = c * CHUNK, min(c * CHUNK + CHUNK, n)
    j = i - begin
    head = f"chunk {c} of {n_chunks(n)} [{begin}, {end}), "
    if not vec:
        return head + f"scalar path, element {i}: iteration {j // 256}, thread {j % 256}"
    body = (end - begin) & ~3
    if j < body:
        return head + f"16-byte path, element {i}: vector body, iteration {j // 1024}, thread {(j // 4) % 256}, lane {j % 4}"
    return head + f"16-byte path, element {i}: tail, thread {j - body}"


def layout(sizes, off, unit):
    """Starts of the tensors inside an arena whose base is 16-byte aligned: start = off modulo `unit` elements, GUARD elements or more
    in front of every tensor and behind the last -> (starts, total)."""
    starts, pos = [], 0
    for n in sizes:
        s = pos + GUARD
        s += (off - s) % unit
        starts.append(s)
        pos = s + n
    return starts, pos + GUARD


# ---------------------------------------------------------------------------------------------------------------- operands
_OPERANDS = {}


def adam_operands(tier, sizes=SIZES):
    """-> dict p, g, m, v: the concatenation of every tensor's fp32 values (CPU), cached and never changed."""
    key = (tier, tuple(sizes))
    if key not in _OPERANDS:
        N = sum(sizes)
        if tier == "exact":
            o = {"p": exact_grid((N,), seed=71, unit=2.0 ** -6, span=64), "g": exact_operands((N,), seed=72, s=3),
                 "m": exact_grid((N,), seed=73, unit=2.0 ** -6, span=64), "v": exact_grid((N,), seed=74, unit=2.0 ** -6, span=32).abs()}
        else:
            gen = torch.Generator().manual_seed(75)
            o = {"p": torch.randn(N, generator=gen), "g": torch.randn(N, generator=gen), "m": 0.1 * torch.randn(N, generator=gen),
                 "v": (0.1 * torch.randn(N, generator=gen)) ** 2}
        _OPERANDS[key] = o
    return _OPERANDS[key]


class AdamCase:
    """One launch: `sizes` tensors in the arenas of `placement`; order "natural" / "shuffled" / a list of (tensor, chunk)."""

    def __init__(self, placement, tier, sizes=SIZES, order="natural"):
        self.placement, self.tier, self.sizes = placement, tier, tuple(sizes)
        pl = PLACEMENTS[placement]
        self.expect_vec, self.has_shadow = pl["vec"], pl["sh"] is not None
        self.offsets = [0]
        for n in self.sizes:
            self.offsets.append(self.offsets[-1] + n)
        self.N = self.offsets[-1]
        self.starts, self.total, self.pos = {}, {}, {}
        for k in ("p", "g", "m", "v", "sh"):
            if k == "sh" and not self.has_shadow:
                continue
            self.starts[k], self.total[k] = layout(self.sizes, pl[k], 8 if k == "sh" else 4)
            self.pos[k] = torch.cat([torch.arange(s, s + n) for s, n in zip(self.starts[k], self.sizes)])
        allc = [(t, c) for t, n in enumerate(self.sizes) for c in range(n_chunks(n))]
        if order == "natural":
            self.chunks = allc
        elif order == "shuffled":
            perm = torch.randperm(len(allc), generator=torch.Generator().manual_seed(5)).tolist()
            self.chunks = [allc[i] for i in perm]
        else:
            self.chunks = list(order)
        self.listed = torch.zeros(self.N, dtype=torch.bool)
        for t, c in self.chunks:
            self.listed[self.offsets[t] + c * CHUNK: self.offsets[t] + min((c + 1) * CHUNK, self.sizes[t])] = True
        self.vec = self.expect_vec          # a device launch overwrites it with the mirror's verdict on the real addresses

    def __repr__(self):
        return f"adam [{self.placement}; {self.tier} tier; {len(self.sizes)} tensors, {len(self.chunks)} chunks]"

    def arenas(self):
        """The arenas before the launch (CPU): p, m, v fp32 and the bf16 shadow with sentinel guards, g with NaN guards."""
        o = adam_operands(self.tier, self.sizes)
        a = {}
        for k in self.starts:
            if k == "sh":
                a[k] = torch.full((self.total[k],), SENT, dtype=torch.bfloat16)
                a[k][self.pos[k]] = o["p"].to(torch.bfloat16)           # what a shadow holds before a step: bf16 of the old p
            else:
                a[k] = torch.full((self.total[k],), math.nan if k == "g" else SENT, dtype=torch.float32)
                a[k][self.pos[k]] = o[k]
        return a

    def table(self, base):
        """The AdamTensor rows for arenas at the byte addresses base[k]."""
        rows = []
        for t, n in enumerate(self.sizes):
            r = [base[k] + 4 * self.starts[k][t] for k in ("p", "g", "m", "v")]
            r.append(base["sh"] + 2 * self.starts["sh"][t] if self.has_shadow else 0)
            rows.append(r + [n])
        return rows

    def locate(self, e):
        t = bisect.bisect_right(self.offsets, e) - 1
        return f"tensor {t} (n = {self.sizes[t]}), " + where(self.sizes[t], e - self.offsets[t], self.vec)


# ---------------------------------------------------------------------------------------------------------------- oracle and mirror
def adam_oracle(case, h):
    """float64 on the fp32 operands -> dict m, v, p, upd (float64) and the bounds Bm, Bv, T (0 on the exact tier)."""
    o = adam_operands(case.tier, case.sizes)
    p, g, m, v = (o[k].double() for k in ("p", "g", "m", "v"))
    s, wd, b1, b2, eps = f32(h.scale), f32(h.wd), f32(h.b1), f32(h.b2), f32(h.eps)
    omb1, omb2 = float(np.float32(1) - np.float32(h.b1)), float(np.float32(1) - np.float32(h.b2))
    L, I = host_numbers(h)
    gs, wp = g * s, wd * p
    gh = gs + wp
    m1 = b1 * m + omb1 * gh
    v1 = b2 * v + omb2 * gh * gh
    if case.tier == "exact":
        for name, t in (("g s", gs), ("wd p", wp), ("g^", gh), ("b1 m", b1 * m), ("(1 - b1) g^", omb1 * gh), ("m'", m1), ("b2 v", b2 * v),
                        ("(1 - b2) g^", omb2 * gh), ("(1 - b2) g^ g^", omb2 * gh * gh), ("v'", v1)):
            assert torch.equal(t.float().double(), t), f"exact tier: {name} is not an fp32 number ({h})"
        Bm = Bv = torch.zeros_like(m1)
    else:
        Bg = C["g"] * EPS32 * (gs.abs() + wp.abs())
        Bm = (C["m"] * EPS32 * ((b1 * m).abs() + (omb1 * gh).abs()) + omb1 * Bg) * SLACK
        Bv = (C["v"] * EPS32 * v1 + omb2 * (2 * gh.abs() * Bg + Bg * Bg)) * SLACK
    D = v1.sqrt() * I + eps
    Dlo, Dhi = (v1 - Bv).clamp_min(0).sqrt() * I + eps, (v1 + Bv).sqrt() * I + eps
    upd = L * m1 / D
    T = L * Bm / Dlo + L * m1.abs() * (Dhi - Dlo) / (D * Dlo)
    return {"m": m1, "v": v1, "p": p - upd, "upd": upd, "Bm": Bm, "Bv": Bv, "T": T}


def p_bound(ora, c=None):
    return (EPS32 * ora["p"].abs() + (C["upd"] if c is None else c) * EPS32 * ora["upd"].abs() + ora["T"]) * SLACK


def upd_need(got_p, ora):
    """The smallest C_u with which got_p passes p_bound everywhere."""
    err = ((got_p.double() - ora["p"]).abs() / SLACK - EPS32 * ora["p"].abs() - ora["T"]).clamp_min(0)
    need = torch.where(err == 0, torch.zeros_like(err), err / (EPS32 * ora["upd"].abs()).clamp_min(1e-300))
    return float(torch.where(torch.isnan(need), torch.full_like(need, math.inf), need).max())


def adam_mirror(case, h, fault=None):
    """adam_kernel's `upd` in float32 on the CPU (every product and sum rounded on its own) -> p', m', v' (fp32).  fault: one of the
    formula faults of tests/test_optim_gate_cpu.py."""
    o = adam_operands(case.tier, case.sizes)
    t = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
    p, g, m, v = o["p"], o["g"], o["m"], o["v"]
    if fault == "m and v swapped":
        m, v = v, m
    b1, b2, one = t(h.b1), t(h.b2), t(1.0)
    L, I = (t(x) for x in host_numbers(h, h.step - 1 if fault == "bias corrections of step - 1" else None))
    gh = (g + t(h.wd) * p) * t(h.scale) if fault == "decay added before the clip scale" else g * t(h.scale) + t(h.wd) * p
    m1 = (b2 if fault == "beta2 used for beta1" else b1) * m + (one - (b2 if fault == "beta2 used for beta1" else b1)) * gh
    v1 = b2 * v + (one - b2) * gh * gh
    D = torch.sqrt(v1 + t(h.eps)) * I if fault == "eps inside the root" else torch.sqrt(v1) * I + t(h.eps)
    p1 = p - L * m1 / D
    if fault == "m and v swapped":
        m1, v1 = v1, m1
    return p1, m1, v1


def adam_written(case, h, fault=None):
    """The arenas as a launch leaves them, built on the CPU from the float32 mirror (exact tier: m, v from the oracle, which the mirror
    equals); the gate's own test plants its faults here.  Elements of chunks the list does not name keep their old values."""
    a = case.arenas()
    p1, m1, v1 = adam_mirror(case, h, fault)
    o = adam_operands(case.tier, case.sizes)
    L = case.listed
    new = {"p": torch.where(L, p1, o["p"]), "m": torch.where(L, m1, o["m"]), "v": torch.where(L, v1, o["v"])}
    for k in ("p", "m", "v"):
        a[k][case.pos[k]] = new[k]
    if case.has_shadow:
        a["sh"][case.pos["sh"]] = new["p"].to(torch.bfloat16)
    return a


# ---------------------------------------------------------------------------------------------------------------- checks
def _fail(case, what, bad, got, want, extra=""):
    e = int(bad.nonzero()[0])
    raise AssertionError(f"{case}: {what}: {int(bad.sum())} of {bad.numel()} elements wrong; first at {case.locate(e)}: "
                         f"got {float(got[e])!r}, want {float(want[e])!r}{extra}")


def check_guards(case, after, keys=("p", "m", "v", "sh")):
    """Every guard element of p / m / v / shadow holds the sentinel bit for bit; names the tensor it sits behind (or in front of)."""
    for k in keys:
        if k not in case.starts:
            continue
        buf = after[k]
        bad = _bits(buf) != _bits(torch.full_like(buf, SENT))
        bad[case.pos[k]] = False
        if bool(bad.any()):
            at = int(bad.nonzero()[0])
            ends = [s + n for s, n in zip(case.starts[k], case.sizes)]
            t = bisect.bisect_right(ends, at) - 1
            side = (f"{at - ends[t]} element(s) behind the end of tensor {t} (n = {case.sizes[t]}), {where(case.sizes[t], case.sizes[t] - 1, case.vec)} is its last element"
                    if t >= 0 else f"in front of tensor 0, {case.starts[k][0] - at} element(s) before its start")
            raise AssertionError(f"{case}: {int(bad.sum())} guard elements of `{k}` were overwritten; first at arena offset {at}: {side}; holds {float(buf[at])!r}")


def adam_check(case, h, after, log=None):
    """The arenas after a launch against the oracle: every element, every guard, g untouched.  -> dict of the shares of the bounds used
    and the need of C_u."""
    before = case.arenas()
    check_guards(case, after)
    bad = _bits(after["g"]) != _bits(before["g"])
    if bool(bad.any()):
        at = int(bad.nonzero()[0])
        inside = (case.pos["g"] == at).nonzero()
        place = case.locate(int(inside[0])) if inside.numel() else "a guard element"
        raise AssertionError(f"{case}: g was overwritten in {int(bad.sum())} places; first at arena offset {at}: {place}; holds {float(after['g'][at])!r}")
    ora = adam_oracle(case, h)
    got = {k: after[k][case.pos[k]] for k in case.starts}
    old = {k: before[k][case.pos[k]] for k in case.starts}
    L = case.listed
    for k in ("p", "m", "v", "sh"):                       # chunks the list does not name: bit-identical
        if k in got and not bool(L.all()):
            bad = (_bits(got[k]) != _bits(old[k])) & ~L
            if bool(bad.any()):
                _fail(case, f"`{k}` changed in a chunk the list does not name", bad, got[k], old[k])
    out = {}
    for k, B in (("m", ora["Bm"]), ("v", ora["Bv"])):
        if case.tier == "exact":
            bad = (_bits(got[k]) != _bits(ora[k].float())) & L
            if bool(bad.any()):
                _fail(case, f"{k} ({h})", bad, got[k], ora[k], " (exact tier: bit for bit)")
            out[k] = 0.0
        else:
            out[k] = _bound(case, f"{k} ({h})", got[k], ora[k], B, L)
    out["p"] = _bound(case, f"p ({h})", got["p"], ora["p"], p_bound(ora), L)
    out["need_upd"] = upd_need(got["p"][L], {k: v[L] for k, v in ora.items()})
    if case.has_shadow:
        want = got["p"].to(torch.bfloat16)
        bad = (_bits(got["sh"]) != _bits(want)) & L
        if bool(bad.any()):
            _fail(case, f"shadow != round-to-nearest-even bf16 of the stored p ({h})", bad, got["sh"].float(), want.float())
    if log is not None:
        for k, v in out.items():
            note(f"{log}:{k if k.startswith('need') else k + ':max_err_over_bound'}", v)
    return out


def _bound(case, what, got, ref, B, L):
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / B.clamp_min(1e-300))
    ratio = torch.where(torch.isnan(ratio) | ~torch.isfinite(got.double()), torch.full_like(ratio, math.inf), ratio)
    ratio = torch.where(L, ratio, torch.zeros_like(ratio))
    worst = float(ratio.max())
    if worst > 1.0:
        e = int(ratio.argmax())
        raise AssertionError(f"{case}: {what}: {int((ratio > 1).sum())} of {int(L.sum())} elements out of bound, worst {worst:.3g}x its bound at {case.locate(e)}: "
                             f"got {float(got[e])!r}, float64 reference {float(ref[e])!r}, bound {float(B[e]):.3g}")
    return worst


def old_gates(case, h, after):
    """What the whole-tensor gates of tests/test_optim_gpu.py say on the same data: the largest rel-L2 over the tensors of p (gate 2e-6)
    and of the moments (gate 5e-6) against float64 -> (rel_p, rel_moments, seen)."""
    ora = adam_oracle(case, h)
    rp = rm = 0.0
    for t in range(len(case.sizes)):
        sl = slice(case.offsets[t], case.offsets[t + 1])
        r = lambda k: float((after[k][case.pos[k]][sl].double() - ora[k][sl]).norm() / (ora[k][sl].norm() + 1e-30))   # noqa: E731
        rp, rm = max(rp, r("p")), max(rm, r("m"), r("v"))
    rp, rm = (math.inf if math.isnan(x) else x for x in (rp, rm))
    return rp, rm, rp >= 2e-6 or rm >= 5e-6


# ---------------------------------------------------------------------------------------------------------------- device launches
REC = np.dtype([("step", "<i8"), ("skipped", "<i8"), ("lr", "<f4"), ("grad_norm", "<f4"), ("clip_coef", "<f4"), ("lr_over_bc1", "<f4"),
                ("inv_sqrt_bc2", "<f4"), ("skip", "<i4"), ("reserved", "<i4", (2,))])    # xvit_adam_state, 48 bytes
REC_WORDS, REC_GUARD = 6, 2
REC_SENT = 0x5A5A5A5A5A5A5A5A
assert REC.itemsize == 48


def record_window(rec):
    """A record between REC_GUARD sentinel words on each side (int64 CPU tensor)."""
    w = torch.full((REC_WORDS + 2 * REC_GUARD,), REC_SENT, dtype=torch.int64)
    w[REC_GUARD:REC_GUARD + REC_WORDS] = torch.from_numpy(np.asarray(rec, dtype=REC).reshape(1).view(np.int64).copy())
    return w


def record_of(name, w):
    """The record of a window after a launch; the sentinels round it must be untouched."""
    w = w.cpu()
    g = torch.cat([w[:REC_GUARD], w[REC_GUARD + REC_WORDS:]])
    assert bool((g == REC_SENT).all()), f"{name}: the words round the state record were overwritten: {[hex(int(x)) for x in g]}"
    return w[REC_GUARD:REC_GUARD + REC_WORDS].numpy().copy().view(REC)[0]


def device_case(case):
    """Upload the arenas, build table and chunk list -> dict for the launchers; asserts the path the mirror picks on the real addresses."""
    dev = _dev()
    d = {k: t.to(dev) for k, t in case.arenas().items()}
    base = {k: t.data_ptr() for k, t in d.items()}
    assert all(b % 16 == 0 for b in base.values()), "arena bases must be 16-byte aligned"
    rows = case.table(base)
    paths = {vec_ok(*r[:5]) for r in rows}
    assert paths == {case.expect_vec}, f"{case}: the mirror of adam_vec_ok picks {paths}, the placement was built for {'16-byte' if case.expect_vec else 'scalar'}"
    case.vec = case.expect_vec
    d["table"] = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev)
    d["chunks"] = torch.from_numpy(np.asarray(case.chunks, dtype=np.int32).reshape(-1, 2)).to(dev)
    return d


def _download(case, d):
    torch.cuda.synchronize()
    return {k: d[k].cpu() for k in case.starts}


def adam_launch(case, h, dev_record=None, skip=0):
    """xvit_adam_step, or (dev_record=True) xvit_adam_step_dev with a record the host wrote from the same fp32 numbers
    -> (rc, arenas after the launch on the CPU)."""
    from xvit import _lib
    lib, d = _lib.load(), device_case(case)
    if dev_record:
        L, I = host_numbers(h)
        rec = np.zeros((), dtype=REC)
        rec["step"], rec["lr"], rec["lr_over_bc1"], rec["inv_sqrt_bc2"], rec["clip_coef"], rec["skip"] = h.step, h.lr, L, I, h.scale, skip
        w = record_window(rec).to(_dev())
        rc = lib.xvit_adam_step_dev(d["table"].data_ptr(), d["chunks"].data_ptr(), len(case.chunks), w.data_ptr() + 8 * REC_GUARD, h.b1, h.b2, h.eps, h.wd, _stream())
        after = _download(case, d)
        assert bytes(record_of(f"{case}: xvit_adam_step_dev", w).tobytes()) == rec.tobytes(), f"{case}: xvit_adam_step_dev changed the record it only reads"
        return rc, after
    rc = lib.xvit_adam_step(d["table"].data_ptr(), d["chunks"].data_ptr(), len(case.chunks), h.lr, h.b1, h.b2, h.eps, h.wd, h.step, h.scale, _stream())
    return rc, _download(case, d)


def assert_same_arenas(case, what, a, b):
    for k in a:
        bad = _bits(a[k]) != _bits(b[k])
        if bool(bad.any()):
            at = int(bad.nonzero()[0])
            inside = (case.pos[k] == at).nonzero()
            place = case.locate(int(inside[0])) if inside.numel() else "a guard element"
            raise AssertionError(f"{case}: {what}: `{k}` differs in {int(bad.sum())} places; first at arena offset {at}: {place}: {float(a[k][at])!r} != {float(b[k][at])!r}")


# ---------------------------------------------------------------------------------------------------------------- gradient-norm partials
def partials_window(n):
    w = torch.full((n + GUARD,), SENT, dtype=torch.float32)
    w[:n] = math.nan
    return w


def sqnorm_launch(case):
    from xvit import _lib
    lib, d = _lib.load(), device_case(case)
    w = partials_window(len(case.chunks)).to(_dev())
    rc = lib.xvit_grad_sqnorm_partials(d["table"].data_ptr(), d["chunks"].data_ptr(), len(case.chunks), w.data_ptr(), _stream())
    after = _download(case, d)
    return rc, w.cpu(), after


def sqnorm_ref(case):
    """float64 sum of g g over each chunk of the list, in list order."""
    g = adam_operands(case.tier, case.sizes)["g"].double()
    return torch.stack([(g[case.offsets[t] + c * CHUNK: case.offsets[t] + min((c + 1) * CHUNK, case.sizes[t])] ** 2).sum() for t, c in case.chunks])


def sqnorm_written(case):
    """The partials window of a correct launch: per chunk a float32 sum (torch's own order)."""
    g = adam_operands(case.tier, case.sizes)["g"]
    w = partials_window(len(case.chunks))
    for k, (t, c) in enumerate(case.chunks):
        x = g[case.offsets[t] + c * CHUNK: case.offsets[t] + min((c + 1) * CHUNK, case.sizes[t])]
        w[k] = (x * x).sum()
    return w


def sqnorm_check(case, w, log=None):
    """The partials window after a launch: the guard behind the last partial, then every partial.  -> the largest share of gamma(n) used."""
    n = len(case.chunks)
    bad = _bits(w[n:]) != _bits(torch.full((GUARD,), SENT))
    assert not bool(bad.any()), f"{case}: the guard behind the {n} partials was overwritten at slot {n + int(bad.nonzero()[0])}: {float(w[n + int(bad.nonzero()[0])])!r}"
    ref, got = sqnorm_ref(case), w[:n]
    worst = 0.0
    for k, (t, c) in enumerate(case.chunks):
        tag = f"{case}: partial {k} = tensor {t} (n = {case.sizes[t]}), chunk {c} of {n_chunks(case.sizes[t])}, {'16-byte' if case.vec else 'scalar'} path"
        if case.tier == "exact":
            assert float(ref[k]) == float(ref[k].float()), "exact tier: a chunk's sum of squares must be an fp32 number"
            assert float(got[k]) == float(ref[k]), f"{tag}: got {float(got[k])!r}, want {float(ref[k])!r} (exact tier: bit for bit)"
        else:
            B = gamma(NORM_ROUNDINGS["vec" if case.vec else "scalar"]) * float(ref[k])
            err = abs(float(got[k]) - float(ref[k]))
            assert err <= B, f"{tag}: got {float(got[k])!r}, float64 {float(ref[k])!r}: error {err:.3g} > bound {B:.3g}"   # NaN fails
            worst = max(worst, err / B)
    if log is not None:
        note(f"{log}:partials:max_err_over_bound", worst)
    return worst


# ---------------------------------------------------------------------------------------------------------------- prologue
def prologue_partials(n, square, seed=0):
    """n partials, integers in [0, 200] times 2^-4 (their double sum is exact in any order); square: the sum is made a perfect square."""
    gen = torch.Generator().manual_seed(81 + n + seed)
    k = torch.randint(0, 201, (n,), generator=gen, dtype=torch.int64)
    if square:                       # sum = (S / 4)^2 = S^2 / 16 with S an integer: in units of 2^-4 the sum must be S^2
        S = int(math.isqrt(int(k.sum()))) + 1
        k[0] += S * S - int(k.sum())
    return k.float() * 2.0 ** -4


def prologue_launch(partials, rec, max_norm, b1, b2, skip_nonfinite):
    """-> (rc, record after).  partials: fp32 CPU tensor or None."""
    from xvit import _lib
    lib, dev = _lib.load(), _dev()
    w = record_window(rec).to(dev)
    pd = None
    if partials is not None:
        pd = torch.cat([partials, torch.full((GUARD,), math.nan)]).to(dev)     # a read past n_partials poisons the norm
    rc = lib.xvit_adam_prologue(pd.data_ptr() if pd is not None else None, 0 if partials is None else partials.numel(), w.data_ptr() + 8 * REC_GUARD,
                                max_norm, b1, b2, int(skip_nonfinite), _stream())
    torch.cuda.synchronize()
    return rc, record_of("xvit_adam_prologue", w)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def prologue_check(name, partials, rec0, rec, max_norm, b1, b2, skip_nonfinite, square=False, log=None):
    """Every field of the record after the prologue against float64."""
    total = float(partials.double().sum()) if partials is not None else 0.0
    norm = math.sqrt(total) if total == total and total >= 0 else math.nan
    got_norm = float(rec["grad_norm"])
    if math.isnan(norm) or math.isinf(norm):
        assert (math.isnan(got_norm) if math.isnan(norm) else got_norm == norm), f"{name}: grad_norm {got_norm!r}, want {norm!r}"
    elif square:
        assert float(np.float32(norm)) == norm and got_norm == norm, f"{name}: grad_norm {got_norm!r} != {norm!r} (the sum {total!r} is a perfect square)"
    else:
        assert abs(got_norm - norm) <= ulp32(norm), f"{name}: grad_norm {got_norm!r}, float64 {norm!r}: more than one fp32 ulp"
    coef = float(rec["clip_coef"])
    if math.isinf(f32(max_norm)):
        assert coef == 1.0, f"{name}: clip_coef {coef!r} with max_norm = inf"
    elif math.isnan(got_norm):
        assert math.isnan(coef), f"{name}: clip_coef {coef!r} for a NaN norm"
    else:
        q = f32(max_norm) / float(np.float32(got_norm) + np.float32(1e-6))      # the fp32 sum the kernel forms, then float64
        if q >= 1.0:
            assert coef == 1.0, f"{name}: clip_coef {coef!r}, want exactly 1 (max_norm / (norm + 1e-6) = {q!r})"
        else:
            assert abs(coef - q) <= C["div"] * EPS32 * q * SLACK, f"{name}: clip_coef {coef!r}, float64 {q!r}"
            if log is not None:
                note(f"{log}:need_div", abs(coef - q) / (EPS32 * q))
    skipped = bool(skip_nonfinite) and not (abs(got_norm) < math.inf)
    if skipped:
        assert int(rec["skip"]) == 1 and int(rec["skipped"]) == int(rec0["skipped"]) + 1 and int(rec["step"]) == int(rec0["step"]), f"{name}: {rec} after a skipped step"
        assert rec["lr_over_bc1"].tobytes() == rec0["lr_over_bc1"].tobytes() and rec["inv_sqrt_bc2"].tobytes() == rec0["inv_sqrt_bc2"].tobytes(), \
            f"{name}: a skipped step changed the bias corrections: {rec}"
    else:
        step = int(rec0["step"]) + 1
        assert int(rec["step"]) == step and int(rec["skip"]) == 0 and int(rec["skipped"]) == int(rec0["skipped"]), f"{name}: {rec}, want step {step}, skip 0"
        bc1, bc2 = 1.0 - math.pow(f32(b1), step), 1.0 - math.pow(f32(b2), step)
        L, I = float(rec0["lr"]) / bc1, 1.0 / math.sqrt(bc2)
        assert abs(float(rec["lr_over_bc1"]) - L) <= ulp32(L), f"{name}: lr_over_bc1 {float(rec['lr_over_bc1'])!r}, host double {L!r}"
        assert abs(float(rec["inv_sqrt_bc2"]) - I) <= ulp32(I), f"{name}: inv_sqrt_bc2 {float(rec['inv_sqrt_bc2'])!r}, host double {I!r}"
    assert rec["lr"].tobytes() == rec0["lr"].tobytes() and bytes(rec["reserved"].tobytes()) == bytes(rec0["reserved"].tobytes()), f"{name}: lr or the reserved words changed"


# ---------------------------------------------------------------------------------------------------------------- dropout mask
MASK64 = (1 << 64) - 1
EPOCH_MUL = 0xD1B54A32D192ED03


def hash32_int(seed, idx):
    """xvit_common.h:274 in Python integers (no numpy): the statement the numpy mirror is checked against."""
    z = (idx * 0x9E3779B97F4A7C15 + seed) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return ((z ^ (z >> 31)) >> 16) & 0xFFFFFFFF


def hash32_np(seed, idx, fault=None):
    """hash32 over a uint64 index array, wrapping multiplies -> uint64 array of 32-bit values."""
    u = np.uint64
    with np.errstate(over="ignore"):
        z = idx.astype(np.uint64) * u(0x9E3779B97F4A7C15) + u(seed & MASK64)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z = z ^ (z >> u(31))
    if fault != "the >> 16 of the hash dropped":
        z = z >> u(16)
    return z & u(0xFFFFFFFF)


def draw24_np(seed, n, start=0, fault=None):
    return hash32_np(seed, np.arange(start, start + n, dtype=np.uint64), fault) & np.uint64(0xFFFFFF)


def drop_params(p, fault=None):
    """The host-side Dropout(p, seed) -> (thr, inv as a float32 scalar)."""
    pf = np.float32(p)
    prod = pf * np.float32(16777216.0)
    thr = int(np.rint(prod)) if fault == "thr rounded instead of truncated" else int(prod)
    return thr, np.float32(1.0) / (np.float32(1.0) - pf)


def epoch_seed(seed, epoch, fault=None):
    if epoch is None:
        return seed & MASK64
    if fault == "the epoch constant added instead of multiplied":
        return (seed + epoch + EPOCH_MUL) & MASK64
    return (seed + epoch * EPOCH_MUL) & MASK64


def keep_mask(n, p, seed, epoch=None, fault=None, draw=None):
    """bool numpy array: element idx of xvit_dropout's mask.  draw: a cached draw24_np(epoch_seed(..), n) of at least n elements."""
    thr, _ = drop_params(p, fault)
    if draw is None:
        draw = draw24_np(epoch_seed(seed, epoch, fault), n, fault=fault)
    d = draw[:n]
    return d > np.uint64(thr) if fault == "> for >= in keep" else d >= np.uint64(thr)


def dropout_expected(x, p, seed, epoch=None, fault=None, draw=None):
    """What xvit_dropout leaves for the CPU tensor x (fp32 or bf16, 1-D): kept = the fp32 product x * inv (bf16: its RNE), dropped = +0."""
    keep = torch.from_numpy(keep_mask(x.numel(), p, seed, epoch, fault, draw))
    _, inv = drop_params(p)
    y = (x.float() * torch.tensor(float(inv), dtype=torch.float32)).to(x.dtype)
    return torch.where(keep, y, torch.zeros_like(y))


THRESHOLD_SEED, THRESHOLD_INDEX = 8, 1752363    # draw24(8, 1752363) == 4194304 == thr at p = 0.25 (hash32 = 0x1d400000); seeds 0..7 have no such index below 2^21 + 3


def where_drop(i):
    """Where element i sits in dropout_kernel (grid_for caps the grid at 4096 blocks of 256 threads)."""
    r, j = divmod(i, 4096 * 256)
    return f"element {i}: grid-stride round {r}, block {j // 256}, thread {j % 256}"


def assert_bits(name, got, want, where_fn=None, nan_ok=None):
    """got == want bit for bit (CPU tensors of one dtype); nan_ok: a bool mask of elements where any NaN is accepted for a NaN."""
    bad = _bits(got) != _bits(want)
    if nan_ok is not None:
        bad &= ~(nan_ok & torch.isnan(got) & torch.isnan(want))
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ; first at {where_fn(i) if where_fn else 'element %d' % i}: "
                             f"got {float(got[i])!r} ({int(_bits(got)[i]) & 0xFFFFFFFF:#x}), want {float(want[i])!r} ({int(_bits(want)[i]) & 0xFFFFFFFF:#x})")


def check_tail_guard(name, buf, n):
    """buf[n:] must still hold the sentinel, bit for bit."""
    g = buf[n:]
    bad = _bits(g) != _bits(torch.full_like(g, SENT))
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} guard elements behind element {n - 1} were overwritten; first at {n + int(bad.nonzero()[0])}: {float(g[int(bad.nonzero()[0])])!r}"


# ---------------------------------------------------------------------------------------------------------------- prologue cases
def prologue_cases():
    """(name, partials, square, max_norm, step0): n_partials x perfect square or not x the four kinds of max_norm; the step count cycles."""
    out, k = [], 0
    for n in (1, 255, 256, 257, 1000):
        for square in (True, False):
            part = prologue_partials(n, square)
            norm = f32(math.sqrt(float(part.double().sum())))
            for kind, mx in (("a third of the norm", f32(norm / 3)), ("0.9 of the norm", f32(0.9 * norm)), ("norm + 1e-6", float(np.float32(norm) + np.float32(1e-6))),
                             ("twice the norm", f32(2 * norm)), ("inf", math.inf)):
                out.append((f"prologue n_partials {n}, {'square' if square else 'non-square'} sum, max_norm {kind}, step {(0, 1, 999)[k % 3]} + 1",
                            part, square, mx, (0, 1, 999)[k % 3]))
                k += 1
    return out


def div_mirror_need():
    """The float32 CPU mirror of clip_coef over the prologue cases: the largest |fl32(max_norm / fl32(norm + 1e-6)) - float64 quotient| in units of u q."""
    need = 0.0
    for _, part, _, mx, _ in prologue_cases():
        if math.isinf(mx):
            continue
        den = np.float32(f32(math.sqrt(float(part.double().sum())))) + np.float32(1e-6)
        q = mx / float(den)
        if q < 1.0:
            need = max(need, abs(float(np.float32(mx) / den) - q) / (EPS32 * q))
    return need
THIRD_SEED, THIRD_INDEX = 13, 421518            # draw24(13, 421518) == 5592405 == thr at p = 1/3 (hash32 = 0xa5555555); seeds 0..12 have none


# ---------------------------------------------------------------------------------------------------------------- rows_combine
def rows_combine_cases(d):
    """Every dtype pairing of dst / dst2 / a / b (None: left out) at rows 1 and 3, and `dst is a` where their dtypes agree."""
    dts = (torch.float32, torch.bfloat16)
    for rows in (1, 3):
        for dst in dts:
            for dst2 in (None,) + dts:
                for a in (None,) + dts:
                    for b in (None,) + dts:
                        yield rows, d, dst, dst2, a, b, False
                        if a == dst:
                            yield rows, d, dst, dst2, a, b, True


def rows_combine_check(rows, d, dst_dt, dst2_dt, a_dt, b_dt, inplace):
    """One launch of xvit_rows_combine with four different row strides larger than d: inputs padded with NaN and a NaN guard row, destinations
    in sentinel windows ([rows + 1, ld], NaN where the kernel must write) compared bit for bit afterwards, results bit for bit against one
    fp32 add (a missing operand is zero) and, with a bf16 dst, its bf16 rounding in BOTH destinations (the rule of the kernel's comment)."""
    from xvit import _lib
    code = {torch.float32: 1, torch.bfloat16: 0, None: 0}
    name = f"rows_combine rows {rows} d {d} dst {dst_dt} dst2 {dst2_dt} a {a_dt} b {b_dt}{' in place' if inplace else ''}"
    gen = torch.Generator().manual_seed(rows + 7 * d)
    ld = {"dst": d + 3, "dst2": d + 5, "a": d + 2, "b": d + 7}

    def inp(dt, key, fill):
        if dt is None:
            return None, None
        v = torch.randn(rows, d, generator=gen).to(dt)
        buf = torch.full((rows + 1, ld[key]), fill, dtype=dt)
        buf[:rows, :d] = v
        return v, buf.to(_dev())
    if inplace:
        ld["a"] = ld["dst"]
    a, ad = inp(a_dt, "a", SENT if inplace else math.nan)
    b, bd = inp(b_dt, "b", math.nan)
    win = lambda dt, key: None if dt is None else torch.full((rows + 1, ld[key]), SENT, dtype=dt)   # noqa: E731
    w1, w2 = win(dst_dt, "dst"), win(dst2_dt, "dst2")
    w1[:rows, :d] = math.nan
    if w2 is not None:
        w2[:rows, :d] = math.nan
    d1 = ad if inplace else w1.to(_dev())
    d2 = w2.to(_dev()) if w2 is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = _lib.load().xvit_rows_combine(ptr(d1), code[dst_dt], ld["dst"], ptr(d2), code[dst2_dt], ld["dst2"] if d2 is not None else 0, ptr(ad), code[a_dt],
                                       ld["a"] if ad is not None else 0, ptr(bd), code[b_dt], ld["b"] if bd is not None else 0, rows, d, _stream())
    assert rc == 0, f"{name}: {last_error()}"
    v = torch.zeros(rows, d)
    if a is not None:
        v = a.float()
    if b is not None:
        v = v + b.float()
    if dst_dt == torch.bfloat16:
        v = v.bfloat16().float()
    for key, got, dt in (("dst", d1, dst_dt), ("dst2", d2, dst2_dt)):
        if got is None:
            continue
        got = got.cpu()
        want = torch.full_like(got, SENT)
        want[:rows, :d] = v.to(dt)
        bad = _bits(got) != _bits(want)
        if bool(bad.any()):
            r, c = (int(x) for x in bad.nonzero()[0])
            place = "the guard row" if r == rows else (f"the padding behind column {d - 1}" if c >= d else f"thread {c % 256}, pass {c // 256} of the column loop")
            raise AssertionError(f"{name}: {key}: {int(bad.sum())} elements differ; first at (row {r}, column {c}), {place}: got {float(got[r, c])!r}, want {float(want[r, c])!r}")
    for key, t0, td in (("a", a, ad), ("b", b, bd)):                 # the inputs come back untouched
        if td is not None and not (inplace and key == "a"):
            assert torch.equal(_bits(td.cpu()[:rows, :d]), _bits(t0)), f"{name}: input {key} was changed"
