"""GPU: the fused attention kernels (csrc/attention.hip) element by element, at every tile edge, in every form and layout.

(a) every element of o, lse, dq, dk and dv against the float64 reference under the gate of tests/_attn_check.py, in the grid form
    (attn_peel 0), the CLS-peel form (2), the default heuristic (1) at its 768-workgroup switch point, and with probability dropout;
(b) a bit-exact uniform softmax (q = 0) at every N of (a) and in all three forms: each key's v enters exactly once;
(c) (b, h) independence, bitwise: one sample alone, and the heads in reverse order, against the full run;
(d) the raw C entry points on separate q / k / v / o / dO allocations with NaN-poisoned padding, NaN-prefilled outputs and
    workspaces, and canaries around every output;
(e) the online softmax's rescale branch forced by a dominant key placed in tile 0, the last full tile, the tail, key 0 and key N - 1.
Every test sets attn_peel itself and restores the default 1; the form a case ran in is asserted through xvit_attn_fwd_workspace_bytes."""
import contextlib
import math

import pytest
import torch

from _attn_check import attn_ref, check_bwd, check_fwd, heads
from _util import dev, exact_operands, randn, rt

pytestmark = pytest.mark.gpu


def _ops():
    from xvit import ops
    return ops


@contextlib.contextmanager
def peel_mode(mode):
    ops = _ops()
    ops.set_option("attn_peel", mode)
    try:
        yield
    finally:
        ops.set_option("attn_peel", 1)


def _is_peel(B, H, N):
    from xvit import _lib
    return _lib.load().xvit_attn_fwd_workspace_bytes(B, H, N) > 0


def _mask(B, H, N, p, seed):
    return _ops().dropout(torch.ones(B, H, N, N, device=dev()), p, seed).cpu()


def _run(qkv, do, B, N, H, scale, dropout=(0.0, 0)):
    """qkv [B, N, 3d] / do [B, N, d] fp32 CPU (bf16 values) -> o, lse, dqkv on the CPU (fp32)."""
    ops = _ops()
    d = H * 64
    qd = qkv.to(dev(), torch.bfloat16).reshape(B * N, 3 * d)
    o, lse = ops.attn_fwd(qd, B, N, H, scale, dropout=dropout)
    dqkv = ops.attn_bwd(qd, o, do.to(dev(), torch.bfloat16).reshape(B * N, d), lse, B, N, H, scale, dropout=dropout)
    return o.float().cpu(), lse.cpu(), dqkv.float().cpu()


def _element_case(B, H, N, mode, scale, *, p=0.0, seed=0, expect_peel=None, qkv=None, tag=""):
    """One case of sweep (a): device forward and backward, then one float64 reference shared by both checks."""
    d = H * 64
    qkv = rt(randn(B, N, 3 * d, seed=seed)) if qkv is None else qkv
    do = rt(randn(B, N, d, seed=seed + 1))
    dseed = 1000 + N
    with peel_mode(mode):
        peel = _is_peel(B, H, N) and p == 0.0
        if expect_peel is not None:
            assert peel == expect_peel, (B, H, N, mode, peel)
        o, lse, dqkv = _run(qkv, do, B, N, H, scale, dropout=(p, dseed))
    layout = "peel" if peel else "grid"
    q, k, v = (heads(t, B, N, H) for t in qkv.split(d, dim=-1))
    ref = attn_ref(q, k, v, scale, mask=_mask(B, H, N, p, dseed) if p else None, o_dev=heads(o, B, N, H), dO=heads(do, B, N, H))
    log = f"attn:{layout}{'-drop' if p else ''}:m{mode}:B{B}H{H}N{N}:s{scale:g}{tag}"
    check_fwd(ref, heads(o, B, N, H), lse, layout=layout, log=log)
    dq, dk, dv = (heads(t, B, N, H) for t in dqkv.split(d, dim=-1))
    check_bwd(ref, dq, dk, dv, layout=layout, log=log)
    return ref, (q, k, v), (heads(o, B, N, H), lse, dq, dk, dv)


# ---------------------------------------------------------------------------------------------------- (a) element-wise sweep
GRID_N = [1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 160, 161, 191, 192, 193, 255, 256, 257, 320, 321, 449, 513]
GRID_CASES = [(2, 3, n) for n in GRID_N] + [(1, 2, n) for n in (1000, 1025, 3376, 4097)] + [(1, 16, 129)]
PEEL_N = [64 * m + 1 for m in (1, 2, 3, 4, 5, 7, 8, 16, 64)]
PEEL_CASES = [(2, 3, n) for n in PEEL_N[:-1]] + [(1, 2, PEEL_N[-1])] + [(5, 3, 193)]   # odd B H: 2 B H N is no multiple of 4 floats


@pytest.mark.parametrize("B,H,N", GRID_CASES)
def test_grid_form_every_element(B, H, N):
    _element_case(B, H, N, 0, 0.125, seed=N, expect_peel=False)


@pytest.mark.parametrize("B,H,N", PEEL_CASES)
def test_peel_form_every_element(B, H, N):
    _element_case(B, H, N, 2, 0.125, seed=N + 1, expect_peel=True)


@pytest.mark.parametrize("B,H,N,peel", [(16, 12, 513, True), (15, 12, 513, False), (2, 16, 4097, True)])
def test_default_heuristic_every_element(B, H, N, peel):
    """attn_peel = 1 switches to the peel form at 768 workgroups: B = 16 x 12 heads x 4 query blocks is 768 (peel), B = 15 is 720."""
    _element_case(B, H, N, 1, 0.125, seed=N + 2, expect_peel=peel)


@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("N", [1, 33, 64, 65, 129, 200, 513])
def test_dropout_every_element(N, p):
    _element_case(2, 3, N, 2, 0.125, p=p, seed=N + 3, expect_peel=False)


@pytest.mark.parametrize("B,H,N,mode,p,peel", [(2, 3, 193, 0, 0.0, False), (1, 2, 1025, 0, 0.0, False), (2, 3, 193, 2, 0.0, True),
                                               (1, 2, 1025, 2, 0.0, True), (16, 12, 513, 1, 0.0, True), (2, 3, 129, 2, 0.1, False)])
def test_large_scale_every_element(B, H, N, mode, p, peel):
    """scale = 4: scores with a standard deviation near 32, many probabilities exactly 0 in fp32, rows dominated by a few keys."""
    _element_case(B, H, N, mode, 4.0, p=p, seed=N + 4, expect_peel=peel)


# ---------------------------------------------------------------------------------------------------- (b) bit-exact uniform softmax
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("N", sorted(set(GRID_N + PEEL_N + [1000, 3376])))
def test_uniform_softmax_bit_exact(N, mode):
    """q = 0: every score is exactly 0 on every path (the peel's token-0 state and merge included), p = exp2(0) = 1, l = N, and
    sum_k v is exact in fp32 in any order (v in {-3..3} / 4, |sum| <= 3 N / 4 < 2^24).  The tile path stores acc * (1 / l) with
    a correctly rounded fp32 reciprocal (no fast-math: -fhip-fp32-correctly-rounded-divide-sqrt is the default), the peel's
    merge stores acc / l: o is that fp32 value rounded to bf16, BIT-EQUAL.  lse = m scale + __logf(l) = ln N to a few fp32 ulps,
    which catches a missing or doubled key that o's rounding would hide (ln N - ln (N - 1) ~ 1 / N)."""
    B, H = 2, 3
    d = H * 64
    qkv = torch.cat((torch.zeros(B, N, d), rt(randn(B, N, d, seed=N)), exact_operands((B, N, d), seed=N, s=2)), dim=-1)
    with peel_mode(mode):
        peel = _is_peel(B, H, N)
        assert peel == (mode == 2 and N % 64 == 1 and N > 1 or mode == 1 and N % 64 == 1 and B * H * ((N + 126) // 128) >= 768)
        ops = _ops()
        o, lse = ops.attn_fwd(qkv.to(dev(), torch.bfloat16).reshape(B * N, 3 * d), B, N, H, 1.0)
    sv = qkv[..., 2 * d:].double().sum(1).float()                         # [B, d], exact
    nf = torch.tensor(float(N), dtype=torch.float32)
    want = (sv * (torch.tensor(1.0, dtype=torch.float32) / nf)).to(torch.bfloat16)
    got = o.cpu().reshape(B, N, d)
    rows = range(1, N) if peel else range(N)
    bad = [n for n in rows if not torch.equal(got[:, n], want)]
    assert not bad, f"o != bf16(sum v * (1/N)) at {len(bad)} rows, first {bad[0]} ({'peel' if peel else 'grid'} form)"
    if peel:   # token 0: the merge kernel divides
        assert torch.equal(got[:, 0], (sv / nf).to(torch.bfloat16)), "o row 0 != bf16(sum v / N) (peel merge)"
    lse_c = lse.cpu().double()
    err = (lse_c - math.log(N)).abs()
    tol = 4 * 2.0 ** -23 * max(math.log(N), 1.0)
    assert float(err.max()) <= tol, f"lse off ln {N} by {float(err.max()):.3g} (> {tol:.3g}) at {int(err.argmax())}"


# ---------------------------------------------------------------------------------------------------- (c) independence, bitwise
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("N", [129, 200])
def test_heads_and_samples_are_independent_bitwise(N, mode):
    B, H = 9, 5
    d = H * 64
    qkv = rt(randn(B, N, 3 * d, seed=N + 5))
    do = rt(randn(B, N, d, seed=N + 6))
    with peel_mode(mode):
        assert _is_peel(B, H, N) == (mode == 2 and N % 64 == 1)
        o, lse, dqkv = _run(qkv, do, B, N, H, 0.125)
        for b in range(B):
            ob, lb, gb = _run(qkv[b:b + 1], do[b:b + 1], 1, N, H, 0.125)
            assert torch.equal(ob, o.reshape(B, N, d)[b].reshape(N, d)), f"o of sample {b} alone"
            assert torch.equal(lb[0], lse[b]), f"lse of sample {b} alone"
            assert torch.equal(gb, dqkv.reshape(B, N, 3 * d)[b].reshape(N, 3 * d)), f"dqkv of sample {b} alone"
        rev = torch.arange(H - 1, -1, -1)
        flip = lambda t: t.reshape(*t.shape[:-1], -1, H, 64)[..., rev, :].reshape(t.shape)   # noqa: E731  (each 64-wide block, per q / k / v)
        qkv_r = torch.cat([flip(t) for t in qkv.split(d, dim=-1)], dim=-1)
        o_r, lse_r, dqkv_r = _run(qkv_r, flip(do), B, N, H, 0.125)
    assert torch.equal(flip(o_r), o), "o with the heads reversed"
    assert torch.equal(lse_r[:, rev], lse), "lse with the heads reversed"
    assert torch.equal(torch.cat([flip(t) for t in dqkv_r.split(d, dim=-1)], dim=-1), dqkv), "dqkv with the heads reversed"


# ---------------------------------------------------------------------------------------------------- (d) raw C entry, poisoned layout
NAN = float("nan")
CANARY = -1088.0     # exact in bf16 and fp32


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _poisoned(B, rows, cols, N, w, data=None, fill=NAN, dtype=torch.bfloat16):
    """[B, rows, cols] buffer on the GPU: the [B, N, w] region holds `data` (or NaN), the padding rows and columns `fill`."""
    t = torch.full((B, rows, cols), fill, dtype=dtype)
    t[:, :N, :w] = data if data is not None else NAN
    return t.to(dev())


def _padding_ok(t, N, w, fill):
    t = t.cpu()
    ref = torch.full_like(t, fill)
    pad = torch.ones(t.shape, dtype=torch.bool)
    pad[:, :N, :w] = False
    return torch.equal(_bits(t)[pad], _bits(ref)[pad])


POISON_CASES = [(f, n, 2, f"{f}-{n}") for f, n in (("grid", 65), ("grid", 129), ("grid", 200), ("peel", 65), ("peel", 129), ("dropout", 65), ("dropout", 200))]
POISON_CASES.append(("peel", 193, 5, "peel-193-B5"))


@pytest.mark.parametrize("form,N,B", [c[:3] for c in POISON_CASES], ids=[c[3] for c in POISON_CASES])
def test_raw_entry_points_poisoned_layout(N, form, B):
    """N = 65, 129: no tail in the peel form, a 1-key tail on the grid; N = 200: an 8-key tail.  B = 5 (odd B H, odd N): the peel
    partials of the backward workspace start on a padded, 16-byte aligned offset."""
    from xvit import _lib
    ops = _ops()
    lib = _lib.load()
    H, scale = 3, 0.125
    d = H * 64
    sn, osn = d + 24, d + 8
    p, seed = (0.1, 77) if form == "dropout" else (0.0, 0)
    qkv = rt(randn(B, N, 3 * d, seed=N + 7))
    do = rt(randn(B, N, d, seed=N + 8))
    with peel_mode(2 if form == "peel" else 0):
        assert _is_peel(B, H, N) == (form == "peel")
        qa, ka, va = (_poisoned(B, N + 3, sn, N, d, data=t) for t in qkv.split(d, dim=-1))
        doa = _poisoned(B, N + 2, osn, N, d, data=do)
        oa = _poisoned(B, N + 2, osn, N, d, fill=CANARY)
        dqa, dka, dva = (_poisoned(B, N + 3, sn, N, d, fill=CANARY) for _ in range(3))
        lse = torch.full((B * H * N + 64,), CANARY, device=dev())
        lse[:B * H * N] = NAN
        fws_b = lib.xvit_attn_fwd_workspace_bytes(B, H, N) if form == "peel" else 0
        bws_b = lib.xvit_attn_bwd_workspace_bytes(B, H, N)
        fws = torch.full((fws_b // 4 + 64,), CANARY, device=dev())
        fws[:fws_b // 4] = NAN
        bws = torch.full((bws_b // 4 + 64,), CANARY, device=dev())
        bws[:bws_b // 4] = NAN
        sb, osb = (N + 3) * sn, (N + 2) * osn
        stream = ops._stream()
        _lib.check(lib.xvit_attn_fwd(qa.data_ptr(), ka.data_ptr(), va.data_ptr(), sb, sn, oa.data_ptr(), osb, osn, lse.data_ptr(), B, H, N, 64,
                                     scale, p, seed, fws.data_ptr() if fws_b else None, fws_b, stream), "xvit_attn_fwd")
        _lib.check(lib.xvit_attn_bwd(qa.data_ptr(), ka.data_ptr(), va.data_ptr(), sb, sn, oa.data_ptr(), doa.data_ptr(), osb, osn, lse.data_ptr(),
                                     bws.data_ptr(), bws_b, dqa.data_ptr(), dka.data_ptr(), dva.data_ptr(), B, H, N, 64, scale, p, seed, stream),
                   "xvit_attn_bwd")
        o_ref, lse_ref, dqkv_ref = _run(qkv, do, B, N, H, scale, dropout=(p, seed))
    torch.cuda.synchronize()
    o, dq, dk, dv = (t.cpu()[:, :N, :d] for t in (oa, dqa, dka, dva))
    for name, t in (("o", o), ("lse", lse[:B * H * N].cpu()), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert not torch.isnan(t.float()).any(), f"{name}: {int(torch.isnan(t.float()).sum())} elements NaN (never written, or a poisoned read)"
    assert _padding_ok(oa, N, d, CANARY), "o: a canary in the padding changed"
    for name, t in (("dq", dqa), ("dk", dka), ("dv", dva)):
        assert _padding_ok(t, N, d, CANARY), f"{name}: a canary in the padding changed"
    for name, t, n in (("lse", lse, B * H * N), ("forward workspace", fws, fws_b // 4), ("backward workspace", bws, bws_b // 4)):
        assert bool((t[n:] == CANARY).all()), f"{name}: a canary past the end changed"
    assert torch.equal(o.float().reshape(B * N, d), o_ref), "o != the packed layout's"
    assert torch.equal(lse[:B * H * N].cpu().reshape(B, H, N), lse_ref), "lse != the packed layout's"
    assert torch.equal(torch.cat((dq, dk, dv), dim=-1).float().reshape(B * N, 3 * d), dqkv_ref), "dq | dk | dv != the packed layout's"


# ---------------------------------------------------------------------------------------------------- (e) forced rescale branches
def _spike_keys(N, peel):
    """The key j the spike goes to: tile 0, the last full tile, the tail (grid form with a tail only), key 0 and key N - 1."""
    g0 = 1 if peel else 0
    ng = N - g0
    full = ng // 64
    out = {"tile0": g0 + 5, "last_full_tile": g0 + 64 * (full - 1) + 7, "key0": 0, "key_last": N - 1}
    if ng % 64:
        out["tail"] = g0 + 64 * full + (ng % 64) // 2
    return out


@pytest.mark.parametrize("mode,N", [(0, 193), (0, 200), (0, 513), (2, 193), (2, 513)])
def test_rescale_branch_forced_everywhere(mode, N):
    """One query per 32-row wave of every workgroup (rows 32 w + 5) shares one q; a key j = 6 q (bf16-rounded) dominates all of
    them, placed in turn in each spot of _spike_keys: their running max jumps late, early, or at the peel's initial state."""
    B, H = 1, 2
    d = H * 64
    peel = mode == 2
    for where, j in _spike_keys(N, peel).items():
        qkv = rt(randn(B, N, 3 * d, seed=N + 11))
        rows = list(range(5, N, 32))
        qkv[:, rows, :d] = qkv[:, 5:6, :d]
        qkv[:, j, d:2 * d] = rt(qkv[:, 5, :d] * 6.0)
        ref, (q, k, _), (o, lse, dq, dk, dv) = _element_case(B, H, N, mode, 0.125, seed=N + 12, expect_peel=peel, qkv=qkv, tag=f":spike-{where}")
        # the rows the spike touches, one by one (a saturated softmax row has dq ~ 0: measure against the typical row norm)
        nq, nk = float(ref["dq"].norm()) / (N * H) ** 0.5, float(ref["dk"].norm()) / (N * H) ** 0.5
        for h in range(H):
            for n, t, r, typ in [(i, dq, ref["dq"], nq) for i in rows] + [(j, dk, ref["dk"], nk)]:
                e = float((t[0, h, n].double() - r[0, h, n]).norm()) / (float(r[0, h, n].norm()) + 0.05 * typ)
                assert e < 2e-2, (where, j, h, n, e)
