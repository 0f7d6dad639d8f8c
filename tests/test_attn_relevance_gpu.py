"""GPU: xvit_attn_relevance_step against float64 on the CPU, fed the same bf16 q / k / v / dO and the GPU forward's lse.

    r_out[b, n] = r_in[b, n] + 1 / H sum_h sum_m r_in[b, m] max(0, P_h[b, m, n] dP_h[b, m, n])
    P_h[b, m, n] = exp(scale q[b, m, h] . k[b, n, h] - lse[b, h, m]),   dP_h[b, m, n] = dO[b, m, h] . v[b, n, h]

Gate: rel-L2 1.8e-7, 1.5 x the largest distance measured on an MI355X (XVIT_MEASURE_LOG: 1.2e-7, one-hot r_in at B = 3, H = 2, N = 130;
random r_in <= 1.2e-7, the peeled forward 8.3e-8), under the ceiling of 1e-6: fp32 accumulation and exp2 of the fp32 scores against float64
on the same rounded operands.  Invariants: two calls are bit-identical (fixed summation order, no
atomics), r_out >= r_in for r_in >= 0 and dO = 0 gives r_out == r_in bit for bit (1 / H times the sum is added to r_in last).  With
the v and dO rows of every head equal to e_0, dP == 1 and the relevance sum is twice the rollout kernel's."""
import pytest
import torch

from _util import dev, note, rel
from xvit import ops

pytestmark = pytest.mark.gpu

GATE = 1.8e-7
SHAPES = [(2, 3, 17), (1, 1, 64), (2, 2, 65), (3, 2, 130), (2, 12, 513), (1, 2, 1025), (1, 2, 4097), (2, 3, 1)]


def _inputs(B, N, H, seed):
    g = torch.Generator().manual_seed(seed)
    d = 64 * H
    qkv = torch.randn(B * N, 3 * d, generator=g).to(torch.bfloat16)
    do = torch.randn(B * N, d, generator=g).to(torch.bfloat16)
    return qkv, do


def _r_in(B, N, kind, seed):
    if kind == "onehot":
        r = torch.zeros(B, N)
        r[:, 0] = 1.0
        return r
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(B, N, generator=g) ** 4            # a spread of magnitudes, small entries included
    return r / r.sum(dim=1, keepdim=True)


def _reference(qkv, do, lse, r, B, N, H, scale):
    x = qkv.double().view(B, N, 3, H, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))                   # [B, H, N, 64]
    dO = do.double().view(B, N, H, 64).permute(0, 2, 1, 3)
    lse, r = lse.double(), r.double()
    acc = torch.zeros(B, N, dtype=torch.float64)
    for h in range(H):
        p = torch.exp(q[:, h] @ k[:, h].transpose(1, 2) * scale - lse[:, h, :, None])   # [B, N(m), N(n)]
        dp = dO[:, h] @ v[:, h].transpose(1, 2)
        acc += torch.einsum("bm,bmn->bn", r, (p * dp).clamp_min(0))
    return r + acc / H


def _run(qkv, do, B, N, H, scale, r, lse=None):
    qg, dg = qkv.to(dev()), do.to(dev())
    if lse is None:
        _, lse = ops.attn_fwd(qg, B, N, H, scale)
    return ops.attn_relevance_step(qg, lse, dg, r.to(dev()), B, N, H, scale), lse


@pytest.mark.parametrize("B,H,N", SHAPES, ids=[f"B{b}H{h}N{n}" for b, h, n in SHAPES])
@pytest.mark.parametrize("kind", ["onehot", "random"])
def test_relevance_step_vs_float64(B, H, N, kind):
    scale = 64 ** -0.5
    qkv, do = _inputs(B, N, H, seed=N + 7 * H + B)
    r = _r_in(B, N, kind, seed=N)
    out, lse = _run(qkv, do, B, N, H, scale, r)
    again, _ = _run(qkv, do, B, N, H, scale, r, lse)
    torch.cuda.synchronize()
    assert torch.equal(out, again), "two calls differ"
    assert (out.cpu() >= r).all(), "r_out < r_in"
    ref = _reference(qkv, do, lse.cpu(), r, B, N, H, scale)
    e = note(f"relevance_step_{kind}_B{B}H{H}N{N}", rel(out, ref))
    assert torch.isfinite(out).all() and e <= GATE, f"rel-L2 {e:.3e} > {GATE:g}"


@pytest.mark.parametrize("B,H,N", [(2, 3, 17), (2, 12, 513), (1, 2, 4097)])
def test_zero_gradient_leaves_r_unchanged(B, H, N):
    scale = 64 ** -0.5
    qkv, do = _inputs(B, N, H, seed=1)
    r = _r_in(B, N, "random", seed=2)
    out, _ = _run(qkv, torch.zeros_like(do), B, N, H, scale, r)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), r), "dO = 0 changed r"


@pytest.mark.parametrize("B,H,N", [(2, 3, 17), (2, 12, 513), (1, 2, 1025)])
def test_unit_gradient_is_twice_the_rollout_sum(B, H, N):
    """v and dO rows e_0 in every head: dP == 1, so relevance(r) - r == (1 / H) sum_h r P_h == 2 (rollout(r) - r / 2)."""
    scale = 64 ** -0.5
    qkv, do = _inputs(B, N, H, seed=5)
    v = qkv.view(B * N, 3, H, 64)[:, 2]
    v.zero_()
    v[..., 0] = 1.0
    do = torch.zeros_like(do)
    do.view(B * N, H, 64)[..., 0] = 1.0
    r = _r_in(B, N, "random", seed=6).to(dev())
    qg = qkv.to(dev())
    _, lse = ops.attn_fwd(qg, B, N, H, scale)
    got = ops.attn_relevance_step(qg, lse, do.to(dev()), r, B, N, H, scale) - r
    want = 2.0 * (ops.attn_rollout_step(qg, lse, r, B, N, H, scale) - 0.5 * r)
    torch.cuda.synchronize()
    e = rel(got, want)
    assert e <= 1e-6, f"relevance vs rollout: rel-L2 {e:.3e}"


def test_relevance_step_strided_and_peeled_forward():
    """q / k / v addressed through the qkv row stride at a shape whose forward takes the CLS-peel form (lse of token 0 from the merge)."""
    from xvit import _lib
    B, H, N, scale = 1, 12, 513, 64 ** -0.5
    lib = _lib.load()
    qkv, do = _inputs(B, N, H, seed=3)
    qg = qkv.to(dev())
    try:
        assert lib.xvit_set_option(b"attn_peel", 2) == 0
        assert lib.xvit_attn_fwd_workspace_bytes(B, H, N) > 0
        _, lse = ops.attn_fwd(qg, B, N, H, scale)
    finally:
        lib.xvit_set_option(b"attn_peel", 1)
    r = _r_in(B, N, "random", seed=9)
    out, _ = _run(qkv, do, B, N, H, scale, r, lse)
    torch.cuda.synchronize()
    e = note("relevance_step_peeled_fwd", rel(out, _reference(qkv, do, lse.cpu(), r, B, N, H, scale)))
    assert e <= GATE, f"rel-L2 {e:.3e} > {GATE:g}"
