"""GPU: xvit_attn_rollout_step against float64 on the CPU, fed the same bf16 q / k and the GPU forward's lse.

    r_out[b, n] = r_in[b, n] / 2 + 1 / (2 H) sum_h sum_m r_in[b, m] exp(scale q[b, m, h] . k[b, n, h] - lse[b, h, m])

Gate: rel-L2 8.5e-8, 1.5 x the largest distance measured on an MI355X (XVIT_MEASURE_LOG: 5.5e-8, random r_in at B = 2, H = 12, N = 513;
one-hot r_in <= 4.5e-8, nearly one-hot rows <= 3.5e-8, N = 1 7.5e-9): fp32 accumulation and exp2 of the fp32 scores against float64 on
the same rounded operands.  Mass is conserved (sum_n r_out = sum_n r_in, since every row of P sums to one) and two calls are
bit-identical (fixed summation order, no atomics)."""
import pytest
import torch

from _util import dev, note, rel
from xvit import ops

pytestmark = pytest.mark.gpu

GATE = 8.5e-8
SHAPES = [(2, 3, 17), (1, 1, 64), (2, 2, 65), (3, 2, 130), (2, 12, 513), (1, 2, 1025), (1, 2, 4097), (2, 3, 1)]


def _qkv(B, N, H, seed, peaked=False):
    g = torch.Generator().manual_seed(seed)
    d = 64 * H
    qkv = torch.randn(B * N, 3 * d, generator=g)
    if peaked:   # key 3 (or the last) gets a large common component with every query: P is nearly one-hot on it
        q3 = qkv.view(B, N, 3, H, 64)
        hot = min(3, N - 1)
        u = torch.randn(64, generator=g)
        q3[:, :, 0] += 2.0 * u
        q3[:, hot, 1] += 2.0 * u
    return qkv.to(torch.bfloat16)


def _reference(qkv, lse, r, B, N, H, scale):
    d = 64 * H
    x = qkv.double().view(B, N, 3, H, 64)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)       # [B, H, N, 64]
    lse = lse.double()
    r = r.double()
    acc = torch.zeros(B, N, dtype=torch.float64)
    for h in range(H):
        p = torch.exp(q[:, h] @ k[:, h].transpose(1, 2) * scale - lse[:, h, :, None])   # [B, N(m), N(n)]
        acc += torch.einsum("bm,bmn->bn", r, p)
    assert d == qkv.shape[1] // 3
    return 0.5 * r + 0.5 / H * acc


def _r_in(B, N, kind, seed):
    if kind == "onehot":
        r = torch.zeros(B, N)
        r[:, 0] = 1.0
        return r
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(B, N, generator=g) ** 4            # a spread of magnitudes, small entries included
    return r / r.sum(dim=1, keepdim=True)


@pytest.mark.parametrize("B,H,N", SHAPES, ids=[f"B{b}H{h}N{n}" for b, h, n in SHAPES])
@pytest.mark.parametrize("kind", ["onehot", "random"])
def test_rollout_step_vs_float64(B, H, N, kind):
    scale = 64 ** -0.5
    qkv = _qkv(B, N, H, seed=N + 7 * H + B)
    qg = qkv.to(dev())
    _, lse = ops.attn_fwd(qg, B, N, H, scale)
    r = _r_in(B, N, kind, seed=N)
    out = ops.attn_rollout_step(qg, lse, r.to(dev()), B, N, H, scale)
    again = ops.attn_rollout_step(qg, lse, r.to(dev()), B, N, H, scale)
    torch.cuda.synchronize()
    assert torch.equal(out, again), "two calls differ"
    ref = _reference(qkv, lse.cpu(), r, B, N, H, scale)
    e = note(f"rollout_step_{kind}_B{B}H{H}N{N}", rel(out, ref))
    assert torch.isfinite(out).all() and e <= GATE, f"rel-L2 {e:.3e} > {GATE:g}"
    s_in, s_out = r.double().sum(dim=1), out.double().cpu().sum(dim=1)
    assert ((s_out - s_in).abs() / s_in).max() <= 1e-5, (s_in, s_out)


@pytest.mark.parametrize("N", [65, 513])
def test_rollout_step_nearly_one_hot_rows(N):
    """One key dominates every row: P is nearly one-hot, the rollout mass moves almost entirely onto that key."""
    B, H, scale = 2, 4, 64 ** -0.5
    qkv = _qkv(B, N, H, seed=11, peaked=True)
    qg = qkv.to(dev())
    _, lse = ops.attn_fwd(qg, B, N, H, scale)
    r = _r_in(B, N, "random", seed=5)
    out = ops.attn_rollout_step(qg, lse, r.to(dev()), B, N, H, scale)
    torch.cuda.synchronize()
    ref = _reference(qkv, lse.cpu(), r, B, N, H, scale)
    assert float(ref[:, 3].min()) > 0.45, "the test's P is not peaked"
    e = note(f"rollout_step_peaked_N{N}", rel(out, ref))
    assert e <= GATE, f"rel-L2 {e:.3e} > {GATE:g}"
    assert ((out.double().cpu().sum(dim=1) - r.double().sum(dim=1)).abs() <= 1e-5).all()


def test_rollout_step_strided_and_peeled_forward():
    """q / k addressed through the qkv row stride at a shape whose forward takes the CLS-peel form (lse of token 0 from the merge)."""
    from xvit import _lib
    B, H, N, scale = 1, 12, 513, 64 ** -0.5
    lib = _lib.load()
    qkv = _qkv(B, N, H, seed=3)
    qg = qkv.to(dev())
    try:
        assert lib.xvit_set_option(b"attn_peel", 2) == 0
        assert lib.xvit_attn_fwd_workspace_bytes(B, H, N) > 0
        _, lse = ops.attn_fwd(qg, B, N, H, scale)
    finally:
        lib.xvit_set_option(b"attn_peel", 1)
    r = _r_in(B, N, "random", seed=9)
    out = ops.attn_rollout_step(qg, lse, r.to(dev()), B, N, H, scale)
    torch.cuda.synchronize()
    e = note("rollout_step_peeled_fwd", rel(out, _reference(qkv, lse.cpu(), r, B, N, H, scale)))
    assert e <= GATE, f"rel-L2 {e:.3e} > {GATE:g}"
