"""GPU: the CLS-query cross-attention kernels (xvit_cls_xattn_fwd / _bwd, csrc/cls_xattn.hip) called the way the fusion's literal order
calls them (xvit.functional.cross_forward / cross_backward with XATTN_FORM = "dense", and always above 16 heads): an fp32 query
(q_f32), the fp32 output copy (want_f32), k and v as the two halves of one [B*N, 2d] tensor, the backward on the query's bf16 copy and
the saved fp32 probabilities.  Every output against a float64 evaluation of the same operands, over head counts up to 32, sequence
lengths from 1 to the LDS bound of the score row (38 908; the dynamic-LDS attribute is raised from 14 333 on), large scores and
probability dropout with the kernels' own masks."""
import pytest
import torch

from _util import TOL_BF16, TOL_F32, dev, note, randn, rel, rt

pytestmark = pytest.mark.gpu

SCALE = 0.125       # 64 ** -0.5, the fusion's scale at its only head width


def _mask(shape, p, seed):
    """The probability-dropout mask of the kernels (0 or 1 / (1 - p)): xvit_dropout on ones, same seed, same element index
    ((b H + h) N + n)."""
    from xvit import ops
    return ops.dropout(torch.ones(*shape, device=dev()), p, seed).cpu()


def _check(B, H, N, seed=0, q_scale=1.0, p=0.0, drop_seed=0, tag=""):
    """One forward + backward against float64; -> the measured distances."""
    from xvit import ops
    d = 64 * H
    q = randn(B, d, seed=seed, scale=q_scale)                              # fp32, NOT bf16-representable: the q_f32 path must read it
    kv = rt(randn(B * N, 2 * d, seed=seed + 1))
    do = rt(randn(B, d, seed=seed + 2))
    kv_d = kv.to(dev(), torch.bfloat16)
    o, probs, of = ops.cls_xattn_fwd(q.to(dev()), kv_d, B, N, H, SCALE, dropout=(p, drop_seed), want_f32=True)
    qb = q.to(dev(), torch.bfloat16)                                       # the backward reads the query's bf16 copy (cross_forward's qb)
    dq, dkv = ops.cls_xattn_bwd(qb, kv_d, probs, do.to(dev(), torch.bfloat16), B, N, H, SCALE, dropout=(p, drop_seed))
    torch.cuda.synchronize()

    # float64 reference
    q64 = q.double().reshape(B, H, 1, 64).requires_grad_()
    k64, v64 = (t.double().reshape(B, N, H, 64).permute(0, 2, 1, 3).contiguous().requires_grad_() for t in kv.reshape(B, N, 2 * d).split(d, dim=-1))
    P = torch.softmax((q64 @ k64.transpose(-1, -2)) * SCALE, dim=-1)     # [B, H, 1, N]
    m = _mask((B, H, N), p, drop_seed).double()[:, :, None, :] if p > 0.0 else 1.0
    o64 = (P * m) @ v64
    o64.backward(do.double().reshape(B, H, 1, 64))
    # dk[n] = scale ds[n] q with the query the backward is handed (its bf16 copy); dq and dv do not read q
    with torch.no_grad():
        dp = (do.double().reshape(B, H, 1, 64) @ v64.transpose(-1, -2)) * m
        ds = P * (dp - (P * dp).sum(-1, keepdim=True)) * SCALE                # [B, H, 1, N]
        dk_ref = ds.transpose(-1, -2) @ qb.cpu().double().reshape(B, H, 1, 64)
        assert rel(ds.transpose(-1, -2) @ q64, k64.grad) < 1e-12            # the closed form is autograd's

    of_c, o_c, p_c = of.cpu(), o.cpu(), probs.cpu()
    assert torch.isfinite(of_c).all() and torch.isfinite(p_c).all() and torch.isfinite(dq.cpu()).all()
    assert torch.equal(o_c, of_c.to(torch.bfloat16)), f"{tag}: the bf16 output is not the rounding of the fp32 one"
    e = {"o_f32": rel(of_c, o64.detach().reshape(B, d)), "p": rel(p_c, P.detach().reshape(B, H, N))}
    dk, dv = (t.reshape(B, N, H, 64).permute(0, 2, 1, 3) for t in dkv.float().cpu().reshape(B, N, 2 * d).split(d, dim=-1))
    if N == 1:
        # one key: p = 1 exactly, ds = p (dp - p dp) = 0 exactly, so dq and dk vanish; dv = p' dO
        assert torch.equal(p_c, torch.ones_like(p_c)), f"{tag}: p != 1 at N = 1"
        assert torch.equal(dq.cpu(), torch.zeros_like(dq.cpu())) and torch.equal(dk, torch.zeros_like(dk)), f"{tag}: dq / dk not exactly 0 at N = 1"
    else:
        e["dq"] = rel(dq.cpu(), q64.grad.reshape(B, d))
        e["dk"] = rel(dk, dk_ref)
    e["dv"] = rel(dv, v64.grad)
    for k, v in e.items():
        note(f"cls_xattn.{tag}.{k}", v)
    # measured worst over every shape here: o_f32 7e-7, p 6e-7, dq 1.8e-6 (large scores), dk 1.8e-3, dv 1.8e-3 (one bf16 rounding)
    gates = {"o_f32": TOL_F32, "p": TOL_F32, "dq": TOL_F32, "dk": TOL_BF16, "dv": TOL_BF16}
    bad = {k: v for k, v in e.items() if not v <= gates[k]}
    assert not bad, f"{tag}: {bad} (gates {gates})"
    return e


# head counts at N = 65 and 513 (H > 16: the only form the fusion has there), sequence lengths at 3 and 20 heads
SHAPES = ([(2, H, N) for N in (65, 513) for H in (1, 3, 12, 16, 20, 32)]
          + [(2, H, N) for H in (3, 20) for N in (1, 2, 31, 32, 33, 3376, 4097)])


@pytest.mark.parametrize("B,H,N", SHAPES)
def test_cls_xattn_as_the_fusion_calls_it(B, H, N):
    _check(B, H, N, seed=B * 1000 + H * 10 + N, tag=f"B{B}H{H}N{N}")


@pytest.mark.parametrize("B,H,N", [(1, 2, 16385), (2, 1, 38908), (1, 3, 38908)])
def test_cls_xattn_large_lds_score_row(B, H, N):
    """N >= 14 333 needs more than 64 KiB of LDS (the kernels raise the function's dynamic-LDS limit); 38 908 is the largest N whose score
    row fits the 160 KiB of a CU."""
    _check(B, H, N, seed=N, tag=f"lds.B{B}H{H}N{N}")


@pytest.mark.parametrize("B,H,N", [(2, 3, 65), (2, 12, 513), (1, 20, 4097)])
def test_cls_xattn_large_scores(B, H, N):
    """A query 15x the usual size: scores with a spread of 15 (up to ~50), so the softmax is dominated by a few keys.  The max subtraction must
    keep everything finite and the outputs on the reference."""
    _check(B, H, N, seed=7 + N, q_scale=15.0, tag=f"big.B{B}H{H}N{N}")


@pytest.mark.parametrize("B,H,N", [(2, 1, 1), (2, 3, 33), (2, 12, 513), (1, 20, 4097), (1, 2, 16385)])
def test_cls_xattn_probability_dropout_as_the_fusion_calls_it(B, H, N):
    """Dropout on the probabilities at the reference's rate (model_cross.py:97): the backward regenerates the forward's mask; both must be
    the mask xvit_dropout draws for the same seed on a [B, H, N] tensor."""
    seed = 0x5EED0000 + N
    m = _mask((B, H, N), 0.25, seed)
    if B * H * N > 1000:
        assert abs(float((m != 0).double().mean()) - 0.75) < 0.03
    _check(B, H, N, seed=11 + N, p=0.25, drop_seed=seed, tag=f"drop.B{B}H{H}N{N}")
