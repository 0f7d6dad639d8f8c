"""GPU: the kernels of the fusion's low-rank form (csrc/head_linear.hip, xvit_xattn_kv_dgrad of csrc/cls_xattn.hip) element by element, through the C
entry points with every stride free, under the gate of tests/_head_check.py: bit for bit where the arithmetic is exact, against float64 under derived
bounds where it is not, sentinels around every destination and NaN behind every input.  The shapes are the smallest at which each mechanism can
fail (see _head_check's docstring for the mirror of the launch geometry that picks them); tests/test_head_gate_cpu.py shows on the CPU that the gate
names planted faults.  The rel-L2 tests of the same kernels (tests/test_head_linear_gpu.py, tests/test_kernels_gpu.py) stay as they are."""
import pytest
import torch

import _head_check as X
from _cls_check import device_keep

pytestmark = pytest.mark.gpu

BS = (1, 31, 32, 33, 65)
HS = (1, 3, 12, 16)


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("B", BS)
def test_head_rows(B, H):
    """The clamp of the rows past B, the second row tile, both production layouts of out, the bf16 copy absent / H / 16 head rows, ldx, ldw > d."""
    for c in X.rows_configs(B, H):
        X.run(c, log="head")


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("B", BS)
def test_head_cols(B, H):
    """The four K-quarters (two 8-deep steps each at H = 1), NaN in the head rows H .. 15 of t, every combination of row_scale / bias / bias_scale
    the model uses plus bias_scale without a bias, scales that differ by head and row, every stride free; two launches bit-equal."""
    for k, c in enumerate(X.cols_configs(B, H)):
        X.run(c, log="head", twice=k in (2, 4))


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("B", (1, 31, 32, 33, 64, 65))
def test_head_wgrad(B, H):
    """The tail of the 32-deep batch loop (padded lanes: scale 0, row 0 re-read; the rows behind B are NaN), row_scale absent / present, strides."""
    for k, c in enumerate(X.wgrad_configs(B, H)):
        X.run(c, log="head", twice=k > 0)


@pytest.mark.parametrize("B", (1, 65))
@pytest.mark.parametrize("d", (64, 768, 1024))
def test_head_bias_grad(d, B):
    """A partial block, three blocks, four; ldx > d, ldw > H."""
    for c in (X.bias_case(B, d), X.bias_case(B, d, wide=False), X.bias_case(B, d, tier="random")):
        X.run(c, log="head")


@pytest.mark.parametrize("H", X.SM_H)
@pytest.mark.parametrize("N", X.SM_N)
def test_cls_softmax_fwd(N, H):
    """Fewer rows than one pass, one pass, one pass plus a row, many passes; the four contents; lds 16 / 24, lde H / 8 / 16; dropout at two rates and
    two seeds with the mask of xvit_dropout on [B, H, N] (N = 1: a dropped column gives stat[2] = 0); two launches bit-equal."""
    p0 = {}
    for c in X.sm_configs(N, H):
        s = X.sm_scores(c)
        wins = X.sm_launch(c, s)
        if c.p == 0:
            X.sm_check(c, s, wins, log=f"head:softmax:{c.kind}")
            again = X.sm_launch(c, s)
            assert all(torch.equal(X._bits(wins[k]), X._bits(again[k])) for k in wins), f"{c}: two launches differ"
            continue
        keep = X.sm_keep(c)
        assert torch.equal(keep, device_keep(c.B * H, N, c.p, c.seed).reshape(c.B, H, N).permute(0, 2, 1)), f"{c}: hash_keep is not the mask of xvit_dropout"
        key = (c.lds, c.lde)
        if key not in p0:
            p0[key] = X.sm_launch(X.sm_case(c.B, H, N, c.kind, lds=c.lds, lde=c.lde), s)
        X.sm_check(c, s, wins, keep=keep, wins0=p0[key], log=f"head:softmax:drop{c.p:g}")
        if N == 1:      # stat[2] of a dropped column is exactly 0, of a kept one stat[1]
            stat = wins["stat"][0, :3 * c.B * H].reshape(3, c.B, H)
            assert torch.equal(stat[2], torch.where(keep[:, 0], stat[1], torch.zeros_like(stat[1]))), f"{c}: stat[2] at N = 1"


@pytest.mark.parametrize("H", X.SM_H)
@pytest.mark.parametrize("N", X.SM_N)
def test_cls_softmax_bwd(N, H):
    """Synthetic exact inputs (both halves of coef and ds_bf16 bit for bit, NaN in e's padding columns) and the forward's own outputs with a random dp
    (float64 on the very inputs), with and without dropout, every stride; two launches bit-equal."""
    for c in X.bw_configs(N, H):
        keep = X.sm_keep(c) if c.p > 0 else None
        i = X.bw_exact_inputs(c)
        wins = X.bw_launch(c, i)
        X.bw_check(c, wins, X.bw_oracle(c, i, keep))
        again = X.bw_launch(c, i)
        assert all(torch.equal(X._bits(wins[k]), X._bits(again[k])) for k in wins), f"{c}: two launches differ"
    for p, seed in ((0.0, 0), (0.25, 5)):
        f = X.sm_case(c.B, H, N, "random", lds=16, lde=16, p=p, seed=seed)
        fw = X.sm_launch(f, X.sm_scores(f))
        r = X.bw_case(c.B, H, N, lde=16, ldp=24, ldb=X.sm_lde(H, 1), p=p, seed=seed, tier="random")
        i = {"e": fw["e"][:c.B * N, :H].reshape(c.B, N, H), "rz": fw["stat"][0, :c.B * H].reshape(c.B, H), "dp": X.bw_random_dp(r)}
        X.bw_check(r, X.bw_launch(r, i, e_padding=0.0), X.bw_oracle(r, i, X.sm_keep(r) if p > 0 else None), log=f"head:softmax_bwd:drop{p:g}")


@pytest.mark.parametrize("H", X.KV_H)
@pytest.mark.parametrize("N", X.KV_N)
def test_xattn_kv_dgrad(N, H):
    """Both sides of every J2 boundary (2 H = 8, 16, 24, 32), one slice / several / a short last one, idle threads at d < 1024, lddh > d, NaN behind
    coef and R; dhn exists only in bf16: the round-to-nearest-even of the exact sum, or inside the bf16 interval of the float64 bound."""
    for c in X.kv_configs(N, H):
        o = X.kv_operands(c)
        X.kv_check(c, X.kv_launch(c, o), X.kv_oracle(c, o))


@pytest.mark.parametrize("H", (1, 5))
def test_xattn_kv_dgrad_second_staging_pass(H):
    """At B <= 3 a block never has more than 32 rows; B = 130, N = 600 gives 8 slices of 75: a full 64-row staging pass and one of 11."""
    assert X.xkv_geometry(130, 600, H)[:2] == (8, 75) and X.xkv_geometry(1, 130, H)[:2] == (5, 26) and X.xkv_geometry(3, 65, H)[:2] == (3, 22)
    c = X.kv_case(130, H, 600, wide=True)
    o = X.kv_operands(c)
    X.kv_check(c, X.kv_launch(c, o), X.kv_oracle(c, o))
