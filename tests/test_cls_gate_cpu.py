"""The gate of the CLS-path kernels (tests/_cls_check.py) has teeth, on the CPU.

Planted faults.  Each starts from the oracle's own output, laid out in the windows a correct launch would leave (`lin_written`,
`small_written`, `ce_written`), plants ONE defect, and states two outcomes: the new check names it (always), and whether the old gate
would have seen it at the same shape.  The old gate is `_util.rel` at 2e-6 for xvit_linear_f32's fp32 outputs (3e-3 for its bf16 ones)
and `_util.assert_close` (1e-3) for small_linear / mean_ce.  Nothing was bent to make it miss; where it does see the fault the table
says so (it never ran at that shape, stride or content: see the paths the issue lists), and both outcomes are asserted.

  fault                                          new check   old gate (rel-L2, same data)
  one element of row M - 1 off by an ulp         caught      4.8e-9: not seen
  one element of column N - 1 off by an ulp      caught      2.7e-9: not seen
  one k term lost in one element                 caught      9.5e-4: seen (a whole product is far above 2e-6 of a 33 x 65 output)
  the last live split lost at K = 400            caught      0.27: seen
  an element never written (NaN)                 caught      NaN: seen (the comparison with NaN is false)
  a padding column overwritten                   caught      0: not seen (it never looks past column N)
  the guard row overwritten                      caught      0: not seen
  y_bf16 one ulp off                             caught      1.2e-3 on the 3e-3 bf16 gate: not seen
  z rounded from the post-GELU value             caught      0.62: seen
  the mask indexed with ldy instead of N         caught      0: not seen (the old suite runs ldy = N, where the fault changes nothing)
  dW with one row chunk missing (M = 9)          caught      0.18: seen
  db doubled                                     caught      1.0: seen
  the loss divided by B M                        caught      0.67: seen
  one dlogits_m copy stale                       caught      9.3e-5 on the 1e-3 gate: not seen

Mirror needs.  The float32 CPU mirror of gelu_parts and of the CE runs over the GPU tests' own inputs; its largest needs are printed,
noted, compared with the table in _cls_check's docstring, and every C is re-derived from them (power of two at or above 4 x the need).
The float64 tier's summation bound is checked against torch's own fp32 matmul on the same random operands."""
import math

import pytest
import torch

import _cls_check as X
from _cls_check import ACT_GELU, LinCase
from _util import TOL_F32, note, rel

OLD_F32, OLD_BF16 = 2e-6, 3e-3        # tests/test_linear_f32_gpu.py


def _caught(what, fn):
    with pytest.raises(AssertionError) as e:
        fn()
    print(f"caught: {what}: {str(e.value)[:300]}")
    return str(e.value)


def _ulp_up(t, r, c):
    t[r, c] = torch.nextafter(t[r, c], torch.tensor(math.inf, dtype=t.dtype))


def _lin(c):
    x, W, b, r = X.lin_operands(c)
    keep = X.hash_keep(c.M, c.N, c.p, c.seed) if c.p > 0 else None
    ora = X.lin_oracle(c, x, W, b, r, keep)
    wins = X.lin_written(c, ora, keep)
    X.lin_check(c, wins, ora)                                       # the unfaulted output passes
    return x, W, b, r, keep, ora, wins


# ---------------------------------------------------------------------------------------------------------------- the mirror of f32_split
def test_split_mirror_reaches_every_path():
    """The GPU cases are picked by the mirror of f32_split; this is what they are picked for."""
    assert [X.f32_split(5, 33, K) for K in (16, 32, 48, 64, 112, 128, 144)] == [1, 1, 1, 1, 1, 2, 2]        # the first split > 1 at K = 128
    assert X.f32_split(5, 33, 2048) == 32 and X.f32_split(5, 33, 3072) == 32                                  # the cap
    assert (X.f32_split(5, 32, 400), X.k_per_split(400, 6), X.live_splits(400, 6)) == (6, 80, 5)              # the last split starts at K
    assert (X.f32_split(5, 33, 2064), X.k_per_split(2064, 32), X.live_splits(2064, 32)) == (32, 80, 26)       # splits 26 .. 31 empty
    assert X.f32_split(126, 768, 768) == 10 and X.f32_split(126, 3072, 768) == 2 and X.f32_split(257, 1856, 128) == 1   # bounded by the tiles
    for M in (1, 33, 257):
        for N in (1, 65, 192):
            assert X.f32_split(M, N, 64) == 1 and X.f32_split(M, N, 256) == 4
    assert X.workspace_bytes(5, 33, 64) == 0 and X.workspace_bytes(5, 33, 256) == 4 * 5 * 33 * 4


# ---------------------------------------------------------------------------------------------------------------- planted faults: linear_f32
SPLIT = dict(bias=True, res=True, yb=True, wide=True)


def _plant_last_row(c, x, W, wins):
    _ulp_up(wins["y"], c.M - 1, 7)


def _plant_last_col(c, x, W, wins):
    _ulp_up(wins["y"], 3, c.N - 1)


def _plant_k_term(c, x, W, wins):
    r, col = 11, 40
    k = int((x[r] * W[col]).nonzero()[-1])
    wins["y"][r, col] -= x[r, k] * W[col, k]


def _plant_split(c, x, W, wins):                                   # K = 400: splits of 80, the last live one is [320, 400)
    wins["y"][:c.M, :c.N] -= x[:, 320:] @ W[:, 320:].T


def _plant_nan(c, x, W, wins):
    wins["y"][2, 5] = math.nan


def _plant_pad(c, x, W, wins):
    wins["y"][4, c.N] = 0.0


def _plant_guard(c, x, W, wins):
    wins["y"][c.M, 0] = 1.0


LIN_FAULTS = {"last_row": (LinCase(33, 65, 256, **SPLIT), _plant_last_row, False), "last_col": (LinCase(33, 65, 64, **SPLIT), _plant_last_col, False),
              "k_term": (LinCase(33, 65, 256, **SPLIT), _plant_k_term, True), "split_lost": (LinCase(5, 32, 400, **SPLIT), _plant_split, True),
              "nan": (LinCase(33, 65, 256, **SPLIT), _plant_nan, True), "pad_column": (LinCase(33, 65, 256, **SPLIT), _plant_pad, False),
              "guard_row": (LinCase(33, 65, 256, **SPLIT), _plant_guard, False)}


@pytest.mark.parametrize("fault", list(LIN_FAULTS))
def test_linear_fault_is_named(fault):
    c, plant, old_sees = LIN_FAULTS[fault]
    x, W, b, r, keep, ora, wins = _lin(c)
    plant(c, x, W, wins)
    msg = _caught(fault, lambda: X.lin_check(c, wins, ora))
    if fault in ("last_row", "last_col", "k_term", "nan"):
        assert "row" in msg and "32x32 tile" in msg
    e = rel(wins["y"][:c.M, :c.N], ora["y"])
    print(f"old gate on {fault}: rel-L2 {e:.3e} against {OLD_F32:g}")
    assert (not e < OLD_F32) == old_sees


def test_y_bf16_one_ulp_off_is_named():
    c = LinCase(33, 65, 256, **SPLIT)
    x, W, b, r, keep, ora, wins = _lin(c)
    t = wins["yb"]
    t[1, 1] = (t[1:2, 1:2].view(torch.int16) + 1).view(torch.bfloat16)[0, 0]
    _caught("y_bf16 one ulp off", lambda: X.lin_check(c, wins, ora))
    e = rel(wins["yb"][:c.M, :c.N].float(), ora["y"])
    print(f"old gate on y_bf16 one ulp off: rel-L2 {e:.3e} against {OLD_BF16:g}")
    assert e < OLD_BF16


def test_z_from_post_gelu_is_named():
    c = LinCase(33, 65, 64, bias=True, act=ACT_GELU, z=True, yb=True)
    x, W, b, r, keep, ora, wins = _lin(c)
    wins["z"][:c.M, :c.N] = X.gelu_mirror(ora["v"].float()).to(torch.bfloat16)
    _caught("z rounded from the post-GELU value", lambda: X.lin_check(c, wins, ora))
    e = rel(wins["z"][:c.M, :c.N].float(), ora["z"])
    print(f"old gate on z from post-GELU: rel-L2 {e:.3e} against {OLD_BF16:g}")
    assert e > OLD_BF16                                              # the old gate sees this one where it looks (one shape, packed)


def test_mask_with_the_wrong_row_stride_is_named():
    c = LinCase(33, 65, 256, p=0.25, seed=8, wide=True)
    x, W, b, r, keep, ora, wins = _lin(c)
    wrong = X.hash_keep(c.M, c.N, c.p, c.seed, row_stride=c.strides()["ldy"])
    assert not torch.equal(wrong, keep)
    wins["y"][:c.M, :c.N] = torch.where(wrong, ora["v"].float() * X.drop_inv(c.p), torch.zeros(c.M, c.N))
    _caught("mask indexed with ldy", lambda: X.lin_check(c, wins, ora))
    # the old suite launches with ldy = N only, where this fault is no fault: the mask it compares is the same
    assert torch.equal(X.hash_keep(c.M, c.N, c.p, c.seed, row_stride=c.N), keep)


# ---------------------------------------------------------------------------------------------------------------- planted faults: small_linear, mean_ce
def _small(M=9, N=2, K=768, with_z=False):
    o = X.small_operands(M, N, K, with_z=with_z)
    ora = X.small_oracle(o)
    wins = X.small_written(o, ora)
    X.small_check("small_linear", o, wins, ora)
    return o, ora, wins


def test_dW_with_a_row_chunk_missing_is_named():
    o, ora, wins = _small()
    M, K = o["x"].shape
    N = o["W"].shape[0]
    wins["dW"][0, :N * K] -= (o["dy"][8:].T @ o["x"][8:].float()).reshape(-1)       # rows = 8: the second chunk is row 8
    _caught("dW without its second row chunk", lambda: X.small_check("small_linear", o, wins, ora))
    e = rel(wins["dW"][0, :N * K].reshape(N, K), ora["dW"])
    print(f"old gate on dW chunk missing: rel-L2 {e:.3e} against {TOL_F32:g}")
    assert e > TOL_F32


def test_db_doubled_is_named():
    o, ora, wins = _small()
    N = o["W"].shape[0]
    wins["db"][0, :N] *= 2
    _caught("db doubled", lambda: X.small_check("small_linear", o, wins, ora))
    e = rel(wins["db"][0, :N], ora["db"])
    print(f"old gate on db doubled: rel-L2 {e:.3e} against {TOL_F32:g}")
    assert e > TOL_F32


def test_small_linear_dx_with_z_mirror_passes_and_truncation_is_named():
    o, ora, wins = _small(M=17, N=3, K=257, with_z=True)
    t = wins["dx"][:17, :257]
    acc = ora["acc"].float() * X.dgelu_mirror(o["z"].float())
    trunc = (acc.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)     # bf16 by truncation, not RNE
    assert not torch.equal(trunc, t)
    wins["dx"][:17, :257] = trunc
    _caught("dx truncated to bf16", lambda: X.small_check("small_linear", o, wins, ora))


def _ce(M=3, B=7, Cn=2, eps=X.f32(0.1), fault=None):
    lm, labels = X.ce_inputs("usual", M, B, Cn)
    return lm, labels, X.ce_ref(lm, labels, eps), X.ce_written(lm, labels, eps, fault=fault)


def test_loss_over_BM_is_named():
    lm, labels, ref, wins = _ce(fault="loss_over_BM")
    _caught("loss divided by B M", lambda: X.ce_check("mean_ce", wins, ref, 3, 7, 2))
    e = rel(wins["loss"][0, 0], ref["loss"])
    print(f"old gate on loss / (B M): rel-L2 {e:.3e} against {TOL_F32:g}")
    assert e > TOL_F32


def test_stale_dlogits_copy_is_named():
    lm, labels, ref, wins = _ce()
    X.ce_check("mean_ce", wins, ref, 3, 7, 2)
    g = torch.Generator().manual_seed(5)
    _, _, old = X.ce_mirror(lm + 1e-3 * torch.randn(lm.shape, generator=g), labels, X.f32(0.1))       # what a launch on slightly other logits left there
    wins["dl"][0, 14:28] = old[1].reshape(-1)
    msg = _caught("dlogits_m copy 1 stale", lambda: X.ce_check("mean_ce", wins, ref, 3, 7, 2))
    e = rel(wins["dl"][0, :42].reshape(3, 7, 2), ref["dl"])
    print(f"old gate on a stale dlogits_m copy: rel-L2 {e:.3e} against {TOL_F32:g}")
    assert e < TOL_F32
    # even a copy that is stale by less than its bound is named: the copies must agree bit for bit
    lm, labels, ref, wins = _ce()
    t = wins["dl"][0, 14:28]
    t[3] = torch.nextafter(t[3], torch.tensor(math.inf))
    assert "copy 1 differs" in _caught("dlogits_m copy 1 one ulp off", lambda: X.ce_check("mean_ce", wins, ref, 3, 7, 2))


# ---------------------------------------------------------------------------------------------------------------- the mirror's needs
def _gelu_inputs():
    """The pre-activations the GPU tests put through GELU: the exact-grid ones of the edge cases and the randn sites."""
    vs = []
    for M, N, K in ((33, 65, 64), (33, 65, 256), (5, 32, 400), (126, 3072, 768)):
        c = LinCase(M, N, K, bias=True, act=ACT_GELU, z=True)
        x, W, b, r = X.lin_operands(c)
        vs.append(X.lin_oracle(c, x, W, b, None, None)["v"].float().reshape(-1))
    for d, f in ((768, 3072), (1024, 4096)):
        c = LinCase(126, f, d, bias=True, act=ACT_GELU, tier="random")
        x, W, b, r = X.lin_operands(c)
        vs.append((x.double() @ W.double().T + b.double()).float().reshape(-1))
    return torch.cat(vs)


def test_gelu_mirror_need_sets_the_constant():
    v = _gelu_inputs()
    need = X.gelu_need(X.gelu_mirror(v), v)
    note("mirror:need_gelu", need)
    print(f"mirror need C_gelu {need:.2f} over {v.numel()} pre-activations in [{float(v.min()):.1f}, {float(v.max()):.1f}]")
    assert X.C["gelu"] == X.pow2_at_or_above(4 * need)
    X.check_bound("gelu mirror", X.gelu_mirror(v).reshape(1, -1), X.gelu64(v).reshape(1, -1), X.gelu_bound(v).reshape(1, -1))


def test_dgelu_mirror_need_sets_the_constant():
    need = 0.0
    for M in (1, 7, 8, 9, 17, 126):
        for K in (64, 200, 256, 257, 768, 1000, 3072):
            z = X.small_operands(M, 2, K, with_z=True)["z"].float()
            need = max(need, X.dgelu_need(X.dgelu_mirror(z), z))
    note("mirror:need_dgelu", need)
    print(f"mirror need C_dgelu {need:.2f}")
    assert X.C["dgelu"] == X.pow2_at_or_above(4 * need)


def test_ce_mirror_needs_set_the_constants():
    needs = {}
    for kind in X.CE_CONTENT:
        worst = {}
        for M in (1, 2, 3):
            for B in (1, 7, 255, 256, 257, 600):
                for Cn in (2, 3, 7):
                    lm, labels = X.ce_inputs(kind, M, B, Cn)
                    for eps in (0.0, X.f32(0.1)):
                        ref = X.ce_ref(lm, labels, eps)
                        got = X.ce_needs(*X.ce_mirror(lm, labels, eps), ref)
                        worst = {k: max(v, worst.get(k, 0.0)) for k, v in got.items()}
                        X.ce_check(f"mirror {kind} {M} {B} {Cn} {eps:g}", X.ce_written(lm, labels, eps), ref, M, B, Cn)
        print(f"mirror mean_ce {kind:9s}: need " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
        for k, v in worst.items():
            note(f"mirror:{kind}:need_{k}", v)
        needs = {k: max(v, needs.get(k, 0.0)) for k, v in worst.items()}
    for k, v in needs.items():
        assert X.C[k] == X.pow2_at_or_above(4 * v), f"{k}: mirror need {v:.3f}, C {X.C[k]:g}"


# ---------------------------------------------------------------------------------------------------------------- the summation bound
@pytest.mark.parametrize("d,f", [(768, 3072), (1024, 4096)])
def test_cpu_fp32_matmul_is_inside_the_float64_tiers_bound(d, f):
    """(K + split_k + 4) 2^-24 S is a worst case for any order of the additions: torch's own fp32 matmul on the sites' random operands
    has to pass it (the bound is not too tight), and does so by a wide margin (printed)."""
    for c in (LinCase(126, d, d, bias=True, res=True, tier="random"), LinCase(126, f, d, bias=True, tier="random"), LinCase(126, d, f, bias=True, res=True, tier="random"),
              LinCase(8, 2, f, bias=True, tier="random")):
        x, W, b, r = X.lin_operands(c)
        ora = X.lin_oracle(c, x, W, b, r, None)
        y = x @ W.T + b + (r if r is not None else 0.0)
        w = X.check_bound(f"{c}: torch fp32 matmul", y, ora["y"], ora["By"])
        print(f"{c}: torch's fp32 matmul uses {w:.4f} of the bound")
