"""The fp32 kernels of the single-token CLS path, element by element: xvit_linear_f32 (MFMA kernel, split-K slab, reduce kernel,
epilogue), xvit_small_linear_fwd / _bwd, xvit_mean_ce, xvit_cls_row_fwd and xvit_embed_bwd, through the C entry points with every
stride free.  Bit for bit where the arithmetic is exact, against float64 under a derived bound where it is not; destinations NaN
where the kernel must write and sentinel everywhere else.  Oracle, launchers and gate: tests/_cls_check.py; the gate's own teeth:
tests/test_cls_gate_cpu.py.  Shapes are small: every case is a few launches of milliseconds."""
import pytest
import torch

import _cls_check as X
from _cls_check import ACT_GELU, LinCase
from _util import dev, note

pytestmark = pytest.mark.gpu

FULL = dict(bias=True, res=True, yb=True)                      # the full epilogue of the edge tests
# d / mlp of configs[1] and of the reference's own run shape
DIMS = ((768, 3072), (1024, 4096))
BATCHES = (1, 8, 126)


def _sites(d, f, B, tier):
    """The model's xvit_linear_f32 sites (functional.py cross_forward / HeadFn.forward).  Dropout next to a residual runs at p = 0.5
    on the exact tier (see _cls_check: the scale 2 is exact), at the reference's 0.25 elsewhere."""
    pr = 0.5 if tier == "exact" else 0.25
    return [LinCase(B, d, d, bias=True, yb=True, tier=tier, name=f"wq d{d} B{B}"),
            LinCase(B, d, d, bias=True, res=True, p=pr, seed=101, tier=tier, name=f"proj d{d} B{B}"),
            LinCase(B, f, d, bias=True, act=ACT_GELU, z=True, yb=True, p=0.25, seed=102, tier=tier, name=f"ffn1 d{d} B{B}"),
            LinCase(B, d, f, bias=True, res=True, p=pr, seed=103, tier=tier, name=f"ffn2 d{d} B{B}"),
            LinCase(B, f, d, bias=True, act=ACT_GELU, z=True, yb=True, tier=tier, name=f"head d{d} B{B}"),
            LinCase(B, 2, f, bias=True, tier=tier, name=f"logits d{d} B{B}")]


# ---------------------------------------------------------------------------------------------------------------- linear_f32, exact
@pytest.mark.parametrize("K", [64, 256])
def test_linear_f32_tile_edges(K):
    """Every edge of the 32x32 tile in M and N, full epilogue; K = 64: epilogue inside the MFMA kernel, K = 256: slab + reduce."""
    for M in (1, 2, 31, 32, 33, 63, 64, 65, 126, 257):
        for N in (1, 2, 31, 32, 33, 64, 65, 96, 192):
            X.lin_run(LinCase(M, N, K, **FULL))


@pytest.mark.parametrize("K", [16, 32, 48, 64, 112, 128, 144, 400, 2048, 2064, 3072])
def test_linear_f32_contraction_edges(K):
    """One step, odd step counts under the unroll by 2, the first split, the empty last split (K = 400), the cap of 32 splits and six
    empty splits (K = 2064)."""
    for wide in (False, True):
        X.lin_run(LinCase(5, 33, K, wide=wide, **FULL))
    if K == 400:
        X.lin_run(LinCase(5, 32, 400, **FULL))            # one tile: six splits of 80, the last one empty


@pytest.mark.parametrize("M,N,K", [(126, 768, 768), (126, 3072, 768), (257, 1856, 128)])
def test_linear_f32_split_bounded_by_tiles(M, N, K):
    X.lin_run(LinCase(M, N, K, **FULL))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("d,f", DIMS)
def test_linear_f32_model_sites_exact(d, f, B):
    for c in _sites(d, f, B, "exact"):
        X.lin_run(c, log=f"cls:exact:{c.name}")


EPILOGUES = {"none": dict(), "bias": dict(bias=True), "bias+res": dict(bias=True, res=True), "gelu+z+bf16": dict(act=ACT_GELU, z=True, yb=True),
             "bias+gelu+drop+z+bf16": dict(bias=True, act=ACT_GELU, p=0.25, seed=7, z=True, yb=True), "drop0.25": dict(p=0.25, seed=8),
             "drop0.5+res+bf16": dict(p=0.5, seed=9, res=True, yb=True), "bias+drop+res": dict(bias=True, p=0.5, seed=10, res=True)}


@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("M,N,K", [(33, 65, 64), (33, 65, 256), (5, 32, 400)])
def test_linear_f32_epilogue_cross(M, N, K, epi):
    for wide in (False, True):
        X.lin_run(LinCase(M, N, K, wide=wide, **EPILOGUES[epi]), log=f"cls:cross:{M}x{N}x{K}:{epi}")


def test_linear_f32_mask_is_the_hash_of_row_times_N():
    """The mask of xvit_dropout on a contiguous [M, N] tensor is hash32(seed, row * N + col): the CPU restatement the gate's own test
    plants its stride fault with is the device's mask."""
    for M, N, p, seed in ((33, 65, 0.25, 8), (5, 32, 0.5, 9), (126, 2, 0.1, 123456789012)):
        assert torch.equal(X.device_keep(M, N, p, seed), X.hash_keep(M, N, p, seed))


@pytest.mark.parametrize("K", [24, 50, 200])
def test_ops_linear_f32_padding_path(K):
    """ops.linear_f32 pads K that is not a multiple of 16 into scratch copies: exact, and the mask index uses N, not the padded K."""
    from xvit import ops
    M, N, p, seed = 5, 33, 0.5, 77
    c = LinCase(M, N, K, bias=True, res=True, p=p, seed=seed)
    x, W, b, r = X.lin_operands(c)
    keep = X.device_keep(M, N, p, seed)
    ora = X.lin_oracle(c, x, W, b, r, keep)
    y, yb, zb = ops.linear_f32(x.to(dev()), W.to(dev()), b.to(dev()), residual=r.to(dev()), want_bf16=True, dropout=(p, seed))
    X.assert_exact(y, ora["y"].float(), f"ops.linear_f32 K = {K}: y")
    X.assert_exact(yb, ora["y"].float(), f"ops.linear_f32 K = {K}: y_bf16")
    cg = LinCase(M, N, K, bias=True, act=ACT_GELU, z=True)
    og = X.lin_oracle(cg, x, W, b, None, None)
    y, _, zb = ops.linear_f32(x.to(dev()), W.to(dev()), b.to(dev()), act=ops.ACT_GELU, want_z=True)
    X.assert_exact(zb, og["z"].float(), f"ops.linear_f32 K = {K}: z_bf16")
    X.check_bound(f"ops.linear_f32 K = {K}: gelu y", y, og["y"], og["By"])


def test_ops_linear_f32_misaligned_view():
    from xvit import ops
    c = LinCase(9, 32, 64, bias=True)
    x, W, b, _ = X.lin_operands(c)
    big = torch.zeros(9, 4 * 64 + 1)
    big[:, 1:65] = x
    xv = big.to(dev())[:, 1:65]                                   # rows start 4 bytes off a 16-byte boundary
    assert xv.data_ptr() % 16 == 4
    y, _, _ = ops.linear_f32(xv, W.to(dev()), b.to(dev()))
    X.assert_exact(y, X.lin_oracle(c, x, W, b, None, None)["y"].float(), "ops.linear_f32 on a view 4 bytes off alignment")


def test_linear_f32_reproducible():
    for c in (LinCase(33, 65, 256, tier="random", **FULL), LinCase(126, 768, 768, tier="random", bias=True, act=ACT_GELU, z=True, yb=True, p=0.25, seed=5)):
        x, W, b, r = X.lin_operands(c)
        (rc1, w1), (rc2, w2) = X.lin_launch(c, x, W, b, r), X.lin_launch(c, x, W, b, r)
        assert rc1 == 0 and rc2 == 0
        for k in w1:
            if k != "ws":
                assert torch.equal(X._bits(w1[k]), X._bits(w2[k])), f"{c}: {k} differs between two launches"


def _set(**kw):
    return lambda a: a.update(kw)


def _bump(key, by):
    return lambda a: a.update({key: a[key] + by})


REFUSALS = {"K % 16": (_set(K=56), "multiple of 16"), "ldx % 4": (_bump("ldx", 2), "ldx/ldw"), "ldy < N": (_bump("ldy", -4), "ldy >= N"),
            "ldr < N": (_bump("ldr", -4), "ldr < N"), "ldz < N": (_bump("ldz", -6), "ldz / ldyb"), "ldyb < N": (_bump("ldyb", -2), "ldz / ldyb"),
            "x misaligned": (_bump("x", 4), "16-byte aligned"), "W misaligned": (_bump("W", 8), "16-byte aligned"), "act": (_set(act=2), "act must be"),
            "p = 1": (_set(p=1.0), "dropout_p"), "workspace null": (_set(ws=None), "workspace"), "workspace one byte short": (_bump("ws_bytes", -1), "workspace")}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_linear_f32_refusals(what):
    """Each returns rc < 0 with a message and leaves every destination as it was."""
    change, msg = REFUSALS[what]
    c = LinCase(5, 33, 256, bias=True, res=True, act=ACT_GELU, z=True, yb=True, p=0.25, seed=3, wide=True)
    x, W, b, r = X.lin_operands(c)
    rc, wins = X.lin_launch(c, x, W, b, r, change=change)
    assert rc < 0 and msg in X.last_error(), f"{what}: rc {rc}, message {X.last_error()!r}"
    before = X.lin_windows(c)
    for k, t in wins.items():
        assert torch.equal(X._bits(t), X._bits(before[k])), f"{what}: the refused call wrote to {k}"


# ---------------------------------------------------------------------------------------------------------------- linear_f32, float64
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("d,f", DIMS)
def test_linear_f32_model_sites_float64(d, f, B):
    for c in _sites(d, f, B, "random"):
        X.lin_run(c, log=f"cls:random:{c.name}")


def test_linear_f32_gelu_need_on_exact_preactivation():
    """GELU of an exactly known fp32 pre-activation: the device's need of C_gelu, logged next to the mirror's."""
    worst = 0.0
    for M, N, K in ((33, 65, 64), (33, 65, 256), (126, 3072, 768)):
        c = LinCase(M, N, K, bias=True, act=ACT_GELU, z=True, yb=True)
        wins, ora = X.lin_run(c)
        worst = max(worst, X.gelu_need(wins["y"][:M, :N], ora["v"].float()))
    note("cls:gelu:need_gelu", worst)
    print(f"device need C_gelu {worst:.2f} (C = {X.C['gelu']:g})")


# ---------------------------------------------------------------------------------------------------------------- small_linear
SMALL_M, SMALL_N, SMALL_K = (1, 7, 8, 9, 17, 126), (1, 2, 3, 7), (64, 200, 256, 257, 768, 1000, 3072)


@pytest.mark.parametrize("M", SMALL_M)
def test_small_linear_exact(M):
    """Forward and backward bit for bit on the exact grid: with and without bias, both values of `deterministic` (M = 9 and up: more than
    one row chunk at rows = 8), x / dx on strided views; with z the GELU' branch, dx against float64 (dW / db stay exact)."""
    for N in SMALL_N:
        for K in SMALL_K:
            for bias, with_z, det in ((True, False, 0), (False, False, 1), (True, True, 0), (False, True, 1)):
                o = X.small_operands(M, N, K, bias=bias, with_z=with_z)
                ora = X.small_oracle(o)
                rc_f, rc_b, wins = X.small_launch(o, det)
                assert rc_f == 0 and rc_b == 0, X.last_error()
                X.small_check(f"small_linear {M}x{N}x{K} bias {bias} z {with_z} deterministic {det}", o, wins, ora,
                              log=f"cls:small:exact:{M}x{N}x{K}" if with_z and N == 2 and det == 0 else None)


@pytest.mark.parametrize("det", [0, 1])
def test_small_linear_random_float64(det):
    """Random operands against float64 under the chain bounds; the deterministic form is bit-equal over two runs."""
    for M, N, K in ((9, 2, 768), (17, 3, 1000), (126, 2, 3072), (126, 7, 257)):
        for with_z in (False, True):
            o = X.small_operands(M, N, K, bias=True, with_z=with_z, tier="random")
            ora = X.small_oracle(o)
            rc_f, rc_b, wins = X.small_launch(o, det)
            assert rc_f == 0 and rc_b == 0, X.last_error()
            X.small_check(f"small_linear random {M}x{N}x{K} z {with_z} deterministic {det}", o, wins, ora, tier="random", log=f"cls:small:random:{M}x{N}x{K}:det{det}")
            if det:
                _, _, again = X.small_launch(o, det)
                for k in wins:
                    assert torch.equal(X._bits(wins[k]), X._bits(again[k])), f"small_linear {M}x{N}x{K}: {k} differs between two deterministic runs"


def test_small_linear_bwd_refuses_K_below_N():
    from xvit import _lib
    lib = _lib.load()
    t = torch.zeros(64, device=dev())
    rc = lib.xvit_small_linear_bwd(t.data_ptr(), t.data_ptr(), 4, t.data_ptr(), None, 0, t.data_ptr(), 4, t.data_ptr(), t.data_ptr(), 3, 7, 4, 0,
                                   torch.cuda.current_stream().cuda_stream)
    assert rc < 0 and "small_linear_bwd" in X.last_error()
    assert not bool(t.any())


# ---------------------------------------------------------------------------------------------------------------- mean_ce
@pytest.mark.parametrize("kind", X.CE_CONTENT)
def test_mean_ce(kind):
    """logits, loss and dlogits_m against float64 at every B around the 256 threads of the one block (B > 256: a thread loops), every
    copy count and class count, smoothing off and on; the M copies of dlogits_m bit-identical."""
    needs = {}
    for M in (1, 2, 3):
        for B in (1, 7, 255, 256, 257, 600):
            for Cn in (2, 3, 7):
                lm, labels = X.ce_inputs(kind, M, B, Cn)
                for eps in (0.0, X.f32(0.1)):
                    ref = X.ce_ref(lm, labels, eps)
                    rc, wins = X.ce_launch(lm, labels, eps)
                    assert rc == 0, X.last_error()
                    name = f"mean_ce {kind} M {M} B {B} C {Cn} smoothing {eps:g}"
                    X.ce_check(name, wins, ref, M, B, Cn)
                    got = X.ce_needs(wins["logits"][0, :B * Cn].reshape(B, Cn), wins["loss"][0, 0], wins["dl"][0, :M * B * Cn].reshape(M, B, Cn), ref)
                    needs = {k: max(v, needs.get(k, 0.0)) for k, v in got.items()}
    for k, v in needs.items():
        note(f"cls:mean_ce:{kind}:need_{k}", v)
    print(f"mean_ce {kind}: device needs " + ", ".join(f"{k} {v:.2f} (C = {X.C[k]:g})" for k, v in needs.items()))


# ---------------------------------------------------------------------------------------------------------------- cls_row / embed_bwd
@pytest.mark.parametrize("MB,N,d", [(1, 1, 4), (6, 17, 192), (3, 513, 768), (5, 2, 1028)])
def test_cls_row_fwd_and_embed_bwd(MB, N, d):
    e = X.embed_inputs(MB, N, d)
    rc, wins = X.embed_launch(e, MB, N, d)
    assert rc == [0, 0, 0], X.last_error()
    X.embed_check(f"embed {MB}x{N}x{d}", wins, X.embed_oracle(e), MB, N, d)


def test_embed_bwd_refuses_d_not_multiple_of_4():
    from xvit import _lib
    t = torch.zeros(64, device=dev())
    rc = _lib.load().xvit_embed_bwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), 2, 3, 6, torch.cuda.current_stream().cuda_stream)
    assert rc < 0 and "embed_bwd" in X.last_error()
    assert not bool(t.any())
