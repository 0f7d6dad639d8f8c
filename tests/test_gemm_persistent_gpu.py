"""The 256x256 GEMM's tile loop (csrc/gemm.hip: gemm_big_loop_kernel; xvit_set_option("gemm_persistent", n)): a few resident
workgroups walk many tiles, the K ring runs across tiles and the epilogue transposes inside the stage just consumed.  Per
tile the arithmetic and its order are those of the one-tile-per-workgroup launch, so C and aux must be bit-identical to
gemm_persistent = 1 on every form; the column sums are summed atomically in no fixed order and are compared with a float64
sum of the stored C instead.

gemm_tile = 2 sends these small grids to the 256x256 kernel.  M = 600 / 1000: 3 / 4 row tiles, the last one partial; N = 768 /
520: whole and partial column tiles; K = 64 / 128 / 768: a tile that is nothing but its boundary step, two steps, production
depth; 2 and 3 workgroups: unequal tile counts per workgroup, and a workgroup whose last tile has no successor.

The loop exists behind the 16-byte-per-lane bf16 epilogues (plain, bias, GELU with aux in both modes on NT, GELU' / x aux on
NN, column sums).  The forms that take the 8-byte-per-lane epilogue (fp32 C, residual, dropout, output segments, accumulate,
GELU on NN, GELU' on NT) launch one workgroup per tile under every setting: they are listed here so that the switch is known
to leave them alone.

Column sums: the kernel sums the fp32 values before their bf16 rounding, the reference the rounded ones.  The operands and the
aux tensor are drawn with a positive mean, so a column's sum grows with M while the rounding noise (2^-9 relative per element,
random sign) grows with sqrt(M): about 1e-4 of the sum at M = 600, inside the 1e-3 relative-L2 gate tests/test_gemm_gpu.py
applies to column sums (_util.assert_close).
"""
import pytest
import torch

from _util import assert_close, dev

gpu = pytest.mark.gpu

SHAPES = [(M, N, K) for M in (600, 1000) for N in (768, 520) for K in (64, 128, 768)]
FORMS = ["plain", "bias", "f32-bias-res", "f32-bias-res-rowmod", "gelu-aux-z", "gelu-aux-deriv", "dgelu-aux-z", "dgelu-aux-deriv", "dropout",
         "out-seg", "accumulate", "colsum"]


def _ops():
    from xvit import ops
    return ops


@pytest.fixture
def big_tile():
    ops = _ops()
    ops.set_option("gemm_tile", 2)
    try:
        yield ops
    finally:
        ops.set_option("gemm_tile", 0)
        ops.set_option("gemm_persistent", 0)


def _case(ops, form, layout, M, N, K, seed=5):
    """Operands and a run(persist) -> (C, aux or None, colsum or None) closure for one form; every run starts from the same
    prefilled destinations."""
    g = torch.Generator(device=dev()).manual_seed(seed + M + 7 * N + 13 * K)

    def rn(*s, mean=0.0, scale=1.0):
        return torch.randn(*s, device=dev(), generator=g) * scale + mean
    a = rn(M, K, mean=0.5, scale=0.5).bfloat16()
    b = rn(*((N, K) if layout == "NT" else (K, N)), mean=0.5 / K, scale=0.5 * K ** -0.5).bfloat16()
    lay = ops.NT if layout == "NT" else ops.NN
    f32 = form in ("f32-bias-res", "f32-bias-res-rowmod", "out-seg", "accumulate")
    kw, rows = {}, M
    if form != "plain" and not form.startswith("dgelu") and form != "colsum":
        kw["bias"] = rn(N, mean=0.25, scale=0.25)
    if form.startswith("f32-bias-res"):
        mod = 513 if form.endswith("rowmod") else 0
        kw["residual"] = rn(mod + 3 if mod else M, N)
        if mod:
            kw["res_row_mod"], kw["res_row_off"] = mod, 3
    if form.startswith("gelu"):
        kw["act"], kw["aux_mode"] = ops.ACT_GELU, int(form.endswith("deriv"))
    if form.startswith("dgelu"):
        kw["act"], kw["aux_mode"] = ops.ACT_DGELU, int(form.endswith("deriv"))
        aux_in = torch.rand(M, N, device=dev(), generator=g).bfloat16()     # gelu'(z) lies in [-0.13, 1.13]; as z: any value
    if form == "dropout":
        kw["dropout"] = (0.25, 1234)
    if form == "out-seg":
        kw["out_seg"] = (100, 3, 2)
        rows = M + (M // 100) * 3 + 2 + 1
    if form == "accumulate":
        kw["accumulate"] = True
    want_cs = form in ("colsum", "dgelu-aux-deriv", "bias")
    prefill = rn(rows, N)

    def run(persist):
        ops.set_option("gemm_persistent", persist)
        C = prefill.clone() if f32 else prefill.bfloat16()
        k2 = dict(kw)
        aux = None
        if form.startswith("gelu"):
            aux = k2["aux"] = torch.full((M, N), -7.0, dtype=torch.bfloat16, device=dev())
        elif "aux_mode" in k2:
            k2["aux"] = aux_in
        cs = None
        if want_cs:
            cs = k2["colsum"] = torch.zeros(N, device=dev())
        ops.gemm(lay, a, b, C, **k2)
        return C, aux, cs
    return run


def _same(x, y, what):
    assert x.dtype == y.dtype and torch.equal(x, y), f"{what}: {int((x != y).sum())} of {x.numel()} elements differ"


@gpu
@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("layout", ["NT", "NN"])
@pytest.mark.parametrize("form", FORMS)
def test_tile_loop_changes_no_bit(big_tile, form, layout, M, N, K):
    run = _case(big_tile, form, layout, M, N, K)
    C1, aux1, _ = run(1)
    assert torch.isfinite(C1.float()).all()
    for n in (2, 3):
        C, aux, cs = run(n)
        _same(C, C1, f"C, gemm_persistent = {n}")
        if aux is not None:
            _same(aux, aux1, f"aux, gemm_persistent = {n}")
        if cs is not None:
            assert_close(cs, C.double().sum(0).cpu(), f"colsum, gemm_persistent = {n}")


@gpu
@pytest.mark.parametrize("layout,form", [("NT", "gelu-aux-deriv"), ("NN", "dgelu-aux-deriv")])
def test_same_call_twice(big_tile, layout, form):
    """A stage handed to the next tile's loads before the epilogue has read it back would show as a run-to-run difference."""
    run = _case(big_tile, form, layout, 1000, 520, 128)
    C0, aux0, _ = run(3)
    C1, aux1, _ = run(3)
    _same(C0, C1, "C")
    if aux0 is not None:
        _same(aux0, aux1, "aux")


def test_switch_values():
    """Host only: 0 (auto), 1 (one workgroup per tile) and 2 .. 4096 (workgroups of the loop) are taken, the rest refused."""
    from xvit import _lib
    lib = _lib.load()
    try:
        for v in (1, 2, 3, 4096):
            assert lib.xvit_set_option(b"gemm_persistent", v) == 0
        assert lib.xvit_set_option(b"gemm_persistent", 4097) < 0 and b"gemm_persistent" in lib.xvit_last_error_string()
        assert lib.xvit_set_option(b"gemm_persistent", -1) < 0
    finally:
        assert lib.xvit_set_option(b"gemm_persistent", 0) == 0
