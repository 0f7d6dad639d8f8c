"""Helpers for the GPU parity tests."""
import torch

# Tolerances: kernel and oracle get the SAME bf16-rounded
# operands; the kernel accumulates in fp32.
TOL_F32 = 1e-3    # fp32 outputs: the north-star's 1e-3 relative gate (observed ~1e-5)
TOL_BF16 = 3e-3   # bf16 outputs: 1e-3 + one bf16 rounding of the result (~1.6e-3 RMS, <=3.9e-3 max)


def dev():
    return torch.device("cuda:0")


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rt(t):
    """bf16 round trip on an fp32 tensor."""
    return t.to(torch.bfloat16).to(torch.float32)


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def assert_close(out, ref, what=""):
    tol = TOL_F32 if out.dtype == torch.float32 else TOL_BF16
    e = rel(out.float(), ref)
    assert torch.isfinite(out.float()).all(), f"{what}: non-finite output"
    assert e <= tol, f"{what}: rel-L2 {e:.3e} > {tol:g} ({out.dtype})"
    return e


def note(name, value):
    """Record a measured distance (XVIT_MEASURE_LOG=path appends "name value"): how the stated gates were calibrated."""
    import os
    path = os.environ.get("XVIT_MEASURE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{name} {value:.4e}\n")
    return value


# ---- exact-arithmetic operands: a bit-exact oracle for the GEMM at any size ------------------------------------------
# Operands in {-3..3} 2^-s are exact in bf16, every product is an integer multiple of 2^-(sa+sb) of magnitude <= 9 units, and
# every partial sum of K <= 2^24 / 9 (~1.8M) of them stays below 2^24 units: the fp32 sum is exact in ANY order (per K-split, in
# the split-K slab sum, with accumulate=True).  A plain fp32 matmul on the CPU is then the exact product, and the kernel's fp32
# output must equal it bit for bit (bf16 outputs: its round-to-nearest-even, ref.to(torch.bfloat16)).

def exact_operands(shape, seed, s):
    """fp32 CPU tensor of values in {-3..3} * 2^-s (exactly representable in bf16)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, tuple(shape), generator=g, dtype=torch.int8).float() * 2.0 ** -s


def exact_grid(shape, seed, unit, span):
    """fp32 CPU tensor of integers in [-span, span] times `unit` (bias / residual / accumulate prefill on the product's grid)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-span, span + 1, tuple(shape), generator=g, dtype=torch.int32).float() * unit


def bf16_ulp(x):
    """Spacing of bf16 numbers at |x| (0 at x = 0): 2^(e - 8) for |x| in [2^(e-1), 2^e)."""
    x = x.double()
    _, e = torch.frexp(x)
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 8))


def gemm_coords(shape, flat, tile=256):
    """Where element `flat` of a GEMM output of `shape` ([..., M, N], or [N]) sits in the 256x256 kernel: batch, (row, col), its
    256x256 tile, the 128x64 sub-tile of the wave (2 x 4 waves) and the 16x16 MFMA fragment inside that sub-tile.  tile=128: in the
    128x128 kernel instead (gemm_kernel): its 128x128 tile, the 64x64 sub-tile of the wave (2 x 2 waves) and the 16x16 fragment."""
    if tile == 128 and len(shape) == 1:
        return f"(col {flat}): 128x128 tile column {flat // 128}, wave sub-tile column {(flat % 128) // 64}, 16x16 fragment column {(flat % 64) // 16}"
    if tile == 128:
        M, N = shape[-2], shape[-1]
        b, rc = divmod(flat, M * N)
        r, c = divmod(rc, N)
        return (f"{'batch %d, ' % b if len(shape) > 2 else ''}(row {r}, col {c}): 128x128 tile ({r // 128}, {c // 128}), "
                f"wave sub-tile ({(r % 128) // 64}, {(c % 128) // 64}), 16x16 fragment ({(r % 64) // 16}, {(c % 64) // 16})")
    if len(shape) == 1:   # a row vector (column sums)
        return f"(col {flat}): 256x256 tile column {flat // 256}, wave sub-tile column {(flat % 256) // 64}, 16x16 fragment column {(flat % 64) // 16}"
    M, N = shape[-2], shape[-1]
    b, rc = divmod(flat, M * N)
    r, c = divmod(rc, N)
    return (f"{'batch %d, ' % b if len(shape) > 2 else ''}(row {r}, col {c}): 256x256 tile ({r // 256}, {c // 256}), "
            f"wave sub-tile ({(r % 256) // 128}, {(c % 256) // 64}), 16x16 fragment ({(r % 128) // 16}, {(c % 64) // 16})")


def assert_exact(out, ref, what="", tol=None, tile=256):
    """out (any device, fp32 / bf16) against the CPU reference: bit-equal to ref rounded to out's dtype, or (tol given: a
    tensor or scalar) |out - ref| <= tol element-wise.  NaN anywhere in out fails, so prefill outputs with NaN: an element
    that is never written fails too.  The message names the number of wrong elements and where the first one sits (tile: in which
    kernel's terms, see gemm_coords).  Returns the number of wrong elements it counted (0, or it would have raised)."""
    o = out.detach().cpu()
    assert o.shape == ref.shape, f"{what}: shape {tuple(o.shape)} != {tuple(ref.shape)}"
    if tol is None:
        bad = o != ref.to(o.dtype)
    else:
        bad = ~((o.double() - ref.double()).abs() <= tol)
    n = int(bad.sum())
    if n:
        flat = int(bad.reshape(-1).nonzero()[0])
        got, want = float(o.reshape(-1)[flat]), float(ref.reshape(-1)[flat])
        raise AssertionError(f"{what}: {n} of {o.numel()} elements wrong; first at {gemm_coords(tuple(o.shape), flat, tile)}: "
                             f"{got!r} != {want!r} ({o.dtype})")
    return n
