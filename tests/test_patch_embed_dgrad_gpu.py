"""GPU: the input gradient of the patch embedding (xvit_patch_embed_dgrad: dX W scattered straight onto the voxel grid) and
xvit_unpatchify, bit for bit.

With the exact-arithmetic operands of _util.exact_operands every fp32 sum is exact in any order, so the kernel's fp32 volume must equal
a CPU dX @ W un-patchified with the oracle's patchify index map (oracle/ref_cpu.py:patchify) bit for bit, and its bf16 volume the
round-to-nearest-even of that.  The CLS rows of dX hold NaN: they are computed but never stored, so the volume stays finite.  The
output sits in a sentinel-filled buffer with margins that must come back untouched."""
import pytest
import torch

from _pe_check import DGRAD_SENTINEL as SENTINEL, MARGIN   # operands, reference and the margined output: shared with test_patch_embed_edges_gpu.py
from _pe_check import dgrad_operands as _operands, dgrad_reference as _reference, index_map as _index_map, sentinel_out as _sentinel_out
from _util import assert_exact, dev, exact_operands

pytestmark = pytest.mark.gpu

# (B, M, (D, H, W), patch, d)
GEOMS = [
    pytest.param(2, 2, (128, 128, 128), (16, 16, 16), 768, id="configs1-2052-rows"),       # 4 x 513 rows: not a multiple of the 256-row tile
    pytest.param(1, 2, (240, 240, 240), (16, 16, 16), 768, id="ucsf-240cube"),              # configs[2]: 15 patches per axis
    pytest.param(2, 3, (128, 128, 64), (16, 16, 8), 1024, id="mist"),                       # the reference's run shape: wp = 8
    pytest.param(5, 1, (64, 64, 64), (8, 8, 8), 256, id="wp8"),
    pytest.param(9, 2, (128, 32, 64), (16, 8, 16), 192, id="wp16-d192"),
    pytest.param(8, 2, (32, 64, 128), (8, 8, 32), 320, id="wp32-d320"),
    pytest.param(4, 4, (64, 32, 128), (4, 8, 64), 128, id="wp64-d128"),
    pytest.param(2, 1, (60, 40, 64), (3, 5, 8), 64, id="pd120-edge-columns"),              # pd = 120 < one 256-wide column tile
]

@pytest.mark.parametrize("B,M,vol,patch,d", GEOMS)
def test_dgrad_bit_exact(B, M, vol, patch, d):
    from xvit import ops
    shape = (B, M, 1, *vol)
    assert ops.patch_embed_dgrad_supported(shape, patch, d)
    dx, w = _operands(B, M, vol, patch, d, seed=B + d)
    ref = _reference(dx, w, B, M, vol, patch)
    gdx, gw = dx.bfloat16().to(dev()), w.bfloat16().to(dev())
    for dtype in (torch.float32, torch.bfloat16):
        buf, out = _sentinel_out(shape, dtype)
        got = ops.patch_embed_dgrad(gdx, gw, shape, patch, dtype, out=out)
        assert got.data_ptr() == out.data_ptr() and got.dtype == dtype
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), f"{dtype}: a CLS row (NaN) reached the volume"
        assert_exact(out, ref, f"dgrad {dtype}")
        margins = torch.cat([buf[:MARGIN], buf[-MARGIN:]]).float()
        assert (margins == SENTINEL).all(), f"{dtype}: a voxel outside the volume was written"
    again = ops.patch_embed_dgrad(gdx, gw, shape, patch, torch.float32)
    assert torch.equal(again, ops.patch_embed_dgrad(gdx, gw, shape, patch, torch.float32)), "not reproducible"


@pytest.mark.parametrize("B,M,vol,patch,d", [GEOMS[0], GEOMS[2]])
def test_fused_matches_fallback(B, M, vol, patch, d, monkeypatch):
    """The NN GEMM + xvit_unpatchify fallback (XVIT_PATCH_EMBED=unfused) computes the same exact volume."""
    import xvit.functional as XF
    shape = (B, M, 1, *vol)
    dx, w = _operands(B, M, vol, patch, d, seed=7)
    gdx, gw = dx.bfloat16().to(dev()), w.bfloat16().to(dev())
    fused = {dt: XF._input_grad(gdx, gw, shape, patch, False, dt) for dt in (torch.float32, torch.bfloat16)}
    monkeypatch.setenv("XVIT_PATCH_EMBED", "unfused")
    for dt, f in fused.items():
        assert torch.equal(XF._input_grad(gdx, gw, shape, patch, False, dt), f), dt


def test_fallback_batch_chunks_modelcross(monkeypatch):
    """The fallback cuts the batch into chunks (a strided batched NN GEMM over the modalities per chunk, then xvit_unpatchify into
    out[b0:b1]); with the chunk limit lowered to two samples, B = 3 runs as chunks of 2 and 1 and must still give the exact volume."""
    import xvit.functional as XF
    B, M, vol, patch, d = 3, 2, (128, 128, 128), (16, 16, 16), 768
    shape = (B, M, 1, *vol)
    P, pd = 512, 4096
    monkeypatch.setattr(XF, "_PATCH_GRAD_CHUNK_BYTES", 2 * M * (1 + P) * pd * 4)
    monkeypatch.setenv("XVIT_PATCH_EMBED", "unfused")
    dx, w = _operands(B, M, vol, patch, d, seed=11)
    ref = _reference(dx, w, B, M, vol, patch)
    gdx, gw = dx.bfloat16().to(dev()), w.bfloat16().to(dev())
    for dtype in (torch.float32, torch.bfloat16):
        assert_exact(XF._input_grad(gdx, gw, shape, patch, False, dtype), ref, f"chunked fallback {dtype}")


def test_fallback_batch_chunks_modelvit(monkeypatch):
    """ModelVIT's concatenated sequence (rows [sample][cls + M P]) in chunks of 2, 2 and 1 samples, against the exact CPU volume."""
    import xvit.functional as XF
    B, M, vol, patch, d = 5, 2, (32, 32, 16), (8, 8, 8), 128
    P, pd = 32, 512
    S = 1 + M * P
    monkeypatch.setattr(XF, "_PATCH_GRAD_CHUNK_BYTES", 2 * S * pd * 4)
    dx = exact_operands((B * S, d), 13, 2)
    w = exact_operands((d, pd), 14, 3)
    dx.view(B, S, d)[:, 0] = float("nan")                   # CLS rows: never read
    idx = _index_map(vol, patch).reshape(-1)
    ref = torch.empty(B, M, vol[0] * vol[1] * vol[2])
    rows = dx.view(B, S, d)[:, 1:].reshape(B, M, P, d)
    for m in range(M):
        ref[:, m].index_copy_(1, idx, (rows[:, m].reshape(B * P, d) @ w).reshape(B, -1))
    ref = ref.reshape(B, M, 1, *vol)
    gdx, gw = dx.bfloat16().to(dev()), w.bfloat16().to(dev())
    for dtype in (torch.float32, torch.bfloat16):
        assert_exact(XF._input_grad(gdx, gw, (B, M, 1, *vol), patch, True, dtype), ref, f"chunked ModelVIT fallback {dtype}")


# ---- xvit_unpatchify ----------------------------------------------------------------------------------------------------------

UNPATCH = [
    pytest.param(3, 2, (32, 32, 16), (8, 8, 8), id="vec-wp8"),
    pytest.param(2, 2, (32, 32, 2), (8, 8, 2), id="scalar-wp2"),         # the tiny config: runs of 2 voxels
    pytest.param(2, 3, (24, 20, 48), (4, 5, 16), id="vec-odd-grid"),
]


def _patch_rows(B, M, vol, patch, concat, seed):
    """Random fp32 patch rows in patchify's layout (CLS rows NaN) and the fp32 volume they come from (oracle index map)."""
    P = (vol[0] // patch[0]) * (vol[1] // patch[1]) * (vol[2] // patch[2])
    pd = patch[0] * patch[1] * patch[2]
    g = torch.Generator().manual_seed(seed)
    tok = torch.randn(B, M, P, pd, generator=g)                        # patch t of (b, m)
    idx = _index_map(vol, patch).reshape(-1)
    ref = torch.empty(B, M, vol[0] * vol[1] * vol[2])
    ref.index_copy_(2, idx, tok.reshape(B, M, -1))
    if concat:    # [B, 1 + M P, pd]
        rows = torch.cat([torch.full((B, 1, pd), float("nan")), tok.reshape(B, M * P, pd)], dim=1).reshape(-1, pd)
    else:         # [M, B, 1 + P, pd]
        rows = torch.cat([torch.full((M, B, 1, pd), float("nan")), tok.transpose(0, 1)], dim=2).reshape(M, B * (1 + P), pd)
    return rows.contiguous(), ref.reshape(B, M, 1, *vol)


@pytest.mark.parametrize("concat", [False, True], ids=["modelcross", "modelvit"])
@pytest.mark.parametrize("B,M,vol,patch", UNPATCH)
def test_unpatchify_bit_exact(B, M, vol, patch, concat):
    from xvit import ops
    rows, ref = _patch_rows(B, M, vol, patch, concat, seed=B * M)
    g = rows.to(dev())
    for dtype in (torch.float32, torch.bfloat16):
        buf, out = _sentinel_out((B, M, 1, *vol), dtype)
        ops.unpatchify(g, out, patch, pad_cls_row=not concat, concat=concat)
        torch.cuda.synchronize()
        assert_exact(out, ref, f"unpatchify {dtype}")
        assert (torch.cat([buf[:MARGIN], buf[-MARGIN:]]).float() == SENTINEL).all()


@pytest.mark.parametrize("concat", [False, True], ids=["modelcross", "modelvit"])
@pytest.mark.parametrize("B,M,vol,patch", UNPATCH + [pytest.param(1, 2, (128, 128, 128), (16, 16, 16), id="configs1")])
def test_unpatchify_inverts_patchify(B, M, vol, patch, concat):
    """unpatchify(patchify(v).float()) == v bit for bit for bf16 volumes, in both placements."""
    from xvit import ops
    v = torch.randn(B, M, 1, *vol, generator=torch.Generator().manual_seed(3)).bfloat16().to(dev())
    p = ops.patchify(v, patch, pad_cls_row=not concat, concat=concat).float()
    back = torch.empty_like(v)
    ops.unpatchify(p, back, patch, pad_cls_row=not concat, concat=concat)
    assert torch.equal(back, v)
    back32 = torch.empty(v.shape, dtype=torch.float32, device=dev())
    ops.unpatchify(p, back32, patch, pad_cls_row=not concat, concat=concat)
    assert torch.equal(back32, v.float())
