"""The element-wise check of the fused patch embedding (xvit_patch_embed_fwd / _wgrad: the gather paths of csrc/gemm.hip), shared by
the GPU test of its grid and split edges (tests/test_patch_embed_edges_gpu.py) and the CPU gate on the check itself
(tests/test_pe_gate_cpu.py); the helpers of the input-gradient check (tests/test_patch_embed_dgrad_gpu.py) live here too.

The volume, W and dx are small integers times a power of two (_util.exact_operands), bias and pos integers on the product's grid
(_util.exact_grid): with at most 8256 terms of at most 9 units, plus 288 units of bias and pos, every partial sum stays far below 2^24
units, so every fp32 sum is exact in ANY order and the kernels' fp32 outputs must equal the CPU reference bit for bit, element by
element.  The reference patch rows come from the oracle's index map (oracle/ref_cpu.py:patchify), not from xvit_patchify.

  reference(case)            CPU: operands and the expected x (by x_ref: with / without bias and pos) and dW
  launch_fwd / launch_wgrad  GPU: the raw C entry points with every stride free; outputs prefilled with NaN where they must be
                             written and a sentinel everywhere else (padding columns and rows, margins); NaN in every operand padding
                             column, in the CLS rows of dx, in two rows behind dx and around the volume; a NaN-filled workspace of
                             exactly the size the library asks for (a split that does not write its zero slab shows up as NaN in dW)
  compare(case, ref, out)    CPU: every written element bit for bit, every element that must not be written against the sentinel
  ideal(case, ref)           the destinations as a faultless kernel leaves them (the CPU gate plants its faults into these)

The host logic that picks the kernels' branches (pe_aligned, pe_wgrad_split, k_per_split of csrc/gemm.hip) is restated in Python
(classify), so that every case records the class it stands for; the GPU test holds the restatement against the library's own
workspace size."""
import ctypes as C
from dataclasses import dataclass
from functools import lru_cache

import torch

import ref_cpu as R
from _util import assert_exact, dev, exact_grid, exact_operands

NAN = float("nan")
SENTINEL = -1232.0       # exact in bf16 and fp32: what every element outside an output holds before and after
MARGIN = 4096            # elements in front of and behind every output (and the volume, and the workspace)
PAD_ROWS = 2             # rows behind the last row of x, dx and dW
X_PAD, POS_PAD, W_PAD, DX_PAD, DW_PAD = 4, 4, 8, 8, 4    # ldx = d + 4, ldpos = d + 4, ldw = pd + 8, lddx = d + 8, lddw = pd + 4
SV, SW, SX = 2, 3, 2     # volume, W, dx in {-3..3} 2^-s: the forward's unit is 2^-(SV + SW), the weight gradient's 2^-(SX + SV)
BK = 64                  # depth of a K-step


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    M: int
    vol: tuple       # (D, H, W)
    patch: tuple     # (dp, hp, wp)
    d: int
    cls: int = 1
    seed: int = 5

    @property
    def grid(self):
        return tuple(v // p for v, p in zip(self.vol, self.patch))      # (Dn, Hn, Wn)

    @property
    def P(self):
        Dn, Hn, Wn = self.grid
        return Dn * Hn * Wn

    @property
    def pd(self):
        return self.patch[0] * self.patch[1] * self.patch[2]

    @property
    def ntok(self):
        return self.cls + self.P

    @property
    def rows(self):
        return self.M * self.B * self.ntok

    @property
    def K(self):
        """The weight gradient's contraction: every patch row, CLS rows skipped."""
        return self.M * self.B * self.P

    @property
    def shape(self):
        return (self.B, self.M, 1) + tuple(self.vol)

    @property
    def tag(self):
        return f"{self.name} B {self.B} M {self.M} volume {self.vol} patch {self.patch} d {self.d}"


# (id, B, M, volume, patch, d[, cls_rows]) -- what each reaches is computed by classify() and pinned by tests/test_pe_gate_cpu.py
CASES = [Case(*c) for c in [
    ("dn64-identity", 16, 2, (64, 8, 32), (1, 8, 32), 256),        # mode 2, nw = 1 (identity k-row order), Wn = 1, rows % 256 = 32
    ("dn64-h2-w2", 4, 2, (64, 16, 64), (1, 8, 32), 256),           # mode 2, nw = 1, Hn = 2, wsteps = 2
    ("dn32-pairs", 8, 4, (32, 8, 64), (1, 8, 32), 256),            # mode 2, nw = 2
    ("dn16-h2", 6, 3, (16, 32, 64), (1, 16, 16), 512),             # mode 2, nw = 4, Hn = 2, 9 K-steps per split
    ("dn8-uneven", 11, 3, (32, 8, 64), (4, 8, 8), 256),            # mode 2, nw = 8, splits of 9, 9, 9, 6 K-steps, rows % 256 = 97
    ("dn4-h3", 6, 2, (16, 24, 128), (4, 8, 8), 256),               # mode 2, nw = 16, Hn = 3
    ("dn2", 16, 2, (8, 8, 256), (4, 8, 8), 256),                   # mode 2, nw = 32
    ("dn1", 8, 2, (4, 16, 512), (4, 8, 8), 256),                   # mode 2, Dn = 1, nw = 64, Hn = 2
    ("wp64", 18, 2, (8, 4, 512), (1, 4, 64), 256),                 # wp = 64, hp = 4
    ("wp16-uneven", 17, 2, (16, 4, 256), (4, 4, 16), 256),         # wp = 16, splits of 9, 9, 9, 7 K-steps
    ("pd1024-d768", 8, 2, (64, 32, 64), (4, 16, 16), 768),         # 3 x 4 output tiles of dW, 16 K-steps in the forward
    ("m2-empty-split", 43, 3, (64, 8, 32), (1, 8, 32), 256),       # mode 2, 16 splits: 14 of 9 K-steps, one of 3, one of nk = -5
    ("m3-9tok-M1", 205, 1, (12, 8, 24), (4, 8, 8), 256),           # mode 3, P = 9: a K-step holds 7+ samples, K % 64 = 53, nb = 205
    ("m3-9tok-M5", 41, 5, (12, 8, 24), (4, 8, 8), 256),            # the same with modality boundaries inside K-steps
    ("m3-1tok", 512, 2, (4, 8, 8), (4, 8, 8), 256),                # P = 1: every divisor but nb is 1, ntok = 2, rows % 256 = 0
    ("m3-1tok-empty", 1040, 4, (4, 8, 8), (4, 8, 8), 256),         # 16 splits: 13 of 5 K-steps, then nk = 0, -4, -9
    ("m3-63tok", 16, 2, (28, 24, 24), (4, 8, 8), 256),             # P = 63
    ("m3-65tok", 16, 2, (20, 104, 8), (4, 8, 8), 256),             # P = 65, Wn = 1
    ("m3-dn128", 8, 1, (128, 16, 32), (1, 8, 32), 512),            # mode 3 with K % 64 = 0, Dn > 64, Wn = 1
    ("m3-3x8x1", 84, 1, (12, 64, 8), (4, 8, 8), 768),              # Wn = 1, K % 64 = 32, three row tiles of dW
    ("m3-5x3x7", 20, 1, (20, 24, 56), (4, 8, 8), 256),             # the 5 x 3 x 7 grid of test_patch_embed_gpu.py at 1/16 of its voxels
    ("m3-cls0", 36, 1, (4, 120, 32), (4, 8, 8), 256, 0),           # cls_rows = 0, Dn = 1 in mode 3
    ("m2-cls0", 33, 1, (32, 8, 64), (4, 8, 8), 256, 0),            # cls_rows = 0 in mode 2, splits of 9, 9, 9, 6 K-steps
    # 1 to 3 rows per sample: the forward's epilogue steps 4 rows at a time through a pos table shorter than that (with m3-1tok: ntok = 2)
    ("m3-2tok", 683, 1, (8, 8, 8), (4, 8, 8), 256),                # P = 2, ntok = 3, rows % 256 = 1
    ("m3-1tok-cls0", 2048, 1, (4, 8, 8), (4, 8, 8), 256, 0),       # P = 1 and cls_rows = 0: ntok = 1, every divisor but nb is 1
]]
BY_NAME = {c.name: c for c in CASES}


# ---- the host logic of csrc/gemm.hip, restated --------------------------------------------------------------------------------
def supported(case):
    """xvit_patch_embed_supported."""
    (D, H, W), (dp, hp, wp), d = case.vol, case.patch, case.d
    if min(case.B, case.M, dp, hp, wp) <= 0 or case.cls not in (0, 1) or D % dp or H % hp or W % wp:
        return False
    if wp % 8 or 64 % wp or (hp * wp) % 64 or case.pd % 256 or d % 256 or d < 256 or case.rows < 2048:
        return False
    return case.B * case.M * D * H * W * 2 < 2 ** 31 and case.rows * d * 4 < 2 ** 31 and case.P <= 2 ** 24


def aligned(case):
    """pe_aligned: 64 consecutive tokens of a sample are whole d-columns of one h-row (mode 2; otherwise mode 3)."""
    Dn, _, Wn = case.grid
    return 64 % Dn == 0 and (Dn * Wn) % 64 == 0


def wgrad_split(case):
    """pe_wgrad_split."""
    tiles = (case.d // 256) * (case.pd // 256)
    ksteps = case.rows // 64
    return max(1, min(256 // max(tiles, 1), ksteps // 8, 16))


def k_per_split(K, split):
    """k_per_split: whole K-steps."""
    ktiles = (K + BK - 1) // BK
    return (ktiles + split - 1) // split * BK


def split_steps(case):
    """K-steps of every split of the weight gradient as gemm_big_kernel counts them (C division: truncated towards zero); a split
    that begins at or behind K has 0 or fewer and still writes its zero slab."""
    split = wgrad_split(case)
    kps = k_per_split(case.K, split)
    out = []
    for s in range(split):
        n = min(case.K, s * kps + kps) - s * kps + BK - 1
        out.append(n // BK if n >= 0 else -(-n // BK))
    return out


def krow_token(case, kr):
    """gather_krow_token: the token of a 64-token group that k-row kr of a mode-2 K-step holds (tokens (w, d) and (w + 1, d) paired)."""
    Dn = case.grid[0]
    nw = 64 // Dn
    if nw & 1:
        return kr
    a, b = kr >> 1, kr & 1
    return a % Dn + Dn * (2 * (a // Dn) + b)


def classify(case):
    """The class a case stands for: which branches of the gather paths it takes."""
    Dn, Hn, Wn = case.grid
    mode = 2 if aligned(case) else 3
    return dict(mode=mode, nw=64 // Dn if mode == 2 else None, wsteps=Dn * Wn // 64 if mode == 2 else None, grid=(Dn, Hn, Wn), P=case.P,
                split=wgrad_split(case), steps=split_steps(case), k_mod_64=case.K % 64, rows_mod_256=case.rows % 256,
                div1=tuple(n for n, v in (("Dn", Dn), ("Wn", Wn), ("pcount", case.P)) if v == 1), nb=case.B, modalities=case.M, wp=case.patch[2],
                tiles=(case.d // 256, case.pd // 256), fwd_ksteps=case.pd // 64, cls=case.cls)


# ---- the CPU reference ---------------------------------------------------------------------------------------------------------
def _compute_reference(case):
    c = case
    vol = exact_operands(c.shape, c.seed, SV)
    W = exact_operands((c.d, c.pd), c.seed + 1, SW)
    dx = exact_operands((c.rows, c.d), c.seed + 2, SX)
    if c.cls:
        dx.view(c.M * c.B, c.ntok, c.d)[:, 0] = NAN                 # CLS rows: skipped by the weight gradient
    unit = 2.0 ** -(SV + SW)
    bias = exact_grid((c.d,), c.seed + 3, unit, 32)
    pos = exact_grid((c.ntok, c.d), c.seed + 4, unit, 256)
    # patch rows in the order of the token matrix: (m B + b) P + t
    patches = torch.stack([R.patchify(vol[:, m, 0], c.patch) for m in range(c.M)]).reshape(c.K, c.pd).contiguous()
    dxp = dx.view(c.M * c.B, c.ntok, c.d)[:, c.cls:].reshape(c.K, c.d)
    return dict(vol=vol, W=W, dx=dx, bias=bias, pos=pos, patches=patches, dxp=dxp, acc=patches @ W.T, dW=dxp.T @ patches)


@lru_cache(maxsize=2)
def reference(case):
    """Operands and expected results of one case (CPU; computed once, shared, not to be modified)."""
    return _compute_reference(case)


def x_ref(case, ref, bias=True, pos=True):
    """The forward's expected [rows, d]: patch rows patch W^T [+ bias] [+ pos[cls + t]], CLS rows [bias] [+ pos[0]] (include/xvit.h)."""
    c = case
    x = torch.zeros(c.M * c.B, c.ntok, c.d)
    x[:, c.cls:] = ref["acc"].view(c.M * c.B, c.P, c.d)
    if bias:
        x += ref["bias"]
    if pos:
        x += ref["pos"]
    return x.reshape(c.rows, c.d)


# ---- destinations --------------------------------------------------------------------------------------------------------------
def _framed(rows, cols, pad_rows, pad_cols, fill):
    """Flat fp32 [MARGIN | (rows + pad_rows) x (cols + pad_cols) | MARGIN] of SENTINEL with `fill` in the rows x cols interior."""
    flat = torch.full((2 * MARGIN + (rows + pad_rows) * (cols + pad_cols),), SENTINEL)
    _body(flat, rows + pad_rows, cols + pad_cols)[:rows, :cols] = fill
    return flat


def _body(flat, rows_alloc, ld):
    return flat[MARGIN:MARGIN + rows_alloc * ld].view(rows_alloc, ld)


def x_body(case, flat):
    return _body(flat, case.rows + PAD_ROWS, case.d + X_PAD)


def dw_body(case, flat):
    return _body(flat, case.d + PAD_ROWS, case.pd + DW_PAD)


def workspace_bytes(case):
    """xvit_patch_embed_wgrad_workspace_bytes by the restatement."""
    split = wgrad_split(case)
    return split * case.d * case.pd * 4 if split > 1 else 0


def buffers(case):
    """CPU images of the destinations as they are before the launch."""
    return dict(x=_framed(case.rows, case.d, PAD_ROWS, X_PAD, NAN), dW=_framed(case.d, case.pd, PAD_ROWS, DW_PAD, NAN),
                ws=_framed(1, workspace_bytes(case) // 4, 0, 0, NAN))


def ideal(case, ref, bias=True, pos=True):
    """The destinations as a faultless kernel leaves them (the workspace's interior holds partial sums nobody checks: zeros here)."""
    out = buffers(case)
    x_body(case, out["x"])[:case.rows, :case.d] = x_ref(case, ref, bias, pos)
    dw_body(case, out["dW"])[:case.d, :case.pd] = ref["dW"]
    out["ws"][MARGIN:len(out["ws"]) - MARGIN] = 0.0
    return out


# ---- the GPU side --------------------------------------------------------------------------------------------------------------
def geom(case):
    from xvit import _lib
    g = _lib.PatchGeom()
    g.B, g.M, (g.D, g.H, g.W), (g.dp, g.hp, g.wp), g.cls_rows = case.B, case.M, case.vol, case.patch, case.cls
    return g


def _padded(t, pad_cols, pad_rows=0):
    """t [rows, cols] inside a NaN-filled [rows + pad_rows, cols + pad_cols]."""
    full = torch.full((t.shape[0] + pad_rows, t.shape[1] + pad_cols), NAN)
    full[:t.shape[0], :t.shape[1]] = t
    return full


def device_operands(case, ref):
    """The operands on the GPU: the volume inside a larger NaN-filled allocation, NaN in every padding column, in the CLS rows of dx
    (they are in ref["dx"] already) and in two rows behind dx."""
    n = ref["vol"].numel()
    vbuf = torch.full((2 * MARGIN + n,), NAN)
    vbuf[MARGIN:MARGIN + n] = ref["vol"].reshape(-1)
    vbuf = vbuf.to(dev(), torch.bfloat16)
    D = dict(vbuf=vbuf, vol=vbuf[MARGIN:MARGIN + n],
             W=_padded(ref["W"], W_PAD).to(dev(), torch.bfloat16), dx=_padded(ref["dx"], DX_PAD, PAD_ROWS).to(dev(), torch.bfloat16),
             pos=_padded(ref["pos"], POS_PAD).to(dev()), bias=ref["bias"].to(dev()))
    for k in ("vol", "W", "dx", "pos", "bias"):
        assert D[k].data_ptr() % 16 == 0, k
    return D


def _interior_ptr(flat):
    p = flat.data_ptr() + MARGIN * flat.element_size()
    assert p % 16 == 0
    return p


def _stream():
    return torch.cuda.current_stream().cuda_stream


def call_fwd(case, D, xbuf, bias=True, pos=True, ldw=None, x_off=0):
    """xvit_patch_embed_fwd on the operands D into the framed buffer xbuf; returns the entry point's return code."""
    from xvit import _lib
    c = case
    return _lib.load().xvit_patch_embed_fwd(D["vol"].data_ptr(), C.byref(geom(c)), D["W"].data_ptr(), c.pd + W_PAD if ldw is None else ldw,
                                            D["bias"].data_ptr() if bias else None, D["pos"].data_ptr() if pos else None, c.d + POS_PAD,
                                            _interior_ptr(xbuf) + x_off, c.d + X_PAD, c.d, _stream())


def call_wgrad(case, D, dwbuf, wsbuf, lddx=None, ws_bytes=None, dx_off=0):
    """xvit_patch_embed_wgrad on the operands D into the framed buffers dwbuf / wsbuf; returns the entry point's return code."""
    from xvit import _lib
    c = case
    L = _lib.load()
    need = L.xvit_patch_embed_wgrad_workspace_bytes(C.byref(geom(c)), c.d)
    assert need == (wsbuf.numel() - 2 * MARGIN) * 4, f"{c.tag}: the library asks for {need} bytes of workspace, the restatement for {workspace_bytes(c)}"
    return L.xvit_patch_embed_wgrad(D["vol"].data_ptr(), C.byref(geom(c)), D["dx"].data_ptr() + dx_off, c.d + DX_PAD if lddx is None else lddx,
                                    _interior_ptr(dwbuf), c.pd + DW_PAD, c.d, _interior_ptr(wsbuf) if need else None,
                                    need if ws_bytes is None else ws_bytes, _stream())


def launch_fwd(case, ref, D=None, bias=True, pos=True):
    from xvit import _lib
    D = D or device_operands(case, ref)
    xbuf = buffers(case)["x"].to(dev())
    _lib.check(call_fwd(case, D, xbuf, bias, pos), "xvit_patch_embed_fwd")
    torch.cuda.synchronize()
    return dict(x=xbuf.cpu())


def launch_wgrad(case, ref, D=None):
    from xvit import _lib
    D = D or device_operands(case, ref)
    B = {k: v.to(dev()) for k, v in buffers(case).items() if k != "x"}
    _lib.check(call_wgrad(case, D, B["dW"], B["ws"]), "xvit_patch_embed_wgrad")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in B.items()}


def launch(case, ref, D=None):
    """Forward (with bias and pos) and weight gradient of one case; the destinations as CPU tensors."""
    D = D or device_operands(case, ref)
    return {**launch_fwd(case, ref, D), **launch_wgrad(case, ref, D)}


# ---- the comparison ------------------------------------------------------------------------------------------------------------
def _untouched(flat, rows_alloc, ld, rows, cols, what):
    """Everything of the framed buffer outside its rows x cols interior still holds SENTINEL, bit for bit."""
    bits = flat.view(torch.int32)
    want = int(torch.tensor(SENTINEL).view(torch.int32))
    body = _body(bits, rows_alloc, ld)
    parts = (("the margin in front", bits[:MARGIN], lambda i: f"element {i[0] - MARGIN} of the output"),
             ("the margin behind", bits[MARGIN + rows_alloc * ld:], lambda i: f"element {i[0]} behind the buffer's end"),
             ("padding columns", body[:, cols:], lambda i: f"destination (row {i[0]}, col {cols + i[1]})"),
             ("padding rows", body[rows:, :cols], lambda i: f"destination (row {rows + i[0]}, col {i[1]})"))
    for name, part, where in parts:
        bad = part != want
        if int(bad.sum()):
            raise AssertionError(f"{what}: {int(bad.sum())} elements outside the output were overwritten ({name}); first at {where(bad.nonzero()[0].tolist())}")


def compare(case, ref, out, bias=True, pos=True):
    """Every destination present in `out` (x: against x_ref with / without bias and pos; dW with the workspace's margins)."""
    c = case
    if "x" in out:
        assert_exact(x_body(c, out["x"])[:c.rows, :c.d], x_ref(c, ref, bias, pos), f"{c.tag}: x")
        _untouched(out["x"], c.rows + PAD_ROWS, c.d + X_PAD, c.rows, c.d, f"{c.tag}: x")
    if "dW" in out:
        assert_exact(dw_body(c, out["dW"])[:c.d, :c.pd], ref["dW"], f"{c.tag}: dW")
        _untouched(out["dW"], c.d + PAD_ROWS, c.pd + DW_PAD, c.d, c.pd, f"{c.tag}: dW")
    if "ws" in out:
        n = out["ws"].numel() - 2 * MARGIN
        _untouched(out["ws"], 1, n, 1, n, f"{c.tag}: workspace")


# ---- the input gradient (xvit_patch_embed_dgrad): the helpers of tests/test_patch_embed_dgrad_gpu.py ---------------------------
DGRAD_SENTINEL = 12288.0     # 3 * 2^12: exact in bf16


def index_map(vol, patch):
    """[P, pd] int64: the flat voxel index (inside one [D, H, W] volume) of every (token, feature) — the oracle's patchify order."""
    D, H, W = vol
    return R.patchify(torch.arange(D * H * W, dtype=torch.int64).reshape(1, D, H, W), patch)[0]


def dgrad_reference(dx, w, B, M, vol, patch, cls=1):
    """fp32 [B, M, 1, D, H, W]: the patch rows of dx @ w (exact) placed on the voxel grid."""
    P = (vol[0] // patch[0]) * (vol[1] // patch[1]) * (vol[2] // patch[2])
    rows = dx.reshape(M, B, cls + P, -1)[:, :, cls:]
    idx = index_map(vol, patch).reshape(-1)
    out = torch.empty(B, M, vol[0] * vol[1] * vol[2])
    for m in range(M):
        out[:, m].index_copy_(1, idx, (rows[m].reshape(B * P, -1) @ w).reshape(B, -1))
    return out.reshape(B, M, 1, *vol)


def sentinel_out(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * MARGIN,), DGRAD_SENTINEL, dtype=dtype, device=dev())
    return buf, buf[MARGIN:MARGIN + n].view(shape)


def dgrad_operands(B, M, vol, patch, d, seed, cls=1):
    P = (vol[0] // patch[0]) * (vol[1] // patch[1]) * (vol[2] // patch[2])
    pd = patch[0] * patch[1] * patch[2]
    dx = exact_operands((M * B * (cls + P), d), seed, 2)
    w = exact_operands((d, pd), seed + 1, 3)
    if cls:
        dx.view(M * B, cls + P, d)[:, 0] = NAN             # CLS rows: never stored
    return dx, w


def check_dgrad(B, M, vol, patch, d, cls=1, seed=None):
    """xvit_patch_embed_dgrad into fp32 and bf16 volumes: every voxel bit for bit, NaN CLS rows kept out, margins untouched, reproducible."""
    from xvit import ops
    shape = (B, M, 1, *vol)
    assert ops.patch_embed_dgrad_supported(shape, patch, d, cls)
    dx, w = dgrad_operands(B, M, vol, patch, d, B + d if seed is None else seed, cls)
    ref = dgrad_reference(dx, w, B, M, vol, patch, cls)
    gdx, gw = dx.bfloat16().to(dev()), w.bfloat16().to(dev())
    for dtype in (torch.float32, torch.bfloat16):
        buf, out = sentinel_out(shape, dtype)
        got = ops.patch_embed_dgrad(gdx, gw, shape, patch, dtype, cls, out=out)
        assert got.data_ptr() == out.data_ptr() and got.dtype == dtype
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), f"{dtype}: a CLS row (NaN) reached the volume"
        assert_exact(out, ref, f"dgrad {dtype}")
        margins = torch.cat([buf[:MARGIN], buf[-MARGIN:]]).float()
        assert (margins == DGRAD_SENTINEL).all(), f"{dtype}: a voxel outside the volume was written"
    again = ops.patch_embed_dgrad(gdx, gw, shape, patch, torch.float32, cls)
    assert torch.equal(again, ops.patch_embed_dgrad(gdx, gw, shape, patch, torch.float32, cls)), "not reproducible"
