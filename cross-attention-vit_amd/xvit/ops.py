"""Thin tensor-level wrappers over the C ABI: pointer/stride extraction, current-stream
plumbing, loud failure.  No autograd here (see functional.py) and no fallback: a tensor that
is not on the GPU is an error."""
from __future__ import annotations

import ctypes as C
import functools
import math
import os

import torch

from . import _lib
from ._lib import GemmArgs

BF16, F32 = 0, 1
NT, NN, TN = 0, 1, 2
ACT_NONE, ACT_GELU, ACT_DGELU = 0, 1, 2


# Host cost matters at the reference's batch (8 volume pairs: ~500 launches per step against 4.4 ms of GPU work): the current device
# and its current stream are read through torch's C entry points (what torch.cuda.current_device / current_stream wrap, without the
# lazy-init checks and the Stream object per call: 9 us -> 0.3 us).
_cur_dev = torch._C._cuda_getDevice
_raw_stream = torch._C._cuda_getCurrentRawStream


def _stream() -> int:
    return _raw_stream(_cur_dev())


class _Entries:
    """The library's entry points as attributes: each is looked up in _lib.load() at its first use and bound here, so a launch
    costs one attribute read."""

    def __getattr__(self, sym):
        fn = getattr(_lib.load(), sym)
        setattr(self, sym, fn)
        return fn


_L = _Entries()

# Optional live per-kernel timing (bench.py): when PROFILE is a list, every wrapper brackets its
# launch with HIP events recorded on the launch stream and appends
# (kernel family, algorithmic work, "flop" | "byte", start_event, end_event).
PROFILE = None
# Deterministic gradients (SURVEY.md 8(b) "Determinism"): XVIT_DETERMINISTIC=1 or set_deterministic(True).  The kernels that
# normally meet in fp32 atomics (LayerNorm dgamma / dbeta and the bias column sums next to it, xvit_colsum, the class-head
# wgrad) then store per-block partial sums and add them in a fixed order, and the GEMM epilogue's fused column sums are
# replaced by a separate xvit_colsum: every .grad is bit-identical from run to run (attention backward and split-K already are).
DETERMINISTIC = os.environ.get("XVIT_DETERMINISTIC", "0") == "1"


def set_deterministic(on: bool = True):
    global DETERMINISTIC
    DETERMINISTIC = bool(on)


GEMM_TILE = 0            # mirror of xvit_set_option("gemm_tile") for the family names below


def set_option(name: str, value: int):
    """xvit_set_option (include/xvit.h): process-wide tuning knobs, e.g. ("gemm_tile", 1) forces the 128x128 kernel."""
    global GEMM_TILE
    _lib.check(_L.xvit_set_option(name.encode(), int(value)), "xvit_set_option")
    if name == "gemm_tile":
        GEMM_TILE = int(value)


_DROP_EPOCH = None       # keeps the registered counter tensor alive


def set_dropout_epoch(counter):
    """xvit_set_dropout_epoch (include/xvit.h): register a one-element int64 device tensor whose value is mixed into every dropout seed at
    kernel run time (captured steps: xvit.graph.GraphedStep increments it at the head of its graph), or None to switch it off."""
    global _DROP_EPOCH
    if counter is not None and not (counter.is_cuda and counter.dtype == torch.int64 and counter.numel() == 1):
        raise RuntimeError("set_dropout_epoch: need a one-element int64 GPU tensor (or None)")
    _lib.check(_L.xvit_set_dropout_epoch(counter.data_ptr() if counter is not None else None), "xvit_set_dropout_epoch")
    _DROP_EPOCH = counter


PROFILE_SHAPES = False   # append the GEMM shape/epilogue to the family name (bench.py --detail)


def _launch(sym, *args):
    """One entry point of the library on the current stream (its last argument), nothing recorded in PROFILE."""
    rc = getattr(_L, sym)(*args, _raw_stream(_cur_dev()))
    if rc:
        _lib.check(rc, sym)


def _call(sym, family, work, kind, *args):
    """_launch, bracketed by two events and recorded under `family` when PROFILE is a list."""
    if PROFILE is None:
        rc = getattr(_L, sym)(*args, _raw_stream(_cur_dev()))
        if rc:
            _lib.check(rc, sym)
        return
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    _launch(sym, *args)
    e.record()
    PROFILE.append((family, float(work), kind, s, e))


# torch.empty of the two dtypes the kernels write: _f32(rows, d, device=x.device)
_f32 = functools.partial(torch.empty, dtype=torch.float32)
_b16 = functools.partial(torch.empty, dtype=torch.bfloat16)


def _ws(nbytes, like):
    """fp32 workspace of `nbytes` (an xvit_*_workspace_bytes answer) on like's device, None for 0."""
    return _f32(nbytes // 4, device=like.device) if nbytes else None


def _drop(dropout):
    """None or (p, seed) -> the kernels' (p, seed) arguments: (0.0, 0) when dropout is off."""
    if dropout is None or not dropout[0] > 0.0:
        return 0.0, 0
    return float(dropout[0]), int(dropout[1])


def _ptr(t) -> int | None:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("xvit: tensor is not on the GPU; the HIP path has no CPU fallback")
    if t.device.index != _cur_dev():
        # launches go to the CURRENT device's current stream (_stream()): a tensor of another GPU would be written by a
        # kernel on the wrong device, unordered with torch's own work on the tensor's device
        raise RuntimeError(f"xvit: tensor lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                           "call torch.cuda.set_device(...) (one process per GPU) or wrap the call in torch.cuda.device(...)")
    return t.data_ptr()


def _dt(t) -> int:
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    raise TypeError(f"xvit: unsupported dtype {t.dtype}")


def _seed64(seed) -> int:
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _rows2d(t):
    """Leading dimension of a 2-D row-major view."""
    assert t.dim() == 2 and t.stride(1) == 1, f"need a row-major 2-D tensor, got shape {tuple(t.shape)} strides {t.stride()}"
    return t.stride(0)


def _ld(t):
    """_rows2d of an optional tensor (0 for None)."""
    return _rows2d(t) if t is not None else 0


def gemm_workspace_bytes(layout, M, N, K, split_k, batch=1):
    """Bytes of fp32 workspace ops.gemm(..., split_k=split_k, workspace=...) needs for this product (0 when split_k <= 1)."""
    a = GemmArgs()
    a.layout, a.M, a.N, a.K, a.split_k, a.batch = layout, M, N, K, split_k, batch
    return _L.xvit_gemm_workspace_bytes(C.byref(a))


def gemm(layout, A, B, C_out, *, bias=None, residual=None, aux=None, act=ACT_NONE, accumulate=False,
         split_k=1, res_row_mod=0, res_row_off=0, out_seg=(0, 0, 0), M=None, N=None, K=None, colsum=None, dropout=None, aux_mode=0, workspace=None):
    """C = op(A) op(B) with the fused epilogue of include/xvit.h.  2-D tensors, or 3-D
    [batch, rows, cols] for a strided batch (all of A, B, C and optional bias 2-D / residual /
    aux 3-D then carry the batch in dim 0).  workspace: an fp32 tensor for the partial tiles of split_k > 1
    (gemm_workspace_bytes), else one is allocated per call."""
    a = GemmArgs()
    batched = A.dim() == 3
    A2, B2, C2 = (A[0], B[0], C_out[0]) if batched else (A, B, C_out)
    if layout == NT:
        m, k = A2.shape; n = B2.shape[0]; assert B2.shape[1] == k
    elif layout == NN:
        m, k = A2.shape; n = B2.shape[1]; assert B2.shape[0] == k
    else:
        k, m = A2.shape; n = B2.shape[1]; assert B2.shape[0] == k
    a.layout, a.M, a.N, a.K = layout, M or m, N or n, K or k
    a.batch = A.shape[0] if batched else 1
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16
    a.c_dtype, a.act, a.accumulate, a.split_k = _dt(C_out), act, int(bool(accumulate)), split_k
    a.res_row_mod, a.res_row_off = res_row_mod, res_row_off
    a.aux_mode = aux_mode             # 1: aux carries gelu'(z) instead of z (include/xvit.h)
    a.out_seg_rows, a.out_seg_skip, a.out_row_off = out_seg
    a.A, a.B, a.C = _ptr(A), _ptr(B), _ptr(C_out)
    a.lda, a.ldb, a.ldc = _rows2d(A2), _rows2d(B2), _rows2d(C2)
    if batched:
        a.stride_a, a.stride_b, a.stride_c = A.stride(0), B.stride(0), C_out.stride(0)
    if bias is not None:
        assert bias.dtype == torch.float32
        a.bias = _ptr(bias)
        if batched:
            a.stride_bias = bias.stride(0)
    if residual is not None:
        assert residual.dtype == torch.float32
        r2 = residual[0] if batched else residual
        a.residual, a.ldr = _ptr(residual), _rows2d(r2)
        if batched:
            a.stride_r = residual.stride(0)
    if aux is not None:
        assert aux.dtype == torch.bfloat16
        x2 = aux[0] if batched else aux
        a.aux, a.ldaux = _ptr(aux), _rows2d(x2)
        if batched:
            a.stride_aux = aux.stride(0)
    if colsum is not None:
        assert colsum.dtype == torch.float32
        a.colsum = _ptr(colsum)
    a.dropout_p, a.dropout_seed = _drop(dropout)
    ws = None
    if split_k > 1:
        need = _L.xvit_gemm_workspace_bytes(C.byref(a))
        if need:
            ws = workspace if workspace is not None else _ws(need, C_out)
            if not (ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() * 4 >= need):
                raise RuntimeError(f"xvit: gemm workspace must be a contiguous fp32 tensor of at least {need} bytes")
            a.workspace, a.workspace_bytes = _ptr(ws), need
    # one family per kernel symbol: gemm_big_kernel<..> (M, N >= 256) vs gemm_kernel<..>; "+splitk" brackets also
    # contain the splitk_epilogue_kernel launch that follows
    big = GEMM_TILE != 1 and a.M >= 256 and a.N >= 256 and ((a.M + 255) // 256) * ((a.N + 255) // 256) * a.batch * max(split_k, 1) > 128   # = use_big_tile() in gemm.hip
    kind = "big" if big else "small"
    tag = f"gemm_{kind}_" + ("nt", "nn", "tn")[layout] + ("+splitk" if split_k > 1 else "")
    if PROFILE is not None and PROFILE_SHAPES:
        epi = ("+b" if bias is not None else "") + ("+gelu" if act == ACT_GELU else "+dgelu" if act == ACT_DGELU else "") + ("+res" if residual is not None else "")
        tag += f"[{a.M}x{a.N}x{a.K}{epi}{'' if a.c_dtype == BF16 else ',f32'}{',s%d' % split_k if split_k > 1 else ''}]"
    _call("xvit_gemm", tag, 2.0 * a.M * a.N * a.K * a.batch, "flop", C.byref(a))
    return C_out


def _alt_ld(x, x_alt, seq_len):
    """Row stride between the x_alt rows of consecutive sequences: x_alt is either a tensor laid out like x (its rows
    k * seq_len are used) or a packed [sequences, d] copy of those rows."""
    if x_alt is None:
        return 0
    rows, d = x.shape
    if x_alt.shape == x.shape and x_alt.stride() == x.stride():
        return seq_len * _rows2d(x)
    assert seq_len > 0 and x_alt.shape == (rows // seq_len, d) and x_alt.stride(1) == 1 and x_alt.dtype == torch.float32
    return x_alt.stride(0)


def layernorm_fwd(x, gamma, beta, eps, *, x_alt=None, seq_len=0, out=None):
    """x fp32 [rows, d] (row stride free) -> (y bf16 [rows, d], mean, rstd)."""
    (rows, d), dev = x.shape, x.device
    y = out if out is not None else _b16(rows, d, device=dev)
    mean, rstd = _f32(rows, device=dev), _f32(rows, device=dev)
    _call("xvit_layernorm_fwd", "layernorm_fwd", rows * d * 6.0, "byte", _ptr(x), _ptr(x_alt), _rows2d(x), seq_len, _alt_ld(x, x_alt, seq_len),
          _ptr(gamma), _ptr(beta), eps, _ptr(y), _rows2d(y), None, 0, _ptr(mean), _ptr(rstd), rows, d)
    return y, mean, rstd


def layernorm_fwd_f32(x, gamma, beta, eps, want_bf16=True):
    """x fp32 [rows, d] (row stride free) -> (y fp32, y bf16 | None, mean, rstd): the single-token CLS path keeps fp32 operands."""
    (rows, d), dev = x.shape, x.device
    yf = _f32(rows, d, device=dev)
    yb = _b16(rows, d, device=dev) if want_bf16 else None
    mean, rstd = _f32(rows, device=dev), _f32(rows, device=dev)
    _launch("xvit_layernorm_fwd", _ptr(x), None, _rows2d(x), 0, 0, _ptr(gamma), _ptr(beta), eps, _ptr(yb), d, _ptr(yf), d, _ptr(mean), _ptr(rstd), rows, d)
    return yf, yb, mean, rstd


def linear_f32(x, W, bias=None, *, act=ACT_NONE, residual=None, want_z=False, want_bf16=False, dropout=None):
    """fp32 Linear of the single-token CLS path (xvit_linear_f32): x fp32 [M, K] (row stride free), W fp32 [N, K] (the master
    weight itself) -> (y fp32 [M, N], y bf16 | None, z bf16 | None); z = the GELU pre-activation (act = ACT_GELU)."""
    M, K = x.shape
    N = W.shape[0]
    assert x.dtype == torch.float32 and W.dtype == torch.float32 and W.shape[1] == K
    if K % 16 or x.data_ptr() % 16 or W.data_ptr() % 16 or x.stride(0) % 4 or W.stride(0) % 4:
        # the kernel walks K in 16-byte steps of aligned rows: a width that is not a multiple of 16 (the reference accepts any
        # hidden_dim / mlp_dim) or an oddly offset view is zero-padded into aligned scratch copies first (exact: the pad adds 0)
        K16 = (K + 15) // 16 * 16
        xp = torch.zeros(M, K16, dtype=torch.float32, device=x.device)
        wp = torch.zeros(N, K16, dtype=torch.float32, device=x.device)
        xp[:, :K].copy_(x)
        wp[:, :K].copy_(W)
        x, W, K = xp, wp, K16
    dev = x.device
    y = _f32(M, N, device=dev)
    yb = _b16(M, N, device=dev) if want_bf16 else None
    zb = _b16(M, N, device=dev) if want_z else None
    need = _L.xvit_linear_f32_workspace_bytes(M, N, K)
    ws = _ws(need, x)
    _call("xvit_linear_f32", "linear_f32", 2.0 * M * N * K, "flop", _ptr(x), _rows2d(x), _ptr(W), _rows2d(W), _ptr(bias), _ptr(y), N, M, N, K, act,
          _ptr(zb), N, _ptr(residual), _ld(residual), _ptr(yb), N, *_drop(dropout), _ptr(ws), need)
    return y, yb, zb


def layernorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, *, x_alt=None, seq_len=0, dres=None, want_bf16=False, dxsum=None, dressum=None):
    """-> (dx fp32, dx_bf16 | None); dgamma/dbeta (fp32, [d]) are accumulated into; so are the optional
    column sums dxsum (of dx) and dressum (of dres)."""
    (rows, d), dev = x.shape, x.device
    dx = _f32(rows, d, device=dev)
    dxb = _b16(rows, d, device=dev) if want_bf16 else None
    nbytes = rows * d * (2.0 + 4.0 + 4.0 + (4.0 if dres is not None else 0.0) + (2.0 if want_bf16 else 0.0))
    ws_bytes = _L.xvit_layernorm_bwd_workspace_bytes(rows, d) if DETERMINISTIC else 0
    ws = _ws(ws_bytes, x)
    _call("xvit_layernorm_bwd", "layernorm_bwd", nbytes, "byte", _ptr(dy), _rows2d(dy), _ptr(x), _ptr(x_alt), _rows2d(x), seq_len, _alt_ld(x, x_alt, seq_len),
          _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dres), _ld(dres), _ptr(dx), d, _ptr(dxb), d,
          _ptr(dgamma), _ptr(dbeta), _ptr(dxsum), _ptr(dressum), rows, d, _ptr(ws), ws_bytes)
    return dx, dxb


def _attn_fwd(sym, family, qkv, B, N, H, scale, *tail):
    """The two forward attention entry points: their outputs and the q | k | v operand arguments; `tail`: what follows scale."""
    d = qkv.shape[1] // 3
    dh = d // H
    o, lse = _b16(B * N, d, device=qkv.device), _f32(B, H, N, device=qkv.device)
    ld = _rows2d(qkv)
    p = _ptr(qkv)
    _call(sym, family, 4.0 * B * H * N * N * dh, "flop", p, p + 2 * d, p + 4 * d, N * ld, ld, _ptr(o), N * d, d, _ptr(lse), B, H, N, dh, scale, *tail)
    return o, lse


def attn_fwd(qkv, B, N, H, scale, dropout=None):
    """qkv bf16 [B*N, 3d] (q | k | v along columns) -> (o bf16 [B*N, d], lse fp32 [B, H, N]).  dropout = (p, seed): dropout
    on the attention probabilities (model.py:169); the mask is that of ops.dropout on a [B, H, N, N] tensor with that seed."""
    p, seed = _drop(dropout)
    need = _L.xvit_attn_fwd_workspace_bytes(B, H, N) if p == 0.0 else 0    # > 0: the CLS-peel form (include/xvit.h)
    ws = _ws(need, qkv)
    return _attn_fwd("xvit_attn_fwd", "attn_fwd", qkv, B, N, H, scale, p, seed, _ptr(ws), need)


def attn_fwd_fp8(qkv, B, N, H, scale):
    """MX-fp8 forward attention (xvit_attn_fwd_fp8): qkv bf16 [B*N, 3d] -> (o bf16 [B*N, d], lse fp32 [B, H, N]); opt-in."""
    need = _L.xvit_attn_fp8_workspace_bytes(B, H, N, qkv.shape[1] // 3 // H)
    ws = torch.empty(need, dtype=torch.uint8, device=qkv.device)
    return _attn_fwd("xvit_attn_fwd_fp8", "attn_fwd_fp8", qkv, B, N, H, scale, _ptr(ws), need)


def _attn_map_step(qkv, lse, r, B, N, H, scale, do=None):
    """attn_rollout_step, or attn_relevance_step when the attention output's gradient `do` is given."""
    d = qkv.shape[1] // 3
    dh = d // H
    assert lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == (B, H, N)
    assert r.dtype == torch.float32 and r.is_contiguous() and tuple(r.shape) == (B, N)
    out = torch.empty_like(r)
    ld = _rows2d(qkv)
    p = _ptr(qkv)
    tail = (_ptr(r), _ptr(out), B, H, N, dh, scale)
    if do is None:
        _call("xvit_attn_rollout_step", "attn_rollout", 2.0 * B * H * N * N * dh, "flop", p, p + 2 * d, N * ld, ld, _ptr(lse), *tail)
    else:
        assert do.dtype == torch.bfloat16 and tuple(do.shape) == (B * N, d)
        ldo = _rows2d(do)
        _call("xvit_attn_relevance_step", "attn_relevance", 4.0 * B * H * N * N * dh, "flop", p, p + 2 * d, p + 4 * d, N * ld, ld, _ptr(lse),
              _ptr(do), N * ldo, ldo, *tail)
    return out


def attn_rollout_step(qkv, lse, r, B, N, H, scale):
    """One attention-rollout step through a self-attention block (xvit_attn_rollout_step): qkv bf16 [B*N, 3d] and lse fp32 [B, H, N] of
    the block's forward, r fp32 [B, N] -> r_out fp32 [B, N] = r / 2 + (r . mean_h P_h) / 2.  P is recomputed from q, k and lse, never stored."""
    return _attn_map_step(qkv, lse, r, B, N, H, scale)


def attn_relevance_step(qkv, lse, do, r, B, N, H, scale):
    """One class-specific relevance step through a self-attention block (xvit_attn_relevance_step): qkv bf16 [B*N, 3d] and lse fp32
    [B, H, N] of the block's forward, do bf16 [B*N, d] the gradient of its attention output, r fp32 [B, N] -> r_out fp32 [B, N] =
    r + r . mean_h relu(P_h * dP_h), dP_h = dO_h V_h^T.  P and dP are recomputed, never stored."""
    return _attn_map_step(qkv, lse, r, B, N, H, scale, do)


def attn_bwd(qkv, o, d_o, lse, B, N, H, scale, dropout=None):
    """-> dqkv bf16 [B*N, 3d]."""
    d = qkv.shape[1] // 3
    dh = d // H
    dqkv = torch.empty_like(qkv)
    need = _L.xvit_attn_bwd_workspace_bytes(B, H, N)
    ws = _ws(need, qkv)                    # rowsum(do*o) | -lse*log2e | CLS-peel partials
    ld = _rows2d(qkv)
    assert dqkv.stride(0) == ld and _rows2d(o) == d and _rows2d(d_o) == d
    p, g = qkv.data_ptr(), dqkv.data_ptr()
    _call("xvit_attn_bwd", "attn_bwd", 10.0 * B * H * N * N * dh, "flop", p, p + 2 * d, p + 4 * d, N * ld, ld, _ptr(o), _ptr(d_o), N * d, d, _ptr(lse),
          _ptr(ws), need, g, g + 2 * d, g + 4 * d, B, H, N, dh, scale, *_drop(dropout))
    return dqkv


def cls_xattn_fwd(q, kv, B, N, H, scale, dropout=None, want_f32=False):
    """q bf16 or fp32 [B, d]; kv bf16 [B*N, 2d] (k | v) -> (o bf16 [B, d], p fp32 [B, H, N]) (+ o fp32 with want_f32)."""
    d, dev = q.shape[1], q.device
    o = _b16(B, d, device=dev)
    of = _f32(B, d, device=dev) if want_f32 else None
    p = _f32(B, H, N, device=dev)
    ld = _rows2d(kv)
    kp = kv.data_ptr()
    qb, qf = (q, None) if q.dtype == torch.bfloat16 else (None, q)
    _call("xvit_cls_xattn_fwd", "cls_xattn_fwd", B * N * 2.0 * d * 2, "byte", _ptr(qb), _ld(qb), _ptr(qf), _ld(qf),
          kp, kp + 2 * d, N * ld, ld, _ptr(o), d, _ptr(of), d, _ptr(p), B, H, N, d // H, scale, *_drop(dropout))
    return (o, p, of) if want_f32 else (o, p)


def cls_xattn_bwd(q, kv, p, d_o, B, N, H, scale, dropout=None, low_rank=False):
    """-> (dq fp32 [B, d], dkv bf16 [B*N, 2d])   or, low_rank: (dq, coef fp32 [B, N, 2H]) with dk[n] = coef[.., h] q_h and
    dv[n] = coef[.., H + h] dO_h (include/xvit.h): the input of xattn_kv_dgrad."""
    d = q.shape[1]
    dq = _f32(B, d, device=q.device)
    ld = _rows2d(kv)
    kp = kv.data_ptr()
    if low_rank:
        out = _f32(B, N, 2 * H, device=q.device)
        gk = gv = None
        work = B * N * 2.0 * d * 2
    else:
        out = torch.empty_like(kv)
        assert out.stride(0) == ld
        gk, gv = out.data_ptr(), out.data_ptr() + 2 * d
        work = B * N * 2.0 * d * 2 * 2
    _call("xvit_cls_xattn_bwd", "cls_xattn_bwd", work, "byte", _ptr(q), _rows2d(q), kp, kp + 2 * d, N * ld, ld, _ptr(p), _ptr(d_o), _rows2d(d_o), _ptr(dq), d,
          gk, gv, _ptr(out) if low_rank else None, B, H, N, d // H, scale, *_drop(dropout))
    return dq, out


def _st0(t):
    """Stride of dim 0 of an optional tensor (0 for None)."""
    return t.stride(0) if t is not None else 0


def head_rows(x, W, out, H, out_bf16=None):
    """out[b, h, :] = x[b, 64h:64h+64] @ W[64h:64h+64, :] (xvit_head_rows; fp32, per head).  x fp32 [B, d]; W fp32 [d, d] (a master
    weight); out fp32 and out_bf16 (optional): any tensors indexable as [b, h, c] with a unit last stride — e.g. a [H, B, d] slab
    transposed to [B, H, d], or a [B, 16, d] GEMM operand buffer, whose head rows H .. 15 the kernel zeroes."""
    B, d = x.shape
    assert x.dtype == torch.float32 and W.dtype == torch.float32 and out.dtype == torch.float32 and out.shape[-1] == d and out.stride(-1) == 1
    ob = out_bf16
    assert ob is None or (ob.dtype == torch.bfloat16 and ob.stride(-1) == 1)
    _call("xvit_head_rows", "head_linear", 2.0 * B * d * 64, "flop", _ptr(x), _rows2d(x), _ptr(W), _rows2d(W), _ptr(out), out.stride(0), out.stride(1),
          _ptr(ob), *((ob.stride(0), ob.stride(1), ob.shape[1]) if ob is not None else (0, 0, 0)), B, H, d)
    return out


def head_cols(t, W, H, row_scale=None, bias=None, want_bf16=False, bias_scale=None):
    """out[b, 64h+e] = row_scale[b, h] * (t[b, h, :] . W[64h+e, :]) + bias_scale[b, h] * bias[64h+e] (xvit_head_cols).  t fp32 [B, >=H, d] -> (fp32 [B, d], bf16 | None)."""
    B, _, d = t.shape
    assert t.dtype == torch.float32 and t.stride(2) == 1 and W.dtype == torch.float32
    assert bias_scale is None or (bias_scale.dtype == torch.float32 and bias_scale.stride(-1) == 1 and bias_scale.shape == (B, H))
    out = _f32(B, d, device=t.device)
    ob = _b16(B, d, device=t.device) if want_bf16 else None
    _call("xvit_head_cols", "head_linear", 2.0 * B * d * 64, "flop", _ptr(t), t.stride(0), t.stride(1), _ptr(W), _rows2d(W), _ptr(row_scale), _st0(row_scale),
          _ptr(bias), _ptr(bias_scale), _st0(bias_scale), _ptr(out), d, _ptr(ob), d, B, H, d)
    return out, ob


def head_wgrad(x, t, H, row_scale=None, out=None):
    """dW[64h+e, :] = sum_b x[b, 64h+e] row_scale[b, h] t[b, h, :] (xvit_head_wgrad) -> fp32 [d, d]."""
    B, d = x.shape
    assert x.dtype == torch.float32 and t.dtype == torch.float32 and t.stride(2) == 1 and t.shape[0] == B and t.shape[2] == d
    dW = out if out is not None else _f32(d, d, device=x.device)
    assert dW.shape == (d, d) and dW.is_contiguous() and dW.dtype == torch.float32
    _call("xvit_head_wgrad", "head_linear", 2.0 * B * d * 64, "flop", _ptr(x), _rows2d(x), _ptr(t), t.stride(0), t.stride(1), _ptr(row_scale), _st0(row_scale),
          _ptr(dW), d, B, H, d)
    return dW


def cls_softmax_fwd(s, H, scale, dropout=None):
    """s fp32 [B, N, 16] (scores of the H heads in the first columns) -> (e bf16 [B, N, 16] = exp(scale (s - max_n s)), zero past H; rz fp32 [B, H] = 1 / sum_n e).
    dropout = (p, seed) on the probabilities (model_cross.py:97): -> (e, stat fp32 [3, B, H] = (rz, rz / (1 - p), rz / (1 - p) * sum_n e_kept), e_kept bf16 [B, N, 16])."""
    B, N, ld = s.shape
    assert s.dtype == torch.float32 and s.is_contiguous() and ld == 16
    e = _b16(B, N, 16, device=s.device)
    p, seed = _drop(dropout)
    drop = p > 0.0
    rz = _f32(*((3, B, H) if drop else (B, H)), device=s.device)
    em = torch.empty_like(e) if drop else None
    _call("xvit_cls_softmax_fwd", "cls_softmax", B * N * 16 * 6.0, "byte", _ptr(s), ld, _ptr(e), 16, _ptr(rz), B, H, N, scale, _ptr(em), p, seed)
    return (e, rz, em) if drop else (e, rz)


def head_bias_grad(x, w, H):
    """out[j] = sum_b x[b, j] w[b, j // 64] (xvit_head_bias_grad): bv's gradient when the weights in front of it are w, not one."""
    B, d = x.shape
    assert x.dtype == torch.float32 and w.dtype == torch.float32 and w.shape == (B, H) and x.stride(1) == 1 and w.stride(1) == 1
    out = _f32(d, device=x.device)
    _call("xvit_head_bias_grad", "head_linear", 2.0 * B * d, "flop", _ptr(x), x.stride(0), _ptr(w), w.stride(0), _ptr(out), B, H, d)
    return out


def cls_softmax_bwd(e, rz, dp, H, scale, dropout=None):
    """-> (coef fp32 [B, N, 2H] = (ds | p'), ds bf16 [B, N, 16]); p = e rz, ds = scale p (dp~ - sum_n p dp~); with dropout = (p, seed) dp~ = m dp / (1 - p) and
    p' = m p / (1 - p) (the forward's mask, regenerated), else dp~ = dp, p' = p.  rz: fp32 [B, H] (row 0 of the forward's stat block under dropout)."""
    B, N, _ = e.shape
    assert rz.shape == (B, H) and rz.is_contiguous()
    assert e.dtype == torch.bfloat16 and e.is_contiguous() and dp.dtype == torch.float32 and dp.is_contiguous() and dp.shape == (B, N, 16)
    coef = _f32(B, N, 2 * H, device=e.device)
    dsb = _b16(B, N, 16, device=e.device)
    _call("xvit_cls_softmax_bwd", "cls_softmax", B * N * (16 * 8.0 + 2 * H * 4.0), "byte", _ptr(e), 16, _ptr(rz), _ptr(dp), 16, _ptr(coef), _ptr(dsb), 16,
          B, H, N, scale, *_drop(dropout))
    return coef, dsb


def xattn_kv_dgrad(coef, R, B, N, H, d):
    """dhn[b, n, :] (bf16) = sum_j coef[b, n, j] R[j, b, :] (xvit_xattn_kv_dgrad); coef fp32 [B, N, 2H], R fp32 [2H, B, d]."""
    assert coef.is_contiguous() and R.is_contiguous() and R.shape == (2 * H, B, d)
    dhn = _b16(B * N, d, device=coef.device)
    _call("xvit_xattn_kv_dgrad", "xattn_kv_dgrad", B * N * d * 2.0 + B * N * 2 * H * 4.0, "byte", _ptr(coef), _ptr(R), _ptr(dhn), d, B, H, N, d)
    return dhn


def _patch_counts(shape, patch):
    """(P, pd) of a [B, M, 1, D, H, W] volume tensor: patches per volume and voxels per patch."""
    (D, H, W), (dp, hp, wp) = shape[3:], patch
    return (D // dp) * (H // hp) * (W // wp), dp * hp * wp


def _patch_place(B, M, P, pad_cls_row, concat):
    """Where patchify puts the patch rows -> ((stride_b, stride_m, row_off, zero_rows, zero_row_stride) in rows, the leading output shape)."""
    if concat:
        rows = M * P + 1
        return (rows, P, 1, B, rows), (B * rows,)
    pad = int(bool(pad_cls_row))
    return (P + pad, B * (P + pad), pad, M * B if pad else 0, P + pad), (M, B * (P + pad))


def patchify(img, patch, pad_cls_row=False, concat=False):
    """img [B, M, 1, D, H, W] fp32|bf16 contiguous -> bf16 patch rows.
      default            [M, B*P, pd]           per modality, no padding
      pad_cls_row        [M, B*(P+1), pd]       per modality, a zero row in front of every sample (ModelCross)
      concat             [B*(M*P+1), pd]        all modalities of a sample in one sequence behind one zero row (ModelVIT)"""
    assert img.dim() == 6 and img.shape[2] == 1 and img.is_contiguous()
    B, M, _, D, H, W = img.shape
    dp, hp, wp = patch
    P, pd = _patch_counts(img.shape, patch)
    place, lead = _patch_place(B, M, P, pad_cls_row, concat)
    out = _b16(*lead, pd, device=img.device)
    _call("xvit_patchify", "patchify", img.numel() * (img.element_size() + 2.0), "byte", _ptr(img), _dt(img), _ptr(out), B, M, D, H, W, dp, hp, wp, *place)
    return out


def _patch_geom(img, patch, cls_rows):
    return _patch_geom_of(tuple(img.shape), patch, cls_rows)


def _patch_geom_of(shape, patch, cls_rows):
    B, M, _, D, H, W = shape
    g = _lib.PatchGeom()
    g.B, g.M, g.D, g.H, g.W = B, M, D, H, W
    g.dp, g.hp, g.wp = patch
    g.cls_rows = int(cls_rows)
    return g


def patch_embed_supported(img, patch, d, cls_rows=1):
    """True when the fused gather kernels (xvit_patch_embed_*) take this input: a contiguous bf16 [B, M, 1, D, H, W] volume
    tensor and a geometry xvit_patch_embed_supported accepts (include/xvit.h).  XVIT_PATCH_EMBED=unfused forces the
    patchify + GEMM path (A/B measurements)."""
    if os.environ.get("XVIT_PATCH_EMBED", "fused") == "unfused":
        return False
    if img.dim() != 6 or img.shape[2] != 1 or img.dtype != torch.bfloat16 or not img.is_contiguous() or not img.is_cuda:
        return False
    return _L.xvit_patch_embed_supported(C.byref(_patch_geom(img, patch, cls_rows)), int(d)) == 1


def patch_embed_fwd(img, patch, w_b, bias, pos, cls_rows=1):
    """x [M*B*(cls_rows + P), d] fp32 = patches(img) W^T + bias + pos[token], the patch matrix never stored
    (model_cross.py:193-197).  w_b: bf16 [d, pd]; pos: fp32 [cls_rows + P, d] or None."""
    g = _patch_geom(img, patch, cls_rows)
    B, M, _, D, H, W = img.shape
    P, pd = _patch_counts(img.shape, patch)
    d = w_b.shape[0]
    assert w_b.dtype == torch.bfloat16 and w_b.shape[1] == pd and (pos is None or pos.shape == (cls_rows + P, d))
    x = _f32(M * B * (cls_rows + P), d, device=img.device)
    _call("xvit_patch_embed_fwd", "gemm_big_nt", 2.0 * M * B * P * d * pd, "flop", _ptr(img), C.byref(g), _ptr(w_b), w_b.stride(0), _ptr(bias),
          _ptr(pos), _st0(pos), _ptr(x), x.stride(0), d)
    return x


def patch_embed_wgrad(img, patch, dx_b, cls_rows=1, out=None):
    """dW [d, pd] fp32 = sum over patch rows of dx[row]^T patch(row); dx_b: bf16 [M*B*(cls_rows + P), d]."""
    g = _patch_geom(img, patch, cls_rows)
    B, M, _, D, H, W = img.shape
    P, pd = _patch_counts(img.shape, patch)
    d = dx_b.shape[1]
    assert dx_b.dtype == torch.bfloat16 and dx_b.shape[0] == M * B * (cls_rows + P) and dx_b.is_contiguous()
    need = _L.xvit_patch_embed_wgrad_workspace_bytes(C.byref(g), d)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=img.device)
    dW = out if out is not None else _f32(d, pd, device=img.device)
    assert dW.shape == (d, pd) and dW.is_contiguous() and dW.dtype == torch.float32
    _call("xvit_patch_embed_wgrad", "gemm_big_tn+splitk", 2.0 * M * B * P * d * pd, "flop", _ptr(img), C.byref(g), _ptr(dx_b), dx_b.stride(0),
          _ptr(dW), dW.stride(0), d, _ptr(ws), need)
    return dW


def patch_embed_dgrad_supported(shape, patch, d, cls_rows=1):
    """True when the fused input gradient (xvit_patch_embed_dgrad) takes a volume of `shape` [B, M, 1, D, H, W]: any dtype, since the
    volume is only written.  XVIT_PATCH_EMBED=unfused forces the NN GEMM + xvit_unpatchify path, as it does for the forward."""
    if os.environ.get("XVIT_PATCH_EMBED", "fused") == "unfused":
        return False
    if len(shape) != 6 or shape[2] != 1:
        return False
    return _L.xvit_patch_embed_dgrad_supported(C.byref(_patch_geom_of(tuple(shape), patch, cls_rows)), int(d)) == 1


def patch_embed_dgrad(dx_b, w_b, shape, patch, dtype=torch.float32, cls_rows=1, out=None):
    """dimg [B, M, 1, D, H, W] (fp32 | bf16) = dx W scattered onto the voxel grid, the patch-gradient matrix never stored
    (xvit_patch_embed_dgrad).  dx_b: bf16 [M*B*(cls_rows + P), d] with its CLS rows (never stored); w_b: bf16 [d, pd]."""
    shape = tuple(shape)
    g = _patch_geom_of(shape, patch, cls_rows)
    B, M, _, D, H, W = shape
    P, pd = _patch_counts(shape, patch)
    d = w_b.shape[0]
    assert dx_b.dtype == torch.bfloat16 and dx_b.shape == (M * B * (cls_rows + P), d) and dx_b.stride(1) == 1
    assert w_b.dtype == torch.bfloat16 and w_b.shape == (d, pd) and w_b.stride(1) == 1
    out = out if out is not None else torch.empty(shape, dtype=dtype, device=dx_b.device)
    assert tuple(out.shape) == shape and out.is_contiguous()
    _call("xvit_patch_embed_dgrad", "patch_embed_dgrad", 2.0 * M * B * P * d * pd, "flop", _ptr(dx_b), dx_b.stride(0), _ptr(w_b), w_b.stride(0), C.byref(g), d,
          _ptr(out), _dt(out))
    return out


def unpatchify(patches, out, patch, pad_cls_row=False, concat=False):
    """The inverse of patchify (xvit_unpatchify): fp32 patch rows laid out as patchify(..., pad_cls_row, concat) lays them out ->
    out [B, M, 1, D, H, W] (fp32 | bf16, contiguous; every voxel written).  CLS rows are never read."""
    assert out.dim() == 6 and out.shape[2] == 1 and out.is_contiguous()
    B, M, _, D, H, W = out.shape
    dp, hp, wp = patch
    P, pd = _patch_counts(out.shape, patch)
    place, lead = _patch_place(B, M, P, pad_cls_row, concat)
    assert patches.dtype == torch.float32 and patches.is_contiguous() and patches.numel() == math.prod(lead) * pd
    _call("xvit_unpatchify", "unpatchify", out.numel() * (4.0 + out.element_size()), "byte", _ptr(patches), _ptr(out), _dt(out), B, M, D, H, W, dp, hp, wp, *place[:3])
    return out


def cls_row_fwd(cls, pos, x, MB, N, d):
    _launch("xvit_cls_row_fwd", _ptr(cls), _ptr(pos), _ptr(x), MB, N, d)


def embed_bwd(dx, dpos, dcls, MB, N, d):
    _call("xvit_embed_bwd", "embed_bwd", float(MB) * N * d * 4, "byte", _ptr(dx), _ptr(dpos), _ptr(dcls), MB, N, d)


def _i32c(t, shape, what):
    assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape), f"{what}: need a contiguous int32 tensor of shape {tuple(shape)}"
    return t


def token_select_draw(keep_idx, slot, B, shared, seed):
    """Patch dropout's draw (xvit_token_select_draw): fills keep_idx int32 [S, K] (kept patch indices of every sequence, ascending) and
    slot int32 [S, P] (position of a kept patch in keep_idx, -1 = dropped); S = M * B, `shared`: one draw per sample for all modalities.
    Runs on the current stream without a host read-back; the dropout epoch (set_dropout_epoch) is mixed into `seed` at run time."""
    S, K = keep_idx.shape
    P = slot.shape[1]
    _i32c(keep_idx, (S, K), "keep_idx"), _i32c(slot, (S, P), "slot")
    _call("xvit_token_select_draw", "token_select_draw", float(S) * (P + K) * 4, "byte", _ptr(keep_idx), _ptr(slot), S, int(B), P, K, int(bool(shared)), int(seed))
    return keep_idx, slot


def patch_occupancy(img, patch, above, out=None):
    """img [B, M, 1, D, H, W] fp32|bf16 contiguous -> int32 [M*B, P]: the voxels of every patch whose value is > above
    (xvit_patch_occupancy; NaN never counts, sequence s = m B + b, patch order of patchify)."""
    assert img.dim() == 6 and img.shape[2] == 1 and img.is_contiguous()
    B, M, _, D, H, W = img.shape
    dp, hp, wp = patch
    P = _patch_counts(img.shape, patch)[0]
    out = out if out is not None else torch.empty(M * B, P, dtype=torch.int32, device=img.device)
    _i32c(out, (M * B, P), "out")
    _call("xvit_patch_occupancy", "patch_occupancy", img.numel() * float(img.element_size()) + M * B * P * 4.0, "byte",
          _ptr(img), _dt(img), _ptr(out), B, M, D, H, W, dp, hp, wp, float(above))
    return out


def token_select_ranked(occ, keep_idx, slot, B, shared, mode, min_count, seed, n_fg=None):
    """The draw ranked by occupancy (xvit_token_select_ranked): occ int32 [S, P] (patch_occupancy) -> keep_idx int32 [S, K] and slot
    int32 [S, P] as token_select_draw fills them.  mode _lib.TOKEN_RANK_RANDOM: patches with at least min_count voxels (summed over the
    modalities of a sample with `shared`) first, the draw's own order inside each class; _lib.TOKEN_RANK_TOP: the K most occupied,
    without seed or epoch.  n_fg int32 [S] (optional) receives the number of foreground patches of every sequence."""
    S, K = keep_idx.shape
    P = slot.shape[1]
    _i32c(occ, (S, P), "occ"), _i32c(keep_idx, (S, K), "keep_idx"), _i32c(slot, (S, P), "slot")
    if n_fg is not None:
        _i32c(n_fg, (S,), "n_fg")
    _call("xvit_token_select_ranked", "token_select_ranked", float(S) * (2 * P + K) * 4, "byte", _ptr(occ), _ptr(keep_idx), _ptr(slot), _ptr(n_fg),
          S, int(B), P, K, int(bool(shared)), int(mode), int(min_count), int(seed))
    return keep_idx, slot


def patchify_select(img, patch, keep_idx, out=None):
    """img [B, M, 1, D, H, W] fp32|bf16 contiguous, keep_idx int32 [M*B, K] -> bf16 [M, B*(K+1), pd]: the rows of
    patchify(img, patch, pad_cls_row=True) that keep_idx names (a zero row in front of every sequence), only the kept voxels read."""
    assert img.dim() == 6 and img.shape[2] == 1 and img.is_contiguous()
    B, M, _, D, H, W = img.shape
    dp, hp, wp = patch
    pd = _patch_counts(img.shape, patch)[1]
    K = keep_idx.shape[1]
    _i32c(keep_idx, (M * B, K), "keep_idx")
    out = out if out is not None else _b16(M, B * (K + 1), pd, device=img.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (M, B * (K + 1), pd)
    _call("xvit_patchify_select", "patchify_select", M * B * K * pd * (img.element_size() + 2.0), "byte",
          _ptr(img), _dt(img), _ptr(out), _ptr(keep_idx), B, M, D, H, W, dp, hp, wp, K)
    return out


def embed_select_fwd(x, cls, pos, keep_idx):
    """In place on x fp32 [S*(K+1), d] (patches W^T + b): + pos[1 + kept patch] on the patch rows, cls + pos[0] on the CLS rows; pos [P+1, d]."""
    S, K = keep_idx.shape
    d = x.shape[1]
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[0] == S * (K + 1)
    assert cls.dtype == torch.float32 and cls.numel() == d and cls.is_contiguous() and pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape[1] == d
    _i32c(keep_idx, (S, K), "keep_idx")
    _call("xvit_embed_select_fwd", "embed_select_fwd", float(x.numel()) * 12, "byte", _ptr(x), _ptr(cls), _ptr(pos), _ptr(keep_idx), S, K, d)
    return x


def embed_select_bwd(dx, slot, dpos, dcls, K):
    """dpos [P+1, d] and dcls [d] += the token gradient dx fp32 [S*(K+1), d] summed over the sequences in order, each pos row from the
    sequences that kept its patch (slot int32 [S, P]); fixed order, no atomics."""
    S, P = slot.shape
    d = dx.shape[1]
    assert dx.dtype == torch.float32 and dx.is_contiguous() and dx.shape[0] == S * (K + 1)
    assert dpos.dtype == torch.float32 and dpos.is_contiguous() and tuple(dpos.shape) == (P + 1, d) and dcls.dtype == torch.float32 and dcls.numel() == d
    _i32c(slot, (S, P), "slot")
    _call("xvit_embed_select_bwd", "embed_select_bwd", float(dx.numel()) * 4, "byte", _ptr(dx), _ptr(slot), _ptr(dpos), _ptr(dcls), S, P, int(K), d)


def token_select_complement(slot, K, drop_idx=None, mslot=None):
    """The dropped side of a draw (xvit_token_select_complement): slot int32 [S, P] with K kept entries per row -> drop_idx int32 [S, P - K]
    (dropped patch indices, ascending) and mslot int32 [S, P] (position of a dropped patch in drop_idx, -1 = kept)."""
    S, P = slot.shape
    K = int(K)
    _i32c(slot, (S, P), "slot")
    drop_idx = drop_idx if drop_idx is not None else torch.empty(S, max(P - K, 0), dtype=torch.int32, device=slot.device)
    mslot = mslot if mslot is not None else torch.empty(S, P, dtype=torch.int32, device=slot.device)
    _i32c(drop_idx, (S, P - K), "drop_idx"), _i32c(mslot, (S, P), "mslot")
    _call("xvit_token_select_complement", "token_select_complement", float(S) * (3 * P - K) * 4, "byte", _ptr(slot), _ptr(drop_idx), _ptr(mslot), S, P, K)
    return drop_idx, mslot


def _f32v(t, shape, what):
    assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape), f"{what}: need a contiguous fp32 tensor of shape {tuple(shape)}"
    return t


def mae_unshuffle_fwd(xe, mask_token, dpos, dmod, slot, out=None):
    """xe fp32 [S, K+1, dd], mask_token [dd], dpos [P+1, dd], dmod [M, dd], slot int32 [S, P] -> y fp32 [S, P+1, dd]: the encoder tokens back
    on the full grid, the mask token in the dropped places, + decoder position and modality embeddings (xvit_mae_unshuffle_fwd)."""
    S, K1, dd = xe.shape
    P, M = slot.shape[1], dmod.shape[0]
    assert S % M == 0, f"mae_unshuffle_fwd: {S} sequences do not divide into {M} modalities"
    _f32v(xe, (S, K1, dd), "xe"), _f32v(mask_token, (dd,), "mask_token"), _f32v(dpos, (P + 1, dd), "dpos"), _f32v(dmod, (M, dd), "dmod"), _i32c(slot, (S, P), "slot")
    y = out if out is not None else _f32(S, P + 1, dd, device=xe.device)
    _f32v(y, (S, P + 1, dd), "y")
    _call("xvit_mae_unshuffle_fwd", "mae_unshuffle_fwd", float(S) * (P + K1) * dd * 4, "byte",
          _ptr(xe), _ptr(mask_token), _ptr(dpos), _ptr(dmod), _ptr(slot), _ptr(y), S, S // M, P, K1 - 1, dd)
    return y


def mae_unshuffle_bwd(dy, keep_idx, slot, M, out=None):
    """dy fp32 [S, P+1, dd] -> (dxe [S, K+1, dd], dmask_token [dd], ddpos_m [M, P+1, dd]) in the fixed orders of xvit_mae_unshuffle_bwd.
    out: (dxe, dmask_token, ddpos_m, scratch [S, dd]) to write into."""
    S, P1, dd = dy.shape
    K = keep_idx.shape[1]
    _f32v(dy, (S, P1, dd), "dy"), _i32c(keep_idx, (S, K), "keep_idx"), _i32c(slot, (S, P1 - 1), "slot")
    assert S % M == 0
    if out is None:
        out = tuple(_f32(*shape, device=dy.device) for shape in ((S, K + 1, dd), (dd,), (M, P1, dd), (S, dd)))
    dxe, dmask, ddpos_m, part = out
    _f32v(dxe, (S, K + 1, dd), "dxe"), _f32v(dmask, (dd,), "dmask_token"), _f32v(ddpos_m, (M, P1, dd), "ddpos_m"), _f32v(part, (S, dd), "scratch")
    _call("xvit_mae_unshuffle_bwd", "mae_unshuffle_bwd", float(S) * (2 * P1 + K + 1) * dd * 4, "byte",
          _ptr(dy), _ptr(keep_idx), _ptr(slot), _ptr(dxe), _ptr(dmask), _ptr(ddpos_m), _ptr(part), S, S // M, P1 - 1, K, dd)
    return dxe, dmask, ddpos_m


def token_rows_gather(x, drop_idx, out=None):
    """x fp32 [S, P+1, dd], drop_idx int32 [S, Rm] -> g fp32 [S*Rm, dd], g[s Rm + j] = x[s, 1 + drop_idx[s][j]] (xvit_token_rows_gather)."""
    S, P1, dd = x.shape
    Rm = drop_idx.shape[1]
    _f32v(x, (S, P1, dd), "x"), _i32c(drop_idx, (S, Rm), "drop_idx")
    g = out if out is not None else _f32(S * Rm, dd, device=x.device)
    _f32v(g, (S * Rm, dd), "g")
    _call("xvit_token_rows_gather", "token_rows_gather", float(S) * Rm * dd * 8, "byte", _ptr(x), _ptr(drop_idx), _ptr(g), S, P1 - 1, Rm, dd)
    return g


def token_rows_scatter(dg, mslot, Rm, out=None):
    """The backward of token_rows_gather: dg fp32 [S*Rm, dd], mslot int32 [S, P] -> dx fp32 [S, P+1, dd], every row written once (zeros for the CLS
    row and the kept patches)."""
    S, P = mslot.shape
    dd = dg.shape[1]
    _f32v(dg, (S * Rm, dd), "dg"), _i32c(mslot, (S, P), "mslot")
    dx = out if out is not None else _f32(S, P + 1, dd, device=dg.device)
    _f32v(dx, (S, P + 1, dd), "dx")
    _call("xvit_token_rows_scatter", "token_rows_scatter", float(S) * (P + 1 + Rm) * dd * 4, "byte", _ptr(dg), _ptr(mslot), _ptr(dx), S, P, int(Rm), dd)
    return dx


def _mae_loss_geom(pred, drop_idx, img, patch):
    assert img.dim() == 6 and img.shape[2] == 1 and img.is_contiguous(), "mae loss: need a contiguous volume tensor [B, M, 1, D, H, W]"
    B, M, _, D, H, W = img.shape
    dp, hp, wp = patch
    Rm, pd = drop_idx.shape[1], _patch_counts(img.shape, patch)[1]
    _i32c(drop_idx, (M * B, Rm), "drop_idx")
    assert pred.dim() == 2 and pred.is_contiguous() and tuple(pred.shape) == (M * B * Rm, pd), \
        f"mae loss: pred must be a contiguous [{M * B * Rm}, {pd}] tensor, got {tuple(pred.shape)}"
    return (B, M, D, H, W, dp, hp, wp, Rm)


def mae_loss_fwd(pred, drop_idx, img, patch, norm_pix=True, out=None):
    """pred [S*Rm, pd] bf16|fp32 against the dropped patches of img [B, M, 1, D, H, W] bf16|fp32 (xvit_mae_loss_fwd; the target matrix is never
    stored) -> (loss fp32 [1], loss_seq fp32 [S], row_loss fp32 [S*Rm], stats fp32 [S*Rm, 2] = (mean, rstd)); out: that tuple to write into."""
    geom = _mae_loss_geom(pred, drop_idx, img, patch)
    B, M, Rm = geom[0], geom[1], geom[8]
    rows = M * B * Rm
    if out is None:
        out = tuple(_f32(*shape, device=pred.device) for shape in ((1,), (M * B,), (rows,), (rows, 2)))
    loss, loss_seq, row_loss, stats = out
    _f32v(loss, (1,), "loss"), _f32v(loss_seq, (M * B,), "loss_seq"), _f32v(row_loss, (rows,), "row_loss"), _f32v(stats, (rows, 2), "stats")
    _call("xvit_mae_loss_fwd", "mae_loss_fwd", float(pred.numel()) * (img.element_size() + pred.element_size()), "byte",
          _ptr(pred), _dt(pred), _ptr(drop_idx), _ptr(img), _dt(img), int(bool(norm_pix)), _ptr(stats), _ptr(row_loss), _ptr(loss_seq), _ptr(loss), *geom)
    return loss, loss_seq, row_loss, stats


def mae_loss_bwd(pred, drop_idx, img, patch, stats, g, out=None):
    """dpred = g 2 (pred - target) / (pd S Rm) in pred's dtype (xvit_mae_loss_bwd); g: one fp32 element on the device (no host read-back)."""
    geom = _mae_loss_geom(pred, drop_idx, img, patch)
    _f32v(stats, (pred.shape[0], 2), "stats")
    assert g.dtype == torch.float32 and g.numel() == 1
    dpred = out if out is not None else torch.empty_like(pred)
    assert dpred.dtype == pred.dtype and dpred.shape == pred.shape and dpred.is_contiguous()
    _call("xvit_mae_loss_bwd", "mae_loss_bwd", float(pred.numel()) * (img.element_size() + 2 * pred.element_size()), "byte",
          _ptr(pred), _dt(pred), _ptr(drop_idx), _ptr(img), _dt(img), _ptr(stats), _ptr(g), _ptr(dpred), *geom)
    return dpred


def cast_bf16(src, out=None):
    """fp32 -> bf16 (contiguous)."""
    assert src.dtype == torch.float32 and src.is_contiguous()
    out = out if out is not None else _b16(src.shape, device=src.device)
    assert out.is_contiguous() and out.numel() == src.numel()
    _call("xvit_cast_f32_bf16", "cast_f32_bf16", src.numel() * 6.0, "byte", _ptr(src), _ptr(out), src.numel())
    return out


def grad_pack_bf16(segments, dst, scale=1.0):
    """dst[off : off + n] = bf16(src * scale) for each (src, off) in `segments`, zeros over the rest of each 64-element slot
    (xvit_grad_pack_bf16): the bf16 wire buffer of a reducer bucket.  src: contiguous fp32, 16-byte aligned; off: a multiple of 64;
    dst: contiguous bf16.  One launch per XVIT_GRAD_PACK_MAX_SEGMENTS segments."""
    assert dst.dtype == torch.bfloat16 and dst.is_contiguous()
    base, m = _ptr(dst), _lib.GRAD_PACK_MAX_SEGMENTS
    for i in range(0, len(segments), m):
        part = segments[i:i + m]
        table = (_lib.GradSegment * len(part))()
        for e, (src, off) in zip(table, part):
            assert src.dtype == torch.float32 and src.is_contiguous()
            e.src, e.dst_offset, e.n = _ptr(src), off, src.numel()
        work = sum(src.numel() for src, _ in part) * 6.0
        _call("xvit_grad_pack_bf16", "grad_pack_bf16", work, "byte", table, len(part), base, dst.numel(), float(scale))
    return dst


def grad_unpack_bf16(src, dst, scale=1.0):
    """dst = float(src) * scale (xvit_grad_unpack_bf16): a reduced bf16 wire buffer back into its fp32 bucket; contiguous, same numel."""
    assert src.dtype == torch.bfloat16 and dst.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
    _call("xvit_grad_unpack_bf16", "grad_unpack_bf16", src.numel() * 6.0, "byte", _ptr(src), _ptr(dst), src.numel(), float(scale))
    return dst


def add_cast(a, b):
    """-> (a + b fp32, its bf16 copy) in one pass (xvit_add_cast_f32_bf16); contiguous fp32 tensors of one shape, numel % 8 == 0."""
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape and a.is_contiguous() and b.is_contiguous()
    out = torch.empty_like(a)
    outb = _b16(a.shape, device=a.device)
    _call("xvit_add_cast_f32_bf16", "add_cast", a.numel() * 14.0, "byte", _ptr(a), _ptr(b), _ptr(out), _ptr(outb), a.numel())
    return out, outb


def rows_combine(dst, a=None, b=None, dst2=None):
    """dst[r, :] (and dst2[r, :]) = a[r, :] + b[r, :] (xvit_rows_combine): 2-D views [rows, d] with a unit last stride and any row stride
    (e.g. t[:, 0] of a [B, N, d] tensor), fp32 or bf16 each; a missing operand is zero; dst may be a or b."""
    rows, d = dst.shape

    def arg(t):
        if t is None:
            return None, 0, 0
        assert t.shape == (rows, d) and t.stride(1) == 1, f"rows_combine: need [rows, d] views with a unit last stride, got {tuple(t.shape)} {t.stride()}"
        return _ptr(t), _dt(t), t.stride(0)
    _call("xvit_rows_combine", "rows_combine", rows * d * 8.0, "byte", *arg(dst), *arg(dst2), *arg(a), *arg(b), rows, d)
    return dst


def colsum(x, out=None, accumulate=False):
    rows, n = x.shape
    if out is None:
        out = _f32(n, device=x.device)
        accumulate = False
    ws_bytes = _L.xvit_colsum_workspace_bytes(rows, n) if DETERMINISTIC else 0
    ws = _ws(ws_bytes, x)
    _call("xvit_colsum", "colsum", float(rows) * n * x.element_size(), "byte", _ptr(x), _dt(x), _rows2d(x), _ptr(out), rows, n, int(accumulate), _ptr(ws), ws_bytes)
    return out


def dropout(x, p, seed, out=None):
    assert x.is_contiguous()
    out = out if out is not None else torch.empty_like(x)
    _launch("xvit_dropout", _ptr(x), _ptr(out), _dt(x), x.numel(), p, seed)
    return out


def small_linear_fwd(x, W, b):
    M, K = x.shape
    N = W.shape[0]
    y = _f32(M, N, device=x.device)
    _launch("xvit_small_linear_fwd", _ptr(x), _rows2d(x), _ptr(W), _ptr(b), _ptr(y), M, N, K)
    return y


def small_linear_bwd(dy, x, W, dW, db, z=None):
    """dx = (dy W) * gelu'(z) if z is given (x = gelu(z))."""
    M, K = x.shape
    N = W.shape[0]
    dx = _b16(M, K, device=x.device)
    _launch("xvit_small_linear_bwd", _ptr(dy), _ptr(x), _rows2d(x), _ptr(W), _ptr(z), _ld(z), _ptr(dx), K, _ptr(dW), _ptr(db), M, N, K, int(DETERMINISTIC))
    return dx


def _mean_ce_out(logits_m):
    """(mean logits [B, C], loss scalar, d loss / d logits_m) of the two cross-entropy kernels."""
    dev = logits_m.device
    return _f32(logits_m.shape[1:], device=dev), _f32((), device=dev), torch.empty_like(logits_m)


def mean_ce(logits_m, labels, smoothing):
    M, B, Cn = logits_m.shape
    logits, loss, dl = _mean_ce_out(logits_m)
    _launch("xvit_mean_ce", _ptr(logits_m), _ptr(labels), smoothing, _ptr(logits), _ptr(loss), _ptr(dl), M, B, Cn)
    return logits, loss, dl


def _mix_table(table, B, what):
    if not (table.dtype == torch.float32 and table.is_contiguous() and tuple(table.shape) == (B, _lib.MIX_NPARAM)):
        raise RuntimeError(f"{what}: the record table is a contiguous fp32 tensor of shape ({B}, {_lib.MIX_NPARAM}), got {table.dtype} {tuple(table.shape)}")
    return table


def mix_draw(config, table, vol_size, seed):
    """xvit_mix_draw (include/xvit.h): fill table fp32 [B, 16] with one Mixup / CutMix record per sample drawn from `config`
    (_lib.MixConfig) and `seed`; vol_size = (D, H, W) of the volumes the CutMix boxes are cut from.  Runs on the current stream without a
    host read-back; the dropout epoch (set_dropout_epoch) is mixed into `seed` at run time."""
    B = table.shape[0]
    _mix_table(table, B, "mix_draw")
    D, H, W = vol_size
    _call("xvit_mix_draw", "mix_draw", table.numel() * 4.0, "byte", C.byref(config), _ptr(table), B, int(D), int(H), int(W), _seed64(seed))
    return table


def mix_apply(img, table, out=None):
    """xvit_mix_apply (include/xvit.h): img [B, M, 1, D, H, W] (bf16 or fp32; every volume contiguous, batch and modality strides free)
    mixed through table fp32 [B, 16] -> a new contiguous tensor of img's shape and dtype.  Out of place: `out` may not overlap img."""
    assert img.dim() == 6 and img.shape[2] == 1, f"mix_apply: need [B, M, 1, D, H, W], got {tuple(img.shape)}"
    B, M, _, D, H, W = img.shape
    if tuple(img.stride()[3:]) != (H * W, W, 1):
        raise RuntimeError(f"mix_apply: every volume must be contiguous, got strides {img.stride()}")
    _mix_table(table, B, "mix_apply")
    out = out if out is not None else torch.empty(img.shape, dtype=img.dtype, device=img.device)
    if not (out.dtype == img.dtype and out.is_contiguous() and out.shape == img.shape):
        raise RuntimeError("mix_apply: out must be contiguous, of img's shape and dtype")
    # one read and one write per voxel; a mixup record reads its partner's volume on top, but which records are mixup ones only the device knows
    _call("xvit_mix_apply", "mix_apply", img.numel() * float(img.element_size()) * 2.0, "byte",
          _ptr(img), _ptr(out), _dt(img), _ptr(table), B, M, D, H, W, img.stride(0), img.stride(1))
    return out


def mean_ce_mix(logits_m, labels, table, smoothing):
    """xvit_mean_ce_mix: mean_ce with the soft target lam smooth(y_b) + oml smooth(y_partner[b]) read from table fp32 [B, 16]."""
    M, B, Cn = logits_m.shape
    if table is None:
        raise RuntimeError("mean_ce_mix: a record table is required (mean_ce is the loss without mixing)")
    _mix_table(table, B, "mean_ce_mix")
    logits, loss, dl = _mean_ce_out(logits_m)
    _call("xvit_mean_ce_mix", "mean_ce_mix", (2.0 * logits_m.numel() + logits.numel() + table.numel()) * 4.0 + B * 8.0, "byte",
          _ptr(logits_m), _ptr(labels), _ptr(table), smoothing, _ptr(logits), _ptr(loss), _ptr(dl), M, B, Cn)
    return logits, loss, dl


def resize_pad_crop_i16(vol, img_size, pad_value=-1.0):
    """int16 [B, M, Ds, Hs, Ws] (NIfTI voxels, on the GPU) -> bf16 [B, M, 1, D, H, W]: the reference's
    ResizeWithPadOrCropd(img_size, constant_values=-1) + float cast (dataset_ucsf.py:84-88,152-158) in one pass."""
    assert vol.dtype == torch.int16 and vol.dim() == 5 and vol.is_contiguous()
    B, M, Ds, Hs, Ws = vol.shape
    D, H, W = img_size
    out = _b16(B, M, 1, D, H, W, device=vol.device)
    _call("xvit_resize_pad_crop_i16", "resize_pad_crop_i16", vol.numel() * 2.0 + out.numel() * 2.0, "byte",
          _ptr(vol), _ptr(out), B * M, Ds, Hs, Ws, D, H, W, float(pad_value))
    return out


I16 = 2   # XVIT_I16: source volumes of augment_apply and volume_stats only


def _src_dt(t) -> int:
    return I16 if t.dtype == torch.int16 else _dt(t)


def _counter_arg(counter, what):
    """The optional call counter of a draw (augment_draw) is checked here, once for the three of them."""
    if counter is not None and not (counter.is_cuda and counter.dtype == torch.int64 and counter.numel() == 1):
        raise RuntimeError(f"{what}: the counter is a one-element int64 GPU tensor (or None)")


def augment_draw(config, params, vol_shape, img_size, seed, counter=None, advance=False):
    """xvit_augment_draw (include/xvit.h): fill params [B, M, 32] (fp32) with one augmentation record per volume drawn from `config`
    (_lib.AugmentConfig) and `seed`; vol_shape / img_size are the source and destination (D, H, W).  counter: optional one-element int64
    device tensor mixed into the seed at kernel run time, advanced by one after it is read when advance is set."""
    assert params.dtype == torch.float32 and params.dim() == 3 and params.shape[2] == _lib.AUG_NPARAM and params.is_contiguous()
    _counter_arg(counter, "augment_draw")
    B, M = params.shape[:2]
    (Ds, Hs, Ws), (D, H, W) = vol_shape, img_size
    _call("xvit_augment_draw", "augment_draw", params.numel() * 4.0, "byte",
          C.byref(config), _ptr(params), B, M, Ds, Hs, Ws, D, H, W, _seed64(seed), _ptr(counter), int(bool(advance)))
    return params


def _augment_apply(name, src, params, img_size, pad_value, out_dtype, elastic=None):
    """augment_apply and augment_apply_elastic: the latter passes elastic = (field, erec), checked before anything is allocated."""
    assert src.dim() == 5 and src.is_contiguous() and params.dtype == torch.float32 and params.is_contiguous()
    B, M, Ds, Hs, Ws = src.shape
    assert tuple(params.shape) == (B, M, _lib.AUG_NPARAM), f"params {tuple(params.shape)} do not match {B} x {M} volumes"
    grid = _elastic_tables(*elastic, B, name) if elastic is not None else None
    D, H, W = img_size
    out = torch.empty(B, M, 1, D, H, W, dtype=out_dtype, device=src.device)
    volumes = (B * M,) if elastic is None else (_ptr(elastic[0]), _ptr(elastic[1]), B * M, M, *grid)
    _call("xvit_" + name, name, src.numel() * float(src.element_size()) + out.numel() * float(out.element_size()), "byte",
          _ptr(src), _src_dt(src), _ptr(out), _dt(out), _ptr(params), *volumes, Ds, Hs, Ws, D, H, W, float(pad_value))
    return out


def augment_apply(src, params, img_size, pad_value=-1.0, out_dtype=torch.bfloat16):
    """xvit_augment_apply (include/xvit.h): src [B, M, Ds, Hs, Ws] (int16, bf16 or fp32) through the records params [B, M, 32] ->
    [B, M, 1, D, H, W] in out_dtype (bf16 or fp32): pad / crop, affine resample (or the exact copy), a v + b, noise, one rounding."""
    return _augment_apply("augment_apply", src, params, img_size, pad_value, out_dtype)


def _elastic_tables(field, erec, B, what):
    G = _lib.ELASTIC_MAX_GRID
    if not (isinstance(field, torch.Tensor) and field.dtype == torch.float32 and field.dim() == 5 and field.shape[0] == B and field.shape[1] == 3
            and all(4 <= n <= G for n in field.shape[2:]) and field.is_contiguous()):
        raise ValueError(f"{what}: the field must be a contiguous fp32 [{B}, 3, Gz, Gy, Gx] tensor with 4 <= G <= {G}, got "
                         f"{getattr(field, 'dtype', type(field))} {tuple(getattr(field, 'shape', ()))}")
    if not (isinstance(erec, torch.Tensor) and erec.dtype == torch.float32 and tuple(erec.shape) == (B, _lib.ELASTIC_NREC) and erec.is_contiguous()):
        raise ValueError(f"{what}: the record must be a contiguous fp32 [{B}, {_lib.ELASTIC_NREC}] tensor, got "
                         f"{getattr(erec, 'dtype', type(erec))} {tuple(getattr(erec, 'shape', ()))}")
    return tuple(field.shape[2:])


def elastic_draw(config, field, erec, seed, counter=None, advance=False):
    """xvit_elastic_draw (include/xvit.h): fill field [B, 3, Gz, Gy, Gx] and erec [B, 8] (fp32) with one B-spline control grid per sample drawn
    from `config` (_lib.ElasticConfig) and `seed`.  counter: as in augment_draw."""
    B = field.shape[0] if isinstance(field, torch.Tensor) and field.dim() == 5 else 0
    Gz, Gy, Gx = _elastic_tables(field, erec, B, "elastic_draw")
    _counter_arg(counter, "elastic_draw")
    _call("xvit_elastic_draw", "elastic_draw", (field.numel() + erec.numel()) * 4.0, "byte",
          C.byref(config), _ptr(field), _ptr(erec), B, Gz, Gy, Gx, _seed64(seed), _ptr(counter), int(bool(advance)))
    return field, erec


def augment_apply_elastic(src, params, field, erec, img_size, pad_value=-1.0, out_dtype=torch.bfloat16):
    """xvit_augment_apply_elastic (include/xvit.h): augment_apply with the B-spline displacement of field [B, 3, Gz, Gy, Gx] composed into
    the resample of every sample whose erec [B, 8] flag is 1; the other samples are processed as augment_apply processes them."""
    return _augment_apply("augment_apply_elastic", src, params, img_size, pad_value, out_dtype, elastic=(field, erec))


def contrast_draw(config, params, seed, counter=None, advance=False):
    """xvit_contrast_draw (include/xvit.h): fill params [B, M, 32] (fp32) with one blur / bias / gamma record per volume drawn from `config`
    (_lib.ContrastConfig) and `seed`.  counter: as in augment_draw."""
    assert params.dtype == torch.float32 and params.dim() == 3 and params.shape[2] == _lib.CON_NPARAM and params.is_contiguous()
    _counter_arg(counter, "contrast_draw")
    nvol = params.shape[0] * params.shape[1]
    _call("xvit_contrast_draw", "contrast_draw", params.numel() * 4.0, "byte", C.byref(config), _ptr(params), nvol, _seed64(seed), _ptr(counter), int(bool(advance)))
    return params


def contrast_apply(src, params, out_dtype=None):
    """xvit_contrast_apply (include/xvit.h): src [B, M, ..., D, H, W] (bf16 or fp32, contiguous) through the records params [B, M, 32] -> a
    new tensor of src's shape in out_dtype (None: src's): blur along x, y, z, bias field, gamma, one rounding."""
    assert src.dim() >= 5 and src.is_contiguous() and params.dtype == torch.float32 and params.is_contiguous()
    B, M = src.shape[:2]
    D, H, W = src.shape[-3:]
    assert src.numel() == B * M * D * H * W, f"volumes {tuple(src.shape)} are not [B, M, (1,) D, H, W]"
    assert tuple(params.shape) == (B, M, _lib.CON_NPARAM), f"params {tuple(params.shape)} do not match {B} x {M} volumes"
    out = torch.empty(src.shape, dtype=out_dtype or src.dtype, device=src.device)
    _call("xvit_contrast_apply", "contrast_apply", src.numel() * float(src.element_size()) + out.numel() * float(out.element_size()), "byte",
          _ptr(src), _ptr(out), _dt(src), _dt(out), _ptr(params), B * M, D, H, W)
    return out


def volume_stats_workspace(nvol, device):
    """The zero-filled histogram workspace of volume_stats for nvol volumes (xvit_volume_stats_workspace_bytes): every call leaves it
    zero again, so it is filled once, here."""
    return torch.zeros(_L.xvit_volume_stats_workspace_bytes(int(nvol)), dtype=torch.uint8, device=device)


def volume_stats(src, config, stats, workspace, params=None):
    """xvit_volume_stats (include/xvit.h): per-volume foreground statistics of src [B, M, ...] (int16 or bf16, contiguous) into stats
    [B, M, 8] (fp64): n, n_w, mean, std, lo, hi, min, max.  config: _lib.NormConfig.  params: the table [B, M, 32] of augment_draw, into
    which the normalisation is folded (mode 1 / 2), or None.  workspace: volume_stats_workspace(B * M, device).  An fp32 source is a
    TypeError carrying the library's message."""
    assert src.dim() >= 3 and src.is_contiguous() and stats.dtype == torch.float64 and stats.is_contiguous()
    B, M = src.shape[:2]
    nvox = src.numel() // (B * M)
    assert tuple(stats.shape) == (B, M, _lib.STATS_NSTAT), f"stats {tuple(stats.shape)} do not match {B} x {M} volumes"
    if params is not None:
        assert params.dtype == torch.float32 and params.is_contiguous() and tuple(params.shape) == (B, M, _lib.AUG_NPARAM)
    try:
        _call("xvit_volume_stats", "volume_stats", src.numel() * float(src.element_size()), "byte", _ptr(src), _src_dt(src), B * M, nvox, C.byref(config),
              _ptr(stats), _ptr(params), _ptr(workspace), workspace.numel() * workspace.element_size())
    except RuntimeError as e:
        if src.dtype == torch.float32:
            raise TypeError(str(e)) from None
        raise
    return stats


def volume_bbox_workspace(nvol, nvox, device):
    """The partial-box workspace of volume_bbox for nvol volumes of nvox voxels (xvit_volume_bbox_workspace_bytes); its contents do not
    matter on entry."""
    return torch.empty(_L.xvit_volume_bbox_workspace_bytes(int(nvol), int(nvox)), dtype=torch.uint8, device=device)


def volume_bbox(src, config, img_size, boxes, crop, workspace, params=None):
    """xvit_volume_bbox (include/xvit.h): the foreground index ranges of src [B, M, Ds, Hs, Ws] (int16, bf16 or fp32, contiguous) into boxes
    [B, M, 8] and the per-sample union, widened and clipped, into crop [B, 8] (both int32).  config: _lib.CropConfig.  params: the table
    [B, M, 32] of augment_draw, into which the crop towards img_size is folded (mode 1 / 2), or None.  workspace:
    volume_bbox_workspace(B * M, Ds * Hs * Ws, device)."""
    assert src.dim() == 5 and src.is_contiguous(), f"need contiguous [B, M, Ds, Hs, Ws] volumes, got {tuple(src.shape)}"
    B, M, Ds, Hs, Ws = src.shape
    assert boxes.dtype == torch.int32 and boxes.is_contiguous() and tuple(boxes.shape) == (B, M, _lib.BBOX_NREC), \
        f"boxes {boxes.dtype} {tuple(boxes.shape)} do not match {B} x {M} volumes"
    assert crop.dtype == torch.int32 and crop.is_contiguous() and tuple(crop.shape) == (B, _lib.BBOX_NREC), \
        f"crop {crop.dtype} {tuple(crop.shape)} does not match {B} samples"
    if params is not None:
        assert params.dtype == torch.float32 and params.is_contiguous() and tuple(params.shape) == (B, M, _lib.AUG_NPARAM)
    D, H, W = img_size
    _call("xvit_volume_bbox", "volume_bbox", src.numel() * float(src.element_size()), "byte", _ptr(src), _src_dt(src), B * M, M, Ds, Hs, Ws, D, H, W,
          C.byref(config), _ptr(boxes), _ptr(crop), _ptr(params), _ptr(workspace), workspace.numel() * workspace.element_size())
    return boxes, crop


def volume_components_workspace(nvol, nvox, device):
    """The workspace of volume_components and volume_bbox_components for nvol volumes of nvox voxels
    (xvit_volume_components_workspace_bytes: the accumulators, one int32 size per voxel and the partial boxes); the calls zero what they
    need, its contents do not matter on entry."""
    return torch.empty(_L.xvit_volume_components_workspace_bytes(int(nvol), int(nvox)), dtype=torch.uint8, device=device)


def _components_args(src, labels, comps):
    assert src.dim() == 5 and src.is_contiguous(), f"need contiguous [B, M, Ds, Hs, Ws] volumes, got {tuple(src.shape)}"
    assert labels.dtype == torch.int32 and labels.is_contiguous() and tuple(labels.shape) == tuple(src.shape), \
        f"labels {labels.dtype} {tuple(labels.shape)} do not match the volumes {tuple(src.shape)}"
    assert comps.dtype == torch.int32 and comps.is_contiguous() and tuple(comps.shape) == (*src.shape[:2], _lib.CC_NREC), \
        f"comps {comps.dtype} {tuple(comps.shape)} do not match {src.shape[0]} x {src.shape[1]} volumes"


def volume_components(src, config, labels, comps, workspace):
    """xvit_volume_components (include/xvit.h): the connected foreground components of src [B, M, Ds, Hs, Ws] (int16, bf16 or fp32,
    contiguous).  labels [B, M, Ds, Hs, Ws] (int32): the smallest flat index of a foreground voxel's component, -1 for background; comps
    [B, M, 8] (int32): the component table.  config: _lib.ComponentConfig.  workspace: volume_components_workspace(B * M, Ds * Hs * Ws,
    device)."""
    _components_args(src, labels, comps)
    B, M, Ds, Hs, Ws = src.shape
    _call("xvit_volume_components", "volume_components", src.numel() * (float(src.element_size()) + 8.0), "byte", _ptr(src), _src_dt(src), B * M, Ds, Hs, Ws,
          C.byref(config), _ptr(labels), _ptr(comps), _ptr(workspace), workspace.numel() * workspace.element_size())
    return labels, comps


def volume_bbox_components(src, config, components, img_size, boxes, crop, labels, comps, workspace, params=None):
    """xvit_volume_bbox_components (include/xvit.h): volume_components, then volume_bbox's boxes, crop and fold over the voxels of the kept
    components only.  config: _lib.CropConfig; components: _lib.ComponentConfig with the same foreground_above; the other arguments are
    those of volume_bbox and volume_components."""
    _components_args(src, labels, comps)
    B, M, Ds, Hs, Ws = src.shape
    assert boxes.dtype == torch.int32 and boxes.is_contiguous() and tuple(boxes.shape) == (B, M, _lib.BBOX_NREC), \
        f"boxes {boxes.dtype} {tuple(boxes.shape)} do not match {B} x {M} volumes"
    assert crop.dtype == torch.int32 and crop.is_contiguous() and tuple(crop.shape) == (B, _lib.BBOX_NREC), \
        f"crop {crop.dtype} {tuple(crop.shape)} does not match {B} samples"
    if params is not None:
        assert params.dtype == torch.float32 and params.is_contiguous() and tuple(params.shape) == (B, M, _lib.AUG_NPARAM)
    D, H, W = img_size
    _call("xvit_volume_bbox_components", "volume_bbox_components", src.numel() * (float(src.element_size()) + 12.0), "byte", _ptr(src), _src_dt(src), B * M, M, Ds,
          Hs, Ws, D, H, W, C.byref(config), C.byref(components), _ptr(boxes), _ptr(crop), _ptr(params), _ptr(labels), _ptr(comps), _ptr(workspace),
          workspace.numel() * workspace.element_size())
    return boxes, crop


def epoch_metrics_update(logits, labels, scores, labels32, preds, state):
    """xvit_epoch_metrics_update (include/xvit.h): append the step's softmax rows, labels and argmax to the epoch buffers at the device-side
    cursor state[0] and fold it into the integer confusion matrix behind the state head.  logits fp32 [B, C] (rows contiguous), labels
    int64 [B]; scores fp32 [cap, C], labels32 / preds int32 [cap], state int64 [EPOCH_STATE_HEAD + C * C].  One launch, no host read."""
    B, Cn = logits.shape
    cap = scores.shape[0]
    assert logits.dtype == torch.float32 and labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == B
    assert scores.dtype == torch.float32 and scores.is_contiguous() and scores.shape[1] == Cn
    assert labels32.dtype == torch.int32 and preds.dtype == torch.int32 and labels32.is_contiguous() and preds.is_contiguous()
    assert labels32.numel() == cap and preds.numel() == cap
    assert state.dtype == torch.int64 and state.is_contiguous() and state.numel() == _lib.EPOCH_STATE_HEAD + Cn * Cn
    _call("xvit_epoch_metrics_update", "epoch_metrics_update", B * Cn * 8.0, "byte",
          _ptr(logits), _rows2d(logits), _ptr(labels), B, Cn, _ptr(scores), _ptr(labels32), _ptr(preds), cap, _ptr(state))


def epoch_rank_stats_max_n() -> int:
    """xvit_epoch_rank_stats_max_n: the largest epoch (samples) xvit_epoch_rank_stats takes with bootstrap replicates."""
    return int(_L.xvit_epoch_rank_stats_max_n())


def epoch_rank_stats(scores, labels32, preds, perm, n_dev, n_max, R, seed):
    """xvit_epoch_rank_stats (include/xvit.h): for replicate 0 (every sample once) and R bootstrap replicates, per class: the tie-aware
    pair count u2, the positive / negative weight, the average precision and the confusion row.  perm int64 [C, >= n_max]: per class the
    samples in descending score order; n_dev: a one-element int64 device tensor (or view) holding the sample count, n_max its host bound.
    Returns (ranks int64 [R + 1, C, 3], ap fp64 [R + 1, C], conf int64 [R + 1, C, C])."""
    Cn = scores.shape[1]
    assert scores.dtype == torch.float32 and scores.is_contiguous() and labels32.dtype == torch.int32 and preds.dtype == torch.int32
    assert labels32.is_contiguous() and preds.is_contiguous() and min(scores.shape[0], labels32.numel(), preds.numel()) >= n_max
    assert perm.dtype == torch.int64 and perm.dim() == 2 and perm.shape[0] == Cn and perm.stride(1) == 1 and perm.shape[1] >= n_max
    assert n_dev.dtype == torch.int64 and n_dev.numel() >= 1
    dev = scores.device
    ranks = torch.empty(R + 1, Cn, _lib.EPOCH_RANK_NSTAT, dtype=torch.int64, device=dev)
    ap = torch.empty(R + 1, Cn, dtype=torch.float64, device=dev)
    conf = torch.empty(R + 1, Cn, Cn, dtype=torch.int64, device=dev)
    _call("xvit_epoch_rank_stats", "epoch_rank_stats", (R + 1) * Cn * float(n_max) * 16.0, "byte", _ptr(scores), _ptr(labels32), _ptr(preds),
          _ptr(perm), perm.stride(0), _ptr(n_dev), int(n_max), Cn, int(R), _seed64(seed), _ptr(ranks), _ptr(ap), _ptr(conf))
    return ranks, ap, conf


def batch_draw(idx, mode, n_cases, seed, *, cdf=None, rank=0, world=1, call=0, counter=None, advance=False):
    """xvit_batch_draw (include/xvit.h): fill idx int32 [B] with the case indices of one batch of a store of n_cases cases.  mode:
    _lib.BATCH_WEIGHTED (cdf: the fp64 [n_cases] inclusive prefix of the normalised weights, on the device), BATCH_SHUFFLE or
    BATCH_SEQUENTIAL.  The call index is `call`, or, with counter (a one-element int64 device tensor), read from it at kernel run time and
    advanced by one behind the read when advance is set."""
    if not (idx.dtype == torch.int32 and idx.dim() == 1 and idx.is_contiguous()):
        raise RuntimeError(f"batch_draw: idx is a contiguous int32 vector, got {idx.dtype} {tuple(idx.shape)}")
    if cdf is not None and not (cdf.dtype == torch.float64 and cdf.is_contiguous() and cdf.numel() == n_cases):
        raise RuntimeError(f"batch_draw: the cdf is a contiguous fp64 vector of {n_cases} entries, got {cdf.dtype} {tuple(cdf.shape)}")
    _counter_arg(counter, "batch_draw")
    B = idx.numel()
    _call("xvit_batch_draw", "batch_draw", B * 4.0, "byte", _ptr(idx), _ptr(cdf), int(n_cases), B, int(mode), int(rank), int(world), _seed64(seed),
          _seed64(call), _ptr(counter), int(bool(advance)))
    return idx


def batch_gather(store, idx, n_cases=None, labels=None, out=None, labels_out=None, status=None):
    """xvit_batch_gather (include/xvit.h): store [capacity, ...] (contiguous, any dtype of 2 or 4 bytes) and idx int32 [B], both on the
    device -> out [B, ...] with out[b] = store[idx[b]] among the first n_cases cases (None: all); labels int64 [capacity] -> labels_out
    int64 [B]; status int32 [B] (optional) receives 1 where an index was out of range (zeros, label -1), else 0.  Returns (out, labels_out)."""
    if not (store.dim() >= 1 and store.is_contiguous() and store.shape[0] > 0):
        raise RuntimeError(f"batch_gather: the store is a contiguous [capacity, ...] tensor, got {tuple(store.shape)} strides {store.stride()}")
    if not (idx.dtype == torch.int32 and idx.dim() == 1 and idx.is_contiguous() and idx.numel() > 0):
        raise RuntimeError(f"batch_gather: idx is a non-empty contiguous int32 vector, got {idx.dtype} {tuple(idx.shape)}")
    n_cases = store.shape[0] if n_cases is None else int(n_cases)
    if not 0 < n_cases <= store.shape[0]:
        raise RuntimeError(f"batch_gather: n_cases={n_cases} must lie in [1, {store.shape[0]}]")
    B = idx.numel()
    case_bytes = store[0].numel() * store.element_size()
    out = out if out is not None else torch.empty((B,) + tuple(store.shape[1:]), dtype=store.dtype, device=store.device)
    if not (out.dtype == store.dtype and out.is_contiguous() and tuple(out.shape) == (B,) + tuple(store.shape[1:])):
        raise RuntimeError("batch_gather: out must be contiguous, of the store's dtype and of shape [B, ...]")
    if labels is not None:
        if not (labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() >= n_cases):
            raise RuntimeError(f"batch_gather: labels is a contiguous int64 vector of at least {n_cases} entries")
        labels_out = labels_out if labels_out is not None else torch.empty(B, dtype=torch.int64, device=store.device)
        if not (labels_out.dtype == torch.int64 and labels_out.is_contiguous() and labels_out.numel() == B):
            raise RuntimeError(f"batch_gather: labels_out is a contiguous int64 vector of {B} entries")
    if status is not None and not (status.dtype == torch.int32 and status.is_contiguous() and status.numel() == B):
        raise RuntimeError(f"batch_gather: status is a contiguous int32 vector of {B} entries")
    # one read and one write per byte of the batch
    _call("xvit_batch_gather", "batch_gather", 2.0 * B * case_bytes, "byte", _ptr(store), case_bytes, n_cases, _ptr(idx), B, _ptr(out),
          _ptr(labels), _ptr(labels_out) if labels is not None else None, _ptr(status))
    return out, (labels_out if labels is not None else None)
