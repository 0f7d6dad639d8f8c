"""Where the model looked: the CLS token's attention maps and attention rollout of ModelCross / ModelVIT, in eval mode.

    maps = xvit.interpret.attention_maps(model, img, rollout=True)      # model.eval(); img [B, M, 1, D, H, W] on the GPU; no labels
    maps.self_attn["transformer.0.blocks.1.0"]    # [B, H, N] fp32: CLS row of that self-attention block (ModelVIT: "transformer.layers.3")
    maps.fusion["transformer.1.fusion.0"]         # [B, H, N] fp32: CLS-query probabilities of that fusion (key 0 = CLS_i, keys 1.. = the
                                                  #   patches of the modality it reads, model_cross.py:140)
    maps.rollout[m]                               # [B, N] fp32: rollout of modality m's self-attention chain (ModelVIT: key 0)
    grid = xvit.interpret.patch_grid(maps.rollout[0][:, 1:], cfg.img_size, cfg.patch_size)   # [B, D/p1, H/p2, W/p3]

    rel = xvit.interpret.relevance_maps(model, img, target=None)         # class-specific: which tokens drove the logit of `target`
    rel.relevance[m]                              # [B, N] fp32: gradient-weighted relevance of modality m's self-attention chain
    rel.fusion["transformer.1.fusion.0"]          # [B, N] fp32: gradient-weighted CLS-query map of that fusion

    att = xvit.interpret.input_attributions(model, img, method="integrated_gradients", steps=32)   # voxel resolution
    att.attributions                              # [B, M, D, H, W] fp32; att.delta [B]: the completeness residual

The reference builds its attention probabilities as tensors (model_cross.py:55-59, :93-97); the fused kernels here never write them.
The maps are taken inside one forward pass instead: the CLS row of a self-attention block is the CLS-query kernel
(xvit_cls_xattn_fwd) run on the block's own qkv, a fusion's map is the probabilities its forward computes anyway, and rollout
recomputes each block's probabilities from its q, k and log-sum-exp (xvit_attn_rollout_step) without storing them.  Relevance adds
one backward: each block's attention-output gradient dO is recorded there, and xvit_attn_relevance_step recomputes P and dP = dO V^T
the same way.  Voxel attributions (input_attributions) take the gradient through the patch embedding back onto the volume grid: the
fused input-gradient GEMM (xvit_patch_embed_dgrad) scatters dX W straight to the voxels.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import torch

from . import functional as XF
from . import ops
from .cross_vit import STREAM_MODE, CrossAttentionBlock, ModelCross, SelfAttentionBlock
from .vit import ModelVIT


@dataclass
class AttentionMaps:
    """Maps keyed by the modules' qualified names (the prefixes of their state_dict keys)."""
    self_attn: dict = field(default_factory=dict)
    fusion: dict = field(default_factory=dict)
    rollout: dict = field(default_factory=dict)
    logits: torch.Tensor | None = None     # the forward's logits: those of model(img, labels) in eval mode


@dataclass
class RelevanceMaps:
    """Class-specific maps keyed like AttentionMaps' rollout (relevance) and fusion (fusion)."""
    relevance: dict = field(default_factory=dict)
    fusion: dict = field(default_factory=dict)
    logits: torch.Tensor | None = None     # the forward's logits: those of model(img, labels) in eval mode
    target: torch.Tensor | None = None     # int64 [B]: the class explained per sample


@dataclass
class InputAttributions:
    """Voxel attributions of input_attributions."""
    attributions: torch.Tensor | None = None   # fp32 [B, M, D, H, W]
    logits: torch.Tensor | None = None     # the forward's logits on img: those of model(img, labels) in eval mode
    target: torch.Tensor | None = None     # int64 [B]: the class explained per sample
    delta: torch.Tensor | None = None      # fp32 [B], integrated_gradients only: sum(attributions) - (logit_t(img) - logit_t(baseline))


class _Recorder:
    """Receives what the forward computed (xvit.functional.ATTN_RECORDER) for the modules it knows, by their first LayerNorm weight."""

    def __init__(self, names, rollout=False, relevance=False):
        self.names = names               # data_ptr of the block's first LayerNorm weight -> qualified name
        self.rollout, self.relevance = rollout, relevance     # relevance: no CLS maps; keep qkv / lse, take dO and the fusions' gradients
        self.self_maps, self.fusion_maps, self.saved = {}, {}, {}
        self.grads, self.fusion_rel, self.bv = {}, {}, {}

    def self_block(self, ln1w, qkv, lse, B, N, H, scale):
        name = self.names.get(ln1w.data_ptr())
        if name is None:
            return
        if not self.relevance:
            d = qkv.shape[1] // 3
            q0 = qkv.view(B, N, 3 * d)[:, 0, :d]            # each sample's CLS query row (row stride N * 3d)
            _, p = ops.cls_xattn_fwd(q0, qkv[:, d:], B, N, H, scale)
            self.self_maps[name] = p
        if self.rollout or self.relevance:
            self.saved[name] = (qkv, lse, B, N, H, scale)

    def self_block_grad(self, ln1w, do):
        name = self.names.get(ln1w.data_ptr())
        if name is not None:
            self.grads[name] = do            # bf16 [B*N, d]: the gradient of the block's attention output

    def fusion(self, ln1w, B, N, H, p=None, e=None, rz=None, bv=None):
        name = self.names.get(ln1w.data_ptr())
        if name is None:
            return
        if p is None:   # low-rank form: p[b, h, n] = e[b, n, h] / sum_n e[b, n, h] (rz is computed from the rounded e: head_linear.hip)
            p = (e[:, :, :H].float() * rz[:, None, :]).permute(0, 2, 1).contiguous()
        self.fusion_maps[name] = p
        if self.relevance and bv is not None:
            self.bv[name] = bv

    def fusion_grad(self, ln1w, B, N, H, doc, dp=None, v=None):
        """doc [B, d]: the gradient of the fusion's attention output.  Low-rank form: dp [B, N, 16] = dO_h . (v_h[n] - bv_h), the
        backward's own product, plus the bias term dO_h . bv_h (constant in n); literal order: v [B*N, d], the second half of kv."""
        name = self.names.get(ln1w.data_ptr())
        if name is None or not self.relevance:
            return
        dh = doc.shape[1] // H
        do = doc.float().view(B, H, dh)
        if v is None:
            dpv = dp[:, :, :H].permute(0, 2, 1) + (do * self.bv[name].float().view(H, dh)).sum(-1)[:, :, None]
        else:
            dpv = torch.einsum("bhk,bnhk->bhn", do, v.float().view(B, N, H, dh))
        self.fusion_rel[name] = (self.fusion_maps[name] * dpv).clamp_min(0).mean(dim=1)


class _InputGradRecorder(_Recorder):
    """Knows no attention module (every map hook returns at once); takes the fp32 volume gradient PatchEmbedFn's backward computes
    when a recorder with input_grad is set (xvit.functional.ATTN_RECORDER)."""
    input_grad = True

    def __init__(self):
        super().__init__({})
        self.dimg = None

    def take_input_grad(self, dimg):
        self.dimg = dimg


def _chains(model):
    """(names of the blocks' first LayerNorm weights, {rollout key: self-attention block names in forward order})."""
    names, chains = {}, {}
    if isinstance(model, ModelCross):
        for prefix, mod in model.named_modules():
            if isinstance(mod, (SelfAttentionBlock, CrossAttentionBlock)):
                names[mod.attn.norm.weight.data_ptr()] = prefix
        for m in range(model.num_modalities):
            chains[m] = [f"transformer.{k}.blocks.{m}.{s}" for k, msb in enumerate(model.transformer) for s in range(len(msb.blocks[m]))]
    else:
        for l, layer in enumerate(model.transformer.layers):
            names[layer[0].norm.weight.data_ptr()] = f"transformer.layers.{l}"
        chains[0] = [f"transformer.layers.{l}" for l in range(len(model.transformer.layers))]
    return names, {k: v for k, v in chains.items() if v}


def _check(model, img, who):
    """The refusals of attention_maps and relevance_maps (`who`: the caller's name in the messages)."""
    if not isinstance(model, (ModelCross, ModelVIT)):
        raise TypeError(f"{who}: need a ModelCross or a ModelVIT, got {type(model).__name__}")
    if model.training:
        raise RuntimeError(f"{who}: the model is in training mode (dropout would make the maps random); call model.eval() first")
    if getattr(model, "eval_patch_dropout", 0.0) > 0.0:
        raise RuntimeError(f"{who}: the model's eval() forward keeps a subset of the patch tokens (eval_patch_dropout = {model.eval_patch_dropout}) and the "
                           "maps are defined on the full grid; set model.eval_patch_dropout = 0 for the maps")
    if os.environ.get("XVIT_ATTN_FP8", "0") == "1":
        raise RuntimeError(f"{who}: the maps are defined on the bf16 attention forward; unset XVIT_ATTN_FP8")
    if not (img.is_cuda and model.pos_embedding.is_cuda):
        raise RuntimeError(f"{who}: model and img must be on the GPU (the maps come from the HIP kernels; there is no CPU path)")
    if isinstance(model, ModelCross):
        blocks = [m for m in model.modules() if isinstance(m, (SelfAttentionBlock, CrossAttentionBlock))]
        heads = [b.attn.fn.heads if isinstance(b, SelfAttentionBlock) else b.attn.fn.num_heads for b in blocks]
    else:
        heads = [layer[0].fn.heads for layer in model.transformer.layers]
    d = model.pos_embedding.shape[-1]
    for H in heads:
        if d // H != 64:
            raise ValueError(f"{who}: head dim {d // H} unsupported (only 64)")


def attention_maps(model, img, rollout=False) -> AttentionMaps:
    """The CLS token's attention maps of every self-attention block and fusion, from one eval forward of `model` on `img`.

    self_attn[name] : [B, H, N] fp32, row 0 (the CLS query) of the block's attention probabilities.
    fusion[name]    : [B, H, N] fp32, the fusion's CLS-query probabilities (key 0 = CLS_i, keys 1.. = modality j's patches).
    rollout[key]    : [B, N] fp32 (rollout=True).  Attention rollout (Abnar & Zuidema 2020) of one branch: starting from r = e_0 (one-hot
                      on token 0), r <- r / 2 + (r . mean_h P_h) / 2 through the branch's self-attention blocks from the last to the first,
                      across all MultiScaleBlocks.  Fusions are not part of it (their maps are reported in `fusion`).  Keys: the modality
                      index m for ModelCross (no entry for a branch without self-attention blocks), 0 for ModelVIT.  Each row sums to one.
    logits          : the forward's logits, bit-identical to those of model(img, labels) in eval mode.

    Runs under torch.no_grad() with zero labels, on the current stream only.  Refuses training mode (dropout would make the maps
    random), XVIT_ATTN_FP8=1 (the maps are defined on the bf16 forward), tensors off the GPU and head dims other than 64.  With rollout
    the qkv and lse of every self-attention block stay alive until the rollout is done (19 MB per block at configs[1], B = 8)."""
    _check(model, img, "attention_maps")
    names, chains = _chains(model)
    rec = _Recorder(names, rollout)
    labels = torch.zeros(img.shape[0], dtype=torch.long, device=img.device)
    tok_rec, tok_mode = XF.ATTN_RECORDER.set(rec), STREAM_MODE.set("0")   # one stream: the map kernels are ordered on the caller's stream
    try:
        with torch.no_grad():
            logits, _ = model(img, labels)
            maps = AttentionMaps(self_attn=rec.self_maps, fusion=rec.fusion_maps, logits=logits)
            if rollout:
                for key, chain in chains.items():
                    B, N = rec.saved[chain[-1]][2:4]
                    r = torch.zeros(B, N, dtype=torch.float32, device=img.device)
                    r[:, 0] = 1.0
                    for name in reversed(chain):
                        qkv, lse, B, N, H, scale = rec.saved[name]
                        r = ops.attn_rollout_step(qkv, lse, r, B, N, H, scale)
                    maps.rollout[key] = r
    finally:
        STREAM_MODE.reset(tok_mode)
        XF.ATTN_RECORDER.reset(tok_rec)
        rec.saved.clear()
    return maps


def relevance_maps(model, img, target=None) -> RelevanceMaps:
    """Class-specific relevance (Chefer, Gur & Wolf, ICCV 2021, "Generic Attention-model Explainability for Interpreting Bi-Modal and
    Encoder-Decoder Transformers") of `model` on `img`: which tokens drove the logit of `target`, per sample.

    target          : None (each sample's argmax), an int, or an int64 tensor [B].
    relevance[key]  : [B, N] fp32.  Starting from r = e_0, r <- r + r . mean_h relu(P_h * dP_h) through the branch's self-attention blocks
                      from the last to the first, across all MultiScaleBlocks (the chains of attention_maps' rollout; keys likewise: the
                      modality index m for ModelCross, 0 for ModelVIT).  dP_h = dO_h V_h^T is the gradient of the target logit with
                      respect to P_h; P and dP are recomputed per block by xvit_attn_relevance_step, never stored.
    fusion[name]    : [B, N] fp32, mean_h relu(p_h * dp_h) of the fusion's CLS-query probabilities p and their gradient dp (key 0 = CLS_i,
                      keys 1.. = modality j's patches).
    logits, target  : the forward's logits (bit-identical to those of model(img, labels) in eval mode) and the classes explained.

    Costs one eval forward with grad enabled and one backward, on the current stream only: torch.autograd.grad of the logits with
    grad_outputs one_hot(target) (samples are independent, so one backward serves the batch).  Every p.grad stays as it was, and no
    weight gradient reaches a data-parallel reducer's buckets (XF.GRAD_SINK is unset for the duration).  Memory: the qkv, lse and dO of
    every self-attention block stay alive until the chains are done (8 d bytes per token: 25 MB per block at configs[1], B = 8).
    Refuses what attention_maps refuses: training mode, XVIT_ATTN_FP8=1, tensors off the GPU and head dims other than 64."""
    _check(model, img, "relevance_maps")
    names, chains = _chains(model)
    B = img.shape[0]
    if target is not None:
        target = torch.as_tensor(target, dtype=torch.int64, device=img.device)
        target = target.expand(B).contiguous() if target.dim() == 0 else target
        if tuple(target.shape) != (B,):
            raise ValueError(f"relevance_maps: target must be an int or an int64 tensor [{B}], got shape {tuple(target.shape)}")
    rec = _Recorder(names, relevance=True)
    labels = torch.zeros(B, dtype=torch.long, device=img.device)
    params = [p for p in model.parameters() if p.requires_grad]
    if not params:
        raise RuntimeError("relevance_maps: no parameter of the model requires grad (the backward would not run)")
    tok_rec, tok_mode = XF.ATTN_RECORDER.set(rec), STREAM_MODE.set("0")   # one stream: the backward and the steps are ordered on it
    sink, arena = XF.GRAD_SINK, list(XF._ARENA)   # the forward opens a zero arena of its own: a pending training backward keeps its one
    XF.GRAD_SINK = None                  # weight gradients go to fresh tensors, never into a reducer's bucket
    try:
        with torch.enable_grad():
            logits, _ = model(img, labels)
            C = logits.shape[1]
            if target is None:
                target = logits.detach().argmax(dim=1)
            elif int(target.min()) < 0 or int(target.max()) >= C:
                raise ValueError(f"relevance_maps: target out of range [0, {C})")
            seed = torch.nn.functional.one_hot(target, C).to(logits.dtype)
            grads = torch.autograd.grad(logits, params, grad_outputs=seed, allow_unused=True)
            del grads
        out = RelevanceMaps(fusion=rec.fusion_rel, logits=logits.detach(), target=target)
        for key, chain in chains.items():
            missing = [n for n in chain if n not in rec.grads]
            if missing:
                raise RuntimeError(f"relevance_maps: the backward did not reach {missing[0]} (do its parameters require grad?)")
            B, N = rec.saved[chain[-1]][2:4]
            r = torch.zeros(B, N, dtype=torch.float32, device=img.device)
            r[:, 0] = 1.0
            for name in reversed(chain):
                qkv, lse, B, N, H, scale = rec.saved[name]
                r = ops.attn_relevance_step(qkv, lse, rec.grads[name], r, B, N, H, scale)
            out.relevance[key] = r
    finally:
        XF.GRAD_SINK = sink
        XF._ARENA[:] = arena
        STREAM_MODE.reset(tok_mode)
        XF.ATTN_RECORDER.reset(tok_rec)
        rec.saved.clear()
        rec.grads.clear()
    return out


ATTRIBUTION_METHODS = ("gradient", "grad_x_input", "integrated_gradients")


def input_attributions(model, img, target=None, method="integrated_gradients", steps=32, baseline=None, batch_size=16) -> InputAttributions:
    """Voxel-level attributions of `model` on `img` [B, M, 1, D, H, W]: which voxels drove the logit of `target`, per sample.

    method          : "gradient"              d logit_t / d img;
                      "grad_x_input"          that gradient times (img - baseline);
                      "integrated_gradients"  (Sundararajan, Taly & Yan, ICML 2017) (img - baseline) times the mean gradient at the
                                              `steps` points baseline + a_k (img - baseline), a_k = (k + 1/2) / steps (midpoint rule).
    target          : None (each sample's argmax), an int, or an integer tensor [B] (floating-point targets are refused); a class
                      out of range is refused before any gradient is seeded.
    baseline        : None (zeros) or a GPU tensor [1 or B, M, 1, D, H, W].
    batch_size      : the volumes of one pass (interpolants of every sample laid along the batch): at most this many per forward +
                      backward, so a single volume's IG scan still fills the GPU.
    attributions    : fp32 [B, M, D, H, W], also for bf16 volumes (the gradient comes out of the fused input-gradient kernel in fp32).
    logits, target  : the forward's logits on img and the classes explained.
    delta           : integrated_gradients only, fp32 [B]: the completeness residual sum(attributions) - (logit_t(img) - logit_t(baseline));
                      it shrinks as `steps` grows.

    Interpolants are built in img's dtype (a bf16 volume keeps the fused patch-embedding forward).  Each pass is one eval forward with
    grad enabled and one backward on the current stream.  The backward computes every weight gradient too (each backward Function
    does): an attribution pass costs a full training backward plus the input-gradient GEMM.  Every p.grad stays as it was, no weight
    gradient reaches a data-parallel reducer's buckets, and the zero arena and stream mode are restored.  Refuses training mode,
    XVIT_ATTN_FP8=1, tensors off the GPU and head dims other than 64."""
    who = "input_attributions"
    if method not in ATTRIBUTION_METHODS:
        raise ValueError(f"{who}: method must be one of {ATTRIBUTION_METHODS}, got {method!r}")
    if int(steps) < 1 or int(batch_size) < 1:
        raise ValueError(f"{who}: steps and batch_size must be >= 1 (got {steps}, {batch_size})")
    steps, batch_size = int(steps), int(batch_size)
    if img.dim() != 6 or img.shape[2] != 1:
        raise ValueError(f"{who}: img must be [B, M, 1, D, H, W], got shape {tuple(img.shape)}")
    B = img.shape[0]
    if target is not None:
        t_in = torch.as_tensor(target)
        if t_in.is_floating_point() or t_in.is_complex() or t_in.dtype == torch.bool:
            raise ValueError(f"{who}: target must be an int or an integer tensor [{B}], got dtype {t_in.dtype} (a class index is never rounded)")
        target = t_in.to(torch.int64)
        target = target.expand(B).contiguous() if target.dim() == 0 else target
        if tuple(target.shape) != (B,):
            raise ValueError(f"{who}: target must be an int or an int64 tensor [{B}], got shape {tuple(target.shape)}")
        if B > 0 and int(target.min()) < 0:
            raise ValueError(f"{who}: target out of range: negative class {int(target.min())}")
    if baseline is not None and (baseline.dim() != 6 or baseline.shape[0] not in (1, B) or baseline.shape[1:] != img.shape[1:]):
        raise ValueError(f"{who}: baseline must be [1 or {B}, {', '.join(str(s) for s in img.shape[1:])}], got shape {tuple(baseline.shape)}")
    _check(model, img, who)
    if baseline is not None and not baseline.is_cuda:
        raise RuntimeError(f"{who}: baseline must be on the GPU")
    dev = img.device
    img = img.detach()
    base = torch.zeros((1,) + tuple(img.shape[1:]), dtype=img.dtype, device=dev) if baseline is None else baseline.detach().to(img.dtype)
    rec = _InputGradRecorder()
    tok_rec, tok_mode = XF.ATTN_RECORDER.set(rec), STREAM_MODE.set("0")   # one stream: forward, backward and the sums are ordered on it
    sink, arena = XF.GRAD_SINK, list(XF._ARENA)
    XF.GRAD_SINK = None                  # weight gradients go to fresh tensors, never into a reducer's bucket

    def forward(x):                      # logits of x in passes of at most batch_size volumes, no graph
        with torch.no_grad():
            return torch.cat([model(x[i:i + batch_size], torch.zeros(min(batch_size, x.shape[0] - i), dtype=torch.long, device=dev))[0]
                              for i in range(0, x.shape[0], batch_size)])

    def check_target(t, C):              # before any one_hot: on the GPU, one_hot leaves its bounds to the scatter kernel
        if int(t.min()) < 0 or int(t.max()) >= C:
            raise ValueError(f"{who}: target out of range [0, {C})")

    def grad_pass(x, t):                 # fp32 d(sum_i logits[i, t[i]]) / dx and the logits: one forward + backward
        xin = x.detach().requires_grad_(True)
        with torch.enable_grad():
            logits, _ = model(xin, torch.zeros(x.shape[0], dtype=torch.long, device=dev))
            if t is None:
                t = logits.detach().argmax(dim=1)
            check_target(t, logits.shape[1])
            seed = torch.nn.functional.one_hot(t, logits.shape[1]).to(logits.dtype)
            rec.dimg = None
            torch.autograd.grad(logits, xin, grad_outputs=seed, allow_unused=True)
        g, rec.dimg = rec.dimg, None
        return g, logits.detach(), t

    try:
        if target is not None:
            target = target.to(dev)
        if method == "integrated_gradients":
            logits = forward(img)
            C = logits.shape[1]
            if target is None:
                target = logits.argmax(dim=1)
            check_target(target, C)
            lb = forward(base)
            lb = lb.expand(B, C) if lb.shape[0] == 1 else lb
            diff = img.float() - base.float()                       # [B, ...] (a [1, ...] baseline broadcasts)
            gsum = torch.zeros(img.shape, dtype=torch.float32, device=dev)
            smp = torch.arange(B, device=dev).repeat_interleave(steps)     # (sample, step) pairs, sample-major
            alpha = ((torch.arange(steps, dtype=torch.float32, device=dev) + 0.5) / steps).repeat(B)
            for i in range(0, B * steps, batch_size):
                j = min(B * steps, i + batch_size)
                idx, a = smp[i:j], alpha[i:j]
                b0 = base[idx] if base.shape[0] == B else base.expand(j - i, *base.shape[1:])
                x = (b0.float() + a.view(-1, 1, 1, 1, 1, 1) * diff[idx]).to(img.dtype)
                g, _, _ = grad_pass(x, target[idx])
                for s in range(i // steps, (j - 1) // steps + 1):           # each sample's rows of this pass, summed in a fixed order
                    lo, hi = max(i, s * steps) - i, min(j, (s + 1) * steps) - i
                    gsum[s] += g[lo:hi].sum(dim=0)
            attr = diff * (gsum / steps)
            gather = lambda l: l.gather(1, target.view(B, 1)).view(B)   # noqa: E731
            delta = attr.reshape(B, -1).sum(dim=1) - (gather(logits) - gather(lb))
            out = InputAttributions(attributions=attr[:, :, 0], logits=logits, target=target, delta=delta)
        else:
            parts, lparts, tparts = [], [], []
            for i in range(0, B, batch_size):
                g, l, t = grad_pass(img[i:i + batch_size], None if target is None else target[i:i + batch_size])
                parts.append(g); lparts.append(l); tparts.append(t)
            g = torch.cat(parts) if len(parts) > 1 else parts[0]
            if method == "grad_x_input":
                g = g * (img.float() - base.float())
            out = InputAttributions(attributions=g[:, :, 0], logits=torch.cat(lparts), target=torch.cat(tparts))
    finally:
        XF.GRAD_SINK = sink
        XF._ARENA[:] = arena
        STREAM_MODE.reset(tok_mode)
        XF.ATTN_RECORDER.reset(tok_rec)
        rec.dimg = None
    return out


def patch_grid(t, img_size, patch_size, num_modalities=1):
    """Patch tokens back onto the volume's patch grid: t [..., P] -> [..., D/p1, H/p2, W/p3] (the volume's (D, H, W) axis order).
    Inverts the reference's token order t = (h Wn + w) Dn + d (model_cross.py:193, oracle/ref_cpu.py:patchify).  Drop token 0 (CLS)
    first: patch_grid(maps.rollout[m][:, 1:], cfg.img_size, cfg.patch_size).

    ModelVIT concatenates the M modalities' patch tokens in order (N - 1 = M P): pass num_modalities=M to get [..., M, D/p1, H/p2, W/p3]."""
    Dn, Hn, Wn = (s // p for s, p in zip(img_size, patch_size))
    P = Dn * Hn * Wn
    if t.shape[-1] != num_modalities * P:
        raise ValueError(f"patch_grid: last dim {t.shape[-1]} is not {num_modalities} x {P} patch tokens (drop the CLS token first)")
    lead = t.shape[:-1]
    g = t.reshape(*lead, num_modalities, Hn, Wn, Dn)
    g = g.permute(*range(len(lead) + 1), -1, -3, -2)       # (h, w, d) -> (d, h, w)
    return g if num_modalities > 1 else g.squeeze(len(lead))
