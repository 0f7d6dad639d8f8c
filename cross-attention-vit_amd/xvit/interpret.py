"""Where the model looked: the CLS token's attention maps and attention rollout of ModelCross / ModelVIT, in eval mode.

    maps = xvit.interpret.attention_maps(model, img, rollout=True)      # model.eval(); img [B, M, 1, D, H, W] on the GPU; no labels
    maps.self_attn["transformer.0.blocks.1.0"]    # [B, H, N] fp32: CLS row of that self-attention block (ModelVIT: "transformer.layers.3")
    maps.fusion["transformer.1.fusion.0"]         # [B, H, N] fp32: CLS-query probabilities of that fusion (key 0 = CLS_i, keys 1.. = the
                                                  #   patches of the modality it reads, model_cross.py:140)
    maps.rollout[m]                               # [B, N] fp32: rollout of modality m's self-attention chain (ModelVIT: key 0)
    grid = xvit.interpret.patch_grid(maps.rollout[0][:, 1:], cfg.img_size, cfg.patch_size)   # [B, D/p1, H/p2, W/p3]

The reference builds its attention probabilities as tensors (model_cross.py:55-59, :93-97); the fused kernels here never write them.
The maps are taken inside one forward pass instead: the CLS row of a self-attention block is the CLS-query kernel
(xvit_cls_xattn_fwd) run on the block's own qkv, a fusion's map is the probabilities its forward computes anyway, and rollout
recomputes each block's probabilities from its q, k and log-sum-exp (xvit_attn_rollout_step) without storing them.
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


class _Recorder:
    """Receives what the forward computed (xvit.functional.ATTN_RECORDER) for the modules it knows, by their first LayerNorm weight."""

    def __init__(self, names, rollout):
        self.names = names               # data_ptr of the block's first LayerNorm weight -> qualified name
        self.rollout = rollout
        self.self_maps, self.fusion_maps, self.saved = {}, {}, {}

    def self_block(self, ln1w, qkv, lse, B, N, H, scale):
        name = self.names.get(ln1w.data_ptr())
        if name is None:
            return
        d = qkv.shape[1] // 3
        q0 = qkv.view(B, N, 3 * d)[:, 0, :d]            # each sample's CLS query row (row stride N * 3d)
        _, p = ops.cls_xattn_fwd(q0, qkv[:, d:], B, N, H, scale)
        self.self_maps[name] = p
        if self.rollout:
            self.saved[name] = (qkv, lse, B, N, H, scale)

    def fusion(self, ln1w, B, N, H, p=None, e=None, rz=None):
        name = self.names.get(ln1w.data_ptr())
        if name is None:
            return
        if p is None:   # low-rank form: p[b, h, n] = e[b, n, h] / sum_n e[b, n, h] (rz is computed from the rounded e: head_linear.hip)
            p = (e[:, :, :H].float() * rz[:, None, :]).permute(0, 2, 1).contiguous()
        self.fusion_maps[name] = p


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


def _check(model, img):
    if not isinstance(model, (ModelCross, ModelVIT)):
        raise TypeError(f"attention_maps: need a ModelCross or a ModelVIT, got {type(model).__name__}")
    if model.training:
        raise RuntimeError("attention_maps: the model is in training mode (dropout would make the maps random); call model.eval() first")
    if os.environ.get("XVIT_ATTN_FP8", "0") == "1":
        raise RuntimeError("attention_maps: the maps are defined on the bf16 attention forward; unset XVIT_ATTN_FP8")
    if not (img.is_cuda and model.pos_embedding.is_cuda):
        raise RuntimeError("attention_maps: model and img must be on the GPU (the maps come from the HIP kernels; there is no CPU path)")
    if isinstance(model, ModelCross):
        blocks = [m for m in model.modules() if isinstance(m, (SelfAttentionBlock, CrossAttentionBlock))]
        heads = [b.attn.fn.heads if isinstance(b, SelfAttentionBlock) else b.attn.fn.num_heads for b in blocks]
    else:
        heads = [layer[0].fn.heads for layer in model.transformer.layers]
    d = model.pos_embedding.shape[-1]
    for H in heads:
        if d // H != 64:
            raise ValueError(f"attention_maps: head dim {d // H} unsupported (only 64)")


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
    _check(model, img)
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
