"""Masked-volume pretraining (MAE, He et al. 2022) of a ModelCross encoder.

    mae = xvit.MaskedVolumeModel(config, mask_ratio=0.75).cuda()
    loss_seq, loss = mae(img)                       # img [B, M, 1, D, H, W]; loss_seq [M, B]; loss.backward() as usual
    ModelCross(config).load_state_dict(mae.encoder.state_dict())      # fine-tune from the pretrained encoder

Every sequence (one modality of one sample) keeps K of its P patches (the draw of patch dropout, xvit_token_select_draw); the encoder runs
on the kept tokens; a light decoder, shared by the modalities, runs on the full grid with a mask token in the dropped places; only the
dropped rows reach the prediction head, and the fused loss kernel scores them against the volume's own voxels (csrc/mae.hip)."""
from __future__ import annotations

import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import _lib
from . import functional as XF
from .cross_vit import ModelCross, SelfAttentionBlock, _lin


class MaskedVolumeModel(nn.Module):
    """forward(img, labels=None) -> (loss_seq [M, B], loss).  `encoder`: a ModelCross, or a config from which one is built."""

    def __init__(self, encoder, decoder_dim=512, decoder_depth=2, decoder_heads=None, mask_ratio=0.75, mask_shared=False, norm_pix_loss=True,
                 decoder_mlp_dim=None):
        super().__init__()
        if not 0.0 < float(mask_ratio) < 1.0:
            raise ValueError(f"MaskedVolumeModel: mask_ratio must be inside (0, 1), got {mask_ratio}")
        if decoder_dim <= 0 or decoder_dim % 64 != 0:
            raise ValueError(f"MaskedVolumeModel: decoder_dim must be a positive multiple of 64 (64-wide attention heads), got {decoder_dim}")
        heads = decoder_dim // 64 if decoder_heads is None else int(decoder_heads)
        if heads * 64 != decoder_dim:
            raise ValueError(f"MaskedVolumeModel: decoder_heads * 64 must equal decoder_dim ({heads} * 64 != {decoder_dim})")
        if decoder_depth < 1:
            raise ValueError(f"MaskedVolumeModel: decoder_depth must be at least 1, got {decoder_depth}")
        if not isinstance(encoder, ModelCross):
            encoder = ModelCross(encoder)
        self.encoder = encoder
        P, d = encoder.pos_embedding.shape[1] - 1, encoder.pos_embedding.shape[2]
        M, dd, pd = encoder.num_modalities, int(decoder_dim), encoder.patch_to_embedding.weight.shape[1]
        if P > _lib.TOKEN_SELECT_MAX_P:
            raise ValueError(f"MaskedVolumeModel: {P} patches per sequence; the mask is drawn for at most {_lib.TOKEN_SELECT_MAX_P}")
        if pd > _lib.MAE_MAX_PD:
            raise ValueError(f"MaskedVolumeModel: a patch of {pd} voxels; the loss kernel takes at most {_lib.MAE_MAX_PD}")
        K = XF.patch_keep_count(P, float(mask_ratio))
        if K >= P:
            raise ValueError(f"MaskedVolumeModel: mask_ratio {mask_ratio} drops none of the {P} patches (K == P): nothing to predict")
        self.mask_ratio, self.mask_shared, self.norm_pix_loss = float(mask_ratio), bool(mask_shared), bool(norm_pix_loss)
        self.num_kept, self.num_dropped = K, P - K
        self.decoder_embed = _lin(d, dd)
        self.mask_token = nn.Parameter(torch.empty(1, 1, dd))
        self.decoder_pos_embed = nn.Parameter(torch.empty(1, P + 1, dd))
        self.decoder_modality_embed = nn.Parameter(torch.empty(M, 1, dd))
        cfg = SimpleNamespace(hidden_dim=dd, num_heads=heads, mlp_dim=int(decoder_mlp_dim or 4 * dd), dropout=0.0)
        self.decoder_blocks = nn.Sequential(*(SelfAttentionBlock(cfg) for _ in range(int(decoder_depth))))
        self.decoder_norm = nn.LayerNorm(dd)
        self.decoder_pred = _lin(dd, pd)
        # int32 [M, B, K] / [M, B, P - K]: the patches the last forward kept / dropped (ascending).  The tensors a capture leaves here are
        # the graph's own and follow its replays
        self.last_token_keep = None
        self.last_token_drop = None
        for mod in (self.decoder_embed, self.decoder_blocks, self.decoder_norm, self.decoder_pred):
            mod.apply(ModelCross.init_weights)
        for t in (self.mask_token, self.decoder_pos_embed, self.decoder_modality_embed):
            nn.init.normal_(t, mean=0.0, std=0.02)

    def _sync_flat_weights(self):
        """One flat fp32 buffer + bf16 operand copy over ALL parameters, the encoder's included (ModelCross._sync_flat_weights; the inner
        encoder's forward is never called, so it builds none of its own)."""
        grp = getattr(self, "_flat", None)
        if grp is None or not grp.intact() or grp.params[0].device != self.mask_token.device:
            if grp is not None:
                XF.SHADOWS.detach(grp)
            grp = XF.FlatWeights(list(self.parameters()))
            object.__setattr__(self, "_flat", grp)
            XF.SHADOWS.attach(grp)
        grp.refresh(force=XF.SHADOWS.force)
        XF.SHADOWS.force = False

    def _decode(self, img, capture=None):
        """Steps 1-10 of the forward -> (pred bf16 [S*Rm, pd], drop_idx [S, Rm], mslot [S, P])."""
        enc = self.encoder
        B, M = img.shape[0], enc.num_modalities
        K, dd = self.num_kept, self.mask_token.shape[-1]
        keep = enc._draw_token_keep(img, rate=self.mask_ratio, shared=self.mask_shared)
        keep_idx, slot = keep
        toks = enc.forward_tokens(img, keep)                                           # M tensors [B, K + 1, d]
        normed = [XF.LayerNormFn.apply(toks[m], enc.norm[m].weight, enc.norm[m].bias, enc.norm[m].eps) for m in range(M)]
        xe = XF.LinearFn.apply(torch.cat(normed, dim=0), self.decoder_embed.weight, self.decoder_embed.bias, True)     # fp32 [S, K + 1, dd]
        drop = XF.ops.token_select_complement(slot, K)
        self.last_token_keep = keep_idx.view(M, B, K)
        self.last_token_drop = drop[0].view(M, B, -1)
        y = XF.MaeUnshuffleFn.apply(xe, self.mask_token, self.decoder_pos_embed, self.decoder_modality_embed, keep)    # fp32 [S, P + 1, dd]
        if capture is not None:
            capture["unshuffled"] = y.detach()
        y = self.decoder_blocks(y)
        if capture is not None:
            capture["decoded"] = y.detach()
        rows = XF.TokenRowsGatherFn.apply(y, drop)                                      # fp32 [S * Rm, dd]: only the dropped rows go on
        rows = XF.LayerNormFn.apply(rows, self.decoder_norm.weight, self.decoder_norm.bias, self.decoder_norm.eps)
        pred = XF.LinearFn.apply(rows, self.decoder_pred.weight, self.decoder_pred.bias, False)                         # bf16 [S * Rm, pd]
        if capture is not None:
            capture["pred"] = pred.detach()
        return pred, drop

    def _prepare(self, img):
        if self.mask_token.is_cuda and os.environ.get("XVIT_FLAT_WEIGHTS", "1") != "0":
            self._sync_flat_weights()
        if img.dim() != 6 or img.shape[1] != self.encoder.num_modalities:
            raise ValueError(f"expected a volume tensor [B, {self.encoder.num_modalities}, 1, D, H, W], got {tuple(img.shape)}")
        if img.requires_grad:
            raise RuntimeError("MaskedVolumeModel: the volume is the target and is embedded through the keep path (patch dropout), which has no "
                               "input-volume gradient: pass a volume that does not require grad")
        if img.is_cuda and torch.is_grad_enabled():
            XF.arena_begin(img.device)
        return img if img.is_contiguous() else img.contiguous()

    def forward(self, img, labels=None, capture=None):
        """labels is accepted and ignored (training loops and GraphedStep keep their call shape).  A mask is drawn in train() and eval()
        alike: masking is the task.  capture (a dict, optional) receives the intermediate tensors the parity tests probe."""
        img = self._prepare(img)
        pred, drop = self._decode(img, capture)
        loss, loss_seq, stats = XF.MaskedPatchLossFn.apply(pred, img, drop[0], self.encoder.patch_size, self.norm_pix_loss)
        if capture is not None:
            capture["stats"] = stats
        return loss_seq.view(self.encoder.num_modalities, img.shape[0]), loss

    @torch.no_grad()
    def reconstruct(self, img, capture=None):
        """One mask, one forward -> (recon fp32 [B, M, 1, D, H, W], mask bool [M, B, P]): the input with its dropped patches (mask True)
        replaced by the prediction, de-normalised with the patch's own mean and standard deviation under norm_pix_loss.  capture: as in
        forward."""
        img = self._prepare(img)
        pred, (drop_idx, mslot) = self._decode(img, capture)
        _, _, stats = XF.MaskedPatchLossFn.apply(pred, img, drop_idx, self.encoder.patch_size, self.norm_pix_loss)
        if capture is not None:
            capture["stats"] = stats
        B, M = img.shape[0], self.encoder.num_modalities
        S, P = mslot.shape
        pd = pred.shape[1]
        vals = pred.float() * (1.0 / stats[:, 1:2]) + stats[:, 0:1]                    # pred * std + mean
        rows = (torch.arange(S, device=img.device)[:, None] * P + drop_idx.long()).reshape(-1)
        full = torch.zeros(S * P, pd, dtype=torch.float32, device=img.device)
        full[rows] = vals
        flag = torch.zeros(S * P, pd, dtype=torch.float32, device=img.device)
        flag[rows] = 1.0
        recon = XF.ops.unpatchify(full, torch.empty(img.shape, dtype=torch.float32, device=img.device), self.encoder.patch_size)
        where = XF.ops.unpatchify(flag, torch.empty(img.shape, dtype=torch.float32, device=img.device), self.encoder.patch_size)
        return torch.where(where > 0, recon, img.float()), (mslot >= 0).view(M, B, P)
