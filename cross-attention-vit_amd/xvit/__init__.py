"""xvit — MI355X-native hot path of the cross-attention 3-D ViT, behind the reference's
own nn.Module signatures (vsahni3/cross-attention-ViT: model_cross.py, model.py).

    from xvit.model_cross import ModelCross          # drop-in for reference model_cross.ModelCross
    from xvit.modelv3 import ModelVIT                # drop-in for reference modelv3.ModelVIT (concatenated-token baseline)
    from xvit.model import Encoder                   # drop-in for reference model.Encoder
    xvit.interpret.attention_maps(model, img)        # CLS attention maps and attention rollout (eval mode)
    xvit.interpret.relevance_maps(model, img)        # class-specific relevance (one backward, eval mode)
    xvit.interpret.input_attributions(model, img)    # voxel attributions: gradient, grad x input, integrated gradients (eval mode)
    xvit.augment.VolumeAugment(img_size)(raw)        # device-side pad / crop + random affine + intensity augmentation of raw volumes
    xvit.augment.ContrastAugment()(img)              # random Gaussian blur, bias field and gamma on the augmented volumes, one fused kernel
    xvit.MaskedVolumeModel(config)                   # masked-volume (MAE) pretraining of a ModelCross encoder
    config.mixup_alpha / config.cutmix_alpha         # Mixup / CutMix with a soft-target loss in ModelCross.train() (fine-tuning)
    config.patch_select = "foreground"               # patch dropout ranked by per-patch foreground; eval_patch_dropout shortens eval() too
    xvit.token_occupancy(img, patch_size)            # the per-patch foreground counts that ranking reads
    xvit.data.VolumeStore / xvit.data.BatchSampler   # raw volumes resident on the device; batches drawn and gathered there, capturable
"""
from . import _lib  # noqa: F401
from .functional import invalidate_shadows, token_occupancy  # noqa: F401   (token_occupancy: per-patch foreground counts, stand-alone)
from .model import Block, Encoder, Mlp, MultiHeadAttention  # noqa: F401
from .modelv3 import ModelVIT, Transformer  # noqa: F401
from .model_cross import (Attention, CrossAttention, CrossAttentionBlock, FeedForward, ModelCross,  # noqa: F401
                          MultiScaleBlock, PreNorm, SelfAttentionBlock)
from .metrics import BinaryEpochMetrics, EpochMetrics  # noqa: F401
from . import interpret  # noqa: F401   (attention maps and rollout: xvit.interpret.attention_maps)
from . import augment  # noqa: F401     (the augmenting input stage: xvit.augment.VolumeAugment)
from .augment import AugmentParams, ContrastAugment, ContrastParams, ForegroundBoxes, ForegroundComponents, VolumeAugment  # noqa: F401
from . import data  # noqa: F401        (the device-resident volume store: xvit.data.VolumeStore, xvit.data.BatchSampler)
from .mae import MaskedVolumeModel  # noqa: F401   (masked-volume pretraining around a ModelCross encoder)
