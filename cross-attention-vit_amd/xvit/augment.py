"""Device-side augmentation of MRI volumes ahead of the patch embedding (include/xvit.h, "Augmenting input stage").

    aug = xvit.augment.VolumeAugment((128, 128, 128), intensity_scale=1 / 1000, seed=0)
    img = aug(raw)                   # raw [B, M, Ds, Hs, Ws] int16 / bf16 / fp32 on the GPU -> [B, M, 1, D, H, W]
    aug.last_params                  # AugmentParams: the table this call drew
    img = aug.apply(raw, params)     # an explicit table: replaying a recorded augmentation, test-time augmentation

It stands where the reference's loader runs MONAI's random transforms on CPU workers (dataset_ucsf.py:94-113).  The transform set and its
ranges are this project's own; parity with MONAI's random stream is not claimed.  All modalities of a sample share one spatial transform
(they are co-registered scans); intensity transforms are drawn per volume.  pad_value is in SOURCE units: it passes through the intensity
affine like every voxel.
"""
from __future__ import annotations

import torch

from . import _lib, ops

NPARAM = _lib.AUG_NPARAM
# slots of a record: enum XVIT_AUG_* of include/xvit.h, by name
MATRIX, SCALE, SHIFT, SIGMA, NOISE_SEED, FLAGS, FLIPS, ANGLES, ZOOMS, TRANSLATION = 0, 12, 13, 14, 15, 16, 17, 20, 23, 26
FLAG_EXACT = 1
_COUNTER_STRIDE = 0xD1B54A32D192ED03   # seed' = seed + call index * this (mod 2^64), on the host here and in the draw kernel alike
_MASK64 = (1 << 64) - 1


def pad_crop_offset(size: int, target: int) -> int:
    """Source index = destination index + offset: the centre pad / crop of xvit_resize_pad_crop_i16 along one axis."""
    return size // 2 - target // 2 if size >= target else -((target - size) // 2)


class AugmentParams:
    """Named views of a parameter table [B, M, 32] (fp32).  Every attribute but `exact` and `noise_seed` is a view: writing through it edits the table."""

    def __init__(self, table: torch.Tensor):
        if table.dtype != torch.float32 or table.dim() != 3 or table.shape[2] != NPARAM:
            raise ValueError(f"AugmentParams: need an fp32 [B, M, {NPARAM}] table, got {table.dtype} {tuple(table.shape)}")
        self.table = table

    @classmethod
    def identity(cls, B, M, vol_shape, img_size, device=None):
        """Pure pad / crop records: A = I, t = the pad / crop offset, a = 1, b = 0, no noise, exact."""
        t = torch.zeros(B, M, NPARAM, dtype=torch.float32)
        for i in range(3):
            t[..., MATRIX + 5 * i] = 1.0
            t[..., MATRIX + 4 * i + 3] = float(pad_crop_offset(vol_shape[i], img_size[i]))
        t[..., SCALE] = 1.0
        t[..., FLAGS] = float(FLAG_EXACT)
        t[..., ZOOMS:ZOOMS + 3] = 1.0
        return cls(t.to(device) if device is not None else t)

    matrix = property(lambda s: s.table[..., MATRIX:MATRIX + 12].unflatten(-1, (3, 4)))
    scale = property(lambda s: s.table[..., SCALE])
    shift = property(lambda s: s.table[..., SHIFT])
    sigma = property(lambda s: s.table[..., SIGMA])
    flags = property(lambda s: s.table[..., FLAGS])
    flips = property(lambda s: s.table[..., FLIPS:FLIPS + 3])
    angles = property(lambda s: s.table[..., ANGLES:ANGLES + 3])
    zooms = property(lambda s: s.table[..., ZOOMS:ZOOMS + 3])
    translation = property(lambda s: s.table[..., TRANSLATION:TRANSLATION + 3])

    @property
    def noise_seed(self):
        return self.table.view(torch.int32)[..., NOISE_SEED].to(torch.int64) & 0xFFFFFFFF

    @property
    def exact(self):
        return (self.table[..., FLAGS].to(torch.int32) & FLAG_EXACT).bool()

    def clone(self):
        return AugmentParams(self.table.clone())


def _prob(name, p):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"VolumeAugment: {name}={p} is not a probability")
    return p


def _ordered(name, r):
    lo, hi = (float(v) for v in r)
    if not lo <= hi:
        raise ValueError(f"VolumeAugment: {name}=({lo}, {hi}) is reversed")
    return lo, hi


def _half_widths(name, r):
    r = tuple(float(v) for v in r)
    if len(r) != 3 or not all(v >= 0.0 for v in r):
        raise ValueError(f"VolumeAugment: {name}={r} needs three half-widths >= 0")
    return r


class VolumeAugment(torch.nn.Module):
    """Pad / crop to img_size, one random affine resample (flips, rotation about the volume centre, per-axis zoom, translation) and one
    random intensity transform (scale, shift, Gaussian noise), in two launches: the draw into a readable table and the resample.

    Call k uses seed + k, so a run is reproducible from `seed`; eval() switches every probability off (pad / crop and the fixed intensity
    affine only) and does not advance k.  capturable=True keeps k in a device counter so that the call can sit inside torch.cuda.graph and
    draw anew at every replay; call the stage once before capturing (it allocates its table and counter then)."""

    def __init__(self, img_size, pad_value=-1.0, flip_prob=(.5, .5, .5), rotate_prob=.5, rotate_range=(.26, .26, .26), zoom_prob=.5,
                 zoom_range=(.9, 1.1), translate_prob=.5, translate_range=(8, 8, 8), scale_intensity_prob=.5, scale_intensity_range=(.9, 1.1),
                 shift_intensity_prob=.5, shift_intensity_range=(-.1, .1), noise_prob=.2, noise_std=.05, intensity_scale=1.0, intensity_shift=0.0,
                 out_dtype=torch.bfloat16, seed=0, capturable=False):
        super().__init__()
        self.img_size = tuple(int(v) for v in img_size)
        if len(self.img_size) != 3 or min(self.img_size) <= 0:
            raise ValueError(f"VolumeAugment: img_size={img_size} needs three positive sizes")
        if out_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"VolumeAugment: out_dtype={out_dtype} must be torch.bfloat16 or torch.float32")
        flip_prob = tuple(flip_prob)
        if len(flip_prob) != 3:
            raise ValueError("VolumeAugment: flip_prob needs one probability per axis")
        c = _lib.AugmentConfig()
        c.flip_prob[:] = [_prob("flip_prob", p) for p in flip_prob]
        c.rotate_prob, c.rotate_range[:] = _prob("rotate_prob", rotate_prob), _half_widths("rotate_range", rotate_range)
        c.zoom_prob, c.zoom_range[:] = _prob("zoom_prob", zoom_prob), _ordered("zoom_range", zoom_range)
        if not c.zoom_range[0] > 0:
            raise ValueError(f"VolumeAugment: zoom_range={tuple(zoom_range)} must be positive")
        c.translate_prob, c.translate_range[:] = _prob("translate_prob", translate_prob), _half_widths("translate_range", translate_range)
        c.scale_prob, c.scale_range[:] = _prob("scale_intensity_prob", scale_intensity_prob), _ordered("scale_intensity_range", scale_intensity_range)
        c.shift_prob, c.shift_range[:] = _prob("shift_intensity_prob", shift_intensity_prob), _ordered("shift_intensity_range", shift_intensity_range)
        c.noise_prob, c.noise_std = _prob("noise_prob", noise_prob), float(noise_std)
        if not c.noise_std >= 0:
            raise ValueError(f"VolumeAugment: noise_std={noise_std} must be >= 0")
        c.intensity_scale, c.intensity_shift = float(intensity_scale), float(intensity_shift)
        self.config = c
        e = _lib.AugmentConfig.from_buffer_copy(c)     # eval(): the same ranges, every probability 0
        e.flip_prob[:] = [0.0, 0.0, 0.0]
        e.rotate_prob = e.zoom_prob = e.translate_prob = e.scale_prob = e.shift_prob = e.noise_prob = 0.0
        self._eval_config = e
        self.pad_value, self.out_dtype, self.seed, self.capturable = float(pad_value), out_dtype, int(seed), bool(capturable)
        self.calls = 0             # host call index (capturable: see call_index)
        self._counter = None       # capturable: the device call index
        self._tables = {}          # capturable: one static table per (B, M, device)
        self.last_params = None

    @property
    def call_index(self) -> int:
        """Training calls made so far (capturable: read from the device counter, a host synchronisation)."""
        return int(self._counter.item()) if self._counter is not None else self.calls

    @staticmethod
    def _volumes(raw):
        if not isinstance(raw, torch.Tensor) or not raw.is_cuda:
            raise RuntimeError("VolumeAugment: the volumes must be a GPU tensor; this stage has no CPU path")
        if raw.dim() == 6 and raw.shape[2] == 1:
            raw = raw[:, :, 0]
        if raw.dim() != 5:
            raise ValueError(f"VolumeAugment: need [B, M, Ds, Hs, Ws] or [B, M, 1, Ds, Hs, Ws], got {tuple(raw.shape)}")
        if raw.dtype not in (torch.int16, torch.bfloat16, torch.float32):
            raise TypeError(f"VolumeAugment: {raw.dtype} volumes are not supported (int16, bfloat16, float32)")
        if not raw.is_contiguous():
            raise ValueError("VolumeAugment: the volumes must be contiguous (the source is read once, in place)")
        return raw

    def _table(self, B, M, device):
        if not self.capturable:
            return torch.empty(B, M, NPARAM, dtype=torch.float32, device=device)
        key = (B, M, device)
        if key not in self._tables or self._counter is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("VolumeAugment(capturable=True): call the stage once on this batch shape before capturing it; "
                                   "its table and counter must not be allocated inside the graph")
            self._tables[key] = torch.empty(B, M, NPARAM, dtype=torch.float32, device=device)
            if self._counter is None:
                self._counter = torch.zeros(1, dtype=torch.int64, device=device)
        return self._tables[key]

    def draw(self, B, M, vol_shape, device) -> AugmentParams:
        """One table for B x M volumes of vol_shape; advances the call index in training mode."""
        table = self._table(B, M, device)
        config = self.config if self.training else self._eval_config
        if self.capturable:
            ops.augment_draw(config, table, vol_shape, self.img_size, self.seed, self._counter, advance=self.training)
        else:
            ops.augment_draw(config, table, vol_shape, self.img_size, (self.seed + self.calls * _COUNTER_STRIDE) & _MASK64)
            self.calls += int(self.training)
        return AugmentParams(table)

    def apply(self, raw, params, out_dtype=None):
        raw = self._volumes(raw)
        table = params.table if isinstance(params, AugmentParams) else params
        return ops.augment_apply(raw, table, self.img_size, self.pad_value, out_dtype or self.out_dtype)

    def forward(self, raw):
        raw = self._volumes(raw)
        self.last_params = self.draw(raw.shape[0], raw.shape[1], tuple(raw.shape[2:]), raw.device)
        return self.apply(raw, self.last_params)
