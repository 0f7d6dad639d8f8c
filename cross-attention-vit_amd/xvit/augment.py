"""Device-side augmentation of MRI volumes ahead of the patch embedding (include/xvit.h, "Augmenting input stage").

    aug = xvit.augment.VolumeAugment((128, 128, 128), intensity_scale=1 / 1000, seed=0)
    img = aug(raw)                   # raw [B, M, Ds, Hs, Ws] int16 / bf16 / fp32 on the GPU -> [B, M, 1, D, H, W]
    aug.last_params                  # AugmentParams: the table this call drew
    img = aug.apply(raw, params)     # an explicit table: replaying a recorded augmentation, test-time augmentation

    aug = xvit.augment.VolumeAugment((128, 128, 128), normalize="zscore")    # per-volume normalisation, also in eval()
    aug.last_stats                   # VolumeStats: n, n_w, mean, std, lo, hi, min, max of every volume's foreground
    aug = xvit.augment.VolumeAugment((128, 128, 128), elastic_prob=.2)       # random elastic deformation inside the same resample
    aug.last_elastic                 # ElasticField: the control grids and records this call drew; aug.apply(raw, params, elastic=...) replays
    xvit.augment.volume_stats(raw)   # the statistics alone
    aug = xvit.augment.VolumeAugment((128, 128, 128), crop_foreground="fit", crop_margin=4)   # window the foreground, not the volume centre
    aug.last_crop                    # ForegroundBoxes: every volume's foreground box and the crop of every sample
    xvit.augment.foreground_boxes(raw)   # the boxes alone
    aug = xvit.augment.VolumeAugment((128, 128, 128), crop_foreground="fit", crop_component="largest")   # ... of the largest component only
    aug.last_crop.components         # ForegroundComponents: every voxel's component label and the per-volume component table
    xvit.augment.foreground_components(raw)   # the labels and the table alone

    con = xvit.augment.ContrastAugment(blur_prob=.2, bias_prob=.2, gamma_prob=.3, seed=0)      # a second stage behind the first
    img = con(aug(raw))              # Gaussian blur, bias field, gamma: one fused kernel, a NEW tensor of the same shape
    con.last_params                  # ContrastParams: the table this call drew

It stands where the reference's loader runs MONAI's random transforms on CPU workers (dataset_ucsf.py:94-113).  The transform set and its
ranges are this project's own; parity with MONAI's random stream is not claimed.  All modalities of a sample share one spatial transform
(they are co-registered scans); intensity transforms are drawn per volume.  pad_value is in SOURCE units: it passes through the intensity
affine like every voxel.

normalize="zscore" | "window" puts a per-volume normalisation in front of the drawn scale / shift (include/xvit.h, "Per-volume intensity
statistics and normalisation"): exact statistics of the foreground voxels (v > foreground_above) of the WHOLE source volume, from a
histogram on the device, folded into the table between the draw and the resample.  With clip=True the resampled value is clamped to the
window [lo, hi] first, pad_value included: the background lands on the window floor.

crop_foreground="center" | "fit" moves the pad / crop window from the centre of the volume to the bounding box of the sample's foreground
(include/xvit.h, "Foreground bounding box and crop"; what MONAI's CropForegroundd followed by ResizeWithPadOrCropd or a resize does in a
loader): two launches that fold the box into the table's A | t between the draw and the statistics fold, so the voxels are still
interpolated once.  The box is the index range of v > crop_above over all modalities of the sample, so one isolated bright background
voxel widens it.  crop_component="largest" | n takes the box over the voxels of every volume's largest 6- or 26-connected foreground
component, or of its components of at least n voxels, instead (include/xvit.h, "Connected foreground components"; what MONAI's
KeepLargestConnectedComponent or RemoveSmallObjects does in front of CropForegroundd): union-find labelling on the device, seven more
launches, 4 bytes of labels per source voxel plus as much workspace.  The box moves the window and masks nothing: a dropped component
that falls inside the window stays in the image.
"""
from __future__ import annotations

import torch

from . import _lib, ops

NPARAM = _lib.AUG_NPARAM
# slots of a record: enum XVIT_AUG_* of include/xvit.h, by name
MATRIX, SCALE, SHIFT, SIGMA, NOISE_SEED, FLAGS, FLIPS, ANGLES, ZOOMS, TRANSLATION = 0, 12, 13, 14, 15, 16, 17, 20, 23, 26
CLAMP_LO, CLAMP_HI = 29, 30
CROP_SCALE = _lib.AUG_CROP_SCALE
FLAG_EXACT, FLAG_CLAMP = 1, 2
NSTAT = _lib.STATS_NSTAT
ELASTIC_MAX_GRID, ELASTIC_NREC = _lib.ELASTIC_MAX_GRID, _lib.ELASTIC_NREC
ELASTIC_FLAG, ELASTIC_U, ELASTIC_MAX_ABS = 0, 1, 2     # slots of an elastic record: enum XVIT_ELASTIC_* of include/xvit.h
_NORM_MODES = {None: _lib.NORM_STATS_ONLY, "zscore": _lib.NORM_ZSCORE, "window": _lib.NORM_WINDOW}
BBOX_NREC = _lib.BBOX_NREC
CC_NREC = _lib.CC_NREC
_CROP_MODES = {None: _lib.CROP_BOXES_ONLY, "center": _lib.CROP_CENTER, "fit": _lib.CROP_FIT}
_COUNTER_STRIDE = 0xD1B54A32D192ED03   # seed' = seed + call index * this (mod 2^64): kSeedStride of csrc/xvit_common.h, on the host
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
    clamp_lo = property(lambda s: s.table[..., CLAMP_LO])
    clamp_hi = property(lambda s: s.table[..., CLAMP_HI])
    crop_scale = property(lambda s: s.table[..., CROP_SCALE])     # the k xvit_volume_bbox folded; 0: no crop folded

    @property
    def noise_seed(self):
        return self.table.view(torch.int32)[..., NOISE_SEED].to(torch.int64) & 0xFFFFFFFF

    @property
    def exact(self):
        return (self.table[..., FLAGS].to(torch.int32) & FLAG_EXACT).bool()

    @property
    def clamped(self):
        return (self.table[..., FLAGS].to(torch.int32) & FLAG_CLAMP).bool()

    def clone(self):
        return AugmentParams(self.table.clone())


class ElasticField:
    """A B-spline control grid per sample (include/xvit.h, "Elastic deformation"): field [B, 3, Gz, Gy, Gx] (fp32; components z, y, x in
    destination voxels) and record [B, 8] (fp32).  `active` and `max_abs` are views of the record."""

    def __init__(self, field: torch.Tensor, record: torch.Tensor):
        G = ELASTIC_MAX_GRID
        if field.dtype != torch.float32 or field.dim() != 5 or field.shape[1] != 3 or not all(4 <= n <= G for n in field.shape[2:]):
            raise ValueError(f"ElasticField: need an fp32 [B, 3, Gz, Gy, Gx] field with 4 <= G <= {G}, got {field.dtype} {tuple(field.shape)}")
        if record.dtype != torch.float32 or tuple(record.shape) != (field.shape[0], ELASTIC_NREC):
            raise ValueError(f"ElasticField: need an fp32 [{field.shape[0]}, {ELASTIC_NREC}] record, got {record.dtype} {tuple(record.shape)}")
        self.field, self.record = field, record

    @classmethod
    def zeros(cls, B, grid, device=None):
        """No sample deformed: zero fields, flags 0.  grid: an int or (Gz, Gy, Gx)."""
        grid = (int(grid),) * 3 if isinstance(grid, int) else tuple(int(v) for v in grid)
        return cls(torch.zeros((B, 3) + grid, dtype=torch.float32, device=device), torch.zeros(B, ELASTIC_NREC, dtype=torch.float32, device=device))

    grid = property(lambda s: tuple(s.field.shape[2:]))
    active = property(lambda s: s.record[:, ELASTIC_FLAG])                               # 1 = the sample is deformed
    draw = property(lambda s: s.record[:, ELASTIC_U])                                    # the uniform behind the decision
    max_abs = property(lambda s: s.record[:, ELASTIC_MAX_ABS:ELASTIC_MAX_ABS + 3])       # max |phi| per component (z, y, x) as drawn

    def clone(self):
        return ElasticField(self.field.clone(), self.record.clone())


class VolumeStats:
    """Named views of a statistics table [B, M, 8] (fp64) of xvit_volume_stats.  The table stays on the device: reading a value is the one
    host synchronisation, paid only by who reads."""

    def __init__(self, table: torch.Tensor):
        if table.dtype != torch.float64 or table.dim() != 3 or table.shape[2] != NSTAT:
            raise ValueError(f"VolumeStats: need an fp64 [B, M, {NSTAT}] table, got {table.dtype} {tuple(table.shape)}")
        self.table = table

    n = property(lambda s: s.table[..., 0])        # foreground voxels
    n_w = property(lambda s: s.table[..., 1])      # ... of them inside [lo, hi]
    mean = property(lambda s: s.table[..., 2])     # over the window
    std = property(lambda s: s.table[..., 3])      # population standard deviation over the window
    lo = property(lambda s: s.table[..., 4])
    hi = property(lambda s: s.table[..., 5])
    min = property(lambda s: s.table[..., 6])      # of the foreground
    max = property(lambda s: s.table[..., 7])

    def clone(self):
        return VolumeStats(self.table.clone())


def norm_config(normalize=None, foreground_above=0.0, percentiles=None, clip=False):
    """_lib.NormConfig from the Python arguments, validated as xvit_volume_stats validates it."""
    if normalize not in _NORM_MODES:
        raise ValueError(f"normalize={normalize!r} must be None, 'zscore' or 'window'")
    fg = float(foreground_above)
    if fg != fg:
        raise ValueError("foreground_above is NaN")
    c = _lib.NormConfig()
    c.mode, c.clip, c.foreground_above = _NORM_MODES[normalize], int(bool(clip)), fg
    if percentiles is None:
        c.q_lo, c.q_hi = -1.0, -1.0
    else:
        q = tuple(float(v) for v in percentiles)
        if len(q) != 2 or not 0.0 <= q[0] <= q[1] <= 1.0:
            raise ValueError(f"percentiles={tuple(percentiles)} need 0 <= q_lo <= q_hi <= 1")
        c.q_lo, c.q_hi = q
    return c


def _stat_volumes(raw, who):
    if not isinstance(raw, torch.Tensor) or not raw.is_cuda:
        raise RuntimeError(f"{who}: the volumes must be a GPU tensor; this stage has no CPU path")
    if raw.dim() < 3:
        raise ValueError(f"{who}: need [B, M, ...] volumes, got {tuple(raw.shape)}")
    if not raw.is_contiguous():
        raise ValueError(f"{who}: the volumes must be contiguous (the source is read once, in place)")
    return raw


def volume_stats(raw, foreground_above=0.0, percentiles=None) -> VolumeStats:
    """Exact per-volume statistics of raw [B, M, ...] (int16 or bf16 on the GPU) over its foreground v > foreground_above: two launches,
    no host synchronisation until the result is read.  percentiles=(q_lo, q_hi): lo / hi by nearest rank and mean / std over [lo, hi]."""
    raw = _stat_volumes(raw, "volume_stats")
    config = norm_config(None, foreground_above, percentiles)
    B, M = raw.shape[:2]
    stats = torch.empty(B, M, NSTAT, dtype=torch.float64, device=raw.device)
    ops.volume_stats(raw, config, stats, ops.volume_stats_workspace(B * M, raw.device))
    return VolumeStats(stats)


class ForegroundBoxes:
    """Named views of the tables of xvit_volume_bbox: boxes [B, M, 8] (int32; the inclusive index range of every volume's foreground along
    z, y, x, its voxel count, zero) and crop [B, 8] (int32; the union over the sample's modalities, widened by the margin and clipped, a
    has-foreground flag, zero).  The tables stay on the device: reading a value is the one host synchronisation."""

    def __init__(self, boxes: torch.Tensor, crop: torch.Tensor, components=None):
        if boxes.dtype != torch.int32 or boxes.dim() != 3 or boxes.shape[2] != BBOX_NREC:
            raise ValueError(f"ForegroundBoxes: need int32 [B, M, {BBOX_NREC}] boxes, got {boxes.dtype} {tuple(boxes.shape)}")
        if crop.dtype != torch.int32 or tuple(crop.shape) != (boxes.shape[0], BBOX_NREC):
            raise ValueError(f"ForegroundBoxes: need an int32 [{boxes.shape[0]}, {BBOX_NREC}] crop, got {crop.dtype} {tuple(crop.shape)}")
        self.boxes, self.crop = boxes, crop
        self.components = components     # ForegroundComponents when the boxes were taken over kept components, else None

    lo = property(lambda s: s.crop[:, 0:6:2])              # [B, 3]: the first index of the sample's crop along z, y, x
    hi = property(lambda s: s.crop[:, 1:6:2])              # ... and the last, inclusive
    nonempty = property(lambda s: s.crop[:, _lib.BBOX_COUNT])    # 1 = the sample has foreground
    count = property(lambda s: s.boxes[..., _lib.BBOX_COUNT])    # [B, M]: foreground voxels of every volume
    volume_lo = property(lambda s: s.boxes[..., 0:6:2])    # [B, M, 3]: every volume's own box (an empty one: lo = size, hi = -1)
    volume_hi = property(lambda s: s.boxes[..., 1:6:2])

    def clone(self):
        return ForegroundBoxes(self.boxes.clone(), self.crop.clone(), None if self.components is None else self.components.clone())


class ForegroundComponents:
    """Named views of the outputs of xvit_volume_components: labels [B, M, Ds, Hs, Ws] (int32; the smallest flat index (z Hs + y) Ws + x of
    a foreground voxel's connected component, -1 for background) and table [B, M, 8] (int32; the number of components, the largest one's
    root and size, the numbers of kept components and kept voxels, the status, two zeros).  They stay on the device."""

    def __init__(self, labels: torch.Tensor, table: torch.Tensor):
        if labels.dtype != torch.int32 or labels.dim() != 5:
            raise ValueError(f"ForegroundComponents: need int32 [B, M, Ds, Hs, Ws] labels, got {labels.dtype} {tuple(labels.shape)}")
        if table.dtype != torch.int32 or tuple(table.shape) != (*labels.shape[:2], CC_NREC):
            raise ValueError(f"ForegroundComponents: need an int32 [{labels.shape[0]}, {labels.shape[1]}, {CC_NREC}] table, got {table.dtype} {tuple(table.shape)}")
        self.labels, self.table = labels, table

    count = property(lambda s: s.table[..., _lib.CC_COUNT])                 # [B, M]: components of every volume
    largest_root = property(lambda s: s.table[..., _lib.CC_LARGEST_ROOT])   # the label of the largest (-1: no foreground)
    largest_size = property(lambda s: s.table[..., _lib.CC_LARGEST_SIZE])   # ... and its voxels
    kept = property(lambda s: s.table[..., _lib.CC_KEPT])                   # components the box was taken over
    kept_voxels = property(lambda s: s.table[..., _lib.CC_KEPT_VOXELS])     # ... and their voxels
    status = property(lambda s: s.table[..., _lib.CC_STATUS])               # 0 = fine

    def clone(self):
        return ForegroundComponents(self.labels.clone(), self.table.clone())


def component_config(component="largest", connectivity=6, above=0.0):
    """_lib.ComponentConfig from the Python arguments ("largest", or an int n >= 1: components of at least n voxels), validated as
    xvit_volume_components validates it."""
    if isinstance(component, bool) or not (component == "largest" or (isinstance(component, int) and 1 <= component < 2 ** 31)):
        raise ValueError(f"crop_component={component!r} must be None, 'largest' or an int >= 1 (components of at least that many voxels)")
    if isinstance(connectivity, bool) or connectivity not in (6, 26):
        raise ValueError(f"crop_connectivity={connectivity!r} must be 6 (faces) or 26 (faces, edges, corners)")
    fg = float(above)
    if fg != fg:
        raise ValueError("the foreground threshold is NaN")
    c = _lib.ComponentConfig()
    c.connectivity, c.foreground_above = connectivity, fg
    c.keep, c.min_voxels = (_lib.CC_LARGEST, 1) if component == "largest" else (_lib.CC_MIN_VOXELS, component)
    return c


def _component_tables(raw):
    """labels, the component table and the workspace for the volumes raw: 4 bytes per voxel, and a little more than that again."""
    B, M = raw.shape[:2]
    return (torch.empty(raw.shape, dtype=torch.int32, device=raw.device), torch.empty(B, M, CC_NREC, dtype=torch.int32, device=raw.device),
            ops.volume_components_workspace(B * M, raw[0, 0].numel(), raw.device))


def foreground_components(raw, foreground_above=0.0, connectivity=6) -> ForegroundComponents:
    """The connected components of the foreground v > foreground_above of raw [B, M, Ds, Hs, Ws] (int16, bf16 or fp32 on the GPU): every
    voxel's label and the per-volume table (the kept set is the largest component), without a host synchronisation until they are read."""
    raw = VolumeAugment._volumes(raw)
    labels, table, workspace = _component_tables(raw)
    ops.volume_components(raw, component_config("largest", connectivity, foreground_above), labels, table, workspace)
    return ForegroundComponents(labels, table)


def crop_config(mode=None, margin=0, upscale=False, above=0.0):
    """_lib.CropConfig from the Python arguments, validated as xvit_volume_bbox validates it."""
    if mode not in _CROP_MODES:
        raise ValueError(f"crop_foreground={mode!r} must be None, 'center' or 'fit'")
    margin = (margin,) * 3 if isinstance(margin, int) and not isinstance(margin, bool) else margin
    if not isinstance(margin, (tuple, list)) or len(margin) != 3 or not all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v < 2 ** 31 for v in margin):
        raise ValueError(f"crop_margin={margin!r} needs one or three ints >= 0 (voxels, z, y, x)")
    fg = float(above)
    if fg != fg:
        raise ValueError("crop_above is NaN")
    c = _lib.CropConfig()
    c.mode, c.margin[:], c.allow_upscale, c.foreground_above = _CROP_MODES[mode], list(margin), int(bool(upscale)), fg
    return c


def _crop_tables(B, M, device, workspace=True):
    """boxes, crop and a workspace that serves B x M volumes of any size (the chunk rule never gives a volume more parts than an
    unbounded one gets); workspace=False: None in its place, for the component path, which brings its own."""
    return (torch.empty(B, M, BBOX_NREC, dtype=torch.int32, device=device), torch.empty(B, BBOX_NREC, dtype=torch.int32, device=device),
            ops.volume_bbox_workspace(B * M, 2 ** 31 - 1, device) if workspace else None)


def foreground_boxes(raw, foreground_above=0.0, margin=0, component=None, connectivity=6) -> ForegroundBoxes:
    """The foreground boxes of raw [B, M, Ds, Hs, Ws] (int16, bf16 or fp32 on the GPU) over v > foreground_above, and per sample their
    union widened by margin: two launches, no host synchronisation until the result is read.  component="largest" | n takes them over the
    voxels of every volume's largest connected component, or of its components of at least n voxels (connectivity 6 or 26); the result's
    .components then holds the labels and the component table."""
    raw = VolumeAugment._volumes(raw)
    config = crop_config(None, margin, False, foreground_above)
    if component is not None:
        comp = component_config(component, connectivity, foreground_above)
        boxes, crop, _ = _crop_tables(raw.shape[0], raw.shape[1], raw.device, workspace=False)
        labels, table, workspace = _component_tables(raw)
        ops.volume_bbox_components(raw, config, comp, (1, 1, 1), boxes, crop, labels, table, workspace)
        return ForegroundBoxes(boxes, crop, ForegroundComponents(labels, table))
    boxes, crop, workspace = _crop_tables(raw.shape[0], raw.shape[1], raw.device)
    ops.volume_bbox(raw, config, (1, 1, 1), boxes, crop, workspace)
    return ForegroundBoxes(boxes, crop)


def _prob(who, name, p):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{who}: {name}={p} is not a probability")
    return p


def _ordered(who, name, r, finite=False):
    """(lo, hi) with lo <= hi; finite=True refuses an infinite end as well, and says so."""
    r = tuple(float(v) for v in r)
    if len(r) != 2 or not r[0] <= r[1] or (finite and not all(v - v == 0.0 for v in r)):
        raise ValueError(f"{who}: {name}={r} is reversed" + (" or not finite" if finite else ""))
    return r


def _half_widths(name, r):
    r = tuple(float(v) for v in r)
    if len(r) != 3 or not all(v >= 0.0 for v in r):
        raise ValueError(f"VolumeAugment: {name}={r} needs three half-widths >= 0")
    return r


def _check_volumes(who, raw, dims, dtypes, why=""):
    """The checks both stages make of their input: a contiguous GPU tensor [B, M, (1,) dims] of one of dtypes."""
    if not isinstance(raw, torch.Tensor) or not raw.is_cuda:
        raise RuntimeError(f"{who}: the volumes must be a GPU tensor; this stage has no CPU path")
    if not (raw.dim() == 5 or (raw.dim() == 6 and raw.shape[2] == 1)):
        raise ValueError(f"{who}: need [B, M, {dims}] or [B, M, 1, {dims}], got {tuple(raw.shape)}")
    if raw.dtype not in dtypes:
        raise TypeError(f"{who}: {raw.dtype} volumes are not supported ({', '.join(str(d).split('.')[1] for d in dtypes)})")
    if not raw.is_contiguous():
        raise ValueError(f"{who}: the volumes must be contiguous{why}")
    return raw


class _CallIndexed(torch.nn.Module):
    """What the random stages share: call k draws from seed + k * stride (mod 2^64).  k is self.calls on the host, or, capturable, a device
    counter that the draw kernel reads and advances, so that a captured call draws anew at every replay; the counter and the static tables
    such a call needs are allocated here, outside a capture only."""

    _WHO = ""                      # the stage's name in its messages

    def __init__(self, seed, capturable):
        super().__init__()
        self.seed, self.capturable = int(seed), bool(capturable)
        self.calls = 0             # host call index (capturable: see call_index)
        self._counter = None       # capturable: the device call index
        self._tables = {}          # capturable: one static table per (B, M, device)

    @property
    def call_index(self) -> int:
        """Training calls made so far (capturable: read from the device counter, a host synchronisation)."""
        return int(self._counter.item()) if self._counter is not None else self.calls

    def _static_table(self, B, M, nparam, device, more=None):
        """A table for one call: a new one, or, capturable, the static one of (B, M, device); more(key) allocates what else the stage
        keeps per key, together with it."""
        if not self.capturable:
            return torch.empty(B, M, nparam, dtype=torch.float32, device=device)
        key = (B, M, device)
        if key not in self._tables or self._counter is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._WHO}(capturable=True): call the stage once on this batch shape before capturing it; "
                                   "its table and counter must not be allocated inside the graph")
            self._tables[key] = torch.empty(B, M, nparam, dtype=torch.float32, device=device)
            if self._counter is None:
                self._counter = torch.zeros(1, dtype=torch.int64, device=device)
            if more is not None:
                more(key)
        return self._tables[key]

    def _draw(self, launch, advance):
        """launch(seed, counter, advance) on this call's index, which `advance` then moves on."""
        if self.capturable:
            launch(self.seed, self._counter, advance)
        else:
            launch((self.seed + self.calls * _COUNTER_STRIDE) & _MASK64, None, False)
            self.calls += int(advance)


class VolumeAugment(_CallIndexed):
    """Pad / crop to img_size, one random affine resample (flips, rotation about the volume centre, per-axis zoom, translation) and one
    random intensity transform (scale, shift, Gaussian noise), in two launches: the draw into a readable table and the resample.
    normalize="zscore" | "window" adds two launches between them (xvit.augment.volume_stats, folded into the table): the drawn scale /
    shift then act on (v - mean) / std, or on (v - lo) / (hi - lo), of the volume's foreground v > foreground_above, lo / hi being the
    `percentiles` by nearest rank (None: min / max) and mean / std taken inside [lo, hi]; clip clamps to [lo, hi] first.  It is not
    random and runs in eval() as in train(); intensity_scale / intensity_shift then apply to the normalised values.

    Call k uses seed + k, so a run is reproducible from `seed`; eval() switches every probability off (pad / crop and the fixed intensity
    affine only) and does not advance k.  capturable=True keeps k in a device counter so that the call can sit inside torch.cuda.graph and
    draw anew at every replay; call the stage once before capturing (it allocates its table, counter and statistics buffers then).

    elastic_prob > 0 adds random elastic deformation (include/xvit.h, "Elastic deformation"): per sample, with that probability, a cubic
    B-spline displacement on elastic_control_points control points per axis (an int or three), each free control point uniform in
    +-elastic_max_displacement destination voxels (a float or three, z, y, x), the outer elastic_locked_borders control layers held at
    zero.  It is composed into the one resample (p = A (q + u(q)) + t), costs one launch more (the field's draw, in front of the table's,
    on the same call index) and is off in eval(); last_elastic holds the ElasticField of the last call (None when nothing was drawn).  A
    displacement above half a control cell is refused unless elastic_allow_folding is set.

    crop_foreground="center" | "fit" adds two launches behind the draw (xvit.augment.foreground_boxes, folded into the table): the pad /
    crop window moves from the centre of the volume to the box of the sample's foreground v > crop_above (None: foreground_above), taken
    over all its modalities and widened by crop_margin voxels (an int or three) inside the volume.  "center" keeps the voxel size (the
    exact copy stays exact); "fit" also zooms out by k = max over the axes of box size / img_size so that the whole box is seen, and
    zooms in (k < 1) only with crop_upscale.  Like normalize it is preprocessing: not random, and it runs in eval() as in train().
    last_crop holds the ForegroundBoxes of the last call and last_params.crop_scale the k that was folded.

    crop_component="largest" | n (an int >= 1) takes every volume's box over its largest connected foreground component, or over its
    components of at least n voxels (the largest when none has n), with crop_connectivity 6 (faces) or 26 (faces, edges, corners): a
    speck of noise or a marker far from the head no longer widens the window (xvit.augment.foreground_components; include/xvit.h,
    "Connected foreground components").  It needs crop_foreground, runs in eval() as in train(), and changes where the window goes only:
    a dropped component inside the window stays in the image.  It costs seven more launches, 4 bytes of labels per source voxel (571 MB
    at B = 8, M = 2, 240 x 240 x 155) and a workspace of xvit_volume_components_workspace_bytes (a little more than the labels again);
    last_crop.components holds the ForegroundComponents of the last call.  With None nothing of it is launched or allocated."""

    _WHO = "VolumeAugment"

    def __init__(self, img_size, pad_value=-1.0, flip_prob=(.5, .5, .5), rotate_prob=.5, rotate_range=(.26, .26, .26), zoom_prob=.5,
                 zoom_range=(.9, 1.1), translate_prob=.5, translate_range=(8, 8, 8), scale_intensity_prob=.5, scale_intensity_range=(.9, 1.1),
                 shift_intensity_prob=.5, shift_intensity_range=(-.1, .1), noise_prob=.2, noise_std=.05, intensity_scale=1.0, intensity_shift=0.0,
                 out_dtype=torch.bfloat16, seed=0, capturable=False, normalize=None, foreground_above=0.0, percentiles=(0.005, 0.995), clip=True,
                 elastic_prob=0.0, elastic_control_points=7, elastic_max_displacement=7.5, elastic_locked_borders=2, elastic_allow_folding=False,
                 crop_foreground=None, crop_margin=0, crop_upscale=False, crop_above=None, crop_component=None, crop_connectivity=6):
        super().__init__(seed, capturable)
        who = self._WHO
        self.img_size = tuple(int(v) for v in img_size)
        if len(self.img_size) != 3 or min(self.img_size) <= 0:
            raise ValueError(f"VolumeAugment: img_size={img_size} needs three positive sizes")
        if out_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"VolumeAugment: out_dtype={out_dtype} must be torch.bfloat16 or torch.float32")
        flip_prob = tuple(flip_prob)
        if len(flip_prob) != 3:
            raise ValueError("VolumeAugment: flip_prob needs one probability per axis")
        c = _lib.AugmentConfig()
        c.flip_prob[:] = [_prob(who, "flip_prob", p) for p in flip_prob]
        c.rotate_prob, c.rotate_range[:] = _prob(who, "rotate_prob", rotate_prob), _half_widths("rotate_range", rotate_range)
        c.zoom_prob, c.zoom_range[:] = _prob(who, "zoom_prob", zoom_prob), _ordered(who, "zoom_range", zoom_range)
        if not c.zoom_range[0] > 0:
            raise ValueError(f"VolumeAugment: zoom_range={tuple(zoom_range)} must be positive")
        c.translate_prob, c.translate_range[:] = _prob(who, "translate_prob", translate_prob), _half_widths("translate_range", translate_range)
        c.scale_prob, c.scale_range[:] = _prob(who, "scale_intensity_prob", scale_intensity_prob), _ordered(who, "scale_intensity_range", scale_intensity_range)
        c.shift_prob, c.shift_range[:] = _prob(who, "shift_intensity_prob", shift_intensity_prob), _ordered(who, "shift_intensity_range", shift_intensity_range)
        c.noise_prob, c.noise_std = _prob(who, "noise_prob", noise_prob), float(noise_std)
        if not c.noise_std >= 0:
            raise ValueError(f"VolumeAugment: noise_std={noise_std} must be >= 0")
        c.intensity_scale, c.intensity_shift = float(intensity_scale), float(intensity_shift)
        self.config = c
        e = _lib.AugmentConfig.from_buffer_copy(c)     # eval(): the same ranges, every probability 0
        e.flip_prob[:] = [0.0, 0.0, 0.0]
        e.rotate_prob = e.zoom_prob = e.translate_prob = e.scale_prob = e.shift_prob = e.noise_prob = 0.0
        self._eval_config = e
        self.pad_value, self.out_dtype = float(pad_value), out_dtype
        try:
            self.norm_config = norm_config(normalize, foreground_above, percentiles, clip)
        except ValueError as e:
            raise ValueError(f"VolumeAugment: {e}") from None
        self.normalize = normalize
        self.elastic_config, self.elastic_grid = self._elastic_arguments(elastic_prob, elastic_control_points, elastic_max_displacement,
                                                                         elastic_locked_borders, elastic_allow_folding)
        self._elastic = {}         # capturable: one static ElasticField per (B, device)
        self.last_elastic = None
        self._stats = {}           # capturable: one static statistics table per (B, M, device)
        self._workspaces = {}      # normalize: the histogram workspace per (B M, device), zero between calls
        try:
            self._crop_config = crop_config(crop_foreground, crop_margin, crop_upscale, foreground_above if crop_above is None else crop_above)
        except ValueError as e:
            raise ValueError(f"VolumeAugment: {e}") from None
        self.crop_foreground = crop_foreground
        self._crops = {}           # capturable: the static box tables and workspace per (B, M, device)
        try:                       # crop_connectivity is checked in any case; it acts with crop_component only
            comp = component_config("largest" if crop_component is None else crop_component, crop_connectivity, self._crop_config.foreground_above)
        except ValueError as e:
            raise ValueError(f"VolumeAugment: {e}") from None
        if crop_component is not None and crop_foreground is None:
            raise ValueError("VolumeAugment: crop_component needs crop_foreground='center' or 'fit'")
        self._component_config = None if crop_component is None else comp
        self.crop_component, self.crop_connectivity = crop_component, crop_connectivity
        self._components = {}      # capturable: the static labels, component table and workspace per (volume shape, device)
        self.last_params = None
        self.last_stats = None
        self.last_crop = None

    def _elastic_arguments(self, prob, control_points, max_displacement, locked_borders, allow_folding):
        """_lib.ElasticConfig and the control grid (Gz, Gy, Gx) from the constructor's arguments.  With prob > 0 a displacement above half a
        control cell, 0.5 (n - 1) / (G - 3) voxels, is refused unless allow_folding: beyond it the map q + u(q) can fold."""
        c = _lib.ElasticConfig()
        c.prob = _prob(self._WHO, "elastic_prob", prob)
        grid = (control_points,) * 3 if isinstance(control_points, int) else tuple(control_points)
        if len(grid) != 3 or not all(isinstance(n, int) and 4 <= n <= ELASTIC_MAX_GRID for n in grid):
            raise ValueError(f"VolumeAugment: elastic_control_points={control_points} needs one or three ints in 4 .. {ELASTIC_MAX_GRID}")
        disp = (max_displacement,) * 3 if isinstance(max_displacement, (int, float)) else tuple(max_displacement)
        disp = tuple(float(v) for v in disp)
        if len(disp) != 3 or not all(v >= 0.0 and v - v == 0.0 for v in disp):
            raise ValueError(f"VolumeAugment: elastic_max_displacement={max_displacement} needs one or three finite displacements >= 0 (voxels)")
        if not (isinstance(locked_borders, int) and 0 <= locked_borders <= 3):
            raise ValueError(f"VolumeAugment: elastic_locked_borders={locked_borders} must be 0, 1, 2 or 3")
        if c.prob > 0.0 and not allow_folding:
            for axis, (m, n, G) in enumerate(zip(disp, self.img_size, grid)):
                half_cell = 0.5 * (n - 1) / (G - 3)
                if m > half_cell:
                    raise ValueError(f"VolumeAugment: elastic_max_displacement={m} along axis {axis} exceeds half a control cell ({half_cell:g} voxels for "
                                     f"{G} control points over {n} voxels): the deformation can fold; lower it, use fewer control points or pass "
                                     "elastic_allow_folding=True")
        c.max_displacement[:] = disp
        c.locked_borders = locked_borders
        return c, grid

    @classmethod
    def _volumes(cls, raw):
        raw = _check_volumes(cls._WHO, raw, "Ds, Hs, Ws", (torch.int16, torch.bfloat16, torch.float32), " (the source is read once, in place)")
        return raw[:, :, 0] if raw.dim() == 6 else raw

    def _table(self, B, M, device):
        def more(key):         # the statistics, their workspace, the elastic field and the box tables of the same batch shape
            if self.crop_foreground is not None:
                self._crops[key] = _crop_tables(B, M, device)
            if self.normalize is not None:
                self._stats[key] = torch.empty(B, M, NSTAT, dtype=torch.float64, device=device)
                self._workspaces[(B * M, device)] = ops.volume_stats_workspace(B * M, device)
            if self.elastic_config.prob > 0.0:
                self._elastic[(B, device)] = ElasticField.zeros(B, self.elastic_grid, device)

        return self._static_table(B, M, NPARAM, device, more)

    def _normalise(self, raw, table):
        """Statistics of raw, folded into the table just drawn (two launches) -> VolumeStats."""
        B, M = raw.shape[:2]
        if self.capturable:
            self._table(B, M, raw.device)                  # the static buffers are allocated together
            stats = self._stats[(B, M, raw.device)]
        else:
            stats = torch.empty(B, M, NSTAT, dtype=torch.float64, device=raw.device)
            if (B * M, raw.device) not in self._workspaces:
                self._workspaces[(B * M, raw.device)] = ops.volume_stats_workspace(B * M, raw.device)
        ops.volume_stats(raw, self.norm_config, stats, self._workspaces[(B * M, raw.device)], table)
        return VolumeStats(stats)

    crop_config = property(lambda self: self._crop_config, doc="_lib.CropConfig of the constructor's crop_* arguments")

    def _crop(self, raw, table):
        """The foreground boxes of raw, folded into the table just drawn (two launches) -> ForegroundBoxes."""
        B, M = raw.shape[:2]
        if self.capturable:
            self._table(B, M, raw.device)                  # the static buffers are allocated together
            boxes, crop, workspace = self._crops[(B, M, raw.device)]
        else:
            boxes, crop, workspace = _crop_tables(B, M, raw.device, workspace=self._component_config is None)
        if self._component_config is None:
            ops.volume_bbox(raw, self.crop_config, self.img_size, boxes, crop, workspace, table)
            return ForegroundBoxes(boxes, crop)
        key = (tuple(raw.shape), raw.device)
        if not self.capturable:
            labels, comps, workspace = _component_tables(raw)
        else:                                                  # static: allocated by the call in front of the capture
            if key not in self._components:
                self._components[key] = _component_tables(raw)
            labels, comps, workspace = self._components[key]
        ops.volume_bbox_components(raw, self.crop_config, self._component_config, self.img_size, boxes, crop, labels, comps, workspace, table)
        return ForegroundBoxes(boxes, crop, ForegroundComponents(labels, comps))

    component_config = property(lambda self: self._component_config, doc="_lib.ComponentConfig of crop_component / crop_connectivity, or None")

    def draw(self, B, M, vol_shape, device) -> AugmentParams:
        """One table for B x M volumes of vol_shape; advances the call index in training mode."""
        table = self._table(B, M, device)
        config = self.config if self.training else self._eval_config
        self._draw(lambda *at: ops.augment_draw(config, table, vol_shape, self.img_size, *at), advance=self.training)
        return AugmentParams(table)

    def draw_elastic(self, B, M, device) -> ElasticField:
        """One control grid per sample for the call that self.draw serves next: the same call index, which it does not advance."""
        if self.capturable:
            self._table(B, M, device)                      # the static buffers and the counter are allocated together, outside a capture
            el = self._elastic[(B, device)]
        else:
            el = ElasticField(torch.empty((B, 3) + self.elastic_grid, dtype=torch.float32, device=device),
                              torch.empty(B, ELASTIC_NREC, dtype=torch.float32, device=device))
        self._draw(lambda *at: ops.elastic_draw(self.elastic_config, el.field, el.record, *at), advance=False)
        return el

    def apply(self, raw, params, out_dtype=None, elastic=None):
        """The resample through an explicit table, and, with elastic= (an ElasticField), through its deformation as well."""
        raw = self._volumes(raw)
        table = params.table if isinstance(params, AugmentParams) else params
        if elastic is None:
            return ops.augment_apply(raw, table, self.img_size, self.pad_value, out_dtype or self.out_dtype)
        if not isinstance(elastic, ElasticField):
            raise TypeError(f"VolumeAugment: elastic= takes an ElasticField, got {type(elastic).__name__}")
        if elastic.field.shape[0] != raw.shape[0] or elastic.field.device != raw.device:
            raise ValueError(f"VolumeAugment: the elastic field is for {elastic.field.shape[0]} samples on {elastic.field.device}, the volumes are "
                             f"{raw.shape[0]} samples on {raw.device}")
        return ops.augment_apply_elastic(raw, table, elastic.field.contiguous(), elastic.record.contiguous(), self.img_size, self.pad_value,
                                         out_dtype or self.out_dtype)

    def forward(self, raw):
        raw = self._volumes(raw)
        if self.normalize is not None and raw.dtype == torch.float32:
            self._normalise(raw, None)     # the library refuses it before any launch (TypeError): nothing is drawn
        elastic = None
        if self.training and self.elastic_config.prob > 0.0:
            elastic = self.draw_elastic(raw.shape[0], raw.shape[1], raw.device)      # first, on the call index the draw below advances
        self.last_elastic = elastic
        self.last_params = self.draw(raw.shape[0], raw.shape[1], tuple(raw.shape[2:]), raw.device)
        if self.crop_foreground is not None:
            self.last_crop = self._crop(raw, self.last_params.table)      # between the draw and the statistics fold
        if self.normalize is not None:
            self.last_stats = self._normalise(raw, self.last_params.table)
        return self.apply(raw, self.last_params, elastic=elastic)


# ---------------------------------------------------------------------------------------------------------------- contrast stage
# slots of a contrast record: enum XVIT_CON_* of include/xvit.h, by name
CON_NPARAM, CON_MAX_RADIUS = _lib.CON_NPARAM, _lib.CON_MAX_RADIUS
CON_FLAGS, CON_SIGMA, CON_RADIUS, CON_GAMMA, CON_WINDOW_LO, CON_WINDOW_HI, CON_BIAS = 0, 1, 4, 7, 8, 9, 10
CON_U_BLUR, CON_U_BIAS, CON_U_GAMMA, CON_BETA = 19, 20, 21, 22
CON_FLAG_BLUR, CON_FLAG_BIAS, CON_FLAG_GAMMA = 1, 2, 4
CON_BIAS_TERMS = ("z", "y", "x", "zz", "yy", "xx", "zy", "zx", "yx")     # the order of the nine bias coefficients


class ContrastParams:
    """Named views of a contrast table [B, M, 32] (fp32): flags, sigma, radius, gamma, window, bias, raw draws.  Every attribute but the
    three booleans is a view: writing through it edits the table."""

    def __init__(self, table: torch.Tensor):
        if table.dtype != torch.float32 or table.dim() != 3 or table.shape[2] != CON_NPARAM:
            raise ValueError(f"ContrastParams: need an fp32 [B, M, {CON_NPARAM}] table, got {table.dtype} {tuple(table.shape)}")
        self.table = table

    @classmethod
    def identity(cls, B, M, device=None, window=(0.0, 1.0)):
        """Copy records: flags 0, gamma 1."""
        t = torch.zeros(B, M, CON_NPARAM, dtype=torch.float32)
        t[..., CON_GAMMA] = 1.0
        t[..., CON_WINDOW_LO], t[..., CON_WINDOW_HI] = float(window[0]), float(window[1])
        return cls(t.to(device) if device is not None else t)

    flags = property(lambda s: s.table[..., CON_FLAGS])
    sigma = property(lambda s: s.table[..., CON_SIGMA:CON_SIGMA + 3])          # z, y, x
    radius = property(lambda s: s.table[..., CON_RADIUS:CON_RADIUS + 3])
    gamma = property(lambda s: s.table[..., CON_GAMMA])
    window = property(lambda s: s.table[..., CON_WINDOW_LO:CON_WINDOW_HI + 1])
    bias = property(lambda s: s.table[..., CON_BIAS:CON_BIAS + 9])             # CON_BIAS_TERMS
    draws = property(lambda s: s.table[..., CON_U_BLUR:CON_U_GAMMA + 1])       # the uniforms behind the blur, bias, gamma decisions
    beta = property(lambda s: s.table[..., CON_BETA])

    def _flag(self, bit):
        return (self.table[..., CON_FLAGS].to(torch.int32) & bit).bool()

    blurred = property(lambda s: s._flag(CON_FLAG_BLUR))
    biased = property(lambda s: s._flag(CON_FLAG_BIAS))
    gamma_on = property(lambda s: s._flag(CON_FLAG_GAMMA))

    def clone(self):
        return ContrastParams(self.table.clone())


class ContrastAugment(_CallIndexed):
    """Random Gaussian blur (per-axis sigma in voxels), smooth multiplicative bias field (order-2 polynomial in the normalised voxel
    coordinates, exponentiated) and gamma (g = exp(beta), inside gamma_window only), drawn per (sample, modality) and applied in this fixed
    order by one fused kernel behind VolumeAugment: `con(aug(raw))`, or torch.nn.Sequential(aug, con).  Two launches: the draw into a
    readable table (last_params) and the apply, which reads the volumes once and writes a NEW tensor once.  Gamma and bias are meant for
    window-normalised volumes (VolumeAugment(normalize="window") puts the foreground on [0, 1]).  The stage has no backward.

    Call k uses seed + k; eval() returns its input tensor itself (no launch, no table, call index not advanced).  capturable=True keeps k
    in a device counter, as VolumeAugment does: call the stage once on the batch shape before capturing it."""

    _WHO = "ContrastAugment"

    def __init__(self, blur_prob=.2, blur_sigma_range=(.5, 1.5), blur_isotropic=False, bias_prob=.2, bias_coeff=.3, gamma_prob=.3,
                 log_gamma_range=(-.3, .3), gamma_window=(0.0, 1.0), out_dtype=None, seed=0, capturable=False):
        super().__init__(seed, capturable)
        who = self._WHO
        if out_dtype not in (None, torch.bfloat16, torch.float32):
            raise ValueError(f"{who}: out_dtype={out_dtype} must be None (the input's), torch.bfloat16 or torch.float32")
        c = _lib.ContrastConfig()
        c.blur_prob, c.bias_prob, c.gamma_prob = _prob(who, "blur_prob", blur_prob), _prob(who, "bias_prob", bias_prob), _prob(who, "gamma_prob", gamma_prob)
        c.blur_sigma_range[:] = _ordered(who, "blur_sigma_range", blur_sigma_range, finite=True)
        if not (c.blur_sigma_range[0] > 0.0 and c.blur_sigma_range[1] <= 2.0):
            raise ValueError(f"{who}: blur_sigma_range={tuple(blur_sigma_range)} needs 0 < lo <= hi <= 2.0 (the radius ceil(3 sigma) is capped at "
                             f"{CON_MAX_RADIUS} voxels)")
        c.blur_isotropic = int(bool(blur_isotropic))
        c.bias_coeff = float(bias_coeff)
        if not (c.bias_coeff >= 0.0 and c.bias_coeff - c.bias_coeff == 0.0):
            raise ValueError(f"{who}: bias_coeff={bias_coeff} must be finite and >= 0")
        c.log_gamma_range[:] = _ordered(who, "log_gamma_range", log_gamma_range, finite=True)
        c.gamma_window[:] = _ordered(who, "gamma_window", gamma_window, finite=True)
        if not c.gamma_window[0] < c.gamma_window[1]:
            raise ValueError(f"{who}: gamma_window={tuple(gamma_window)} needs lo < hi")
        self.config = c
        self.out_dtype = out_dtype
        self.last_params = None

    @classmethod
    def _volumes(cls, img):
        img = _check_volumes(cls._WHO, img, "D, H, W", (torch.bfloat16, torch.float32))
        if img.requires_grad:
            raise RuntimeError("ContrastAugment: the stage has no backward; detach the volumes")
        return img

    def _table(self, B, M, device):
        return self._static_table(B, M, CON_NPARAM, device)

    def draw(self, B, M, device) -> ContrastParams:
        """One table for B x M volumes; advances the call index."""
        table = self._table(B, M, device)
        self._draw(lambda *at: ops.contrast_draw(self.config, table, *at), advance=True)
        return ContrastParams(table)

    def apply(self, img, params, out_dtype=None):
        img = self._volumes(img)
        table = params.table if isinstance(params, ContrastParams) else params
        B, M = img.shape[:2]
        if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or tuple(table.shape) != (B, M, CON_NPARAM):
            raise ValueError(f"ContrastAugment: the table must be fp32 [{B}, {M}, {CON_NPARAM}] for these volumes, got "
                             f"{getattr(table, 'dtype', type(table))} {tuple(getattr(table, 'shape', ()))}")
        if table.device != img.device:
            raise ValueError(f"ContrastAugment: the table is on {table.device}, the volumes on {img.device}")
        return ops.contrast_apply(img, table.contiguous(), out_dtype or self.out_dtype)

    def forward(self, img):
        if not self.training:
            return img
        img = self._volumes(img)
        self.last_params = self.draw(img.shape[0], img.shape[1], img.device)
        return self.apply(img, self.last_params)
