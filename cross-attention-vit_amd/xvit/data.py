"""A device-resident volume store whose batches are drawn and gathered on the GPU.

The reference reads its cases through a DataLoader with five workers and a WeightedRandomSampler (main_mist.py:194-207).  At its shape
(8 samples of 2 x 240 x 240 x 155 int16) that is 286 MB per step, against a captured step of a few milliseconds: no host loader keeps
up.  The data set is small (501 cases, 18 GB at two modalities), so it lives on the device:

    store = VolumeStore((M, Ds, Hs, Ws), capacity=len(cases), device="cuda")
    for vol, label in cases:                                # once, before training
        store.add(vol, label)
    sampler = BatchSampler(store, 8, mode="weighted", weights=class_balanced_weights(store.labels[:len(store)]), seed=0, capturable=True)
    aug = xvit.VolumeAugment(img_size, capturable=True)
    sampler(); aug(sampler()[0])                            # allocate the static buffers outside the capture
    step = GraphedStep(model, img0, y0, optimizer=opt, source=lambda: (lambda r, y: (aug(r), y))(*sampler()))
    for _ in range(steps):
        step()                                              # draw -> gather -> augment -> forward -> backward -> optimizer: one replay

Two launches per batch (include/xvit.h, "Device-resident volume store"): xvit_batch_draw writes the batch's case indices from
(seed, global sample ordinal), xvit_batch_gather copies the cases those indices name.  The indices never leave the device.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops

_MODES = {"weighted": _lib.BATCH_WEIGHTED, "shuffle": _lib.BATCH_SHUFFLE, "sequential": _lib.BATCH_SEQUENTIAL}
_DTYPES = (torch.int16, torch.bfloat16, torch.float32)
_MASK64 = (1 << 64) - 1


def class_balanced_weights(labels) -> torch.Tensor:
    """Inverse class frequency per case, fp64 [n]: a case of a class with c members weighs 1 / c, so every class present is drawn equally
    often.  This is the usual input to WeightedRandomSampler; the reference's own create_sampler is not available to this project, and
    parity with its exact rule is not claimed."""
    labels = torch.as_tensor(labels).detach().cpu().to(torch.int64).reshape(-1)
    if labels.numel() == 0:
        raise ValueError("class_balanced_weights: no labels")
    _, inverse, counts = torch.unique(labels, return_inverse=True, return_counts=True)
    return 1.0 / counts.to(torch.float64)[inverse]


def make_cdf(weights) -> torch.Tensor:
    """The fp64 inclusive prefix of the normalised weights as xvit_batch_draw reads it: non-decreasing, and exactly 1 from the last
    positive weight on, so that a zero-weight case is never drawn."""
    w = torch.as_tensor(weights).detach().cpu().to(torch.float64).reshape(-1).numpy()
    if w.size == 0 or not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
        raise ValueError("BatchSampler: weights must be finite and non-negative with a positive sum")
    cdf = np.cumsum(w) / w.sum()
    cdf[int(np.nonzero(w > 0)[0][-1]):] = 1.0
    return torch.from_numpy(np.minimum(cdf, 1.0))


class VolumeStore:
    """The raw volumes of every case in ONE device allocation [capacity, M, Ds, Hs, Ws] (int16, bf16 or fp32), with their labels (int64, on
    the host and on the device) and sampling weights (fp64, on the host).  The allocation is made at construction and never replaced: a
    captured graph holds its address.  add / extend accept host or device tensors and copy them once."""

    def __init__(self, case_shape, capacity, dtype=torch.int16, device="cuda"):
        case_shape = tuple(int(s) for s in case_shape)
        if len(case_shape) != 4 or min(case_shape) <= 0:
            raise ValueError(f"VolumeStore: case_shape is (M, Ds, Hs, Ws), all positive, got {case_shape}")
        if not (isinstance(capacity, int) and capacity > 0):
            raise ValueError(f"VolumeStore: capacity must be a positive integer, got {capacity!r}")
        if dtype not in _DTYPES:
            raise TypeError(f"VolumeStore: dtype {dtype} is not supported (int16, bfloat16 or float32)")
        self.case_shape, self.capacity, self.dtype, self.device = case_shape, capacity, dtype, torch.device(device)
        self.volumes = torch.zeros((capacity,) + case_shape, dtype=dtype, device=self.device)
        self.labels = torch.full((capacity,), -1, dtype=torch.int64)                  # host
        self.weights = torch.zeros(capacity, dtype=torch.float64)                      # host
        self.labels_dev = torch.full((capacity,), -1, dtype=torch.int64, device=self.device)
        self._n = 0

    def __len__(self):
        return self._n

    @property
    def case_bytes(self) -> int:
        return int(np.prod(self.case_shape)) * self.volumes.element_size()

    def add(self, volumes, label, weight=1.0):
        """One case: volumes [M, Ds, Hs, Ws] of the store's dtype, on the host or on any device."""
        if not isinstance(volumes, torch.Tensor) or tuple(volumes.shape) != self.case_shape:
            raise ValueError(f"VolumeStore.add: a case is a tensor of shape {self.case_shape}, got {tuple(getattr(volumes, 'shape', ()))}")
        return self.extend(volumes[None], [int(label)], [float(weight)])

    def extend(self, volumes, labels, weights=None):
        """Several cases: volumes [k, M, Ds, Hs, Ws], labels [k], weights [k] (None: 1 each)."""
        if not isinstance(volumes, torch.Tensor) or volumes.dim() != 5 or tuple(volumes.shape[1:]) != self.case_shape:
            raise ValueError(f"VolumeStore.extend: cases are a tensor of shape [k, {', '.join(map(str, self.case_shape))}], got {tuple(getattr(volumes, 'shape', ()))}")
        if volumes.dtype != self.dtype:
            raise TypeError(f"VolumeStore: the store holds {self.dtype}, got {volumes.dtype} (no silent conversion)")
        k = volumes.shape[0]
        labels = torch.as_tensor(labels).detach().cpu().to(torch.int64).reshape(-1)
        weights = torch.ones(k, dtype=torch.float64) if weights is None else torch.as_tensor(weights).detach().cpu().to(torch.float64).reshape(-1)
        if labels.numel() != k or weights.numel() != k:
            raise ValueError(f"VolumeStore.extend: {k} cases need {k} labels and weights, got {labels.numel()} and {weights.numel()}")
        if not bool(torch.isfinite(weights).all()) or bool((weights < 0).any()):
            raise ValueError("VolumeStore: weights must be finite and non-negative")
        if self._n + k > self.capacity:
            raise RuntimeError(f"VolumeStore: {self._n} + {k} cases exceed the capacity of {self.capacity} (the allocation is never replaced: a captured "
                               "graph holds its address)")
        if k == 0:
            return self
        lo, hi = self._n, self._n + k
        self.volumes[lo:hi].copy_(volumes)                   # the one copy, host -> device or device -> device
        self.labels[lo:hi] = labels
        self.weights[lo:hi] = weights
        self.labels_dev[lo:hi].copy_(labels)
        self._n = hi
        return self

    def gather(self, idx, out=None, labels_out=None, status=None):
        """(raw [B, M, Ds, Hs, Ws], y [B]) of the cases idx names.  A host idx is validated here and copied; a device idx (int32) is taken
        as it is and read by the kernel only: an index outside [0, len(store)) then gives a zero-filled case, label -1 and status 1."""
        if len(self) == 0:
            raise RuntimeError("VolumeStore.gather: the store is empty")
        idx = torch.as_tensor(idx)
        if idx.dim() != 1 or idx.numel() == 0 or idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"VolumeStore.gather: idx is a non-empty vector of int32 or int64 indices, got {idx.dtype} {tuple(idx.shape)}")
        if not idx.is_cuda:
            if int(idx.min()) < 0 or int(idx.max()) >= len(self):
                raise IndexError(f"VolumeStore.gather: indices must lie in [0, {len(self)}), got [{int(idx.min())}, {int(idx.max())}]")
            idx = idx.to(torch.int32).to(self.device)
        elif idx.dtype != torch.int32:
            idx = idx.to(torch.int32)
        return ops.batch_gather(self.volumes, idx.contiguous(), len(self), labels=self.labels_dev, out=out, labels_out=labels_out, status=status)


class BatchSampler:
    """The reference's sampler drawn on the device, and the batch it names.  raw, y = sampler() runs two launches: the draw of batch_size
    case indices and their gather from `store`.

    mode "weighted" draws with replacement from `weights` (None: the store's own; WeightedRandomSampler(replacement=True) in kind, not
    torch's random stream); "shuffle" walks a keyed permutation per epoch, so that every case is seen once per len(store) samples and the
    ranks of an epoch are disjoint; "sequential" walks the cases in order.  Sample i of call c on rank r is the global sample
    (c * world_size + r) * batch_size + i, and is a function of (seed, that ordinal) alone.

    len(store) and the weights are snapshotted at construction: cases added later are not seen (build a new sampler).

    capturable=True keeps the call index in a device counter that the draw kernel reads and advances: the call can sit inside
    torch.cuda.graph (or behind GraphedStep(source=...)) and every replay draws the next batch.  Call the sampler once before capturing; the
    first call allocates its static buffers.  last_indices (int32 [B]) and last_status (int32 [B], 1 where an index was refused) are the
    device tensors of the last call, static when capturable.  state_dict() / load_state_dict() carry the call index: a resumed run
    continues the same sample stream."""

    def __init__(self, store, batch_size, mode="weighted", weights=None, seed=0, rank=0, world_size=1, capturable=False):
        if not isinstance(store, VolumeStore):
            raise TypeError(f"BatchSampler: store is a VolumeStore, got {type(store).__name__}")
        if len(store) == 0:
            raise RuntimeError("BatchSampler: the store is empty")
        if not (isinstance(batch_size, int) and batch_size > 0):
            raise ValueError(f"BatchSampler: batch_size must be a positive integer, got {batch_size!r}")
        if mode not in _MODES:
            raise ValueError(f"BatchSampler: mode is one of {sorted(_MODES)}, got {mode!r}")
        if not (isinstance(world_size, int) and isinstance(rank, int) and world_size > 0 and 0 <= rank < world_size):
            raise ValueError(f"BatchSampler: rank={rank!r} must lie in [0, world_size={world_size!r})")
        self.store, self.batch_size, self.mode, self.seed = store, batch_size, mode, int(seed)
        self.rank, self.world_size, self.capturable = rank, world_size, bool(capturable)
        self.n_cases = len(store)
        self.cdf = None
        if mode == "weighted":
            w = store.weights[:self.n_cases] if weights is None else torch.as_tensor(weights).reshape(-1)
            if w.numel() != self.n_cases:
                raise ValueError(f"BatchSampler: {self.n_cases} cases need {self.n_cases} weights, got {w.numel()}")
            self.cdf = make_cdf(w).to(store.device)
        elif weights is not None:
            raise ValueError(f"BatchSampler: weights are read in the weighted mode only, not in {mode!r}")
        self.calls = 0             # host call index (capturable: see call_index)
        self._counter = None       # capturable: the device call index
        self._static = None        # capturable: (idx, status, raw, y)
        self.last_indices = self.last_status = None

    @property
    def call_index(self) -> int:
        """Calls made so far (capturable: read from the device counter, a host synchronisation)."""
        return int(self._counter.item()) if self._counter is not None else self.calls

    def _buffers(self):
        dev, B = self.store.device, self.batch_size
        if self.capturable and self._static is not None:
            return self._static
        if self.capturable and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("BatchSampler(capturable=True): call the sampler once before capturing it; its buffers and counter must not be "
                               "allocated inside the graph")
        bufs = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                torch.empty((B,) + self.store.case_shape, dtype=self.store.dtype, device=dev), torch.empty(B, dtype=torch.int64, device=dev))
        if self.capturable:
            self._static = bufs
            self._counter = torch.full((1,), self.calls, dtype=torch.int64, device=dev)
        return bufs

    def __call__(self):
        idx, status, raw, y = self._buffers()
        common = dict(cdf=self.cdf, rank=self.rank, world=self.world_size)
        if self.capturable:
            ops.batch_draw(idx, _MODES[self.mode], self.n_cases, self.seed, counter=self._counter, advance=True, **common)
        else:
            ops.batch_draw(idx, _MODES[self.mode], self.n_cases, self.seed, call=self.calls, **common)
            self.calls += 1
        ops.batch_gather(self.store.volumes, idx, self.n_cases, labels=self.store.labels_dev, out=raw, labels_out=y, status=status)
        self.last_indices, self.last_status = idx, status
        return raw, y

    def state_dict(self):
        return {"call_index": self.call_index, "seed": self.seed, "mode": self.mode, "batch_size": self.batch_size, "rank": self.rank,
                "world_size": self.world_size, "n_cases": self.n_cases}

    def load_state_dict(self, state):
        for key in ("seed", "mode", "batch_size", "world_size", "n_cases"):
            if key in state and state[key] != getattr(self, key):
                raise ValueError(f"BatchSampler.load_state_dict: {key}={state[key]!r} was saved, this sampler has {getattr(self, key)!r}: "
                                 "the sample stream would not be the one that was interrupted")
        k = int(state["call_index"])
        if not 0 <= k <= _MASK64:
            raise ValueError(f"BatchSampler.load_state_dict: call_index={k} is not a 64-bit count")
        self.calls = k
        if self._counter is not None:
            self._counter.fill_(k if k < (1 << 63) else k - (1 << 64))
