"""Fused Adam for the drop-in models: same update as the reference's
`torch.optim.Adam(self.parameters(), lr=self.lr, weight_decay=self.weight_decay)` (model_cross.py:277), one HIP launch
per parameter group instead of a foreach chain, and the bf16 GEMM-operand copy of every flat-stored weight is written
by the same kernel (so `FlatWeights.refresh` has nothing to re-cast after a step).

    opt = xvit.optim.FusedAdam(model.parameters(), lr=1e-4, weight_decay=0.0)
    ... loss.backward(); opt.step(); opt.zero_grad()

Three keyword-only options, all off by default (without them `step()` runs exactly the launches it always ran):

`max_grad_norm=c`: global-norm gradient clipping fused into the step, `torch.nn.utils.clip_grad_norm_(params, c)` followed by Adam:
one extra read of the gradients (per-chunk sums of squares, fixed order, no atomics: bit-identical from run to run), a one-block
prologue that turns them into the norm and the clip coefficient on the device, and the Adam kernel multiplies every gradient by that
coefficient in registers.  The norm runs over all parameter groups together.  UNLIKE `clip_grad_norm_`, `p.grad` IS NOT RESCALED IN
MEMORY: it stays the unclipped gradient (that saves a read-modify-write pass over all gradients); `opt.last_grad_norm` is the
pre-clip norm as a 0-dim device tensor (reading it is the caller's synchronisation).

`capturable=True`: nothing about a step is a host number any more.  The tensor tables, the per-group step count, the learning rate,
the bias corrections and the clip coefficient live on the device; they are built once (at the first `step()`, or `prepare()`, from
the parameters that have a gradient then) and after that `step()` allocates nothing, copies nothing and synchronises nothing: it
enqueues the norm, prologue and Adam launches on the current stream, so it can be captured into a HIP graph (`torch.cuda.graph`, or
`xvit.graph.GraphedStep(..., optimizer=opt)` for the whole training step).  The graph holds addresses: parameters and gradients must stay
where they were (`zero_grad(set_to_none=False)` in an eager loop), which `step()` checks.  The learning rate is the one hyper-parameter
that may change after a capture: `sync_lr()` writes `group["lr"]` into the device record when it differs from what is there, so any
torch scheduler works; betas, eps, weight decay and max_grad_norm are frozen into a captured launch.

`skip_nonfinite=True` (needs `capturable=True`: only a device-side step count can stand still without a synchronisation): a step whose
gradient norm is inf or NaN changes no parameter, no moment and not the step count; `opt.skipped_steps` counts them on the device.

Both classes run one skeleton.  A step works on LAUNCH SETS (`_Set`): the tensors that go into one table, their chunk list, their offset
into the norm partials and one device record.  FusedAdam makes one set per parameter group, FusedAdamW one per (betas, eps, step count)
across groups; a subclass says how tensors are keyed into sets (`_set_key`), what a set carries beside its table and chunk list and
which rate its record gets (`_fill`), and which entry point steps it (`_launch_step`).  Everything else stands once, in FusedAdam.
"""
from __future__ import annotations

import math
import weakref

import numpy as np
import torch

from . import _lib
from . import functional as XF
from . import ops

CHUNK = 16384
# struct xvit_adam_state (include/xvit.h) as 6 int64 words / 12 fp32 words
_REC_WORDS = 6
_REC_DTYPE = np.dtype([("step", "<i8"), ("skipped", "<i8"), ("lr", "<f4"), ("grad_norm", "<f4"), ("clip_coef", "<f4"), ("lr_over_bc1", "<f4"),
                       ("inv_sqrt_bc2", "<f4"), ("skip", "<i4"), ("reserved", "<i4", (2,))])
_F_LR, _F_NORM = 4, 5          # fp32 word index of lr / grad_norm
assert _REC_DTYPE.itemsize == 8 * _REC_WORDS
# struct xvit_adamw_extra (include/xvit.h): one row per row of the tensor table
_EXTRA_DTYPE = np.dtype([("ema", "<u8"), ("lr_scale", "<f4"), ("weight_decay", "<f4")])
assert _EXTRA_DTYPE.itemsize == 16


class _Set:
    """One launch set.  Host side: the tensors (each with its group index `gis` and its index in that group `idx`), their table rows
    and chunk list, the step count they share.  Device side, once uploaded: `table`, `chunk_t`, the record at `rec_ptr`, and whatever
    the optimizer's `_fill` adds.  Eager mode builds the sets anew every step; capturable mode keeps them (`p_ptrs`, `g_ptrs`, `lr`,
    `lr_view` are what check_addresses() and sync_lr() compare against)."""
    __slots__ = ("step", "steps", "params", "gis", "idx", "rows", "chunks", "keep", "n_chunks", "off", "table", "chunk_t", "rec_ptr", "lr", "lr_view",
                 "p_ptrs", "g_ptrs", "groups", "extras", "extras_host", "seen")

    def __init__(self):
        self.steps, self.params, self.gis, self.idx, self.rows, self.chunks, self.keep = set(), [], [], [], [], [], []
        self.extras = None

    def add(self, row, p, gi=None, i=None):
        """Append one tensor: its table row (FusedAdam._row) and one (row index, chunk index) pair per CHUNK elements."""
        t = len(self.rows)
        self.chunks.extend((t, c) for c in range((row[5] + CHUNK - 1) // CHUNK))
        self.rows.append(row); self.params.append(p); self.gis.append(gi); self.idx.append(i)

    def upload(self, dev, non_blocking):
        self.n_chunks = len(self.chunks)
        self.table = _upload(np.asarray(self.rows, dtype=np.int64), dev, non_blocking)
        self.chunk_t = _upload(np.asarray(self.chunks, dtype=np.int32), dev, non_blocking)


def _upload(a, dev, non_blocking):
    """A host array on the device; a structured one (records, extras) as rows of int64 words."""
    if a.dtype.names:
        a = a.view(np.int64).reshape(len(a), -1)
    return torch.from_numpy(a).to(dev, non_blocking=non_blocking)


class FusedAdam(torch.optim.Optimizer):
    _SET = "parameter group"          # what one launch set is, in messages

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, *, max_grad_norm=None, capturable=False,
                 skip_nonfinite=False):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        if max_grad_norm is not None and not (max_grad_norm > 0 and math.isfinite(max_grad_norm)):
            raise ValueError(f"max_grad_norm must be a positive finite number or None, got {max_grad_norm!r}")
        if skip_nonfinite and not capturable:
            raise ValueError("skip_nonfinite=True needs capturable=True (the step count has to live on the device to stand still without a sync)")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.capturable = bool(capturable)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.lr_copies = 0            # how many times sync_lr() wrote a learning rate to the device
        self._entries = None          # capturable mode: the launch sets, built by prepare()
        self._records = self._partials = self._last_norm = None
        self._touched, self._unshadowed = [], []

    @staticmethod
    def _validate(p, g):
        if not p.is_cuda or p.dtype != torch.float32 or g.dtype != torch.float32 or g.is_sparse:
            raise RuntimeError("xvit FusedAdam: parameters and gradients must be dense fp32 tensors on the GPU")
        if not p.is_contiguous():
            raise RuntimeError("xvit FusedAdam: non-contiguous parameter")

    def _state_of(self, p):
        st = self.state[p]
        if not st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    @property
    def _needs_norm(self):
        return self.max_grad_norm is not None or self.skip_nonfinite

    @property
    def last_grad_norm(self):
        """Total L2 norm of the last step's gradients before clipping: 0-dim fp32 device tensor (no sync here), or None when the
        optimizer takes no norm (neither max_grad_norm nor skip_nonfinite) or has not stepped yet."""
        return self._last_norm

    @property
    def skipped_steps(self):
        """Number of steps skip_nonfinite dropped: 0-dim int64 device tensor (capturable mode after the first step), else None."""
        return None if self._entries is None else self._records[0, 1]

    def _describe(self, s, i):
        gi, idx, p = s.gis[i], s.idx[i], s.params[i]
        names = self.param_groups[gi].get("param_names")
        return f"parameter {idx} of group {gi}" + (f" ({names[idx]})" if names else "") + f", shape {tuple(p.shape)}"

    def _one_step(self, s, steps, found):
        """The step count a capturable launch set keeps in its one record; `found` words the refusal when its tensors disagree."""
        if len(steps) != 1:
            raise ValueError(f"xvit {type(self).__name__}(capturable=True) keeps one step count per {self._SET}; {found} steps {sorted(steps)} in the "
                             f"{self._SET} over group(s) {sorted(set(s.gis))}")
        return next(iter(steps))

    # ------------------------------------------------------------------------------------------------------------------------
    # what a subclass replaces
    # ------------------------------------------------------------------------------------------------------------------------
    def _set_key(self, gi, group, step):
        """Tensors with equal keys share a launch set (eager mode splits further by step count, which the host keeps per parameter)."""
        return gi

    def _fill(self, s, dev, eager):
        """After the table and the chunk list: the rate the set's record (or by-value launch) carries, and any further device table."""
        s.lr = float(self.param_groups[s.gis[0]]["lr"])

    def _launch_step(self, lib, s, by_value, stream):
        """The update of one set: numbers by value (eager without a norm: step count s.step + 1) or from the record at s.rec_ptr."""
        group = self.param_groups[s.gis[0]]
        b1, b2 = group["betas"]
        if by_value:
            _lib.check(lib.xvit_adam_step(s.table.data_ptr(), s.chunk_t.data_ptr(), s.n_chunks, s.lr, b1, b2, group["eps"], group["weight_decay"], s.step + 1,
                                          1.0, stream), "xvit_adam_step")
        else:
            _lib.check(lib.xvit_adam_step_dev(s.table.data_ptr(), s.chunk_t.data_ptr(), s.n_chunks, s.rec_ptr, b1, b2, group["eps"], group["weight_decay"],
                                              stream), "xvit_adam_step_dev")

    # ------------------------------------------------------------------------------------------------------------------------
    # host bookkeeping after the kernels wrote the parameters
    # ------------------------------------------------------------------------------------------------------------------------
    def mark_updated(self):
        """Host bookkeeping that belongs to a step, without launching anything (xvit.graph.GraphedStep calls it after a replay, when no
        Python step() ran).  The kernel rewrote p in place through raw pointers (no version bump) AND its bf16 copy: the flat weight
        groups are marked fresh; every other parameter (ModelVIT, the model.py Encoder, stand-alone modules, XVIT_FLAT_WEIGHTS=0) keeps
        a per-parameter bf16 copy keyed by the version counter, which a raw-pointer write does not move, so those copies are dropped."""
        for ref in self._touched:
            grp = ref()
            if grp is not None:
                grp.stamp = sum(q._version for q in grp.params)
        XF.SHADOWS.drop(self._unshadowed)
        self._opt_called = True       # what torch's lr_scheduler checks before its first step(): a replayed step counts as one

    def _mark(self, marks):
        touched, unshadowed = marks
        self._touched = [weakref.ref(g) for g in touched.values()]
        self._unshadowed = unshadowed

    # ------------------------------------------------------------------------------------------------------------------------
    # launch sets: the walk, the tables, the records, the launches
    # ------------------------------------------------------------------------------------------------------------------------
    def _row(self, p, g, marks=None):
        """The table row of p (struct AdamTensor in csrc/misc.hip): p, g, both moments, the bf16 operand copy an intact flat weight group
        keeps of p (0: none) and numel.  `marks` = ({}, []) collects what mark_updated() needs: the flat groups written, and the
        parameters that have no such copy."""
        st = self.state[p]
        sh = 0
        for grp in XF.SHADOWS.groups:
            i = grp.index.get(id(p))
            if i is not None and grp.params[i] is p and grp.intact():
                sh = grp.view16[i].data_ptr()
                if marks is not None:
                    marks[0][id(grp)] = grp
                break
        else:
            if marks is not None:
                marks[1].append(p)
        return (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), sh, p.numel())

    def _collect(self, eager):
        """Every parameter that has a gradient, keyed into launch sets (first-seen order) and uploaded.  Eager: advances the host step
        counts and takes a contiguous copy of a strided gradient (the set keeps it alive).  Capturable: refuses one, and a set whose
        tensors sit at different step counts."""
        sets, marks = {}, ({}, [])
        for gi, group in enumerate(self.param_groups):
            by_step = {}                    # step count -> the set this group's tensors at that count go to: one key per count, not per tensor
            for i, p in enumerate(group["params"]):
                g = p.grad
                if g is None:
                    continue
                self._validate(p, g)
                st = self._state_of(p)
                step = int(st["step"])
                s = by_step.get(step)
                if s is None:
                    key = self._set_key(gi, group, step)
                    s = by_step[step] = sets.setdefault((key, step) if eager else key, _Set())
                    s.steps.add(step)
                if not g.is_contiguous():
                    if not eager:
                        raise RuntimeError(f"xvit {type(self).__name__}(capturable=True): non-contiguous gradient")
                    g = g.contiguous()
                    s.keep.append(g)
                if eager:
                    st["step"] = step + 1
                s.add(self._row(p, g, marks), p, gi, i)
        sets, off = list(sets.values()), 0
        for s in sets:
            s.step = self._one_step(s, s.steps, "it finds parameters at")
            dev = s.params[0].device
            s.upload(dev, eager)
            s.off = off
            off += s.n_chunks
            self._fill(s, dev, eager)
        self._mark(marks)
        return sets

    def _device_state(self, sets, non_blocking):
        """-> (one record per set, holding its step count and rate; one norm partial per chunk of all sets, or None without a norm)."""
        dev = sets[0].table.device
        rec = np.zeros(len(sets), dtype=_REC_DTYPE)
        rec["step"] = [s.step for s in sets]          # the prologue advances it
        rec["lr"] = [s.lr for s in sets]
        records = _upload(rec, dev, non_blocking)
        for k, s in enumerate(sets):
            s.rec_ptr = records.data_ptr() + 8 * _REC_WORDS * k
        partials = torch.empty(sum(s.n_chunks for s in sets), dtype=torch.float32, device=dev) if self._needs_norm else None
        return records, partials

    def _launch(self, lib, sets, partials, stream, by_value=False):
        """The launches of one step: the norm partials of every set (when a norm is taken), then per set one prologue, which turns ALL
        partials into norm and clip coefficient and advances the set's record, and the update.  by_value: the update alone."""
        if partials is not None:
            for s in sets:
                _lib.check(lib.xvit_grad_sqnorm_partials(s.table.data_ptr(), s.chunk_t.data_ptr(), s.n_chunks, partials.data_ptr() + 4 * s.off, stream),
                           "xvit_grad_sqnorm_partials")
        part, n_part = (partials.data_ptr(), partials.numel()) if partials is not None else (None, 0)
        max_norm = self.max_grad_norm if self.max_grad_norm is not None else math.inf
        for s in sets:
            if not by_value:
                b1, b2 = self.param_groups[s.gis[0]]["betas"]
                _lib.check(lib.xvit_adam_prologue(part, n_part, s.rec_ptr, max_norm, b1, b2, int(self.skip_nonfinite), stream), "xvit_adam_prologue")
            self._launch_step(lib, s, by_value, stream)

    # ------------------------------------------------------------------------------------------------------------------------
    # eager mode: sets per step, as the step count is kept per parameter on the host
    # ------------------------------------------------------------------------------------------------------------------------
    def _step_eager(self, lib):
        sets = self._collect(eager=True)
        if sets:
            cur = torch.cuda.current_stream()
            records, partials = self._device_state(sets, True) if self._needs_norm else (None, None)
            self._launch(lib, sets, partials, cur.cuda_stream, by_value=records is None)
            for s in sets:
                for t in (s.table, s.chunk_t, s.extras):
                    if t is not None:
                        t.record_stream(cur)
            if records is not None:
                records.record_stream(cur); partials.record_stream(cur)
                self._last_norm = records[0].view(torch.float32)[_F_NORM]
        self.mark_updated()

    # ------------------------------------------------------------------------------------------------------------------------
    # capturable mode: everything built once
    # ------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prepare(self):
        """capturable=True: build the device tables, chunk lists, norm partials and state records of every launch set from the
        parameters that have a gradient NOW (allocation + host-to-device copies: not capturable, so call it, or take one eager step,
        before a capture).  Later calls do nothing."""
        name = type(self).__name__
        if not self.capturable:
            raise RuntimeError(f"xvit {name}.prepare: only for capturable=True")
        if self._entries is not None:
            return
        sets = self._collect(eager=False)
        if not sets:
            raise RuntimeError(f"xvit {name}.prepare: no parameter has a gradient yet (run one backward, or set the static .grad buffers, first)")
        self._records, self._partials = self._device_state(sets, False)
        for k, s in enumerate(sets):
            s.lr_view = self._records[k].view(torch.float32)[_F_LR]
        self._entries = sets
        self._last_norm = self._records[0].view(torch.float32)[_F_NORM] if self._needs_norm else None
        self.rebind()

    @torch.no_grad()
    def rebind(self):
        """Re-read the addresses of the parameters, their CURRENT .grad tensors and bf16 copies into the existing device tables (a
        host-to-device copy: outside any capture).  The launches hold only the tables' own addresses, so a graph captured before stays
        valid: xvit.graph.GraphedStep captures the step first and binds the gradient buffers the capture allocated afterwards."""
        for s in self._entries:
            for i, p in enumerate(s.params):
                if p.grad is None or p.grad.shape != p.shape or not p.grad.is_contiguous() or p.grad.dtype != torch.float32:
                    raise RuntimeError(f"xvit FusedAdam.rebind: {self._describe(s, i)} has no dense contiguous fp32 gradient to bind")
            s.rows = [self._row(p, p.grad) for p in s.params]
            s.table.copy_(torch.from_numpy(np.asarray(s.rows, dtype=np.int64)))
            s.p_ptrs = [r[0] for r in s.rows]
            s.g_ptrs = [r[1] for r in s.rows]

    def check_addresses(self, grads: bool = True):
        """capturable mode: every parameter (and, with grads=True, its .grad) still lives at the address in the device table."""
        for s in self._entries or ():
            for i, p in enumerate(s.params):
                if p.data_ptr() != s.p_ptrs[i]:
                    raise RuntimeError(f"xvit FusedAdam(capturable=True): the storage of {self._describe(s, i)} moved after the tables were built "
                                       "(model.to(...), a re-built flat weight buffer); build a new optimizer")
                if grads and (p.grad is None or p.grad.data_ptr() != s.g_ptrs[i]):
                    raise RuntimeError(f"xvit FusedAdam(capturable=True): the gradient of {self._describe(s, i)} is no longer the tensor the device table "
                                       "points to (typically zero_grad(set_to_none=True) in an eager loop, which makes backward allocate a new one): "
                                       "use zero_grad(set_to_none=False), or xvit.graph.GraphedStep(..., optimizer=opt), which owns static gradient buffers")

    def _sync_rate(self, s, lr):
        if lr != s.lr:
            s.lr_view.fill_(lr)
            s.lr = lr
            self.lr_copies += 1

    def sync_lr(self):
        """Write group["lr"] into the device record of every group whose rate changed since the last call (one tiny asynchronous fill
        on the current stream, value passed as a kernel argument: no host buffer to keep alive); nothing is issued otherwise.  step()
        calls it in eager mode, GraphedStep before each replay; call it yourself before replaying your own capture of step()."""
        for s in self._entries or ():
            self._sync_rate(s, float(self.param_groups[s.gis[0]]["lr"]))

    def enqueue(self):
        """capturable mode: the launches of one step on the current stream and nothing else (no check, no bookkeeping): the gradient
        norm (when one is taken), then one prologue + step pair per launch set."""
        self._launch(_lib.load(), self._entries, self._partials, ops._stream())

    # ------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self.capturable:
            self._step_eager(_lib.load())
            return loss
        self.prepare()
        self.check_addresses()
        if not torch.cuda.is_current_stream_capturing():
            self.sync_lr()
        self.enqueue()
        self.mark_updated()
        return loss

    # ------------------------------------------------------------------------------------------------------------------------
    # state_dict: torch's key names in both modes
    # ------------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """exp_avg / exp_avg_sq / step per parameter, as torch.optim.Adam names them (FusedAdamW: and `ema`).  In capturable mode `step`
        is read from the device counters here (a synchronisation)."""
        if self._entries is not None:
            steps = self._records[:, 0].tolist()
            for s, step in zip(self._entries, steps):
                for p in s.params:
                    self.state[p]["step"] = int(step)
        return super().state_dict()

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Accepts a state dict of either mode and of either class (or of torch.optim.Adam / AdamW).  Once the capturable tables exist,
        the values are copied INTO the existing buffers and device counters, so a captured graph stays valid."""
        old = {p: self.state[p] for s in self._entries or () for p in s.params}
        super().load_state_dict(state_dict)
        for p, st in list(self.state.items()):
            if "step" in st:
                st["step"] = int(st["step"])
            if "exp_avg" in st:
                self._state_of(p)               # adds what this class keeps beside the moments
        for k, s in enumerate(self._entries or ()):
            steps = set()
            for i, p in enumerate(s.params):
                new = self.state.get(p)
                if not new or "exp_avg" not in new:
                    raise ValueError(f"xvit {type(self).__name__}.load_state_dict: no state for {self._describe(s, i)}, which the capturable tables hold")
                keep = old[p]
                for name, buf in keep.items():
                    if name != "step":
                        buf.copy_(new[name])
                keep["step"] = new["step"]
                steps.add(new["step"])
                self.state[p] = keep
            self._records[k, 0].fill_(self._one_step(s, steps, "the loaded state has"))


# ============================================================================================================================
# AdamW with layer-wise rates and a fused weight EMA
# ============================================================================================================================
class _EmaWeights:
    def __init__(self, opt):
        self.opt = opt

    def __enter__(self):
        self.opt._swap()
        return self.opt

    def __exit__(self, *exc):
        self.opt._swap()
        return False


class FusedAdamW(FusedAdam):
    """`torch.optim.AdamW` (decoupled=True, the default) or `torch.optim.Adam` (decoupled=False) with a rate and a decay PER TENSOR in one
    launch, and an optional exponential moving average of the weights updated by the same kernel.

        opt = xvit.optim.FusedAdamW(xvit.optim.layer_decay_groups(model, 0.75, 0.05), lr=1e-3, ema_decay=0.9999, capturable=True)

    Groups.  Every group may carry `lr_scale` (default 1.0) beside `lr` and `weight_decay`: a tensor's rate is group["lr"] * group["lr_scale"],
    its decay group["weight_decay"].  Groups that agree on betas, eps and step count form one launch set (`opt.launch_sets`): one tensor
    table, one table of per-tensor extras, one device record and one prologue + step launch pair, however many groups there are.  The
    record holds the rate of the set's first group (the first non-zero one, should that be 0 while others are not); every tensor's scale
    is fp32(lr_scale * lr / that rate).  `sync_lr()` therefore costs one fill (`lr_copies`) while the groups of a set share their `lr`, which
    is what every torch scheduler does to groups built with one base rate, and one host-to-device copy of the extras table
    (`scale_copies`) when the rates diverge.  As with FusedAdam, betas, eps, weight decay and max_grad_norm are frozen into a capture.

    `ema_decay=d`: state[p]["ema"], an fp32 copy of p created together with the moments, follows e += w (p' - e) with w = 1 - d, or with
    `ema_warmup=True` w = 1 - min(d, (1 + t) / (10 + t)) at step t (timm's ModelEma warm-up).  A skipped step leaves it alone.  It is part
    of state_dict() / load_state_dict(); A LOADED STATE WITHOUT `ema` (one of FusedAdam or torch.optim.AdamW) STARTS THE AVERAGE AT THE
    CURRENT p.  `with opt.ema_weights(): ...` exchanges weights and average in place (and back on exit; addresses do not move, so a captured
    graph stays valid); `opt.ema_state_dict(model)` is the average under the model's own state_dict keys."""
    _SET = "launch set"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, decoupled=True, ema_decay=None, ema_warmup=False,
                 max_grad_norm=None, capturable=False, skip_nonfinite=False):
        if ema_decay is not None and not 0 <= ema_decay < 1:          # NaN fails too
            raise ValueError(f"ema_decay must lie in [0, 1) or be None, got {ema_decay!r}")
        if ema_warmup and ema_decay is None:
            raise ValueError("ema_warmup=True needs ema_decay")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm, capturable=capturable,
                         skip_nonfinite=skip_nonfinite)
        self.defaults["lr_scale"] = 1.0
        for gi, group in enumerate(self.param_groups):
            s = group.setdefault("lr_scale", 1.0)
            if not (s >= 0 and math.isfinite(s)):
                raise ValueError(f"lr_scale of group {gi} must be a finite number >= 0, got {s!r}")
            b1, b2 = group["betas"]
            if not (group["weight_decay"] >= 0 and group["lr"] >= 0 and group["eps"] >= 0 and 0 <= b1 < 1 and 0 <= b2 < 1):
                raise ValueError(f"invalid AdamW hyper-parameter in group {gi}")
        self.decoupled = bool(decoupled)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.scale_copies = 0         # how many times sync_lr() rewrote the per-tensor scale column on the device

    # ------------------------------------------------------------------------------------------------------------------------
    def _state_of(self, p):
        st = super()._state_of(p)
        if self.ema_decay is not None and "ema" not in st:
            st["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
        return st

    @staticmethod
    def _key(group, step):
        return (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]), int(step))

    def _set_key(self, gi, group, step):
        return self._key(group, step)

    @property
    def launch_sets(self):
        """Number of launch sets: of the device tables in capturable mode once they exist, else of the next eager step."""
        if self._entries is not None:
            return len(self._entries)
        return len({self._key(g, self.state[p].get("step", 0) if p in self.state else 0) for g in self.param_groups for p in g["params"]})

    @staticmethod
    def _rates(groups):
        """-> (the rate the launch or the record carries, fp32 scale per group) for the groups of one set."""
        lrs = [float(g["lr"]) for g in groups]
        ref = lrs[0] if lrs[0] != 0 else next((x for x in lrs if x != 0), 0.0)
        return ref, [float(np.float32(float(g["lr_scale"]) if x == ref else float(g["lr_scale"]) * x / ref)) for g, x in zip(groups, lrs)]

    def _scales(self, s):
        """-> (the rate of set s, the fp32 scale of each of its tensors)."""
        lr, scales = self._rates([self.param_groups[gi] for gi in s.groups])
        scale_of = dict(zip(s.groups, scales))
        return lr, np.asarray([scale_of[gi] for gi in s.gis], dtype=np.float32)

    def _ema_weight(self, step):
        """The weight the record path forms on the device, in the same fp32 arithmetic."""
        if self.ema_decay is None:
            return 1.0
        d = np.float32(self.ema_decay)
        if self.ema_warmup:
            t = np.float32(step)
            d = min(d, (np.float32(1) + t) / (np.float32(10) + t))
        return float(np.float32(1) - d)

    def _extras_of(self, params, scales, decays, with_ema):
        x = np.zeros(len(params), dtype=_EXTRA_DTYPE)
        x["ema"] = [self.state[p]["ema"].data_ptr() if with_ema else 0 for p in params]
        x["lr_scale"], x["weight_decay"] = scales, decays
        return x

    def _seen(self, s):
        return tuple((float(self.param_groups[gi]["lr"]), float(self.param_groups[gi]["lr_scale"])) for gi in s.groups)

    def _fill(self, s, dev, eager):
        """The xvit_adamw_extra table; capturable mode keeps its host mirror and the rates it was built from, for sync_lr()."""
        s.groups = list(dict.fromkeys(s.gis))
        s.lr, scales = self._scales(s)
        x = self._extras_of(s.params, scales, [self.param_groups[gi]["weight_decay"] for gi in s.gis], self.ema_decay is not None)
        s.extras = _upload(x, dev, eager)
        if not eager:
            s.extras_host, s.seen = x, self._seen(s)

    def _launch_step(self, lib, s, by_value, stream):
        group = self.param_groups[s.gis[0]]
        b1, b2 = group["betas"]
        tables = (s.table.data_ptr(), s.extras.data_ptr(), s.chunk_t.data_ptr(), s.n_chunks)
        if by_value:
            _lib.check(lib.xvit_adamw_step(*tables, s.lr, b1, b2, group["eps"], s.step + 1, 1.0, int(self.decoupled), self._ema_weight(s.step + 1), stream),
                       "xvit_adamw_step")
        else:
            _lib.check(lib.xvit_adamw_step_dev(*tables, s.rec_ptr, b1, b2, group["eps"], int(self.decoupled), self.ema_decay or 0.0, int(self.ema_warmup),
                                               stream), "xvit_adamw_step_dev")

    def sync_lr(self):
        """Bring the device in line with group["lr"] / group["lr_scale"]: while the groups of a set share one rate a change is ONE fill of the
        record (`lr_copies`); when they diverge the per-tensor scale column is rewritten with one host-to-device copy of the extras table,
        into the same addresses (`scale_copies`; a copy, so outside any capture).  Nothing is issued when nothing changed."""
        for s in self._entries or ():
            seen = self._seen(s)
            if seen == s.seen:
                continue
            s.seen = seen
            lr, column = self._scales(s)
            self._sync_rate(s, lr)
            if not np.array_equal(column, s.extras_host["lr_scale"]):
                s.extras_host["lr_scale"] = column
                s.extras.copy_(torch.from_numpy(s.extras_host.view(np.int64).reshape(-1, 2)))
                self.scale_copies += 1

    # ------------------------------------------------------------------------------------------------------------------------
    # the average
    # ------------------------------------------------------------------------------------------------------------------------
    def _swap(self):
        if self.ema_decay is None:
            raise RuntimeError("xvit FusedAdamW.ema_weights: the optimizer keeps no average (ema_decay=None)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("xvit FusedAdamW.ema_weights: the exchange is not part of a captured step; call it outside the capture")
        lib = _lib.load()
        cur = torch.cuda.current_stream()
        if self._entries is not None:
            self.check_addresses(grads=False)
            sets = self._entries
        else:                             # eager: one set of every parameter that has an average, p standing in for the gradient
            params = [p for g in self.param_groups for p in g["params"] if p in self.state and "ema" in self.state[p]]
            if not params:
                raise RuntimeError("xvit FusedAdamW.ema_weights: no parameter has an average yet (take a step first)")
            s, marks = _Set(), ({}, [])
            for p in params:
                s.add(self._row(p, p, marks), p)
            s.upload(params[0].device, True)
            s.extras = _upload(self._extras_of(params, 1.0, 0.0, True), params[0].device, True)
            self._mark(marks)
            sets = [s]
        for s in sets:
            _lib.check(lib.xvit_ema_swap(s.table.data_ptr(), s.extras.data_ptr(), s.chunk_t.data_ptr(), s.n_chunks, cur.cuda_stream), "xvit_ema_swap")
            if self._entries is None:
                for t in (s.table, s.chunk_t, s.extras):
                    t.record_stream(cur)
        called = getattr(self, "_opt_called", False)
        self.mark_updated()
        self._opt_called = called     # an exchange is not a step

    def ema_weights(self):
        """Context manager: inside, every parameter that has an average holds it (and its bf16 operand copy follows), and state[p]["ema"]
        holds the trained weights; on exit they are exchanged back, bit for bit.  One launch per launch set each way; no allocation in
        capturable mode.  Raises while the current stream is capturing."""
        if self.ema_decay is None:
            raise RuntimeError("xvit FusedAdamW.ema_weights: the optimizer keeps no average (ema_decay=None)")
        return _EmaWeights(self)

    @torch.no_grad()
    def ema_state_dict(self, model):
        """The average under `model`'s own state_dict keys: parameters this optimizer averages come from `ema`, everything else (buffers,
        parameters without an average) is copied from the model.  Loadable with strict=True."""
        if self.ema_decay is None:
            raise RuntimeError("xvit FusedAdamW.ema_state_dict: the optimizer keeps no average (ema_decay=None)")
        by_name = dict(model.named_parameters(remove_duplicate=False))
        out = {}
        for k, v in model.state_dict().items():
            p = by_name.get(k)
            st = self.state.get(p) if p is not None else None
            out[k] = (st["ema"] if st and "ema" in st else v).detach().clone()
        return out

    # ------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """As FusedAdam.load_state_dict; a state without `ema` starts the average at the current p.  As with every torch optimizer the saved
        groups' hyper-parameters replace the current ones; a saved group that has no `lr_scale` (FusedAdam, torch.optim.AdamW) keeps the one
        this optimizer was built with."""
        scales = [g["lr_scale"] for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, s in zip(self.param_groups, scales):
            group.setdefault("lr_scale", s)


# ----------------------------------------------------------------------------------------------------------------------------
def _layer_of(name, S, L):
    """Layer id of a parameter name (see layer_decay_groups)."""
    import re
    if name.startswith("encoder."):
        name = name[len("encoder."):]
    if name in ("pos_embedding", "cls_token") or name.startswith("patch_to_embedding.") or name.startswith("embeddings."):
        return 0
    m = re.match(r"transformer\.(\d+)\.blocks\.\d+\.(\d+)\.", name)
    if m and S is not None:
        return 1 + int(m.group(1)) * (S + 1) + int(m.group(2))
    m = re.match(r"transformer\.(\d+)\.fusion\.\d+\.", name)
    if m and S is not None:
        return 1 + int(m.group(1)) * (S + 1) + S
    m = re.match(r"(?:transformer\.layers|layers)\.(\d+)\.", name)
    if m and S is None:
        return 1 + int(m.group(1))
    return L


def layer_decay_groups(model, layer_decay=0.75, weight_decay=0.05, no_decay_names=("cls_token", "pos_embedding", "mask_token")):
    """Parameter groups for layer-wise learning-rate decay (BEiT / MAE fine-tuning): one group per (layer id, decays or not) pair with
    `params`, `param_names`, `layer`, `lr_scale = layer_decay ** (L - layer)` and `weight_decay` (0 for 1-D tensors, for biases and for the
    names given).  Host-only; works on CPU models.

    Layer ids.  ModelCross with S = num_self_blocks and K = num_multi_blocks: pos_embedding, cls_token, patch_to_embedding.* -> 0;
    transformer.k.blocks.m.i.* -> 1 + k (S + 1) + i;  transformer.k.fusion.c.* -> 1 + k (S + 1) + S;  norm.*, mlp_head.* and any
    unknown name -> L = K (S + 1) + 1 (scale 1).  A MaskedVolumeModel maps its encoder.* the same way; decoder, mask token and
    prediction head get L.  ModelVIT and the model.py Encoder: embedding 0, block i -> 1 + i, head L = depth + 1."""
    import re
    if not (0 < layer_decay and math.isfinite(layer_decay)) or weight_decay < 0:
        raise ValueError("layer_decay must be a positive finite number and weight_decay >= 0")
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    S = K = depth = None
    for k, _ in named:
        m = re.match(r"(?:encoder\.)?transformer\.(\d+)\.blocks\.\d+\.(\d+)\.", k)
        if m:
            K, S = max(K or 0, int(m.group(1)) + 1), max(S or 0, int(m.group(2)) + 1)
        m = re.match(r"(?:encoder\.)?transformer\.(\d+)\.fusion\.", k)
        if m:
            K, S = max(K or 0, int(m.group(1)) + 1), S or 0
        m = re.match(r"(?:encoder\.)?(?:transformer\.layers|layers)\.(\d+)\.", k)
        if m:
            depth = max(depth or 0, int(m.group(1)) + 1)
    L = K * (S + 1) + 1 if K is not None else (depth or 0) + 1
    groups, seen = {}, {}
    for k, p in named:
        if id(p) in seen:
            raise ValueError(f"layer_decay_groups: {k} and {seen[id(p)]} are the same parameter: it would land in two groups")
        seen[id(p)] = k
        layer = _layer_of(k, S if K is not None else None, L)
        plain = p.dim() <= 1 or k.endswith(".bias") or k.split(".")[-1] in no_decay_names
        g = groups.setdefault((layer, plain), dict(params=[], param_names=[], layer=layer, lr_scale=float(layer_decay) ** (L - layer),
                                                   weight_decay=0.0 if plain else float(weight_decay)))
        g["params"].append(p); g["param_names"].append(k)
    return [groups[k] for k in sorted(groups)]
