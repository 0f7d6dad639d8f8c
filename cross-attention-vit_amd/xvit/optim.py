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


class _Entry:
    """The static launch arguments of one parameter group in capturable mode."""
    __slots__ = ("gi", "params", "idx", "table", "chunks", "n_chunks", "off", "p_ptrs", "g_ptrs", "rec", "lr_view", "lr")


class FusedAdam(torch.optim.Optimizer):
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
        self._entries = None          # capturable mode: built by prepare()
        self._records = self._partials = self._last_norm = None
        self._touched, self._unshadowed = [], []

    @staticmethod
    def _shadow_of(p):
        for grp in XF.SHADOWS.groups:
            i = grp.index.get(id(p))
            if i is not None and grp.params[i] is p and grp.intact():
                return grp, grp.view16[i]
        return None, None

    @staticmethod
    def _validate(p):
        if not p.is_cuda or p.dtype != torch.float32 or p.grad.dtype != torch.float32 or p.grad.is_sparse:
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

    def _describe(self, e, i):
        names = self.param_groups[e.gi].get("param_names")
        p = e.params[i]
        return f"parameter {e.idx[i]} of group {e.gi}" + (f" ({names[e.idx[i]]})" if names else "") + f", shape {tuple(p.shape)}"

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

    # ------------------------------------------------------------------------------------------------------------------------
    # eager mode: tables per step, as the step count is kept per parameter on the host
    # ------------------------------------------------------------------------------------------------------------------------
    def _step_eager(self, lib):
        touched, unshadowed, launches = {}, [], []
        for group in self.param_groups:
            buckets, keep = {}, []          # step count -> (rows, chunks): torch keeps the step per parameter
            for p in group["params"]:
                if p.grad is None:
                    continue
                self._validate(p)
                st = self._state_of(p)
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                grp, sh = self._shadow_of(p)
                if grp is not None:
                    touched[id(grp)] = grp
                else:
                    unshadowed.append(p)
                keep.append(g)
                rows, chunks = buckets.setdefault(st["step"], ([], []))
                t = len(rows)
                rows.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                             sh.data_ptr() if sh is not None else 0, p.numel()))
                chunks.extend((t, c) for c in range((p.numel() + CHUNK - 1) // CHUNK))
            launches.extend((group, step, rows, chunks, keep) for step, (rows, chunks) in buckets.items())
        if self.max_grad_norm is None:
            for group, step, rows, chunks, _ in launches:
                b1, b2 = group["betas"]
                dev = group["params"][0].device
                table = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev, non_blocking=True)
                chunk_t = torch.from_numpy(np.asarray(chunks, dtype=np.int32)).to(dev, non_blocking=True)
                _lib.check(lib.xvit_adam_step(table.data_ptr(), chunk_t.data_ptr(), len(chunks), float(group["lr"]), b1, b2, group["eps"],
                                              group["weight_decay"], step, 1.0, torch.cuda.current_stream().cuda_stream), "xvit_adam_step")
                table.record_stream(torch.cuda.current_stream()); chunk_t.record_stream(torch.cuda.current_stream())
        elif launches:
            # norm over ALL groups and step buckets -> one prologue per bucket (its own step count and learning rate) -> Adam
            dev = launches[0][0]["params"][0].device
            cur = torch.cuda.current_stream()
            rec = np.zeros(len(launches), dtype=_REC_DTYPE)
            rec["step"] = [step - 1 for _, step, _, _, _ in launches]          # the prologue advances it
            rec["lr"] = [group["lr"] for group, _, _, _, _ in launches]
            records = torch.from_numpy(rec.view(np.int64).reshape(-1, _REC_WORDS)).to(dev, non_blocking=True)
            total = sum(len(chunks) for _, _, _, chunks, _ in launches)
            partials = torch.empty(total, dtype=torch.float32, device=dev)
            tables, off = [], 0
            for _, _, rows, chunks, _ in launches:
                table = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev, non_blocking=True)
                chunk_t = torch.from_numpy(np.asarray(chunks, dtype=np.int32)).to(dev, non_blocking=True)
                _lib.check(lib.xvit_grad_sqnorm_partials(table.data_ptr(), chunk_t.data_ptr(), len(chunks), partials.data_ptr() + 4 * off,
                                                         cur.cuda_stream), "xvit_grad_sqnorm_partials")
                tables.append((table, chunk_t))
                off += len(chunks)
            for k, ((group, _, _, chunks, _), (table, chunk_t)) in enumerate(zip(launches, tables)):
                b1, b2 = group["betas"]
                state_ptr = records.data_ptr() + 8 * _REC_WORDS * k
                _lib.check(lib.xvit_adam_prologue(partials.data_ptr(), total, state_ptr, self.max_grad_norm, b1, b2, 0, cur.cuda_stream), "xvit_adam_prologue")
                _lib.check(lib.xvit_adam_step_dev(table.data_ptr(), chunk_t.data_ptr(), len(chunks), state_ptr, b1, b2, group["eps"],
                                                  group["weight_decay"], cur.cuda_stream), "xvit_adam_step_dev")
                table.record_stream(cur); chunk_t.record_stream(cur)
            records.record_stream(cur); partials.record_stream(cur)
            self._last_norm = records[0].view(torch.float32)[_F_NORM]
        self._touched = [weakref.ref(g) for g in touched.values()]
        self._unshadowed = unshadowed
        self.mark_updated()

    # ------------------------------------------------------------------------------------------------------------------------
    # capturable mode: everything built once
    # ------------------------------------------------------------------------------------------------------------------------
    def _rows_of(self, e):
        rows = []
        for p in e.params:
            st = self.state[p]
            _, sh = self._shadow_of(p)
            rows.append((p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                         sh.data_ptr() if sh is not None else 0, p.numel()))
        return rows

    @torch.no_grad()
    def prepare(self):
        """capturable=True: build the device tables, chunk lists, norm partials and state records from the parameters that have a
        gradient NOW (allocation + host-to-device copies: not capturable, so call it, or take one eager step, before a capture).
        Later calls do nothing."""
        if not self.capturable:
            raise RuntimeError("xvit FusedAdam.prepare: only for capturable=True")
        if self._entries is not None:
            return
        entries, touched, unshadowed, off = [], {}, [], 0
        for gi, group in enumerate(self.param_groups):
            e = _Entry()
            e.gi, e.params, e.idx = gi, [], []
            chunks, steps = [], set()
            for i, p in enumerate(group["params"]):
                if p.grad is None:
                    continue
                self._validate(p)
                if not p.grad.is_contiguous():
                    raise RuntimeError("xvit FusedAdam(capturable=True): non-contiguous gradient")
                steps.add(int(self._state_of(p)["step"]))
                grp, _ = self._shadow_of(p)
                if grp is not None:
                    touched[id(grp)] = grp
                else:
                    unshadowed.append(p)
                chunks.extend((len(e.params), c) for c in range((p.numel() + CHUNK - 1) // CHUNK))
                e.params.append(p); e.idx.append(i)
            if not e.params:
                continue
            if len(steps) != 1:
                raise ValueError(f"xvit FusedAdam(capturable=True) keeps one step count per parameter group; group {gi} holds parameters at steps {sorted(steps)}")
            dev = e.params[0].device
            e.lr = float(group["lr"])
            e.n_chunks, e.off = len(chunks), off
            off += len(chunks)
            e.chunks = torch.from_numpy(np.asarray(chunks, dtype=np.int32)).to(dev)
            e.table = torch.empty(len(e.params), 6, dtype=torch.int64, device=dev)
            entries.append((e, steps.pop()))
        if not entries:
            raise RuntimeError("xvit FusedAdam.prepare: no parameter has a gradient yet (run one backward, or set the static .grad buffers, first)")
        rec = np.zeros(len(entries), dtype=_REC_DTYPE)
        rec["step"] = [step for _, step in entries]
        rec["lr"] = [e.lr for e, _ in entries]
        dev = entries[0][0].table.device
        self._records = torch.from_numpy(rec.view(np.int64).reshape(-1, _REC_WORDS)).to(dev)
        self._partials = torch.empty(off, dtype=torch.float32, device=dev) if self._needs_norm else None
        for k, (e, _) in enumerate(entries):
            e.rec = self._records[k]
            e.lr_view = e.rec.view(torch.float32)[_F_LR]
        self._entries = [e for e, _ in entries]
        self._last_norm = self._records[0].view(torch.float32)[_F_NORM] if self._needs_norm else None
        self._touched = [weakref.ref(g) for g in touched.values()]
        self._unshadowed = unshadowed
        self.rebind()

    @torch.no_grad()
    def rebind(self):
        """Re-read the addresses of the parameters, their CURRENT .grad tensors and bf16 copies into the existing device tables (a
        host-to-device copy: outside any capture).  The launches hold only the tables' own addresses, so a graph captured before stays
        valid: xvit.graph.GraphedStep captures the step first and binds the gradient buffers the capture allocated afterwards."""
        for e in self._entries:
            for i, p in enumerate(e.params):
                if p.grad is None or p.grad.shape != p.shape or not p.grad.is_contiguous() or p.grad.dtype != torch.float32:
                    raise RuntimeError(f"xvit FusedAdam.rebind: {self._describe(e, i)} has no dense contiguous fp32 gradient to bind")
            rows = self._rows_of(e)
            e.table.copy_(torch.from_numpy(np.asarray(rows, dtype=np.int64)))
            e.p_ptrs = [r[0] for r in rows]
            e.g_ptrs = [r[1] for r in rows]

    def check_addresses(self, grads: bool = True):
        """capturable mode: every parameter (and, with grads=True, its .grad) still lives at the address in the device table."""
        for e in self._entries or ():
            for i, p in enumerate(e.params):
                if p.data_ptr() != e.p_ptrs[i]:
                    raise RuntimeError(f"xvit FusedAdam(capturable=True): the storage of {self._describe(e, i)} moved after the tables were built "
                                       "(model.to(...), a re-built flat weight buffer); build a new optimizer")
                if grads and (p.grad is None or p.grad.data_ptr() != e.g_ptrs[i]):
                    raise RuntimeError(f"xvit FusedAdam(capturable=True): the gradient of {self._describe(e, i)} is no longer the tensor the device table "
                                       "points to (typically zero_grad(set_to_none=True) in an eager loop, which makes backward allocate a new one): "
                                       "use zero_grad(set_to_none=False), or xvit.graph.GraphedStep(..., optimizer=opt), which owns static gradient buffers")

    def sync_lr(self):
        """Write group["lr"] into the device record of every group whose rate changed since the last call (one tiny asynchronous fill
        on the current stream, value passed as a kernel argument: no host buffer to keep alive); nothing is issued otherwise.  step()
        calls it in eager mode, GraphedStep before each replay; call it yourself before replaying your own capture of step()."""
        for e in self._entries or ():
            lr = float(self.param_groups[e.gi]["lr"])
            if lr != e.lr:
                e.lr_view.fill_(lr)
                e.lr = lr
                self.lr_copies += 1

    def enqueue(self):
        """capturable mode: the launches of one step on the current stream and nothing else (no check, no bookkeeping)."""
        lib = _lib.load()
        stream = ops._stream()
        if self._partials is not None:
            for e in self._entries:
                _lib.check(lib.xvit_grad_sqnorm_partials(e.table.data_ptr(), e.chunks.data_ptr(), e.n_chunks, self._partials.data_ptr() + 4 * e.off, stream),
                           "xvit_grad_sqnorm_partials")
        part, n_part = (self._partials.data_ptr(), self._partials.numel()) if self._partials is not None else (None, 0)
        max_norm = self.max_grad_norm if self.max_grad_norm is not None else math.inf
        for e in self._entries:
            group = self.param_groups[e.gi]
            b1, b2 = group["betas"]
            _lib.check(lib.xvit_adam_prologue(part, n_part, e.rec.data_ptr(), max_norm, b1, b2, int(self.skip_nonfinite), stream), "xvit_adam_prologue")
            _lib.check(lib.xvit_adam_step_dev(e.table.data_ptr(), e.chunks.data_ptr(), e.n_chunks, e.rec.data_ptr(), b1, b2, group["eps"],
                                              group["weight_decay"], stream), "xvit_adam_step_dev")

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
        """exp_avg / exp_avg_sq / step per parameter, as torch.optim.Adam names them.  In capturable mode `step` is read from the
        device counters here (a synchronisation)."""
        if self._entries is not None:
            steps = self._records[:, 0].tolist()
            for e, step in zip(self._entries, steps):
                for p in e.params:
                    self.state[p]["step"] = int(step)
        return super().state_dict()

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Accepts a state dict of either mode (or of torch.optim.Adam).  Once the capturable tables exist, the values are copied INTO the
        existing moment buffers and device counters, so a captured graph stays valid."""
        old = {p: self.state[p] for e in self._entries or () for p in e.params}
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if "step" in st:
                st["step"] = int(st["step"])
        for k, e in enumerate(self._entries or ()):
            steps = set()
            for i, p in enumerate(e.params):
                new = self.state.get(p)
                if not new or "exp_avg" not in new:
                    raise ValueError(f"xvit FusedAdam.load_state_dict: no state for {self._describe(e, i)}, which the capturable tables hold")
                keep = old[p]
                keep["exp_avg"].copy_(new["exp_avg"])
                keep["exp_avg_sq"].copy_(new["exp_avg_sq"])
                keep["step"] = new["step"]
                steps.add(new["step"])
                self.state[p] = keep
            if len(steps) != 1:
                raise ValueError(f"xvit FusedAdam(capturable=True) keeps one step count per parameter group; the loaded state has steps {sorted(steps)} in group {e.gi}")
            self._records[k, 0].fill_(steps.pop())


# ============================================================================================================================
# AdamW with layer-wise rates and a fused weight EMA
# ============================================================================================================================
# struct xvit_adamw_extra (include/xvit.h): one row per row of the tensor table
_EXTRA_DTYPE = np.dtype([("ema", "<u8"), ("lr_scale", "<f4"), ("weight_decay", "<f4")])
assert _EXTRA_DTYPE.itemsize == 16


class _Set(_Entry):
    """The static launch arguments of one launch set in capturable mode: every group that agrees on betas, eps and step count."""
    __slots__ = ("groups", "gis", "extras", "extras_host", "seen")


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

    def _ema_weight(self, step):
        """The weight the record path forms on the device, in the same fp32 arithmetic."""
        if self.ema_decay is None:
            return 1.0
        d = np.float32(self.ema_decay)
        if self.ema_warmup:
            t = np.float32(step)
            d = min(d, (np.float32(1) + t) / (np.float32(10) + t))
        return float(np.float32(1) - d)

    def _describe(self, e, i):
        gi = e.gis[i]
        names = self.param_groups[gi].get("param_names")
        p = e.params[i]
        return f"parameter {e.idx[i]} of group {gi}" + (f" ({names[e.idx[i]]})" if names else "") + f", shape {tuple(p.shape)}"

    @staticmethod
    def _extras_of(params, states, scales, decays, with_ema):
        x = np.zeros(len(params), dtype=_EXTRA_DTYPE)
        x["ema"] = [states[p]["ema"].data_ptr() if with_ema else 0 for p in params]
        x["lr_scale"], x["weight_decay"] = scales, decays
        return x

    @staticmethod
    def _upload(x, dev):
        return torch.from_numpy(x.view(np.int64).reshape(-1, 2)).to(dev, non_blocking=True)

    # ------------------------------------------------------------------------------------------------------------------------
    # eager mode
    # ------------------------------------------------------------------------------------------------------------------------
    def _step_eager(self, lib):
        touched, unshadowed, sets = {}, [], {}
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                self._validate(p)
                st = self._state_of(p)
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                grp, sh = self._shadow_of(p)
                if grp is not None:
                    touched[id(grp)] = grp
                else:
                    unshadowed.append(p)
                s = sets.setdefault(self._key(group, st["step"]), dict(group=group, step=st["step"], gis=[], params=[], rows=[], chunks=[], keep=[]))
                t = len(s["rows"])
                s["rows"].append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), sh.data_ptr() if sh is not None else 0, p.numel()))
                s["chunks"].extend((t, c) for c in range((p.numel() + CHUNK - 1) // CHUNK))
                s["gis"].append(gi); s["params"].append(p); s["keep"].append(g)
        sets = list(sets.values())
        if not sets:
            return
        dev = sets[0]["params"][0].device
        cur = torch.cuda.current_stream()
        for s in sets:
            order = list(dict.fromkeys(s["gis"]))
            s["lr"], scales = self._rates([self.param_groups[gi] for gi in order])
            scale_of = dict(zip(order, scales))
            x = self._extras_of(s["params"], self.state, [scale_of[gi] for gi in s["gis"]], [self.param_groups[gi]["weight_decay"] for gi in s["gis"]],
                                self.ema_decay is not None)
            s["table"] = torch.from_numpy(np.asarray(s["rows"], dtype=np.int64)).to(dev, non_blocking=True)
            s["chunk_t"] = torch.from_numpy(np.asarray(s["chunks"], dtype=np.int32)).to(dev, non_blocking=True)
            s["extras"] = self._upload(x, dev)
        if self.max_grad_norm is None:
            for s in sets:
                b1, b2 = s["group"]["betas"]
                _lib.check(lib.xvit_adamw_step(s["table"].data_ptr(), s["extras"].data_ptr(), s["chunk_t"].data_ptr(), len(s["chunks"]), s["lr"], b1, b2,
                                               s["group"]["eps"], s["step"], 1.0, int(self.decoupled), self._ema_weight(s["step"]), cur.cuda_stream), "xvit_adamw_step")
        else:
            rec = np.zeros(len(sets), dtype=_REC_DTYPE)
            rec["step"] = [s["step"] - 1 for s in sets]          # the prologue advances it
            rec["lr"] = [s["lr"] for s in sets]
            records = torch.from_numpy(rec.view(np.int64).reshape(-1, _REC_WORDS)).to(dev, non_blocking=True)
            total = sum(len(s["chunks"]) for s in sets)
            partials = torch.empty(total, dtype=torch.float32, device=dev)
            off = 0
            for s in sets:
                _lib.check(lib.xvit_grad_sqnorm_partials(s["table"].data_ptr(), s["chunk_t"].data_ptr(), len(s["chunks"]), partials.data_ptr() + 4 * off,
                                                         cur.cuda_stream), "xvit_grad_sqnorm_partials")
                off += len(s["chunks"])
            for k, s in enumerate(sets):
                b1, b2 = s["group"]["betas"]
                state_ptr = records.data_ptr() + 8 * _REC_WORDS * k
                _lib.check(lib.xvit_adam_prologue(partials.data_ptr(), total, state_ptr, self.max_grad_norm, b1, b2, 0, cur.cuda_stream), "xvit_adam_prologue")
                _lib.check(lib.xvit_adamw_step_dev(s["table"].data_ptr(), s["extras"].data_ptr(), s["chunk_t"].data_ptr(), len(s["chunks"]), state_ptr, b1, b2,
                                                   s["group"]["eps"], int(self.decoupled), self.ema_decay or 0.0, int(self.ema_warmup), cur.cuda_stream),
                           "xvit_adamw_step_dev")
            records.record_stream(cur); partials.record_stream(cur)
            self._last_norm = records[0].view(torch.float32)[_F_NORM]
        for s in sets:
            for t in (s["table"], s["chunk_t"], s["extras"]):
                t.record_stream(cur)
        self._touched = [weakref.ref(g) for g in touched.values()]
        self._unshadowed = unshadowed
        self.mark_updated()

    # ------------------------------------------------------------------------------------------------------------------------
    # capturable mode
    # ------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prepare(self):
        """capturable=True: build the device tables of every launch set from the parameters that have a gradient NOW (allocation +
        host-to-device copies: call it, or take one eager step, before a capture).  Later calls do nothing."""
        if not self.capturable:
            raise RuntimeError("xvit FusedAdamW.prepare: only for capturable=True")
        if self._entries is not None:
            return
        sets, touched, unshadowed = {}, {}, []
        for gi, group in enumerate(self.param_groups):
            for i, p in enumerate(group["params"]):
                if p.grad is None:
                    continue
                self._validate(p)
                if not p.grad.is_contiguous():
                    raise RuntimeError("xvit FusedAdamW(capturable=True): non-contiguous gradient")
                step = int(self._state_of(p)["step"])
                grp, _ = self._shadow_of(p)
                if grp is not None:
                    touched[id(grp)] = grp
                else:
                    unshadowed.append(p)
                key = self._key(group, step)
                if key not in sets:
                    e = sets[key] = _Set()
                    e.gi, e.params, e.idx, e.gis, e.chunks = gi, [], [], [], []
                e = sets[key]
                e.chunks.extend((len(e.params), c) for c in range((p.numel() + CHUNK - 1) // CHUNK))
                e.params.append(p); e.idx.append(i); e.gis.append(gi)
        if not sets:
            raise RuntimeError("xvit FusedAdamW.prepare: no parameter has a gradient yet (run one backward, or set the static .grad buffers, first)")
        entries, off = list(sets.values()), 0
        dev = entries[0].params[0].device
        rec = np.zeros(len(entries), dtype=_REC_DTYPE)
        for k, (key, e) in enumerate(sets.items()):
            e.groups = list(dict.fromkeys(e.gis))
            e.n_chunks, e.off = len(e.chunks), off
            off += e.n_chunks
            e.chunks = torch.from_numpy(np.asarray(e.chunks, dtype=np.int32)).to(dev)
            e.table = torch.empty(len(e.params), 6, dtype=torch.int64, device=dev)
            e.lr, scales = self._rates([self.param_groups[gi] for gi in e.groups])
            scale_of = dict(zip(e.groups, scales))
            e.extras_host = self._extras_of(e.params, self.state, [scale_of[gi] for gi in e.gis], [self.param_groups[gi]["weight_decay"] for gi in e.gis],
                                            self.ema_decay is not None)
            e.extras = self._upload(e.extras_host, dev)
            e.seen = self._seen(e)
            rec["step"][k], rec["lr"][k] = key[3], e.lr
        self._records = torch.from_numpy(rec.view(np.int64).reshape(-1, _REC_WORDS)).to(dev)
        self._partials = torch.empty(off, dtype=torch.float32, device=dev) if self._needs_norm else None
        for k, e in enumerate(entries):
            e.rec = self._records[k]
            e.lr_view = e.rec.view(torch.float32)[_F_LR]
        self._entries = entries
        self._last_norm = self._records[0].view(torch.float32)[_F_NORM] if self._needs_norm else None
        self._touched = [weakref.ref(g) for g in touched.values()]
        self._unshadowed = unshadowed
        self.rebind()

    def _seen(self, e):
        return tuple((float(self.param_groups[gi]["lr"]), float(self.param_groups[gi]["lr_scale"])) for gi in e.groups)

    def sync_lr(self):
        """Bring the device in line with group["lr"] / group["lr_scale"]: while the groups of a set share one rate a change is ONE fill of the
        record (`lr_copies`); when they diverge the per-tensor scale column is rewritten with one host-to-device copy of the extras table,
        into the same addresses (`scale_copies`; a copy, so outside any capture).  Nothing is issued when nothing changed."""
        for e in self._entries or ():
            seen = self._seen(e)
            if seen == e.seen:
                continue
            e.seen = seen
            lr, scales = self._rates([self.param_groups[gi] for gi in e.groups])
            if lr != e.lr:
                e.lr_view.fill_(lr)
                e.lr = lr
                self.lr_copies += 1
            scale_of = dict(zip(e.groups, scales))
            column = np.asarray([scale_of[gi] for gi in e.gis], dtype=np.float32)
            if not np.array_equal(column, e.extras_host["lr_scale"]):
                e.extras_host["lr_scale"] = column
                e.extras.copy_(torch.from_numpy(e.extras_host.view(np.int64).reshape(-1, 2)))
                self.scale_copies += 1

    def enqueue(self):
        """capturable mode: the launches of one step on the current stream and nothing else: the gradient norm (when one is taken), then one
        prologue + step pair per launch set."""
        lib = _lib.load()
        stream = ops._stream()
        if self._partials is not None:
            for e in self._entries:
                _lib.check(lib.xvit_grad_sqnorm_partials(e.table.data_ptr(), e.chunks.data_ptr(), e.n_chunks, self._partials.data_ptr() + 4 * e.off, stream),
                           "xvit_grad_sqnorm_partials")
        part, n_part = (self._partials.data_ptr(), self._partials.numel()) if self._partials is not None else (None, 0)
        max_norm = self.max_grad_norm if self.max_grad_norm is not None else math.inf
        for e in self._entries:
            group = self.param_groups[e.gi]
            b1, b2 = group["betas"]
            _lib.check(lib.xvit_adam_prologue(part, n_part, e.rec.data_ptr(), max_norm, b1, b2, int(self.skip_nonfinite), stream), "xvit_adam_prologue")
            _lib.check(lib.xvit_adamw_step_dev(e.table.data_ptr(), e.extras.data_ptr(), e.chunks.data_ptr(), e.n_chunks, e.rec.data_ptr(), b1, b2, group["eps"],
                                               int(self.decoupled), self.ema_decay or 0.0, int(self.ema_warmup), stream), "xvit_adamw_step_dev")

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
            for e in self._entries:
                _lib.check(lib.xvit_ema_swap(e.table.data_ptr(), e.extras.data_ptr(), e.chunks.data_ptr(), e.n_chunks, cur.cuda_stream), "xvit_ema_swap")
        else:
            params = [p for g in self.param_groups for p in g["params"] if p in self.state and "ema" in self.state[p]]
            if not params:
                raise RuntimeError("xvit FusedAdamW.ema_weights: no parameter has an average yet (take a step first)")
            rows, chunks, touched, unshadowed = [], [], {}, []
            for t, p in enumerate(params):
                st = self.state[p]
                grp, sh = self._shadow_of(p)
                if grp is not None:
                    touched[id(grp)] = grp
                else:
                    unshadowed.append(p)
                rows.append((p.data_ptr(), p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), sh.data_ptr() if sh is not None else 0, p.numel()))
                chunks.extend((t, c) for c in range((p.numel() + CHUNK - 1) // CHUNK))
            dev = params[0].device
            table = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev, non_blocking=True)
            chunk_t = torch.from_numpy(np.asarray(chunks, dtype=np.int32)).to(dev, non_blocking=True)
            extras = self._upload(self._extras_of(params, self.state, 1.0, 0.0, True), dev)
            _lib.check(lib.xvit_ema_swap(table.data_ptr(), extras.data_ptr(), chunk_t.data_ptr(), len(chunks), cur.cuda_stream), "xvit_ema_swap")
            for t in (table, chunk_t, extras):
                t.record_stream(cur)
            self._touched = [weakref.ref(g) for g in touched.values()]
            self._unshadowed = unshadowed
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
        """Accepts a state dict of either mode, of FusedAdam or of torch.optim.Adam / AdamW.  Once the capturable tables exist the values are
        copied INTO the existing moment and average buffers and device counters.  A state without `ema` starts the average at the current p.
        As with every torch optimizer the saved groups' hyper-parameters replace the current ones; a saved group that has no `lr_scale` keeps the
        one this optimizer was built with."""
        old = {p: self.state[p] for e in self._entries or () for p in e.params}
        scales = [g["lr_scale"] for g in self.param_groups]
        torch.optim.Optimizer.load_state_dict(self, state_dict)
        for group, s in zip(self.param_groups, scales):
            group.setdefault("lr_scale", s)        # a saved group without one (FusedAdam, torch.optim.AdamW) keeps the constructed scale
        for p, st in self.state.items():
            if "step" in st:
                st["step"] = int(st["step"])
            if self.ema_decay is not None and "exp_avg" in st and "ema" not in st:
                st["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
        for k, e in enumerate(self._entries or ()):
            steps = set()
            for i, p in enumerate(e.params):
                new = self.state.get(p)
                if not new or "exp_avg" not in new:
                    raise ValueError(f"xvit FusedAdamW.load_state_dict: no state for {self._describe(e, i)}, which the capturable tables hold")
                keep = old[p]
                for name in ("exp_avg", "exp_avg_sq") + (("ema",) if self.ema_decay is not None else ()):
                    keep[name].copy_(new[name])
                keep["step"] = new["step"]
                steps.add(new["step"])
                self.state[p] = keep
            if len(steps) != 1:
                raise ValueError(f"xvit FusedAdamW(capturable=True) keeps one step count per launch set; the loaded state has steps {sorted(steps)} in one set")
            self._records[k, 0].fill_(steps.pop())


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
