"""Data-parallel gradient reduction for the hot path: one process per GPU, batch sharded across
ranks, ONE exchange step per iteration — the mean of all parameter gradients (SURVEY.md §8(e);
the reference gets this implicitly from Lightning's DDP, main_mist.py:211-218).

Design for xGMI (point-to-point links, per-link-bound rings): few, large buckets (32 MiB fp32 by
default -> 12 collectives for the 93 M-parameter config) filled in the order gradients become
ready during backward (reverse registration order: heads -> last MultiScaleBlock -> ... -> the
shared patch embedding last).  When the last gradient of a bucket has been accumulated its
all-reduce is issued immediately on a SIDE stream behind an event, so RCCL traffic overlaps the
rest of backward; `finish()` makes the compute stream wait for the tail.  After `finish()` every
`p.grad` is a view into its bucket (no copy back).  One backward per `finish()`: a second gradient for a
parameter (or for a bucket already on the wire) in the same round is refused, not dropped.

No pack pass for the weight matrices: `grad_sink()` maps every 2-D parameter (by the address of the fp32 master and of
its bf16 operand copy) to its bucket view, and with `xvit.functional.GRAD_SINK` set to it the weight-gradient kernels
write straight into the buckets (the gradient autograd hands on IS the view); the 1/world of the mean rides on the
collective itself (ReduceOp.AVG on RCCL).  What is left to copy are the 1-D gradients (biases, norms: 0.3 % of the bytes).
The sink's rule in eager mode: a view is handed out only while its parameter has NO .grad.  A kept p.grad (zeroed in place, or
accumulating over several backward + finish() rounds) IS the view after finish(); a kernel writing there would make AccumulateGrad add
the view to itself.  The kernel then gets a fresh tensor, autograd adds it into the view, and p.grad = reduce(p.grad_old + g_local) as
with plain autograd.

With a captured step (`xvit.graph.GraphedStep(model, img, labels, reducer=...)`) the same logic runs from TENSOR hooks on
the step's leaf aliases while the graph is being captured, so the bucket all-reduces become nodes of the graph, forked
onto the comm stream behind the events of their last gradients and joined before the graph ends: a replay launches the
whole step, collectives included, and they overlap the rest of the captured backward exactly as in the eager form.

The class is device-agnostic (CPU tensors + gloo skip the stream logic), which is what the
world_size-2 tests in tests/test_ddp_gloo.py run.

Wire format (`comm_dtype`, default from XVIT_GRAD_COMM = fp32 | bf16; fp32 when unset).  fp32 is the path described above.  bf16
halves the bytes on the links: each bucket also owns a bf16 buffer of the same slot layout (bucket boundaries are planned in fp32
bytes either way, so they are identical in both formats).  On the comm stream, behind the same events, one pack launch per bucket
(xvit_grad_pack_bf16: 32 segments per launch) reads every gradient of the bucket (its fp32 view, or the separate 1-D p.grad) and writes
bf16(g * scale) with zeroed slot padding; the all-reduce runs on the bf16 buffer; a second side stream (unpack_stream) waits for the
collective and xvit_grad_unpack_bf16 writes the result back into the fp32 bucket; finish() waits for that unpack.  p.grad are the fp32
bucket views exactly as in fp32 mode.
Numerics: each rank's gradient is rounded to bf16 once (relative error <= 2^-8, the unit round-off of an 8-bit significand); RCCL
then sums in bf16, which can add up to W - 1 further roundings on a ring of W ranks.  This is the contract of DDP's
bf16_compress_hook.  On the CPU (gloo, no AVG) the same steps run as torch casts: pre-scale by 1/world and round in the pack, SUM,
widen in finish().
"""
from __future__ import annotations

import os

import torch
import torch.distributed as dist

from . import ops

_COMM_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def comm_dtype_from(comm_dtype=None):
    """The reducer's wire dtype: torch.float32 or torch.bfloat16 as given, or (None) from XVIT_GRAD_COMM (fp32, the default, or bf16)."""
    if comm_dtype is None:
        env = os.environ.get("XVIT_GRAD_COMM", "") or "fp32"
        if env not in _COMM_DTYPES:
            raise ValueError(f"XVIT_GRAD_COMM={env!r}: expected one of {sorted(_COMM_DTYPES)}")
        return _COMM_DTYPES[env]
    if isinstance(comm_dtype, torch.dtype) and comm_dtype in (torch.float32, torch.bfloat16):
        return comm_dtype
    raise ValueError(f"comm_dtype={comm_dtype!r}: expected None, torch.float32 or torch.bfloat16")


class _Bucket:
    __slots__ = ("params", "flat", "views", "offsets", "wire", "done", "pending", "seen", "work", "launched", "events", "waited")

    def __init__(self, params, device, comm_dtype=torch.float32):
        self.params = params
        slot = lambda p: (p.numel() + 63) // 64 * 64          # noqa: E731 — every view starts on a 256-byte boundary: kernels write into them (16-byte stores)
        self.flat = torch.zeros(sum(slot(p) for p in params), dtype=torch.float32, device=device)
        self.views, self.offsets, o = [], [], 0
        for p in params:
            self.views.append(self.flat[o:o + p.numel()].view_as(p))
            self.offsets.append(o)
            o += slot(p)
        # bf16 wire format: the communication buffer (same slot layout) and, on the GPU, the event of its unpack (unpack_stream)
        self.wire = torch.zeros(self.flat.numel(), dtype=comm_dtype, device=device) if comm_dtype != torch.float32 else None
        self.done = torch.cuda.Event() if self.wire is not None and device.type == "cuda" else None
        self.pending, self.work, self.launched = len(params), None, False
        self.seen = set()     # id(p) of the parameters whose gradient has arrived since the last finish()
        self.events = {}      # stream id -> (stream, event): the latest gradient write of this bucket on each stream; emptied by finish()
        self.waited = 0       # how many of them the last launch waited for


def plan_buckets(params, bucket_bytes: int):
    """Partition `params` into buckets of >= bucket_bytes fp32 (the last one may be smaller), walking the list in
    REVERSE registration order — approximately the order backward produces the gradients.  For ModelCross that is
    heads -> final norms -> transformer.1 -> transformer.0 -> the shared cls_token / patch_to_embedding / pos_embedding
    last (their gradients are complete only after the embed backward of every modality)."""
    buckets, cur, size = [], [], 0
    for p in reversed(list(params)):
        cur.append(p)
        size += p.numel() * 4
        if size >= bucket_bytes:
            buckets.append(cur)
            cur, size = [], 0
    if cur:
        buckets.append(cur)
    return buckets


class GradSink(dict):
    """{address of a weight matrix (fp32 master or bf16 operand copy) -> its bucket view}, plus the owner of every view: what
    BucketedGradReducer.grad_sink() returns and xvit.functional._grad_out reads."""

    def __init__(self, reducer):
        super().__init__()
        self.reducer = reducer
        self.owner = {}       # view address -> parameter

    def free(self, view) -> bool:
        """May a weight-gradient kernel write into `view` now?  Captured step: always (p.grad IS the view by design, the step takes its
        gradients with autograd.grad).  Eager: only while the owner has no .grad, else AccumulateGrad would add the view to itself."""
        return self.reducer._graph_mode or self.owner[view.data_ptr()].grad is None


class BucketedGradReducer:
    """comm_dtype: the wire format of the all-reduces, torch.float32 or torch.bfloat16; None reads XVIT_GRAD_COMM (module docstring).
    bf16: each rank's gradient is rounded to bf16 once (relative error <= 2^-8) and RCCL sums in bf16, up to W - 1 further roundings
    on a ring of W ranks — the contract of DDP's bf16_compress_hook.  p.grad, the optimizer and the gradient sink see fp32 either way."""

    def __init__(self, params, process_group=None, bucket_bytes: int = 32 << 20, broadcast: bool = True, comm_dtype=None):
        self.comm_dtype = comm_dtype_from(comm_dtype)
        self.group = process_group
        self.world = dist.get_world_size(process_group)
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("no parameters to reduce")
        self.device = params[0].device
        self.cuda = self.device.type == "cuda"
        self.comm_stream = torch.cuda.Stream(device=self.device) if self.cuda else None
        self.unpack_stream = torch.cuda.Stream(device=self.device) if self.cuda and self.comm_dtype != torch.float32 else None
        if broadcast:  # replicas start identical (DDP does the same at wrap time)
            for p in params:
                dist.broadcast(p.data, src=dist.get_global_rank(process_group, 0) if process_group is not None else 0, group=process_group)
        self.buckets = [_Bucket(ps, self.device, self.comm_dtype) for ps in plan_buckets(params, bucket_bytes)]
        self._bucket_of = {id(p): b for b in self.buckets for p in b.params}
        self._view_of = {id(p): v for b in self.buckets for p, v in zip(b.params, b.views)}
        self._hooks = [p.register_post_accumulate_grad_hook(self._on_grad) for p in params]
        self.exposed_launches = 0
        self._avg = self.cuda and dist.get_backend(process_group) == "nccl"     # RCCL applies the 1/world itself; gloo has no AVG
        self._graph_mode = False

    def grad_sink(self, model=None):
        """{address -> bucket view} for every weight matrix: its fp32 master and, when `model` keeps a flat bf16 operand copy
        (ModelCross: xvit.functional.FlatWeights), that copy's view.  Assign to xvit.functional.GRAD_SINK.  In eager mode a view is
        handed out only while its parameter has no .grad (GradSink.free; module docstring)."""
        sink = GradSink(self)
        for b in self.buckets:
            for p, v in zip(b.params, b.views):
                if p.dim() == 2:
                    sink[p.data_ptr()] = v
                    sink.owner[v.data_ptr()] = p
        flat = getattr(model, "_flat", None) if model is not None else None
        if flat is not None:
            for p, v16 in zip(flat.params, flat.view16):
                v = self._view_of.get(id(p))
                if v is not None:
                    sink[v16.data_ptr()] = v
                    sink.owner[v.data_ptr()] = p
        return sink

    # ---- per-gradient hook (runs inside backward) ----------------------------------------------
    def _on_grad(self, p):
        b = self._bucket_of[id(p)]
        if b.launched or id(p) in b.seen:
            raise RuntimeError("BucketedGradReducer: a second gradient arrived for a " + ("bucket whose all-reduce has already been issued" if b.launched else
                               "parameter") + " in this round, so it would never be reduced. Call finish() after every backward (gradient accumulation: "
                               "one finish() per backward, keeping p.grad)")
        b.seen.add(id(p))
        if self.cuda:
            # The model's modality branches and fusions run on their own streams, and autograd replays each backward node
            # on the stream of its forward, so the gradients of ONE bucket are written on several streams.  The hook runs
            # with the stream that produced p.grad current: (re-)record that stream's event; _launch waits for all of them.
            st = torch.cuda.current_stream(self.device)
            ent = b.events.get(st.cuda_stream)
            if ent is None:
                ent = b.events[st.cuda_stream] = (st, torch.cuda.Event())
            ent[1].record(st)
        b.pending -= 1
        if b.pending == 0 and not b.launched:
            self._launch(b)

    # ---- captured step: the same bookkeeping from tensor hooks on the step's leaf aliases (xvit.graph.GraphedStep) -----------
    def attach_leaves(self, leaves):
        """`leaves`: [(parameter, alias tensor the captured step differentiates)].  Returns hook handles.  Each alias gradient is
        moved into its bucket view (a no-op for the weight matrices written there by the kernels) and counted like p.grad."""
        handles = []
        for p, a in leaves:
            def hook(g, p=p):
                v = self._view_of[id(p)]
                if g.data_ptr() != v.data_ptr():
                    v.copy_(g)
                self._on_grad(p)
                return None
            handles.append(a.register_hook(hook))
        return handles

    def drain(self):
        """Block until the process group's watchdog has retired every collective issued so far (RCCL).  It polls their events from its
        own thread, and an event query while a graph is being captured aborts the process (hipErrorStreamCaptureUnsupported): the
        captured step (xvit.graph.GraphedStep) calls this between its eager warm-up and the capture.  gloo keeps no such list."""
        if self.cuda and dist.get_backend(self.group) == "nccl":
            (self.group if self.group is not None else dist.group.WORLD)._wait_for_pending_works()

    def set_graph_mode(self, on: bool):
        """While True the gradients are taken to sit in the bucket views already (attach_leaves put them there) and p.grad is not read."""
        self._graph_mode = bool(on)

    def _launch(self, b):
        b.launched = True
        if self._graph_mode:
            grads = list(b.views)
        else:
            grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in b.params]
        scale = 1.0 / self.world
        if self.cuda:
            cur = torch.cuda.current_stream(self.device)
            ent = b.events.get(cur.cuda_stream)        # the zero-filled stand-ins above / a launch from finish() are on `cur`
            if ent is None:
                ent = b.events[cur.cuda_stream] = (cur, torch.cuda.Event())
            ent[1].record(cur)
            with torch.cuda.stream(self.comm_stream):
                for _, ev in b.events.values():        # every stream that wrote one of this bucket's gradients
                    self.comm_stream.wait_event(ev)
                b.waited = len(b.events)
                if not torch.cuda.is_current_stream_capturing():
                    for g in grads:                    # allocated on a branch stream, last read here
                        g.record_stream(self.comm_stream)
                op = dist.ReduceOp.AVG if self._avg else dist.ReduceOp.SUM
                if b.wire is None:
                    self._pack(b, grads, None if self._avg else scale)
                    b.work = dist.all_reduce(b.flat, op=op, group=self.group, async_op=True)
                else:
                    self._pack_wire(b, grads, 1.0 if self._avg else scale)
                    b.work = dist.all_reduce(b.wire, op=op, group=self.group, async_op=True)
            if b.wire is not None:
                # the unpack waits for the collective on a stream of its own: the comm stream cannot wait on the collective's stream,
                # which waits on the comm stream: with two forked streams waiting on each other the capture crashed
                with torch.cuda.stream(self.unpack_stream):
                    b.work.wait()
                    ops.grad_unpack_bf16(b.wire, b.flat)
                    b.done.record(self.unpack_stream)
        elif b.wire is None:
            self._pack(b, grads, scale)
            b.work = dist.all_reduce(b.flat, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        else:
            wire = [b.wire[o:o + g.numel()].view_as(g) for g, o in zip(grads, b.offsets)]
            torch._foreach_copy_(wire, torch._foreach_mul(grads, scale))    # bf16(g / world): the same rounding as the GPU pack
            b.work = dist.all_reduce(b.wire, op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    @staticmethod
    def _pack(b, grads, scale):
        """Gradients that are not in their bucket view yet (1-D ones; every one without a GRAD_SINK) are copied there; `scale` is
        the 1/world of the mean where the collective cannot apply it itself."""
        srcs = [g for g, v in zip(grads, b.views) if g.data_ptr() != v.data_ptr()]
        dsts = [v for g, v in zip(grads, b.views) if g.data_ptr() != v.data_ptr()]
        if srcs:
            torch._foreach_copy_(dsts, srcs)
        if scale is not None:
            b.flat.mul_(scale)

    @staticmethod
    def _pack_wire(b, grads, scale):
        """bf16 wire buffer <- bf16(g * scale) for every gradient of the bucket, slot padding zeroed, in one launch per 32 gradients.
        The kernel reads a gradient where it is (its bucket view, or a separate contiguous, 16-byte aligned fp32 p.grad); any other
        layout is first copied into its view."""
        segs = []
        for g, v, o in zip(grads, b.views, b.offsets):
            if g.data_ptr() != v.data_ptr() and not (g.dtype == torch.float32 and g.is_contiguous() and g.data_ptr() % 16 == 0):
                v.copy_(g)
                g = v
            segs.append((g, o))
        ops.grad_pack_bf16(segs, b.wire, scale)

    # ---- after backward ------------------------------------------------------------------------
    def finish(self):
        """Wait (stream-side on GPU) for every bucket and point p.grad at the reduced values."""
        for b in self.buckets:
            if not b.launched:  # some gradient never arrived (unused parameter): reduce zeros for it
                self.exposed_launches += 1
                self._launch(b)
        for b in self.buckets:
            if b.done is not None:     # bf16 on the GPU: the current stream waits for the unpack behind the collective
                torch.cuda.current_stream(self.device).wait_event(b.done)
            else:
                b.work.wait()  # NCCL/RCCL: the current stream waits; gloo: the host waits
                if b.wire is not None:
                    b.flat.copy_(b.wire)
            for p, v in zip(b.params, b.views):
                p.grad = v
            b.pending, b.work, b.launched = len(b.params), None, False
            b.seen.clear()
            b.events.clear()   # the collective is behind them; events of a captured round must never be waited for by an eager one

    def zero_grad(self):
        """Drop gradients (set_to_none semantics) so the next backward writes fresh tensors."""
        for b in self.buckets:
            for p in b.params:
                p.grad = None

    def remove(self):
        for h in self._hooks:
            h.remove()
