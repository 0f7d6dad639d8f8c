"""On-device epoch statistics for the reference's log_stats (model_cross.py:243-255 -> utils.py:18-62).

The reference computes accuracy / precision / recall / specificity / F1 / NPV with torchmetrics and reads each back with
.item(), plus an AUROC, on EVERY step (seven host syncs after a step of a few tens of milliseconds), and logs them with
on_epoch=True, i.e. as batch-size-weighted epoch means.  BinaryEpochMetrics.update() is one tiny kernel launch and never
touches the host; compute() reads the 16-double state once (per epoch) and returns the same seven epoch values under the
reference's log names, plus the pooled confusion counts.

    stats = BinaryEpochMetrics(device)
    for x, y in loader:
        logits, loss = model(x, y); ...; stats.update(logits, y)       # no sync
    print(stats.compute("train"))                                      # {'train_acc': ..., 'train_auc_roc': ..., 'train_confusion': {...}}
    stats.reset()
"""
from __future__ import annotations

import math

import torch

from . import _lib, ops

KEYS = ("acc", "prec", "rec", "spec", "f1", "npv", "auc_roc")     # log-name suffixes of model_cross.py:246-255
STATE = 16


class BinaryEpochMetrics:
    def __init__(self, device):
        self.state = torch.zeros(STATE, dtype=torch.float64, device=device)

    def reset(self):
        self.state.zero_()

    @torch.no_grad()
    def update(self, logits: torch.Tensor, labels: torch.Tensor):
        if not logits.is_cuda:
            raise RuntimeError("BinaryEpochMetrics: logits must live on the GPU (there is no CPU path)")
        if logits.dim() != 2 or logits.shape[1] != 2:
            raise ValueError(f"binary classification expected, got logits of shape {tuple(logits.shape)}")
        lg = logits.detach()
        if lg.dtype != torch.float32 or lg.stride(1) != 1:
            lg = lg.float().contiguous()
        lb = labels.detach()
        if lb.dtype != torch.int64 or not lb.is_contiguous():
            lb = lb.to(torch.int64).contiguous()
        st = torch.cuda.current_stream(lg.device).cuda_stream
        _lib.check(_lib.load().xvit_binary_metrics_step(lg.data_ptr(), lg.stride(0), lb.data_ptr(), lg.shape[0], 2, self.state.data_ptr(), st),
                   "xvit_binary_metrics_step")

    def compute(self, name: str = "", sync_dist: bool = True, group=None) -> dict:
        """The epoch values (ONE host sync).  With torch.distributed initialised and sync_dist=True the state is summed
        over `group` (default: the world) first: the exact batch-size-weighted mean over all ranks, the counterpart of
        the reference's sync_dist=True."""
        s = self.state
        if sync_dist and torch.distributed.is_available() and torch.distributed.is_initialized():
            s = s.clone()
            torch.distributed.all_reduce(s, group=group)
        return summarize(s.cpu(), name)


def summarize(state: torch.Tensor, name: str = "") -> dict:
    """state (16 doubles on the host) -> {f'{name}_acc': ..., ..., f'{name}_confusion': {...}}"""
    s = state.double().tolist()
    n = s[4]
    pre = f"{name}_" if name else ""
    out = {pre + k: (s[6 + i] / n if n > 0 else 0.0) for i, k in enumerate(KEYS)}
    out[pre + "confusion"] = {"tn": int(s[0]), "fp": int(s[1]), "fn": int(s[2]), "tp": int(s[3]), "samples": int(n), "steps": int(s[5])}
    return out


CLASS_KEYS = ("prec", "rec", "spec", "f1", "npv")                 # per class (one-vs-rest) and macro-averaged
RANK_KEYS = ("auroc", "ap")                                       # per class (one-vs-rest) and macro-averaged


def epoch_metric_keys(num_classes):
    """The scalar keys of EpochMetrics.compute(), without the name prefix; with a bootstrap every one also has a `<key>_ci` pair."""
    C = int(num_classes)
    keys = ["acc", "balanced_acc"]
    for k in CLASS_KEYS + RANK_KEYS:
        keys += [f"{k}_{c}" for c in range(C)] + [f"macro_{k}"]
    return tuple(keys + (["auc_roc"] if C == 2 else []))


def gather_epoch_rows(scores, labels32, preds, n, group=None):
    """The stored rows of all ranks in rank order: (scores [N, C], labels32 [N], preds [N], N).  Counts first, then buffers padded to the
    largest count (all_gather needs equal shapes).  Device-agnostic: works on whatever device the tensors and the backend share."""
    dist = torch.distributed
    world = dist.get_world_size(group)
    count = torch.tensor([int(n)], dtype=torch.int64, device=scores.device)
    counts = [torch.zeros_like(count) for _ in range(world)]
    dist.all_gather(counts, count, group=group)
    counts = [int(c.item()) for c in counts]
    top = max(max(counts), 1)

    def gathered(t):
        pad = torch.zeros((top,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        pad[:n] = t[:n]
        parts = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(parts, pad, group=group)
        return torch.cat([p[:c] for p, c in zip(parts, counts)])

    return gathered(scores), gathered(labels32), gathered(preds), sum(counts)


def _nearest_rank(sorted_vals, q):
    """The max(1, ceil(q m))-th smallest of m sorted values, the definition xvit_volume_stats uses (q m rounded to 1e-9 before the
    ceiling, so that 0.025 * 1000 is 25)."""
    m = len(sorted_vals)
    return sorted_vals[min(max(1, math.ceil(round(q * m, 9))), m) - 1]


class EpochMetrics:
    """Pooled epoch metrics for any number of classes, with exact one-vs-rest AUROC / average precision and percentile-bootstrap
    intervals (xvit_epoch_metrics_update / xvit_epoch_rank_stats, include/xvit.h).

    update() is one launch and never touches the host: the step's softmax rows, labels and predictions are appended to device buffers
    of `capacity` rows and its confusion counts are added to an integer matrix.  compute() synchronises once, sorts every score column
    (torch.sort, plumbing), runs the rank kernel over replicate 0 (every sample once) and `bootstrap` resamples, and does float64
    arithmetic on the (R + 1) x C integer outputs only.  BinaryEpochMetrics keeps means of per-step values, as the reference logs them;
    the values here are those of the pooled epoch.

        stats = EpochMetrics(3, device, bootstrap=1000)
        for x, y in loader: ...; stats.update(logits, y)
        out = stats.compute("val")       # val_acc, val_macro_auroc, val_auroc_0, ..., val_macro_auroc_ci = (lo, hi), val_confusion, ...
    """

    def __init__(self, num_classes, device, capacity=65_535, bootstrap=0, ci=0.95, seed=0):
        if not 2 <= int(num_classes) <= _lib.EPOCH_MAX_C:
            raise ValueError(f"EpochMetrics: {num_classes} classes outside 2..{_lib.EPOCH_MAX_C}")
        if int(capacity) < 1 or int(bootstrap) < 0 or not 0.0 < float(ci) < 1.0:
            raise ValueError(f"EpochMetrics: need capacity >= 1, bootstrap >= 0 and 0 < ci < 1 (got {capacity}, {bootstrap}, {ci})")
        self.C, self.capacity, self.bootstrap, self.ci, self.seed = int(num_classes), int(capacity), int(bootstrap), float(ci), int(seed)
        self.scores = torch.empty(self.capacity, self.C, dtype=torch.float32, device=device)
        self.labels32 = torch.empty(self.capacity, dtype=torch.int32, device=device)
        self.preds = torch.empty(self.capacity, dtype=torch.int32, device=device)
        self.state = torch.zeros(_lib.EPOCH_STATE_HEAD + self.C * self.C, dtype=torch.int64, device=device)

    def reset(self):
        self.state.zero_()

    @torch.no_grad()
    def update(self, logits: torch.Tensor, labels: torch.Tensor):
        if not logits.is_cuda:
            raise RuntimeError("EpochMetrics: logits must live on the GPU (there is no CPU path)")
        if logits.dim() != 2 or logits.shape[1] != self.C:
            raise ValueError(f"logits of shape [batch, {self.C}] expected, got {tuple(logits.shape)}")
        lg = logits.detach()
        if lg.dtype != torch.float32 or lg.stride(1) != 1:
            lg = lg.float().contiguous()
        lb = labels.detach()
        if lb.dtype != torch.int64 or not lb.is_contiguous():
            lb = lb.to(torch.int64).contiguous()
        ops.epoch_metrics_update(lg, lb, self.scores, self.labels32, self.preds, self.state)

    def compute(self, name: str = "", sync_dist: bool = True, group=None) -> dict:
        """The pooled epoch values.  With torch.distributed initialised and sync_dist=True the counters are summed and the stored rows of
        all ranks gathered (in rank order) first, so every rank computes the same values from the same seed."""
        C, R = self.C, self.bootstrap
        dist = sync_dist and torch.distributed.is_available() and torch.distributed.is_initialized()
        st = self.state.clone()
        n_local = None
        if dist:
            n_local = int(self.state[_lib.EPOCH_STORED].item())
            torch.distributed.all_reduce(st, group=group)
        head = st.cpu().tolist()                                    # the one host synchronisation of a single-process epoch
        n, overflow = head[_lib.EPOCH_STORED], head[_lib.EPOCH_OVERFLOW]
        if overflow > 0:
            raise RuntimeError(f"EpochMetrics: {overflow} samples did not fit the capacity of {self.capacity} rows, so rank values would cover "
                               f"part of the epoch only; construct EpochMetrics with capacity >= {n + overflow} (or reset() more often)")
        scores, labels32, preds = self.scores, self.labels32, self.preds
        if dist:
            scores, labels32, preds, n = gather_epoch_rows(scores, labels32, preds, n_local, group)
        if n > 0:
            perm = scores[:n].t().contiguous().sort(dim=1, descending=True).indices
        else:
            perm = torch.zeros(C, 0, dtype=torch.int64, device=scores.device)
        ranks, ap, conf = ops.epoch_rank_stats(scores, labels32, preds, perm, st[_lib.EPOCH_STORED:_lib.EPOCH_STORED + 1], n, R, self.seed)
        ranks, ap, conf = ranks.cpu(), ap.cpu(), conf.cpu()
        conf[0] = torch.tensor(head[_lib.EPOCH_STATE_HEAD:], dtype=torch.int64).view(C, C)      # the pooled counts (equal to replicate 0's)

        vals = _scalars(conf.double(), ranks.double(), ap)            # {key: float64 [R + 1]}
        pre = f"{name}_" if name else ""
        out = {pre + k: float(v[0]) for k, v in vals.items()}
        out[pre + "samples"] = int(conf[0].sum())
        for k, i in (("steps", _lib.EPOCH_STEPS), ("ignored", _lib.EPOCH_IGNORED), ("nonfinite", _lib.EPOCH_NONFINITE)):
            out[pre + k] = int(head[i])
        out[pre + "confusion"] = conf[0].tolist()
        if R > 0:
            valid = {}
            q_lo, q_hi = (1.0 - self.ci) / 2.0, (1.0 + self.ci) / 2.0
            for k, v in vals.items():
                reps = v[1:]
                reps = sorted(reps[~torch.isnan(reps)].tolist())
                valid[k] = len(reps)
                ok = len(reps) > 0 and 2 * len(reps) >= R
                out[pre + k + "_ci"] = (_nearest_rank(reps, q_lo), _nearest_rank(reps, q_hi)) if ok else (math.nan, math.nan)
            out[pre + "bootstrap_valid"] = valid
        return out


def _scalars(conf, ranks, ap):
    """Float64 arithmetic on the integer outputs: conf [R + 1, C, C], ranks [R + 1, C, 3], ap [R + 1, C] -> {key: [R + 1]}; nan = undefined."""
    C = conf.shape[1]
    zero = torch.zeros((), dtype=torch.float64)

    def div(a, b):                                                  # torchmetrics' _safe_divide
        return torch.where(b > 0, a / torch.where(b > 0, b, 1.0), zero)

    total = conf.sum(dim=(1, 2))
    tp = conf.diagonal(dim1=1, dim2=2)
    fn, fp = conf.sum(dim=2) - tp, conf.sum(dim=1) - tp
    tn = total[:, None] - tp - fn - fp
    per = {"prec": div(tp, tp + fp), "rec": div(tp, tp + fn), "spec": div(tn, tn + fp), "f1": div(2 * tp, 2 * tp + fp + fn), "npv": div(tn, tn + fn)}
    out = {"acc": div(tp.sum(dim=1), total)}
    present = (tp + fn > 0).double()
    out["balanced_acc"] = div((per["rec"] * present).sum(dim=1), present.sum(dim=1))     # recall averaged over the classes that occur
    for k in CLASS_KEYS:
        for c in range(C):
            out[f"{k}_{c}"] = per[k][:, c]
        out[f"macro_{k}"] = per[k].sum(dim=1) / C
    u2, wpos, wneg = ranks[..., _lib.EPOCH_RANK_U2], ranks[..., _lib.EPOCH_RANK_WPOS], ranks[..., _lib.EPOCH_RANK_WNEG]
    ok = (wpos > 0) & (wneg > 0)
    nan = torch.full((), math.nan, dtype=torch.float64)
    rank = {"auroc": torch.where(ok, 0.5 * u2 / torch.where(ok, wpos * wneg, 1.0), nan), "ap": torch.where(ok, ap, nan)}
    for k in RANK_KEYS:
        for c in range(C):
            out[f"{k}_{c}"] = rank[k][:, c]
        out[f"macro_{k}"] = rank[k].sum(dim=1) / C                  # nan as soon as one class is undefined
    if C == 2:
        out["auc_roc"] = out["auroc_1"]
    return out


def epoch_metrics_config(config):
    """(epoch_metrics, epoch_metrics_bootstrap) of a model config: optional fields, "reference" and 0 when absent."""
    mode, boot = getattr(config, "epoch_metrics", "reference"), int(getattr(config, "epoch_metrics_bootstrap", 0))
    if mode not in ("reference", "pooled") or boot < 0:
        raise ValueError(f'epoch_metrics must be "reference" or "pooled" and epoch_metrics_bootstrap >= 0, got {mode!r}, {boot}')
    return mode, boot


class EpochStatsMixin:
    """log_stats of the reference models (model_cross.py:243-255; modelv3.py has the same method): same log names and
    epoch values, accumulated on the device.  The reference computes seven torchmetrics values with seven host syncs per
    step and logs them on_epoch; here a step is one tiny launch and the epoch values are logged once, from
    on_train_epoch_end / on_validation_epoch_end (or read with epoch_stats(name)).

    Two-class logits go to BinaryEpochMetrics (the reference's per-step means) unless the model's config asked for
    epoch_metrics = "pooled"; any other class count goes to EpochMetrics, with config.epoch_metrics_bootstrap replicates."""

    def log_stats(self, name, logits, labels):
        stats = self.__dict__.setdefault("_stats", {})
        pooled = logits.shape[-1] != 2 or getattr(self, "epoch_metrics", "reference") == "pooled"
        acc = stats.get(name)
        if acc is None or acc.state.device != logits.device or isinstance(acc, EpochMetrics) != pooled or (pooled and acc.C != logits.shape[-1]):
            if pooled:
                acc = EpochMetrics(logits.shape[-1], logits.device, bootstrap=int(getattr(self, "epoch_metrics_bootstrap", 0)))
            else:
                acc = BinaryEpochMetrics(logits.device)
            stats[name] = acc
        acc.update(logits, labels)

    def epoch_stats(self, name, reset=True):
        """{f'{name}_acc', _prec, _rec, _spec, _f1, _npv, _auc_roc, _confusion}: one host sync (summed over the ranks)."""
        acc = self.__dict__.get("_stats", {}).get(name)
        if acc is None:
            return {}
        out = acc.compute(name)
        if reset:
            acc.reset()
        return out

    def _log_epoch_stats(self, name):
        for k, v in self.epoch_stats(name).items():
            if not k.endswith("_confusion") and isinstance(v, (int, float)):      # scalars only: no confusion, no interval tuples
                self.log(k, v, sync_dist=False)        # epoch_stats already reduced over the ranks

    def on_train_epoch_end(self):
        self._log_epoch_stats("train")

    def on_validation_epoch_end(self):
        self._log_epoch_stats("val")

    # ---- test loop surface of both reference models (model_cross.py:294-308, modelv3.py:229-243): logits / targets on the host
    def on_test_epoch_start(self):
        self.test_logits = []
        self.test_targets = []

    def test_step(self, batch, batch_idx):
        x, labels = batch
        logits, _ = self(x, labels)
        self.test_logits.append(logits.detach().cpu())
        self.test_targets.append(labels.cpu())

    def on_test_epoch_end(self):
        self.test_logits = torch.cat(self.test_logits)
        self.test_targets = torch.cat(self.test_targets)
