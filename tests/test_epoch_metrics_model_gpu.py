"""GPU: xvit.metrics.EpochMetrics and its place in the models' log_stats, against the restatement in tests/_epoch_metrics_check.py.

The rank values are functions of the fp32 scores the update kernel stored (tests/test_epoch_metrics_kernels_gpu.py compares those with a
float64 softmax), so the restatement ranks the stored scores; labels, predictions and confusion come from the logits themselves."""
import math

import pytest
import torch

import _epoch_metrics_check as E
import ref_cpu as R
from _util import dev

pytestmark = pytest.mark.gpu


def _steps(seed, sizes, C):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(b, C, generator=g) * 2.0, torch.randint(0, C, (b,), generator=g)) for b in sizes]


def _compare(got, acc_scores, steps, C, boot, seed, pre="", ci=0.95):
    """compute()'s dict against the restatement of `steps`, ranked on the stored scores."""
    _, labels, preds, conf, cnt = E.update_reference(steps, C, cap=10 ** 9)
    n = cnt["stored"]
    scores = acc_scores[:n].cpu().numpy()
    point, inter = E.epoch_reference(scores, labels, preds, C, boot, seed, ci)
    assert got[pre + "confusion"] == conf.tolist() and got[pre + "samples"] == n and got[pre + "steps"] == cnt["steps"]
    assert got[pre + "ignored"] == cnt["ignored"] and got[pre + "nonfinite"] == cnt["nonfinite"]
    ap_tol = E.ap_bound(n)

    def close(a, b, k):
        if math.isnan(b):
            return math.isnan(a)
        return abs(a - b) <= (ap_tol * abs(b) if "ap" in k else 1e-12)

    for k, v in point.items():
        assert close(got[pre + k], v, k), (k, got[pre + k], v)
    for k, ((lo, hi), valid) in inter.items():
        assert got[pre + "bootstrap_valid"][k] == valid, (k, got[pre + "bootstrap_valid"][k], valid)
        g_lo, g_hi = got[pre + k + "_ci"]
        assert close(g_lo, lo, k) and close(g_hi, hi, k), (k, (g_lo, g_hi), (lo, hi))
    return point, inter, n


def test_pooled_metrics_and_intervals_over_ragged_steps():
    from xvit.metrics import EpochMetrics, epoch_metric_keys
    C, boot, seed = 3, 40, 1234
    steps = _steps(0, (126, 37, 1, 8), C)
    labels = torch.cat([b for _, b in steps])
    assert all(3 <= int((labels == c).sum()) <= len(labels) - 3 for c in range(C))      # >= 3 positives and negatives per class
    acc = EpochMetrics(C, dev(), capacity=256, bootstrap=boot, seed=seed)
    for lg, lb in steps:
        acc.update(lg.to(dev()), lb.to(dev()))
    got = acc.compute("val", sync_dist=False)
    point, inter, n = _compare(got, acc.scores, steps, C, boot, seed, pre="val_")
    assert n == 172
    keys = epoch_metric_keys(C)
    assert set(got) == ({f"val_{k}" for k in keys} | {f"val_{k}_ci" for k in keys}
                        | {"val_samples", "val_steps", "val_ignored", "val_nonfinite", "val_confusion", "val_bootstrap_valid"})
    for k in keys:                                           # every class occurs often enough: no replicate is left out
        assert got["val_bootstrap_valid"][k] == boot == inter[k][1], k
        lo, hi = got[f"val_{k}_ci"]
        assert lo <= hi and 0.0 <= lo and hi <= 1.0
    acc.reset()
    empty = acc.compute(sync_dist=False)
    assert empty["samples"] == 0 and empty["acc"] == 0.0 and math.isnan(empty["macro_auroc"]) and math.isnan(empty["auroc_0_ci"][0])


def test_binary_pooled_auroc_is_not_the_mean_of_per_step_aurocs():
    from xvit.metrics import BinaryEpochMetrics, EpochMetrics
    steps = _steps(5, (8,) * 12, 2)
    pooled, per_step = EpochMetrics(2, dev(), capacity=128), BinaryEpochMetrics(dev())
    for lg, lb in steps:
        pooled.update(lg.to(dev()), lb.to(dev()))
        per_step.update(lg.to(dev()), lb.to(dev()))
    got, ref = pooled.compute(sync_dist=False), per_step.compute(sync_dist=False)
    _compare(got, pooled.scores, steps, 2, 0, 0)
    assert got["auc_roc"] == got["auroc_1"] and abs(got["auroc_0"] - got["auroc_1"]) < 1e-12      # two classes: the same pairs
    assert abs(got["auc_roc"] - ref["auc_roc"]) > 1e-3                                            # the reference's value is a mean of 12 small AUROCs
    assert abs(got["acc"] - ref["acc"]) < 1e-12                                                   # accuracy pools either way
    skm = pytest.importorskip("sklearn.metrics")
    y = torch.cat([b for _, b in steps]).numpy()
    p1 = pooled.scores[:96, 1].cpu().numpy()
    assert abs(got["auc_roc"] - skm.roc_auc_score(y, p1)) < 1e-12
    assert abs(got["ap_1"] - skm.average_precision_score(y, p1)) < 1e-12


def test_overflow_raises_and_a_missing_class_is_undefined():
    from xvit.metrics import EpochMetrics
    steps = _steps(9, (30, 30), 3)
    small = EpochMetrics(3, dev(), capacity=50)
    for lg, lb in steps:
        small.update(lg.to(dev()), lb.to(dev()))
    with pytest.raises(RuntimeError) as err:
        small.compute(sync_dist=False)
    assert "capacity of 50" in str(err.value) and "10 samples" in str(err.value) and "capacity >= 60" in str(err.value)
    # class 2 never occurs: its rank values and the macro values are nan (never 0); the other classes keep theirs
    lg, lb = steps[0][0], steps[0][1] % 2
    acc = EpochMetrics(3, dev(), capacity=64, bootstrap=6)
    acc.update(lg.to(dev()), lb.to(dev()))
    got = acc.compute(sync_dist=False)
    assert math.isnan(got["auroc_2"]) and math.isnan(got["ap_2"]) and math.isnan(got["macro_auroc"]) and math.isnan(got["macro_ap"])
    assert 0.0 <= got["auroc_0"] <= 1.0 and 0.0 <= got["ap_1"] <= 1.0 and got["rec_2"] == 0.0
    assert got["bootstrap_valid"]["auroc_2"] == 0 and math.isnan(got["auroc_2_ci"][0]) and math.isnan(got["macro_auroc_ci"][1])
    _compare(got, acc.scores, [(lg, lb)], 3, 6, 0)


def _run_validation(cfg, batches=((1, 5), (2, 5), (3, 2))):
    import xvit
    model = xvit.ModelCross(cfg).to(dev())
    model.eval()
    seen = []
    hook = model.register_forward_hook(lambda m, i, o: seen.append((o[0].detach().float().cpu(), i[1].cpu())))
    for seed, b in batches:
        img, labels = R.make_inputs(cfg, b, seed=seed)
        with torch.no_grad():
            model.validation_step((img.to(dev()), labels.to(dev())), 0)
    hook.remove()
    return model, seen


def test_three_class_model_runs_validation_steps_and_reports_pooled_values():
    """ModelCross with num_classes = 3: log_stats used to raise ValueError("binary classification expected ...") at the first step."""
    from xvit.metrics import EpochMetrics
    model, seen = _run_validation(R.make_config("tiny", num_classes=3))
    acc = model._stats["val"]
    assert isinstance(acc, EpochMetrics) and acc.C == 3
    got = model.epoch_stats("val")
    _compare(got, acc.scores, seen, 3, 0, 0, pre="val_")
    assert got["val_samples"] == 12 and got["val_steps"] == 3
    assert model.epoch_stats("val")["val_samples"] == 0                       # reset by the read
    logged = {}
    model.log = lambda k, v, **kw: logged.__setitem__(k, v)
    model._stats["val"].update(seen[0][0].to(dev()), seen[0][1].to(dev()))
    model.on_validation_epoch_end()
    assert logged and all(isinstance(v, (int, float)) for v in logged.values()) and "val_confusion" not in logged and "val_macro_auroc" in logged


def test_binary_model_can_choose_the_pooled_accumulator():
    from xvit.metrics import EpochMetrics
    model, seen = _run_validation(R.make_config("tiny", epoch_metrics="pooled", epoch_metrics_bootstrap=8))
    acc = model._stats["val"]
    assert isinstance(acc, EpochMetrics) and acc.C == 2 and acc.bootstrap == 8
    got = model.epoch_stats("val")
    _compare(got, acc.scores, seen, 2, 8, 0, pre="val_")
    assert "val_auc_roc" in got and "val_auc_roc_ci" in got


def test_default_binary_model_keeps_the_reference_keys_and_values():
    from xvit.metrics import KEYS, BinaryEpochMetrics
    model, seen = _run_validation(R.make_config("tiny"))
    assert isinstance(model._stats["val"], BinaryEpochMetrics) and model.epoch_metrics == "reference"
    got = model.epoch_stats("val")
    assert set(got) == {f"val_{k}" for k in KEYS} | {"val_confusion"}
    ref = R.epoch_metrics(seen)
    for k, v in ref.items():
        assert abs(got[f"val_{k}"] - v) < 1e-9, k
    assert set(got["val_confusion"]) == {"tn", "fp", "fn", "tp", "samples", "steps"} and got["val_confusion"]["samples"] == 12
