"""CPU: the gates of the Mixup / CutMix tests have teeth, and the restated draw (tests/_mix_check.py) has the distribution it claims.

Teeth.  Each planted fault is put into the restatement itself (`fault=`), rounded once to the kernel's output type as a correct kernel would
round, and handed to the gate the GPU tests use, which must refuse it; the same data without the fault must pass."""
import math

import numpy as np
import pytest
import torch

import _cls_check as X
import _mix_check as K


def _caught(what, fn):
    try:
        fn()
    except AssertionError as e:
        return str(e)
    raise AssertionError(f"the gate let through: {what}")


# ---------------------------------------------------------------------------------------------------------------- apply gate
def _apply_case(bf16, poison):
    """B = 3 samples, M = 2, (5, 6, 8): record 0 mixup with sample 1, record 1 CutMix with sample 2, record 2 a copy.  poison: NaN in every
    partner voxel a record must not read."""
    g = torch.Generator().manual_seed(5)
    src = torch.randn(3, 2, 5, 6, 8, generator=g)
    src = (src.to(torch.bfloat16) if bf16 else src).double().numpy()
    table = np.stack([K.record(K.MIXUP, 1, 0.3), K.record(K.CUTMIX, 2, 0.8, box=(1, 3, 2, 5, 3, 7)), K.record(0, 0, 1.0)])
    if poison:                                                # sample 2 is read by record 1 inside its box only (and by its own copy record)
        src = src.copy()
        outside = np.ones((5, 6, 8), dtype=bool)
        outside[1:3, 2:5, 3:7] = False
        src[2][:, outside] = np.nan
    return src, table


@pytest.mark.parametrize("bf16", [False, True])
def test_apply_gate_passes_the_restatement_and_catches_every_planted_fault(bf16):
    src, table = _apply_case(bf16, poison=False)
    ref, bound, exact = K.apply(src, table, bf16)
    K.check_apply("clean", K.to_dtype(ref, bf16), ref, bound, exact)
    assert not exact[0].any() and exact[1:].all() and float(bound[0].min()) >= 0 and float(bound[1:].max()) == 0
    for fault, where in (("swapped_lam_oml", "mixup voxels out of bound"), ("partner_off_by_one", ""), ("box_shifted", "copied voxels differ")):
        bad, _, _ = K.apply(src, table, bf16, fault=fault)
        msg = _caught(fault, lambda: K.check_apply(fault, K.to_dtype(bad, bf16), ref, bound, exact))
        assert where in msg, msg
    # the bound is tight enough to see one ulp of the output type beyond it: the correctly rounded mix moved by two ulps fails
    good = K.to_dtype(ref, bf16)
    step = torch.nextafter(torch.nextafter(good[0].float(), torch.tensor(math.inf)), torch.tensor(math.inf)) if not bf16 else \
        (good[0].view(torch.int16) + 2).view(torch.bfloat16)
    moved = good.clone()
    moved[0] = step.to(good.dtype)
    _caught("two ulps off", lambda: K.check_apply("two ulps", moved, ref, bound, exact))


@pytest.mark.parametrize("bf16", [False, True])
def test_apply_gate_sees_a_voxel_taken_from_both_sources(bf16):
    """On finite data an arithmetic select is bit-identical to the copy, so the gate alone cannot see it: the NaN the tests put into every
    partner voxel outside the box does."""
    src, table = _apply_case(bf16, poison=False)
    ref, bound, exact = K.apply(src, table, bf16)
    both, _, _ = K.apply(src, table, bf16, fault="both_sources")
    K.check_apply("finite data hides it", K.to_dtype(both, bf16), ref, bound, exact)
    src, table = _apply_case(bf16, poison=True)
    ref, bound, exact = K.apply(src, table, bf16)
    assert np.isfinite(ref[:2]).all()                          # the poison reaches no output of the two records that read a partner
    K.check_apply("clean, poisoned", K.to_dtype(ref, bf16), ref, bound, exact)
    both, _, _ = K.apply(src, table, bf16, fault="both_sources")
    assert "must not read" in _caught("both sources", lambda: K.check_apply("both", K.to_dtype(both, bf16), ref, bound, exact))


# ---------------------------------------------------------------------------------------------------------------- loss gate
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_loss_gate_passes_the_restatement_and_catches_every_planted_fault(eps):
    M, B, Cn = 2, 5, 5
    lm, _ = X.ce_inputs("usual", M, B, Cn)
    labels = torch.tensor([0, 1, 2, 3, 4])
    table = np.stack([K.record(K.MIXUP, (b + 2) % B, 0.3) for b in range(B)])
    e32 = X.f32(eps)
    ref = K.ce_ref(lm, labels, table, e32)
    X.ce_check("clean", K.ce_written(ref, M, B, Cn), ref, M, B, Cn)
    faults = ["swapped_lam_oml", "partner_off_by_one"] + (["partner_unsmoothed"] if eps > 0 else [])
    for fault in faults:
        bad = K.ce_ref(lm, labels, table, e32, fault=fault)
        _caught(fault, lambda: X.ce_check(fault, K.ce_written(bad, M, B, Cn), ref, M, B, Cn))


def test_loss_restatement_reduces_to_the_hard_label_reference():
    M, B, Cn = 3, 7, 5
    lm, labels = X.ce_inputs("usual", M, B, Cn)
    for table in (np.stack([K.record(K.MIXUP, (b + 1) % B, 1.0) for b in range(B)]), np.stack([K.record(0, 0, 0.25) for b in range(B)]),
                  np.stack([K.record(K.CUTMIX, B, 0.25) for b in range(B)]), np.stack([K.record(K.MIXUP, 1.5, 0.25) for b in range(B)])):
        a, b = K.ce_ref(lm, labels, table, X.f32(0.1)), X.ce_ref(lm, labels, X.f32(0.1))
        for k in a:
            assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------- the restated draw
N_REC = 65536
ALPHAS = (0.4, 0.8, 1.0, 2.0)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_restated_lam0_has_the_moments_of_beta(alpha):
    """lam0 ~ Beta(a, a): mean 1/2, variance v = 1 / (4 (2a + 1)), excess kurtosis -6 / (2a + 3).  Over n records the sample mean has
    standard error sqrt(v / n) and the sample variance sqrt((m4 - v^2) / n) = v sqrt((2 - 6 / (2a + 3)) / n); gate: 6 standard errors."""
    table, margin = K.draw(dict(mixup_alpha=alpha, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, per_sample=True), N_REC, 8, 8, 8, seed=1234)
    assert (table[:, K.MODE] == K.MIXUP).all() and np.isfinite(margin).all()
    lam0 = table[:, K.LAM0].astype(np.float64)
    assert (lam0 >= 0).all() and (lam0 <= 1).all() and (table[:, K.LAM] == table[:, K.LAM0]).all()
    v = 1.0 / (4.0 * (2.0 * alpha + 1.0))
    se_mean, se_var = math.sqrt(v / N_REC), v * math.sqrt((2.0 - 6.0 / (2.0 * alpha + 3.0)) / N_REC)
    print(f"alpha {alpha}: mean {lam0.mean():.5f} (se {se_mean:.5f}) var {lam0.var():.5f} / {v:.5f} (se {se_var:.5f}), margin < 1e-9: {(margin < K.MARGIN).mean():.2e}")
    assert abs(lam0.mean() - 0.5) <= 6 * se_mean
    assert abs(lam0.var() - v) <= 6 * se_var
    assert (margin < K.MARGIN).mean() <= K.MAX_SKIPPED


def test_restated_mix_and_switch_frequencies():
    prob, sw = 0.7, 0.3
    table, _ = K.draw(dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=prob, switch_prob=sw, per_sample=True), N_REC, 8, 8, 8, seed=99)
    mixed = table[:, K.MODE] != 0
    n = int(mixed.sum())
    assert abs(n - prob * N_REC) <= 6 * math.sqrt(N_REC * prob * (1 - prob))
    cut = int((table[:, K.MODE] == K.CUTMIX).sum())
    assert abs(cut - sw * n) <= 6 * math.sqrt(n * sw * (1 - sw))
    off = table[~mixed]
    assert (off[:, K.LAM] == 1).all() and (off[:, K.OML] == 0).all() and (off[:, K.PARTNER] == np.nonzero(~mixed)[0]).all() and (off[:, K.BOX:K.BOX + 6] == 0).all()
    # one positive alpha decides alone; prob 0 and both alphas 0 mix nothing; per batch every record shares the decision
    t, _ = K.draw(dict(mixup_alpha=0.0, cutmix_alpha=1.0, prob=1.0, switch_prob=0.0, per_sample=True), 64, 8, 8, 8, seed=3)
    assert (t[:, K.MODE] == K.CUTMIX).all()
    t, _ = K.draw(dict(mixup_alpha=1.0, cutmix_alpha=0.0, prob=1.0, switch_prob=1.0, per_sample=True), 64, 8, 8, 8, seed=3)
    assert (t[:, K.MODE] == K.MIXUP).all()
    for cfg in (dict(mixup_alpha=1.0, cutmix_alpha=1.0, prob=0.0, switch_prob=0.5, per_sample=True), dict(mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, per_sample=False)):
        assert (K.draw(cfg, 64, 8, 8, 8, seed=3)[0][:, K.MODE] == 0).all()
    t, _ = K.draw(dict(mixup_alpha=1.0, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, per_sample=False), 64, 8, 8, 8, seed=3)
    assert (t[:, [K.MODE, K.LAM, K.LAM0] + list(range(K.BOX, K.BOX + 6))] == t[0, [K.MODE, K.LAM, K.LAM0] + list(range(K.BOX, K.BOX + 6))]).all()


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 7, 64])
def test_restated_partner_map_is_a_derangement_and_the_box_gives_lam(B, per_sample):
    D, H, W = 5, 12, 9
    seen_shift = set()
    for seed in range(24):
        table, _ = K.draw(dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, per_sample=per_sample), B, D, H, W, seed=seed)
        if B == 1:
            assert (table[:, K.MODE] == 0).all() and table[0, K.PARTNER] == 0 and table[0, K.LAM] == 1
            continue
        p = table[:, K.PARTNER].astype(int)
        assert sorted(p.tolist()) == list(range(B)) and (p != np.arange(B)).all()          # a permutation without a fixed point
        shift = (p[0] - 0) % B
        assert (p == (np.arange(B) + shift) % B).all() and 1 <= shift <= B - 1
        seen_shift.add(shift)
        for rec in table:
            d0, d1, h0, h1, w0, w1 = (int(v) for v in rec[K.BOX:K.BOX + 6])
            assert (rec[K.BOX:K.BOX + 6] == [d0, d1, h0, h1, w0, w1]).all()
            if rec[K.MODE] == K.CUTMIX:
                assert 0 <= d0 <= d1 <= D and 0 <= h0 <= h1 <= H and 0 <= w0 <= w1 <= W          # inside the volume
                assert rec[K.LAM] == np.float32(1.0 - (d1 - d0) * (h1 - h0) * (w1 - w0) / (D * H * W))   # lam is the clipped box fraction
                r = (1.0 - float(rec[K.LAM0])) ** (1.0 / 3.0)
                assert d1 - d0 <= math.floor(D * r + 1e-6) and h1 - h0 <= math.floor(H * r + 1e-6) and w1 - w0 <= math.floor(W * r + 1e-6)
            else:
                assert rec[K.LAM] == rec[K.LAM0] and (rec[K.BOX:K.BOX + 6] == 0).all()
            assert rec[K.OML] == np.float32(1.0) - rec[K.LAM] and (rec[K.LAM0 + 1:] == 0).all()
    if B >= 7:
        assert len(seen_shift) > 1                                                              # the shift is drawn, not fixed


def test_restated_draw_follows_the_epoch():
    cfg = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, per_sample=True)
    a = K.draw(cfg, 16, 8, 8, 8, seed=77)[0]
    assert np.array_equal(a, K.draw(cfg, 16, 8, 8, 8, seed=77)[0])
    assert not np.array_equal(a, K.draw(cfg, 16, 8, 8, 8, seed=77, epoch=1)[0])
    assert np.array_equal(K.draw(cfg, 16, 8, 8, 8, seed=77 + K.EPOCH_STRIDE)[0], K.draw(cfg, 16, 8, 8, 8, seed=77, epoch=1)[0])


@pytest.mark.parametrize("case", K.DRAW_CASES, ids=K.draw_case_id)
def test_the_gpu_draw_cases_meet_the_margin_cap_on_the_restatement_alone(case):
    cfg, B, vol, seed = case
    table, margin = K.draw(cfg, B, *vol, seed)
    assert (margin < K.MARGIN).mean() <= K.MAX_SKIPPED
    K.check_draw(K.draw_case_id(case), table, table, margin)
    for e in (1, 2):                                                    # the epochs test_draw_follows_the_device_epoch steps through
        assert (K.draw(cfg, B, *vol, seed, epoch=e)[1] < K.MARGIN).mean() <= K.MAX_SKIPPED
    cfg64 = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, per_sample=True)
    for e in (None, 1, 2):
        assert (K.draw(cfg64, 64, 6, 10, 12, 4242, epoch=e)[1] < K.MARGIN).mean() <= K.MAX_SKIPPED
