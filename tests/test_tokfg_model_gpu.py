"""GPU: foreground-ranked token selection through ModelCross, GraphedStep, MaskedVolumeModel and xvit.interpret.

Oracle configs tiny ((32,32,2)/(8,8,2): P = 16, K = 8, M = 2; one voxel per lane in the occupancy kernel) and small ((32,32,16)/(8,8,8):
P = 32, K = 16, M = 3; 16-byte runs).  The volumes are negative noise (at or below the threshold 0) with a box of positive noise: in the
even samples the box covers a quarter of the patches (n_fg < K), in the odd ones three quarters (n_fg > K); both counts are checked with
the NumPy restatement inside the tests.  What the model ranks by, keeps and counts is compared with the restatement bit for bit; logits,
loss and gradients are held against the oracle run on the kept tokens with the helpers and gates of tests/test_tokdrop_model_gpu.py."""
import numpy as np
import pytest
import torch

import ref_cpu as R
import _tokdrop_check as T
import _tokfg_check as F
from _util import dev, rel
from test_tokdrop_model_gpu import GRAD_TOL, _model, _step, forward_kept

pytestmark = pytest.mark.gpu


def boxed_inputs(cfg, batch, seed=0, per_modality=False):
    """Negative noise with a box of positive noise, from the oracle's inputs.  The box of sample b spans the patch rows d < 2 + b % 2 and
    h < 2 + 2 (b % 2) and all of W: 4 / 12 of tiny's 16 patches, 8 / 24 of small's 32.  per_modality: modality m's box starts one patch row
    (8 voxels) further along H per m, cut at the edge, so that the modalities of a sample disagree."""
    img, labels = R.make_inputs(cfg, batch, seed=seed)
    out = -img.abs()
    for b in range(batch):
        for m in range(img.shape[1]):
            h0 = 8 * m if per_modality else 0
            d1, h1 = 16 + 8 * (b % 2), min(32, h0 + 16 + 16 * (b % 2))
            out[b, m, 0, :d1, h0:h1] = img[b, m, 0, :d1, h0:h1].abs() + 0.5
    return out, labels


def next_drop_seed(torch_seed, nth=1):
    """The nth seed the next forward takes from the dropout seed stream (functional.drop_seeds), as tests/test_tokdrop_model_gpu.py restates it."""
    import xvit.functional as XF
    return ((torch_seed & 0xFFFFFFFF) * 0x9E3779B1 + (XF._DROP_CALLS + nth) * 0x85EBCA77) & 0x7FFFFFFFFFFFFFFF


def check_against_oracle(name, cfg, sd, model, img, labels, keep, logits, loss, grads):
    """The forward and gradient gates of test_model_cross_with_patch_dropout_vs_oracle_on_the_kept_tokens, on keep int64 [M, B, K]."""
    with R.emulate_bf16():
        ref_logits, ref_loss = forward_kept(sd, img, labels, cfg, keep)
    print(f"tokfg model {name}: logits {rel(logits, ref_logits):.3e} loss {abs(float(loss.detach()) - float(ref_loss)):.3e}")
    assert rel(logits, ref_logits) < 1.5e-2, rel(logits, ref_logits)
    assert abs(float(loss) - float(ref_loss)) < 2e-3
    if not grads:
        return
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    forward_kept(leaf, img, labels, cfg, keep)[1].backward()
    for i, (k, p) in enumerate(sorted(model.named_parameters())):
        assert p.grad is not None, k
        ref_g = leaf[k].grad
        ref_n = float(ref_g.double().norm())
        if k.endswith("wk.bias"):
            assert float(p.grad.abs().max()) < 1e-3  # analytically zero
            continue
        got_n = float(p.grad.double().norm())
        assert abs(got_n - ref_n) <= 0.03 * ref_n + 1e-7, (k, got_n, ref_n)
        idx = R.sample_idx(p.numel(), 16, 7919 + i)
        got = p.grad.reshape(-1)[idx.to(dev())].cpu().double()
        ref = ref_g.reshape(-1)[idx].double()
        assert float((got - ref).norm()) <= GRAD_TOL * float(ref.norm()) + 0.03 * ref_n / max(p.numel(), 1) ** 0.5 * 4, k


def restated(cfg, img, batch, K, shared, mode, seed=0, epoch=None, above=0.0, fraction=0.05):
    """-> (occ [M B, P], keep_idx, slot, n_fg) by the NumPy restatement, for the model's defaults."""
    g = R.derived(cfg)
    occ = F.occupancy(img, cfg.patch_size, above)
    return (occ,) + F.ranked(occ, batch, K, shared, mode, F.min_count(g.pd, fraction, g.M if shared else 1), seed, epoch)


# ---- train() ------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,batch", [("tiny", 4), ("small", 2)])
def test_training_keeps_foreground_first_and_matches_the_oracle_on_the_kept_tokens(name, batch):
    import xvit.functional as XF
    cfg, sd, model = _model(name, patch_dropout=0.5, patch_select="foreground")
    g = R.derived(cfg)
    K = XF.patch_keep_count(g.P, 0.5)
    img, labels = boxed_inputs(cfg, batch)
    model.train()
    torch.manual_seed(7)
    occ, rk, rs, rn = restated(cfg, img, batch, K, False, F.RANDOM, next_drop_seed(7))
    rn = rn.reshape(g.M, batch)
    assert bool((rn[:, 0] == g.P // 4).all()) and bool((rn[:, 1] == 3 * g.P // 4).all()) and g.P // 4 < K < 3 * g.P // 4     # one sample below K, one above
    logits, loss = model(img.to(dev()), labels.to(dev()))
    loss.backward()
    assert model.last_token_occupancy.shape == (g.M, batch, g.P) and model.last_token_occupancy.dtype == torch.int32
    assert np.array_equal(model.last_token_occupancy.cpu().numpy().reshape(-1, g.P), occ)
    assert np.array_equal(model.last_token_foreground.cpu().numpy(), rn)
    keep = model.last_token_keep
    assert keep.shape == (g.M, batch, K) and np.array_equal(keep.cpu().numpy().reshape(-1, K), rk)
    fg = torch.from_numpy(occ >= F.min_count(g.pd, 0.05)).reshape(g.M, batch, g.P)
    kept_fg = torch.gather(fg, 2, keep.cpu().long()).sum(dim=2)
    assert bool((kept_fg[:, 0] == g.P // 4).all()) and bool((kept_fg[:, 1] == K).all())      # all the tissue where it fits, nothing but tissue where it does not
    check_against_oracle(name, cfg, sd, model, img, labels, keep.cpu().long(), logits, loss, grads=True)


def test_explicit_random_is_the_model_without_the_fields(monkeypatch):
    from xvit import ops
    import xvit.functional as XF
    monkeypatch.setattr(ops, "DETERMINISTIC", True)            # gradients bit for bit (tests/test_tokdrop_model_gpu.py)
    img, labels = (t.to(dev()) for t in boxed_inputs(R.make_config("small"), 2))
    runs = []
    calls = XF._DROP_CALLS
    for over in (dict(), dict(patch_select="random", patch_foreground_above=0.3, patch_foreground_min_fraction=0.5, eval_patch_dropout=0.0)):
        cfg, sd, model = _model("small", patch_dropout=0.5, **over)
        model.train()
        XF._DROP_CALLS = calls
        torch.manual_seed(5)
        logits, loss, keep = _step(model, img, labels)
        assert model.last_token_occupancy is None and model.last_token_foreground is None
        runs.append((logits, loss, keep, {k: p.grad.clone() for k, p in model.named_parameters()}))
        model.eval()
        with torch.no_grad():
            runs[-1] += (model(img, labels)[0].clone(),)
        assert model.last_token_keep is None and model.last_token_occupancy is None
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and torch.equal(runs[0][4], runs[1][4])
    for k in runs[0][3]:
        assert torch.equal(runs[0][3][k], runs[1][3][k]), k


def test_occupancy_is_taken_from_the_mixed_volume():
    import xvit.functional as XF
    cfg, sd, model = _model("small", patch_dropout=0.5, patch_select="foreground", mixup_alpha=0.4)
    img, labels = boxed_inputs(cfg, 2)
    model.train()
    torch.manual_seed(13)
    token_seed = next_drop_seed(13, 1)                           # today's order: the token seed, then the mix seed
    logits, loss = model(img.to(dev()), labels.to(dev()))
    assert model.last_mix is not None and bool(torch.isfinite(loss))
    mixed = XF.mix_volumes(img.to(dev()), model.last_mix).cpu()
    assert not torch.equal(mixed, img)
    occ, rk, rs, rn = restated(cfg, mixed, 2, 16, False, F.RANDOM, token_seed)
    assert not np.array_equal(occ, F.occupancy(img, cfg.patch_size, 0.0))                      # the mix moved counts
    assert np.array_equal(model.last_token_occupancy.cpu().numpy().reshape(-1, 32), occ)
    assert np.array_equal(model.last_token_keep.cpu().numpy().reshape(-1, 16), rk)
    assert np.array_equal(model.last_token_foreground.cpu().numpy().reshape(-1), rn)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_shared_selection_ranks_by_the_summed_counts(training):
    cfg, sd, model = _model("small", patch_dropout=0.5, eval_patch_dropout=0.5, patch_dropout_shared=True, patch_select="foreground")
    img, labels = boxed_inputs(cfg, 2, per_modality=True)
    model.train(training)
    torch.manual_seed(17)
    seed = next_drop_seed(17)
    with torch.set_grad_enabled(training):
        model(img.to(dev()), labels.to(dev()))
    keep = model.last_token_keep.cpu().numpy()
    occ, rk, rs, rn = restated(cfg, img, 2, 16, True, F.RANDOM if training else F.TOP, seed)
    assert not np.array_equal(occ[0:2], occ[2:4])                                               # the modalities' own counts differ
    assert bool((keep == keep[0]).all()) and not np.array_equal(keep[0, 0], keep[0, 1])
    assert np.array_equal(keep.reshape(-1, 16), rk) and np.array_equal(model.last_token_foreground.cpu().numpy().reshape(-1), rn)
    own = F.ranked(occ, 2, 16, False, F.RANDOM if training else F.TOP, F.min_count(512, 0.05), seed)[0]
    assert not np.array_equal(own, rk)                                                          # ranking each modality alone gives another answer


# ---- eval() -------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,batch", [("tiny", 4), ("small", 2)])
def test_eval_keeps_the_most_occupied_patches_without_a_seed(name, batch):
    import xvit.functional as XF
    cfg, sd, model = _model(name, patch_dropout=0.5, eval_patch_dropout=0.5, patch_select="foreground")
    g = R.derived(cfg)
    K = XF.patch_keep_count(g.P, 0.5)
    img, labels = boxed_inputs(cfg, batch)
    img[0, 0, 0, :8, :8] = -1.0                                  # one box patch of sequence 0 emptied, its neighbour halved: counts that differ
    img[0, 0, 0, 8:12, :8] = -1.0
    x, y = img.to(dev()), labels.to(dev())
    occ, rk, rs, rn = restated(cfg, img, batch, K, False, F.TOP)
    Wn = cfg.img_size[2] // cfg.patch_size[2]
    assert int(rn[0]) == g.P // 4 - Wn and int(rn[1]) == 3 * g.P // 4 and len(np.unique(occ[0])) >= 3
    model.eval()
    calls = XF._DROP_CALLS
    with torch.no_grad():
        logits, loss = model(x, y)
        keep = model.last_token_keep.clone()
        logits2, loss2 = model(x, y)
    assert XF._DROP_CALLS == calls                                                              # no seed taken
    assert torch.equal(logits, logits2) and torch.equal(loss, loss2) and torch.equal(keep, model.last_token_keep)
    assert logits.shape[0] == batch and keep.shape == (g.M, batch, K)
    assert np.array_equal(keep.cpu().numpy().reshape(-1, K), rk)
    assert np.array_equal(model.last_token_occupancy.cpu().numpy().reshape(-1, g.P), occ) and np.array_equal(model.last_token_foreground.cpu().numpy().reshape(-1), rn)
    check_against_oracle(name, cfg, sd, model, img, labels, keep.cpu().long(), logits, loss, grads=False)
    # a training run draws the same subsets with and without validation in between
    model.train()
    XF._DROP_CALLS = calls
    torch.manual_seed(23)
    alone = _step(model, x, y)[2]
    XF._DROP_CALLS = calls
    torch.manual_seed(23)
    model.eval()
    with torch.no_grad():
        model(x, y)
    model.train()
    after = _step(model, x, y)[2]
    assert torch.equal(alone, after) and not torch.equal(alone, keep)
    # eval_patch_dropout = 0 is the full grid
    model.eval_patch_dropout = 0.0
    model.eval()
    with torch.no_grad():
        model(x, y)
    assert model.last_token_keep is None and model.last_token_occupancy is None and model.last_token_foreground is None


# ---- GraphedStep ----------------------------------------------------------------------------------------------------------------------------


def test_graphed_step_ranks_anew_at_every_replay_and_matches_eager_on_the_same_subset(monkeypatch):
    from xvit import ops
    from xvit.graph import GraphedStep
    calls = []
    real = ops.token_select_ranked

    def recording(occ, keep_idx, slot, B, shared, mode, min_count, seed, n_fg=None):
        calls.append((occ, keep_idx, slot, seed, min_count, n_fg))
        return real(occ, keep_idx, slot, B, shared, mode, min_count, seed, n_fg)

    monkeypatch.setattr(ops, "token_select_ranked", recording)
    cfg, sd, model = _model("tiny", patch_dropout=0.5, patch_select="foreground")
    assert cfg.dropout == 0.0
    img, labels = boxed_inputs(cfg, 4)
    x, y = img.to(dev()), labels.to(dev())
    model.train()
    torch.manual_seed(3)
    step = GraphedStep(model, x, y)
    assert step._epoch is not None and ops._DROP_EPOCH is None
    occ_t, keep_t, slot_t, seed, min_count, n_fg_t = calls[-1]                                   # the capture's own tensors
    assert model.last_token_keep.data_ptr() == keep_t.data_ptr() and model.last_token_occupancy.data_ptr() == occ_t.data_ptr()
    ref_occ = F.occupancy(img, cfg.patch_size, 0.0)

    def replay():
        logits, loss = step()
        torch.cuda.synchronize()
        rk, rs, rn = F.ranked(ref_occ, 4, 8, False, F.RANDOM, min_count, seed, epoch=int(step._epoch))
        assert np.array_equal(occ_t.cpu().numpy(), ref_occ) and np.array_equal(keep_t.cpu().numpy(), rk) and np.array_equal(slot_t.cpu().numpy(), rs)
        assert np.array_equal(n_fg_t.cpu().numpy(), rn)
        return logits.clone(), float(loss), model.last_token_keep.clone(), {k: p.grad.clone() for k, p in model.named_parameters()}

    logits1, loss1, keep1, grads1 = replay()
    _, _, keep2, _ = replay()
    assert keep1.shape == (2, 4, 8) and not torch.equal(keep1, keep2)
    # the eager step on the subset of the first replay: the ranked draw is replaced by a copy of that subset
    slot1 = torch.from_numpy(T.slot_of(keep1.reshape(8, 8).cpu().numpy(), 16)).to(dev())

    def fixed(occ, keep_idx, slot, B, shared, mode, min_count, seed, n_fg=None):
        keep_idx.copy_(keep1.reshape(keep_idx.shape))
        slot.copy_(slot1)
        n_fg.zero_()
        return keep_idx, slot

    monkeypatch.setattr(ops, "token_select_ranked", fixed)
    le, losse, keepe = _step(model, x, y)
    assert torch.equal(keepe, keep1)
    assert torch.equal(le, logits1) and losse == loss1               # same kernels, same order: bit-identical
    for k, p in model.named_parameters():                            # gates of tests/test_graph_gpu.py between graph and eager
        assert rel(p.grad, grads1[k]) < 1e-5 or float(grads1[k].abs().max()) < 1e-6, k


# ---- the neighbours -----------------------------------------------------------------------------------------------------------------------


def test_masked_pretraining_keeps_its_uniform_mask():
    import xvit
    import xvit.functional as XF
    img = boxed_inputs(R.make_config("small"), 2)[0].to(dev())
    masks = []
    calls = XF._DROP_CALLS
    for over in (dict(), dict(patch_select="foreground", patch_dropout=0.5, eval_patch_dropout=0.5)):
        cfg = R.make_config("small", **over)
        mae = xvit.MaskedVolumeModel(cfg, decoder_dim=128, decoder_depth=1, mask_ratio=0.5).to(dev())
        XF._DROP_CALLS = calls
        torch.manual_seed(29)
        seed = next_drop_seed(29)
        for mode in (mae.train, mae.eval):
            mode()
            with torch.no_grad():
                mae(img)
            masks.append((mae.last_token_keep.clone(), mae.last_token_drop.clone()))
            assert mae.encoder.last_token_occupancy is None
        assert np.array_equal(masks[-2][0].cpu().numpy().reshape(-1, 16), T.draw(6, 2, 32, 16, False, seed)[0])    # the plain draw, box or no box
    for a, b in zip(masks[:2], masks[2:]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_interpret_refuses_a_model_that_shortens_eval():
    import xvit
    cfg, sd, model = _model("tiny", patch_dropout=0.5, eval_patch_dropout=0.5, patch_select="foreground")
    img = boxed_inputs(cfg, 2)[0].to(dev())
    model.eval()
    for call in (lambda: xvit.interpret.attention_maps(model, img), lambda: xvit.interpret.relevance_maps(model, img),
                 lambda: xvit.interpret.input_attributions(model, img, method="gradient")):
        with pytest.raises(RuntimeError, match="eval_patch_dropout = 0"):
            call()
    model.eval_patch_dropout = 0.0
    xvit.interpret.attention_maps(model, img)                        # and serves it once the full grid is back
