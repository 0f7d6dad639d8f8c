"""GPU: Mixup / CutMix through ModelCross and GraphedStep, golden configs `tiny` at batch 4 and `small` at batch 2, dropout 0.

Plumbing: in deterministic mode the mixing model equals, bit for bit, a mix-off twin fed ops.mix_apply(img, model.last_mix) and closed with
MeanMixCrossEntropyFn on the same table.  Arithmetic: the bf16-emulating oracle on the NumPy-mixed volume with a float64 soft-target loss,
at the gates tests/test_tokdrop_model_gpu.py uses for the same configs (logits 1.5e-2, loss 2e-3, gradient norms 0.03, samples GRAD_TOL).
The draw: the model's table is what tests/_mix_check.py predicts for the seed the forward takes — the first of the dropout seed stream, the
second when patch dropout draws in front of it."""
import numpy as np
import pytest
import torch

import ref_cpu as R
import _mix_check as K
import _tokdrop_check as T
from _util import dev, rel

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-2       # tests/test_modules_gpu.py
MIX = dict(mixup_alpha=0.8, cutmix_alpha=1.0, mix_prob=1.0, mix_switch_prob=0.5, mix_per_sample=True, dropout=0.0, label_smoothing=0.1)
OFF = dict(dropout=0.0, label_smoothing=MIX["label_smoothing"])       # the same model without mixing
CASES = [("tiny", 4), ("small", 2)]


def _model(name, **over):
    import xvit
    cfg = R.make_config(name, **over)
    sd = R.make_state_dict(cfg, seed=0)
    model = xvit.ModelCross(cfg).to(dev())
    model.load_state_dict(sd)
    return cfg, sd, model


def _draw_cfg(model):
    return dict(mixup_alpha=model.mixup_alpha, cutmix_alpha=model.cutmix_alpha, prob=model.mix_prob, switch_prob=model.mix_switch_prob, per_sample=model.mix_per_sample)


def _drop_seed(torch_seed, nth):
    """functional.drop_seeds restated: the nth seed (1-based) the next forward takes under torch.manual_seed(torch_seed)."""
    import xvit.functional as XF
    return ((torch_seed & 0xFFFFFFFF) * 0x9E3779B1 + (XF._DROP_CALLS + nth) * 0x85EBCA77) & 0x7FFFFFFFFFFFFFFF


def _labels(cfg, B):
    """0, 1, 0, 1, ...: under an odd partner shift every sample meets the other class (the oracle's random labels of a batch of 2 or 4 may
    all agree, and a mixed target of two equal labels is the hard target)."""
    return torch.arange(B) % cfg.num_classes


def _seed_with_both_modes(model, B, vol, nth=1):
    """A torch seed under which, by the restatement, the model's next table holds a mixup AND a CutMix record with a non-empty box, an odd
    partner shift (see _labels), some lam below 0.9, all decision margins clear: (torch seed, table, margin)."""
    for seed in range(400):
        table, margin = K.draw(_draw_cfg(model), B, *vol, _drop_seed(seed, nth))
        modes = set(table[:, K.MODE].tolist())
        cut = table[table[:, K.MODE] == K.CUTMIX]
        if {1.0, 2.0} <= modes and (cut[:, K.LAM] < 1).all() and (margin >= K.MARGIN).all() and int(table[0, K.PARTNER]) % 2 == 1 \
                and (table[:, K.LAM] < 0.9).any():
            return seed, table, margin
    raise AssertionError("no seed below 400 draws both modes")


def _step(model, img, labels):
    for p in model.parameters():
        p.grad = None
    logits, loss = model(img, labels)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}


def _close_with_the_mix_loss(monkeypatch, table):
    """The mix-off twin's loss node becomes MeanMixCrossEntropyFn on `table`."""
    import xvit.functional as XF
    mix_fn = XF.MeanMixCrossEntropyFn

    class Closed:
        @staticmethod
        def apply(logits_m, labels, smoothing):
            return mix_fn.apply(logits_m, labels, table, smoothing)

    monkeypatch.setattr(XF, "MeanCrossEntropyFn", Closed)


def _soft_targets(table, labels, Cn, eps):
    """[B, C] float64: lam smooth(y_b) + oml smooth(y_partner[b]) for the mixed records, smooth(y_b) for the others."""
    smooth = torch.nn.functional.one_hot(labels, Cn).double() * (1.0 - eps) + eps / Cn
    tgt = smooth.clone()
    for b in range(len(labels)):
        if K.is_mixed(table[b], len(labels)):
            tgt[b] = float(table[b, K.LAM]) * smooth[b] + float(table[b, K.OML]) * smooth[int(table[b, K.PARTNER])]
    return tgt


@pytest.mark.parametrize("name,batch", CASES)
def test_mixing_model_is_its_parts_bit_for_bit(name, batch, monkeypatch):
    from xvit import ops
    monkeypatch.setattr(ops, "DETERMINISTIC", True)
    cfg, sd, model = _model(name, **MIX)
    img, labels = R.make_inputs(cfg, batch, seed=0)[0].to(dev()), _labels(cfg, batch).to(dev())
    model.train()
    seed, predicted, margin = _seed_with_both_modes(model, batch, cfg.img_size)
    torch.manual_seed(seed)
    logits, loss, grads = _step(model, img, labels)
    table = model.last_mix.clone()
    assert table.shape == (batch, K.NPARAM) and table.dtype == torch.float32
    K.check_draw(f"{name} model draw", table.cpu().numpy(), predicted, margin)
    _, _, twin = _model(name, **OFF)
    twin.train()
    _close_with_the_mix_loss(monkeypatch, table)
    mixed = ops.mix_apply(img, table)
    assert not torch.equal(mixed, img)
    logits2, loss2, grads2 = _step(twin, mixed, labels)
    assert twin.last_mix is None
    assert torch.equal(logits, logits2) and torch.equal(loss, loss2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k


@pytest.mark.parametrize("name,batch", CASES)
def test_mixing_model_vs_oracle_on_the_mixed_volume(name, batch):
    cfg, sd, model = _model(name, **MIX)
    img, labels = R.make_inputs(cfg, batch, seed=0)[0], _labels(cfg, batch)
    model.train()
    seed, predicted, _ = _seed_with_both_modes(model, batch, cfg.img_size)
    torch.manual_seed(seed)
    logits, loss, grads = _step(model, img.to(dev()), labels.to(dev()))
    table = model.last_mix.cpu().numpy()
    mixed64, _, _ = K.apply(img[:, :, 0].double().numpy(), table, False)
    mixed = torch.from_numpy(mixed64).float()[:, :, None]
    assert mixed.shape == img.shape and not torch.equal(mixed, img)
    eps = float(cfg.label_smoothing)
    tgt = _soft_targets(table, labels, cfg.num_classes, eps)
    with R.emulate_bf16():
        ref_logits, _ = R.model_cross_forward(sd, mixed, labels, cfg)
    ref_loss = float(-(tgt * torch.log_softmax(ref_logits.double(), -1)).sum(-1).mean())
    hard_loss = float(R.cross_entropy(ref_logits.double(), labels, eps))
    print(f"mix model {name}: logits {rel(logits, ref_logits):.3e} loss {abs(float(loss) - ref_loss):.3e} (soft {ref_loss:.5f}, hard-label {hard_loss:.5f})")
    assert rel(logits, ref_logits) < 1.5e-2, rel(logits, ref_logits)
    assert abs(float(loss) - ref_loss) < 2e-3
    hard = torch.nn.functional.one_hot(labels, cfg.num_classes).double() * (1.0 - eps) + eps / cfg.num_classes
    assert float((tgt - hard).abs().max()) > 0.05             # the labels really are mixed: some sample's target moved by (1 - lam) (1 - eps) > 0.05
    # gradients: fp32 autograd of the oracle on the mixed volume under the soft target
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    lg, _ = R.model_cross_forward(leaf, mixed, labels, cfg)
    (-(tgt.float() * torch.log_softmax(lg, -1)).sum(-1).mean()).backward()
    for i, (k, p) in enumerate(sorted(model.named_parameters())):
        ref_g = leaf[k].grad
        ref_n = float(ref_g.double().norm())
        if k.endswith("wk.bias"):
            assert float(grads[k].abs().max()) < 1e-3  # analytically zero
            continue
        got_n = float(grads[k].double().norm())
        assert abs(got_n - ref_n) <= 0.03 * ref_n + 1e-7, (k, got_n, ref_n)
        idx = R.sample_idx(p.numel(), 16, 7919 + i)
        got = grads[k].reshape(-1)[idx.to(dev())].cpu().double()
        ref = ref_g.reshape(-1)[idx].double()
        assert float((got - ref).norm()) <= GRAD_TOL * float(ref.norm()) + 0.03 * ref_n / max(p.numel(), 1) ** 0.5 * 4, k


@pytest.mark.parametrize("name,batch", CASES)
def test_model_draws_what_the_restatement_predicts_with_patch_dropout_in_front(name, batch):
    import xvit.functional as XF
    cfg, sd, model = _model(name, patch_dropout=0.5, **MIX)
    g = R.derived(cfg)
    Kp = XF.patch_keep_count(g.P, 0.5)
    img, labels = (t.to(dev()) for t in R.make_inputs(cfg, batch, seed=0))
    model.train()
    seed, predicted, margin = _seed_with_both_modes(model, batch, cfg.img_size, nth=2)      # the mix seed is taken AFTER the token draw's
    keep_pred, _ = T.draw(g.M * batch, batch, g.P, Kp, False, _drop_seed(seed, 1))
    calls = XF._DROP_CALLS
    torch.manual_seed(seed)
    logits, loss, grads = _step(model, img, labels)
    assert XF._DROP_CALLS == calls + 2
    K.check_draw(f"{name} behind patch dropout", model.last_mix.cpu().numpy(), predicted, margin)
    assert np.array_equal(model.last_token_keep.reshape(-1, Kp).cpu().numpy(), keep_pred)     # patch dropout's own subset is unchanged by mixing
    assert bool(torch.isfinite(logits).all()) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    # the same subset as the model without mixing draws from the same seed stream
    _, _, plain = _model(name, patch_dropout=0.5, **OFF)
    plain.train()
    XF._DROP_CALLS = calls
    torch.manual_seed(seed)
    _step(plain, img, labels)
    assert XF._DROP_CALLS == calls + 1 and torch.equal(plain.last_token_keep, model.last_token_keep) and plain.last_mix is None


def test_eval_and_alpha_zero_mix_nothing_and_take_no_seed(monkeypatch):
    import xvit.functional as XF
    from xvit import ops
    cfg, sd, model = _model("small", **MIX)
    _, _, plain = _model("small", **OFF)
    _, _, zero = _model("small", mixup_alpha=0.0, cutmix_alpha=0.0, mix_prob=1.0, **OFF)
    img, labels = (t.to(dev()) for t in R.make_inputs(cfg, 2, seed=0))
    launched = []
    for fn in ("mix_draw", "mix_apply", "mean_ce_mix"):
        real = getattr(ops, fn)
        monkeypatch.setattr(ops, fn, lambda *a, _real=real, _fn=fn, **kw: (launched.append(_fn), _real(*a, **kw))[1])
    model.train()
    _step(model, img, labels)
    assert launched == ["mix_draw", "mix_apply", "mean_ce_mix"] and model.last_mix is not None
    del launched[:]
    calls = XF._DROP_CALLS
    model.eval(), plain.eval()
    with torch.no_grad():
        a, la = model(img, labels)
        assert model.last_mix is None                           # the table of the training forward does not linger
        b, lb = plain(img, labels)
    assert torch.equal(a, b) and torch.equal(la, lb)
    zero.train(), plain.train()
    lz, lossz, gz = _step(zero, img, labels)
    lp, lossp, gp = _step(plain, img, labels)
    assert zero.last_mix is None and torch.equal(lz, lp) and torch.equal(lossz, lossp)
    assert launched == [] and XF._DROP_CALLS == calls
    # forward_tokens (masked pretraining's path) never mixes; a volume that requires grad is refused in train(), served in eval()
    model.train()
    toks = model.forward_tokens(img)
    assert launched == [] and toks[0].shape[0] == 2
    with pytest.raises(RuntimeError, match="mixing"):
        model(img.clone().requires_grad_(), labels)
    model.eval()
    vol = img.clone().requires_grad_()
    model(vol, labels)[1].backward()
    assert vol.grad is not None and bool(torch.isfinite(vol.grad).all())


def test_training_step_logs_against_the_callers_labels():
    cfg, sd, model = _model("tiny", **MIX)
    img, labels = (t.to(dev()) for t in R.make_inputs(cfg, 4, seed=0))
    model.train()
    seen = {}
    model.log_stats = lambda split, logits, lab: seen.update(split=split, labels=lab, logits=logits)
    loss = model.training_step((img, labels), 0)
    assert seen["split"] == "train" and seen["labels"] is labels and seen["logits"].shape == (4, cfg.num_classes) and bool(torch.isfinite(loss))


def test_graphed_step_draws_a_new_table_per_replay_and_matches_eager_on_it(monkeypatch):
    """Two replays leave different tables in the graph's own last_mix tensor, each what the restatement says for the captured seed at the
    replay's epoch; each replay equals the eager model on that table (logits and loss bit for bit, gradients at the gate tests/test_graph_gpu.py
    uses between graph and eager); and the replays survive an eager step at another batch."""
    from xvit import ops
    from xvit.graph import GraphedStep
    calls = []
    real = ops.mix_draw

    def recording(config, table, vol_size, seed):
        calls.append((table, seed))
        return real(config, table, vol_size, seed)

    monkeypatch.setattr(ops, "mix_draw", recording)
    cfg, sd, model = _model("tiny", **MIX)
    img, labels = (t.to(dev()) for t in R.make_inputs(cfg, 4, seed=0))
    img3, lab3 = (t.to(dev()) for t in R.make_inputs(cfg, 3, seed=1))
    model.train()
    torch.manual_seed(3)
    step = GraphedStep(model, img, labels, optimizer=None)
    assert step._epoch is not None and ops._DROP_EPOCH is None          # a positive alpha alone switches the device epoch on
    graph_table, seed = calls[-1]
    assert model.last_mix.data_ptr() == graph_table.data_ptr()

    def replay():
        logits, loss = step()
        torch.cuda.synchronize()
        table = graph_table.clone()
        ref, margin = K.draw(_draw_cfg(model), 4, *cfg.img_size, seed, epoch=int(step._epoch))
        K.check_draw(f"replay at epoch {int(step._epoch)}", table.cpu().numpy(), ref, margin)
        return table, logits.clone(), loss.clone(), {k: p.grad.clone() for k, p in model.named_parameters()}

    def eager_on(table):
        def fixed(config, t, vol_size, seed):
            t.copy_(table)
            return t
        monkeypatch.setattr(ops, "mix_draw", fixed)
        out = _step(model, img, labels)
        assert torch.equal(model.last_mix, table) and model.last_mix.data_ptr() != graph_table.data_ptr()
        monkeypatch.setattr(ops, "mix_draw", recording)
        return out

    def same(r, e):
        assert torch.equal(r[1], e[0]) and torch.equal(r[2], e[1])
        for k in e[2]:
            assert rel(r[3][k], e[2][k]) < 1e-5 or float(e[2][k].abs().max()) < 1e-6, k

    r1 = replay()
    r2 = replay()
    assert not torch.equal(r1[0], r2[0]) and not torch.equal(r1[1], r2[1])
    same(r1, eager_on(r1[0]))
    same(r2, eager_on(r2[0]))
    n = len(calls)
    _step(model, img3, lab3)                                            # the ragged tail of an epoch, eagerly
    assert len(calls) == n + 1 and calls[-1][0].shape == (3, K.NPARAM) and calls[-1][0].data_ptr() != graph_table.data_ptr()
    ref3, margin3 = K.draw(_draw_cfg(model), 3, *cfg.img_size, calls[-1][1])
    K.check_draw("eager batch 3", model.last_mix.cpu().numpy(), ref3, margin3)
    r3 = replay()
    assert not torch.equal(r3[0], r2[0])
    same(r3, eager_on(r3[0]))
