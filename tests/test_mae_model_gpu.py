"""GPU: MaskedVolumeModel end to end against its restatement on the oracle's blocks (tests/_mae_check.py model_forward).

R.make_config("small") ((32,32,16)/(8,8,8), P = 32, d = 256, M = 3), B = 2, decoder_dim = 128, decoder_depth = 2, mask_ratio = 0.5 (K = 16),
all dropout 0, weights bf16-rounded.  The restated forward runs on the model's own last_token_keep.
  decoder output tokens vs the restatement under R.emulate_bf16():   < 3e-3   (the project's block-output gate against the emulating oracle)
  predicted rows vs the fp32 restatement:                            < BLOCK_TOL = 6e-3
  loss, loss_seq vs the fp32 restatement:                            the Cauchy-Schwarz bound that follows from BLOCK_TOL (_mae_check.loss_gate)
  every parameter gradient vs fp32 autograd of the restatement:      GRAD_TOL = 2e-2 with the norm floor of tests/test_modules_gpu.py
Measured on an MI355X (MEASURED below)."""
import numpy as np
import pytest
import torch

import ref_cpu as R
import _mae_check as C
from _util import dev, note, rel

pytestmark = pytest.mark.gpu

BLOCK_TOL = 6e-3      # tests/test_modules_gpu.py
GRAD_TOL = 2e-2
MEASURED = """decoded vs emulating restatement 2.744e-03 (unshuffled 1.656e-03); pred vs fp32 restatement 3.883e-03;
|loss - ref| 8.7e-06 under a gate of 9.2e-03, loss_seq worst |diff| / gate 3.9e-03; largest sampled-gradient distance / its gate 0.237
(encoder.transformer.0.fusion.2.attn.fn.wq.weight); captured replays: |loss - ref| 2.1e-05 and 1.5e-05 under gates of 9.1e-03"""


def _model(mask_shared=False, seed=0, **kw):
    """The model with bf16-rounded weights: the encoder from the oracle's generator, the decoder from its own initialisation plus small
    random biases and LayerNorm weights, so that a dropped bias or scale cannot hide."""
    import xvit
    cfg = R.make_config("small")
    mae = xvit.MaskedVolumeModel(cfg, decoder_dim=128, decoder_depth=2, mask_ratio=0.5, mask_shared=mask_shared, **kw)
    mae.encoder.load_state_dict(R.make_state_dict(cfg, seed=seed))
    gen = torch.Generator().manual_seed(77 + seed)
    with torch.no_grad():
        for name, p in mae.named_parameters():
            if name.startswith("encoder."):
                pass
            elif name.endswith("norm.weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=gen))
            elif name.endswith(".bias"):
                p.copy_((0.05 if "norm" in name else 0.02) * torch.randn(p.shape, generator=gen))
            p.copy_(R.bf16_round(p))
    return cfg, mae.to(dev())


def _sd(mae):
    return {k: v.detach().cpu().clone() for k, v in mae.state_dict().items()}


def _inputs(cfg, B=2, seed=0):
    img, labels = R.make_inputs(cfg, B, seed=seed)
    return R.bf16_round(img) * 1.5 + 0.75, labels            # exact in fp32 on both sides, away from zero


def test_forward_and_gradients_against_the_restatement():
    cfg, mae = _model()
    sd = _sd(mae)
    img, labels = _inputs(cfg)
    mae.train()
    torch.manual_seed(3)
    cap = {}
    loss_seq, loss = mae(img.to(dev()), labels.to(dev()), capture=cap)
    loss.backward()
    torch.cuda.synchronize()
    keep = mae.last_token_keep.cpu().long()
    assert keep.shape == (3, 2, 16) and loss_seq.shape == (3, 2) and not loss_seq.requires_grad
    with R.emulate_bf16():
        emu = C.model_forward(sd, img, cfg, keep)
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = C.model_forward(leaf, img, cfg, keep)
    ref["loss"].backward()
    assert np.array_equal(ref["drop_idx"].reshape(3, 2, 16).numpy(), mae.last_token_drop.cpu().numpy())
    e_dec = note("mae.model.decoded_vs_emulation", rel(cap["decoded"], emu["decoded"]))
    e_pred = note("mae.model.pred_vs_fp32", rel(cap["pred"].float(), ref["pred"]))
    print(f"mae model: decoded vs emulation {e_dec:.3e}, unshuffled vs emulation {rel(cap['unshuffled'], emu['unshuffled']):.3e}, pred vs fp32 {e_pred:.3e}")
    assert e_dec < 3e-3, e_dec
    assert e_pred < BLOCK_TOL, e_pred
    gate, gate_seq = C.loss_gate(ref, BLOCK_TOL)
    d_loss = abs(float(loss.detach()) - float(ref["loss"].detach()))
    d_seq = (loss_seq.cpu().double() - ref["loss_seq"].detach().double()).abs()
    print(f"mae model: loss {float(loss.detach()):.6f} ref {float(ref['loss'].detach()):.6f} |diff| {d_loss:.3e} gate {gate:.3e}; loss_seq worst diff / gate {float((d_seq / gate_seq).max()):.3e}")
    assert d_loss <= gate, (d_loss, gate)
    assert bool((d_seq <= gate_seq).all()), (d_seq, gate_seq)
    worst = (0.0, None)
    for i, (k, p) in enumerate(sorted(mae.named_parameters())):
        ref_g = leaf[k].grad
        if k.startswith("encoder.mlp_head."):
            assert p.grad is None and ref_g is None, k                      # the heads are present and untrained
            continue
        assert p.grad is not None and ref_g is not None, k
        if k.endswith("wk.bias"):
            assert float(p.grad.abs().max()) < 1e-3                          # analytically zero (a constant on every score of a softmax row)
            continue
        ref_n = float(ref_g.double().norm())
        idx = R.sample_idx(p.numel(), 16, 7919 + i)
        got = p.grad.reshape(-1)[idx.to(dev())].cpu().double()
        want = ref_g.reshape(-1)[idx].double()
        dist, allowed = float((got - want).norm()), GRAD_TOL * float(want.norm()) + 0.03 * ref_n / max(p.numel(), 1) ** 0.5 * 4
        if dist / allowed > worst[0]:
            worst = (dist / allowed, k)
        assert dist <= allowed, (k, dist, allowed)
    print(f"mae model: largest sampled-gradient distance / gate {worst[0]:.3e} ({worst[1]})")


def test_dropped_rows_are_exactly_zero_with_zeroed_embeddings():
    cfg, mae = _model()
    with torch.no_grad():
        for t in (mae.mask_token, mae.decoder_pos_embed, mae.decoder_modality_embed, mae.decoder_embed.bias):
            t.zero_()
    img, labels = _inputs(cfg)
    cap = {}
    with torch.no_grad():
        mae(img.to(dev()), capture=cap)
    y = cap["unshuffled"].cpu()                                              # [S, P + 1, dd]
    drop, keep = mae.last_token_drop.cpu().long().reshape(6, 16), mae.last_token_keep.cpu().long().reshape(6, 16)
    for s in range(6):
        assert bool((y[s, 1 + drop[s]] == 0).all()), s
        assert bool((y[s, 1 + keep[s]] != 0).any(dim=1).all()), s
    assert bool((y[:, 0] != 0).any(dim=1).all())


def _draw(mae, img):
    with torch.no_grad():
        mae(img)
    torch.cuda.synchronize()
    return mae.last_token_keep.cpu().clone(), mae.last_token_drop.cpu().clone()


def test_draw_properties():
    import xvit.functional as XF
    cfg, mae = _model()
    img = _inputs(cfg)[0].to(dev())
    for mode in (mae.train, mae.eval):                                        # masking is the task: eval() draws as well
        mode()
        calls = XF._DROP_CALLS
        torch.manual_seed(11)
        keep, drop = _draw(mae, img)
        assert keep.shape == (3, 2, 16) and drop.shape == (3, 2, 16) and keep.dtype == torch.int32 and drop.dtype == torch.int32
        assert bool((keep[..., 1:] > keep[..., :-1]).all()) and bool((drop[..., 1:] > drop[..., :-1]).all())
        both = torch.cat((keep, drop), dim=-1).sort(dim=-1).values
        assert bool((both == torch.arange(32, dtype=torch.int32)).all())       # disjoint, and together the whole grid
        assert not torch.equal(keep[0], keep[1])
        keep2, _ = _draw(mae, img)
        assert not torch.equal(keep, keep2)                                    # every forward draws anew
        XF._DROP_CALLS = calls
        torch.manual_seed(11)
        keep3, drop3 = _draw(mae, img)
        assert torch.equal(keep, keep3) and torch.equal(drop, drop3)           # the same seed, the same mask
    _, shared = _model(mask_shared=True)
    keep, drop = _draw(shared, img)
    assert bool((keep == keep[0]).all()) and bool((drop == drop[0]).all()) and not torch.equal(keep[0, 0], keep[0, 1])


def test_reconstruct():
    cfg, mae = _model()
    img = _inputs(cfg)[0]
    cap = {}
    recon, mask = mae.reconstruct(img.to(dev()), capture=cap)
    torch.cuda.synchronize()
    assert recon.shape == img.shape and recon.dtype == torch.float32 and mask.shape == (3, 2, 32) and mask.dtype == torch.bool
    keep, drop = mae.last_token_keep.cpu().numpy().reshape(6, 16), mae.last_token_drop.cpu().numpy().reshape(6, 16)
    assert bool((mask.sum(dim=-1) == 16).all())
    assert np.array_equal(np.nonzero(mask.cpu().numpy().reshape(6, 32))[1].reshape(6, 16), drop)
    got, src = recon.cpu().numpy(), img.numpy()
    kept_got, kept_src = C.patch_rows(got, cfg.patch_size, keep), C.patch_rows(src, cfg.patch_size, keep)
    assert np.array_equal(kept_got.view(np.int32), kept_src.view(np.int32))     # kept patches: the input, bit for bit
    stats, pred = cap["stats"], cap["pred"]
    want = (pred.float() * (1.0 / stats[:, 1:2]) + stats[:, 0:1]).cpu().numpy()    # pred * std + mean
    assert np.array_equal(C.patch_rows(got, cfg.patch_size, drop).view(np.int32), want.view(np.int32))
    # and the statistics are the dropped patches' own
    v = C.patch_rows(src.astype(np.float64), cfg.patch_size, drop)
    assert np.allclose(stats[:, 0].cpu().numpy(), v.mean(axis=1), rtol=0, atol=1e-4)
    assert np.allclose(stats[:, 1].cpu().numpy(), 1.0 / np.sqrt(v.var(axis=1, ddof=1) + 1e-6), rtol=1e-4)


def test_graphed_step_draws_a_new_mask_per_replay_and_matches_the_restatement():
    from xvit import ops
    from xvit.graph import GraphedStep
    cfg, mae = _model()
    sd = _sd(mae)
    img, labels = _inputs(cfg)
    mae.train()
    torch.manual_seed(5)
    step = GraphedStep(mae, img.to(dev()), labels.to(dev()))
    assert step._epoch is not None and ops._DROP_EPOCH is None
    seen = []
    for _ in range(2):
        loss_seq, loss = step()
        torch.cuda.synchronize()
        seen.append((mae.last_token_keep.cpu().long().clone(), mae.last_token_drop.cpu().clone(), loss_seq.cpu().clone(), float(loss)))
        assert all(bool(torch.isfinite(p.grad).all()) for k, p in mae.named_parameters() if not k.startswith("encoder.mlp_head."))
        assert all(p.grad is None or not bool(p.grad.any()) for k, p in mae.named_parameters() if k.startswith("encoder.mlp_head."))
    assert not torch.equal(seen[0][1], seen[1][1])                               # two replays, two masks
    for keep, drop, loss_seq, loss in seen:                                      # each replay against the eager restatement on ITS published mask
        ref = C.model_forward(sd, img, cfg, keep)
        assert np.array_equal(ref["drop_idx"].reshape(3, 2, 16).numpy(), drop.numpy())
        gate, gate_seq = C.loss_gate(ref, BLOCK_TOL)
        print(f"mae graph: loss {loss:.6f} ref {float(ref['loss']):.6f} gate {gate:.3e}")
        assert abs(loss - float(ref["loss"])) <= gate
        assert bool(((loss_seq.double() - ref["loss_seq"].double()).abs() <= gate_seq).all())
