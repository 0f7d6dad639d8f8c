"""GPU: patch dropout through PatchEmbedFn, ModelCross and GraphedStep.

PatchEmbedFn with a hand-made keep, at (32,32,16)/(8,8,8) (P = 32), K = 16, M = 3, B = 2, d = 256, against float64 autograd of the restated
embedding on the bf16-rounded operands.  The gate of each quantity is twice the distance of the unselected stored-matrix path
(XVIT_PATCH_EMBED=unfused, all P tokens) to its own float64 reference at the same shape: selection adds no arithmetic, so twice the
unselected distance covers another tile choice at the smaller row count.  The upstream gradient is generic fp32, as in training; for dW
the reference takes its bf16 rounding, the operand of the weight-gradient GEMM.  (A bf16-exact upstream gradient would make dpos and
dcls exact sums on both paths, so that the gate compared zero with zero.)  Measured on an MI355X (relative L2; unselected / selected):
    x     9.386e-08 / 9.200e-08
    dW    7.366e-08 / 5.243e-08
    db    8.197e-08 / 7.330e-08
    dcls  4.554e-08 / 4.554e-08   (the same CLS rows summed in the same order)
    dpos  4.436e-08 / 3.706e-08
    x at K = P with the identity keep against the unselected path's x: 0 (bit-identical)

ModelCross in train() with patch_dropout = 0.5 against the bf16-emulating oracle run on the tokens the model kept (gates of
test_model_cross_vs_bf16_emulating_oracle) and its gradients against fp32 autograd of the same restated forward (gates of
_check_model_vs_golden); the draw's properties; and a captured step that draws a new subset at every replay."""
import numpy as np
import pytest
import torch

import ref_cpu as R
import _tokdrop_check as T
from _util import dev, note, rel

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-2       # tests/test_modules_gpu.py


# ---- the restated embedding (torch, so that autograd and the bf16 emulation run through it) -----------------------------------------


def embed_kept(sd, img, cfg, keep):
    """R.embed on the kept tokens: keep int64 [M, B, K] (None: every token) -> list of M tensors [B, K + 1, d]."""
    toks = []
    B = img.shape[0]
    pos = sd["pos_embedding"]
    for m in range(img.shape[1]):
        p = R.patchify(img[:, m, 0], cfg.patch_size)                                        # [B, P, pd]
        rows = torch.arange(p.shape[1]).expand(B, -1) if keep is None else keep[m]
        p = torch.gather(p, 1, rows[:, :, None].expand(-1, -1, p.shape[2]))
        x = R.linear(p, sd["patch_to_embedding.weight"], sd["patch_to_embedding.bias"])
        x = torch.cat((sd["cls_token"].expand(B, -1, -1), x), dim=1)
        idx = torch.cat((torch.zeros(B, 1, dtype=torch.int64), 1 + rows), dim=1)            # pos row of every token
        toks.append(x + pos[0][idx])
    return toks


def forward_kept(sd, img, labels, cfg, keep, capture=None):
    """R.model_cross_forward with the restated embedding in front: the oracle's own blocks, the heads and the loss as it writes them."""
    xs = embed_kept(sd, img, cfg, keep)
    for b in range(cfg.num_multi_blocks):
        xs = R.multi_scale_block(sd, f"transformer.{b}", xs, cfg)
        if capture is not None:
            capture[f"msb{b}"] = list(xs)
    per_mod = []
    for m, x in enumerate(xs):
        c = R.layer_norm(x, sd[f"norm.{m}.weight"], sd[f"norm.{m}.bias"])[:, 0]
        h = R.gelu(R.linear(c, sd[f"mlp_head.{m}.0.weight"], sd[f"mlp_head.{m}.0.bias"], exact=True))
        per_mod.append(R.linear(h, sd[f"mlp_head.{m}.3.weight"], sd[f"mlp_head.{m}.3.bias"], exact=True))
    logits = torch.stack(per_mod).mean(dim=0)
    return logits, R.cross_entropy(logits, labels, cfg.label_smoothing)


# ---- PatchEmbedFn ------------------------------------------------------------------------------------------------------------------


def _embed_operands():
    cfg = R.make_config("small")                          # (32, 32, 16) / (8, 8, 8): P = 32, pd = 512, d = 256, M = 3
    B, M, P, d, pd = 2, 3, 32, 256, 512
    g = torch.Generator().manual_seed(42)
    img = R.bf16_round(torch.randn(B, M, 1, *cfg.img_size, generator=g))
    sd = {"patch_to_embedding.weight": R.bf16_round(torch.randn(d, pd, generator=g) / pd ** 0.5), "patch_to_embedding.bias": torch.randn(d, generator=g) * 0.1,
          "cls_token": torch.randn(1, 1, d, generator=g), "pos_embedding": torch.randn(1, P + 1, d, generator=g)}
    G = torch.randn(M, B, P + 1, d, generator=g)                    # the upstream gradient of every token: generic fp32, as in training
    keep = torch.stack([torch.randperm(P, generator=g)[:16].sort().values for _ in range(M * B)]).view(M, B, 16)
    return cfg, sd, img, G, keep


def _rows_of(G, keep):
    """The upstream gradient of the kept tokens [M, B, K + 1, d]."""
    if keep is None:
        return G
    idx = torch.cat((torch.zeros(*keep.shape[:2], 1, dtype=torch.int64), 1 + keep), dim=2)
    return torch.gather(G, 2, idx[..., None].expand(-1, -1, -1, G.shape[-1]))


NAMES = ("x", "dW", "db", "dcls", "dpos")


def _embed_ref64(cfg, sd, img, G, keep):
    """float64 autograd on the operands the kernels see: the bf16-rounded volume and weight and, for dW alone, the bf16-rounded token
    gradient (the weight-gradient GEMM's operand; dpos, dcls and db are summed from the fp32 gradient)."""
    out = {}
    for names, g in ((("x", "db", "dcls", "dpos"), G), (("dW",), R.bf16_round(G))):
        leaf = {k: v.double().requires_grad_() for k, v in sd.items()}
        x = torch.stack(embed_kept(leaf, img.double(), cfg, keep))
        (x * _rows_of(g, keep).double()).sum().backward()
        got = dict(zip(NAMES, (x.detach(), leaf["patch_to_embedding.weight"].grad, leaf["patch_to_embedding.bias"].grad, leaf["cls_token"].grad, leaf["pos_embedding"].grad)))
        out.update({k: got[k] for k in names})
    return out


def _embed_gpu(cfg, sd, img, G, keep):
    import xvit.functional as XF
    leaf = {k: v.to(dev()).requires_grad_() for k, v in sd.items()}
    kp = None
    if keep is not None:
        keep_idx = keep.reshape(-1, keep.shape[-1]).to(torch.int32)
        kp = (keep_idx.to(dev()), torch.from_numpy(T.slot_of(keep_idx.numpy(), leaf["pos_embedding"].shape[1] - 1)).to(dev()))
    outs = XF.PatchEmbedFn.apply(img.to(dev()), leaf["patch_to_embedding.weight"], leaf["patch_to_embedding.bias"], leaf["cls_token"], leaf["pos_embedding"],
                                 tuple(cfg.patch_size), 0.0, False, kp)
    x = torch.stack(outs)
    (x * _rows_of(G, keep).to(dev())).sum().backward()
    torch.cuda.synchronize()
    return dict(zip(NAMES, (x.detach(), leaf["patch_to_embedding.weight"].grad, leaf["patch_to_embedding.bias"].grad, leaf["cls_token"].grad, leaf["pos_embedding"].grad)))


def test_patch_embed_with_a_hand_made_keep(monkeypatch):
    """See the module docstring for the gate and the measured distances."""
    monkeypatch.setenv("XVIT_PATCH_EMBED", "unfused")
    cfg, sd, img, G, keep = _embed_operands()
    full_ref, full_gpu = _embed_ref64(cfg, sd, img, G, None), _embed_gpu(cfg, sd, img, G, None)
    gate = {k: 2.0 * note(f"tokdrop.embed.unselected.{k}", rel(full_gpu[k], full_ref[k])) for k in NAMES}
    sel_ref, sel_gpu = _embed_ref64(cfg, sd, img, G, keep), _embed_gpu(cfg, sd, img, G, keep)
    dist = {k: note(f"tokdrop.embed.selected.{k}", rel(sel_gpu[k], sel_ref[k])) for k in NAMES}
    ident = torch.arange(32).expand(3, 2, -1).contiguous()
    x_ident = _embed_gpu(cfg, sd, img, G, ident)["x"]
    d_ident = note("tokdrop.embed.identity_vs_unselected.x", rel(x_ident, full_gpu["x"]))
    for k in NAMES:
        print(f"tokdrop embed {k}: unselected {gate[k] / 2:.3e} selected {dist[k]:.3e}")
    print(f"tokdrop embed identity x vs unselected x: {d_ident:.3e}")
    assert sel_gpu["x"].shape == (3, 2, 17, 256) and sel_gpu["dpos"].shape == (1, 33, 256)
    for k in NAMES:
        assert dist[k] <= gate[k], (k, dist[k], gate[k])
    assert d_ident <= gate["x"], (d_ident, gate["x"])
    # pos rows that no sequence kept get exactly nothing
    unkept = sorted(set(range(32)) - set(keep.reshape(-1).tolist()))
    assert bool((sel_gpu["dpos"][0, [1 + p for p in unkept]] == 0).all())


def test_patch_embed_refuses_input_gradients_under_keep():
    import xvit.functional as XF
    cfg, sd, img, G, keep = _embed_operands()
    keep_idx = keep.reshape(-1, 16).to(torch.int32)
    kp = (keep_idx.to(dev()), torch.from_numpy(T.slot_of(keep_idx.numpy(), 32)).to(dev()))
    leaf = {k: v.to(dev()).requires_grad_() for k, v in sd.items()}
    args = (leaf["patch_to_embedding.weight"], leaf["patch_to_embedding.bias"], leaf["cls_token"], leaf["pos_embedding"], tuple(cfg.patch_size), 0.0, False)
    with pytest.raises(RuntimeError, match="patch dropout"):
        XF.PatchEmbedFn.apply(img.to(dev()).requires_grad_(), *args, kp)
    outs = XF.PatchEmbedFn.apply(img.to(dev()).requires_grad_(), *args, None)      # without keep the volume gradient is there as before
    assert outs[0].shape == (2, 33, 256)


# ---- ModelCross ----------------------------------------------------------------------------------------------------------------------


def _model(name, **over):
    import xvit
    cfg = R.make_config(name, **over)
    sd = R.make_state_dict(cfg, seed=0)
    model = xvit.ModelCross(cfg).to(dev())
    model.load_state_dict(sd)
    return cfg, sd, model


def _seed_with_an_unkept_patch(M, B, P, K, shared=False):
    """A torch seed under which, by the restatement, the model's next draw leaves at least one patch to nobody: (seed, keep_idx [M*B, K]).
    Coupled to the host side on purpose, so that "the model draws what the restatement predicts" can be asserted: it restates
    functional.drop_seeds (initial seed and call counter) and takes the draw to be the FIRST seed a forward asks for.  A forward that
    takes a dropout seed before its draw makes the callers' `predicted` comparison fail; that, not the kernel, is then what changed."""
    import xvit.functional as XF
    for seed in range(200):
        drop_seed = ((seed & 0xFFFFFFFF) * 0x9E3779B1 + (XF._DROP_CALLS + 1) * 0x85EBCA77) & 0x7FFFFFFFFFFFFFFF      # functional.drop_seeds
        keep_idx, _ = T.draw(M * B, B, P, K, shared, drop_seed)
        if len(np.unique(keep_idx)) < P:
            return seed, keep_idx
    raise AssertionError("no seed below 200 leaves a patch unkept")


@pytest.mark.parametrize("name,batch", [("tiny", 4), ("small", 2)])
def test_model_cross_with_patch_dropout_vs_oracle_on_the_kept_tokens(name, batch):
    import xvit.functional as XF
    cfg, sd, model = _model(name, patch_dropout=0.5)
    g = R.derived(cfg)
    K = XF.patch_keep_count(g.P, 0.5)
    assert K == g.P // 2
    img, labels = R.make_inputs(cfg, batch, seed=0)
    model.train()
    seed, predicted = _seed_with_an_unkept_patch(g.M, batch, g.P, K)
    torch.manual_seed(seed)
    caps = {}
    hooks = [blk.register_forward_hook(lambda m, i, o, b=b: caps.__setitem__(b, [t.detach() for t in o])) for b, blk in enumerate(model.transformer)]
    logits, loss = model(img.to(dev()), labels.to(dev()))
    loss.backward()
    for h in hooks:
        h.remove()
    keep = model.last_token_keep
    assert keep.shape == (g.M, batch, K) and keep.dtype == torch.int32
    keep = keep.cpu().long()
    assert np.array_equal(keep.reshape(-1, K).numpy(), predicted)            # the model draws what the restatement says for its seed
    assert caps[0][0].shape == (batch, K + 1, g.d)
    # forward: the bf16-emulating oracle on the same tokens
    cap = {}
    with R.emulate_bf16():
        ref_logits, ref_loss = forward_kept(sd, img, labels, cfg, keep, capture=cap)
    for b in range(cfg.num_multi_blocks):
        for m in range(g.M):
            e_all, e_cls = rel(caps[b][m], cap[f"msb{b}"][m]), rel(caps[b][m][:, 0], cap[f"msb{b}"][m][:, 0])
            print(f"tokdrop model {name} msb{b} mod{m}: all {e_all:.3e} cls {e_cls:.3e}")
            assert e_all < 3e-3, (b, m, e_all)
            assert e_cls < 5.5e-3, (b, m, e_cls)
    print(f"tokdrop model {name}: logits {rel(logits, ref_logits):.3e} loss {abs(float(loss) - float(ref_loss)):.3e}")
    assert rel(logits, ref_logits) < 1.5e-2, rel(logits, ref_logits)
    assert abs(float(loss) - float(ref_loss)) < 2e-3
    # gradients: fp32 autograd of the same restated forward
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
    unkept = sorted(set(range(g.P)) - set(keep.reshape(-1).tolist()))
    assert unkept, "the seed was chosen so that some patch is kept by nobody"
    assert bool((model.pos_embedding.grad[0, [1 + p for p in unkept]] == 0).all())
    assert bool((model.pos_embedding.grad[0, 1 + int(keep[0, 0, 0])] != 0).any())


def _step(model, img, labels):
    for p in model.parameters():
        p.grad = None
    logits, loss = model(img, labels)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), float(loss.detach()), model.last_token_keep.clone() if model.last_token_keep is not None else None


def test_draw_properties_of_the_model():
    import xvit.functional as XF
    cfg, sd, model = _model("small", patch_dropout=0.5)
    img, labels = (t.to(dev()) for t in R.make_inputs(cfg, 2, seed=0))
    model.train()
    calls = XF._DROP_CALLS
    torch.manual_seed(11)
    l1, loss1, k1 = _step(model, img, labels)
    l2, loss2, k2 = _step(model, img, labels)
    assert k1.shape == (3, 2, 16) and not torch.equal(k1, k2) and not torch.equal(l1, l2)          # every forward draws anew
    assert bool((k1[:, :, 1:] > k1[:, :, :-1]).all()) and int(k1.min()) >= 0 and int(k1.max()) < 32
    assert not torch.equal(k1[0], k1[1])                                                              # modalities draw on their own
    XF._DROP_CALLS = calls
    torch.manual_seed(11)                                                                             # the seed stream from its start: the same draws
    l3, loss3, k3 = _step(model, img, labels)
    assert torch.equal(k1, k3) and torch.equal(l1, l3) and loss1 == loss3
    XF._DROP_CALLS = calls
    torch.manual_seed(12)
    assert not torch.equal(_step(model, img, labels)[2], k1)
    # eval() keeps every token and is the model without the option, bit for bit
    _, _, plain = _model("small")
    model.eval(), plain.eval()
    with torch.no_grad():
        a, la = model(img, labels)
        assert model.last_token_keep is None
        b, lb = plain(img, labels)
    assert torch.equal(a, b) and torch.equal(la, lb)
    # a volume that requires grad is refused in train(), served in eval()
    model.train()
    with pytest.raises(RuntimeError, match="patch dropout"):
        model(img.clone().requires_grad_(), labels)
    model.eval()
    vol = img.clone().requires_grad_()
    model(vol, labels)[1].backward()
    assert vol.grad is not None and bool(torch.isfinite(vol.grad).all())


def test_shared_draw_gives_every_modality_the_same_patches():
    cfg, sd, model = _model("small", patch_dropout=0.5, patch_dropout_shared=True)
    img, labels = (t.to(dev()) for t in R.make_inputs(cfg, 2, seed=0))
    model.train()
    _, _, keep = _step(model, img, labels)
    assert bool((keep == keep[0]).all()) and not torch.equal(keep[0, 0], keep[0, 1])                  # equal over modalities, not over samples


def test_patch_dropout_composes_with_the_embedding_dropout():
    """config.dropout > 0 as well: the embedding dropout's mask is keyed by the index in the SHORTER stacked token tensor, in the forward and
    in the backward (which then takes the stacked-gradient route).  The step repeats bit for bit from the same seeds, differs from the
    step without dropout on the same subset, and leaves finite gradients with zero position rows for the patches nobody kept."""
    import xvit.functional as XF
    cfg, sd, model = _model("small", patch_dropout=0.5, dropout=0.1)
    img, labels = (t.to(dev()) for t in R.make_inputs(cfg, 2, seed=0))
    model.train()
    seed, predicted = _seed_with_an_unkept_patch(3, 2, 32, 16)
    calls = XF._DROP_CALLS
    runs = []
    for _ in range(2):
        XF._DROP_CALLS = calls
        torch.manual_seed(seed)
        logits, loss, keep = _step(model, img, labels)
        runs.append((logits, loss, keep, model.pos_embedding.grad.clone(), model.patch_to_embedding.weight.grad.clone()))
    assert np.array_equal(runs[0][2].reshape(-1, 16).cpu().numpy(), predicted)
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and torch.equal(runs[0][3], runs[1][3]) and torch.equal(runs[0][4], runs[1][4])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    unkept = sorted(set(range(32)) - set(predicted.reshape(-1).tolist()))
    assert unkept and bool((runs[0][3][0, [1 + p for p in unkept]] == 0).all())
    _, _, plain = _model("small", patch_dropout=0.5)
    plain.train()
    XF._DROP_CALLS = calls
    torch.manual_seed(seed)
    logits0, _, keep0 = _step(plain, img, labels)
    assert torch.equal(keep0, runs[0][2]) and not torch.equal(logits0, runs[0][0])       # the same subset, other activations: the masks are real


def test_gradients_are_bit_reproducible_in_deterministic_mode(monkeypatch):
    import xvit.functional as XF
    from xvit import ops
    monkeypatch.setattr(ops, "DETERMINISTIC", True)
    cfg, sd, model = _model("small", patch_dropout=0.5)
    img, labels = (t.to(dev()) for t in R.make_inputs(cfg, 2, seed=0))
    model.train()
    runs = []
    calls = XF._DROP_CALLS
    for _ in range(2):
        XF._DROP_CALLS = calls
        torch.manual_seed(5)
        logits, loss, keep = _step(model, img, labels)
        runs.append((logits, loss, keep, {k: p.grad.clone() for k, p in model.named_parameters()}))
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    for k in runs[0][3]:
        assert torch.equal(runs[0][3][k], runs[1][3][k]), k


# ---- GraphedStep -----------------------------------------------------------------------------------------------------------------------


def test_graphed_step_draws_a_new_subset_per_replay_and_matches_eager_on_the_same_subset(monkeypatch):
    from xvit import ops
    from xvit.graph import GraphedStep
    cfg, sd, model = _model("tiny", patch_dropout=0.5)
    assert cfg.dropout == 0.0                                        # patch dropout alone must switch the epoch counter on
    img, labels = (t.to(dev()) for t in R.make_inputs(cfg, 4, seed=0))
    model.train()
    torch.manual_seed(3)
    step = GraphedStep(model, img, labels)
    assert step._epoch is not None and ops._DROP_EPOCH is None
    logits1, loss1 = step()
    torch.cuda.synchronize()
    keep1, logits1, loss1 = model.last_token_keep.clone(), logits1.clone(), float(loss1)
    grads1 = {k: p.grad.clone() for k, p in model.named_parameters()}
    step()
    torch.cuda.synchronize()
    keep2 = model.last_token_keep.clone()
    assert keep1.shape == (2, 4, 8) and not torch.equal(keep1, keep2)
    # the eager step on the subset of the first replay: the draw is replaced by a copy of that subset
    slot1 = torch.from_numpy(T.slot_of(keep1.reshape(8, 8).cpu().numpy(), 16)).to(dev())

    def fixed_draw(keep_idx, slot, B, shared, seed):
        keep_idx.copy_(keep1.reshape(keep_idx.shape))
        slot.copy_(slot1)
        return keep_idx, slot

    monkeypatch.setattr(ops, "token_select_draw", fixed_draw)
    le, losse, keepe = _step(model, img, labels)
    assert torch.equal(keepe, keep1)
    assert torch.equal(le, logits1) and losse == loss1               # same kernels, same order: bit-identical
    for k, p in model.named_parameters():                            # gates of tests/test_graph_gpu.py between graph and eager
        assert rel(p.grad, grads1[k]) < 1e-5 or float(grads1[k].abs().max()) < 1e-6, k


def test_replays_survive_eager_steps_at_another_batch(monkeypatch):
    """The last batch of an epoch is ragged: an eager train() step at batch 3 between the replays of a step captured at batch 4.  The draw's
    two tensors belong to the graph's pool, so the replay after it still draws into them what the restatement says for the captured
    seed and the epoch of that replay, follows it through the model, and the eager step is an ordinary one."""
    from xvit import ops
    from xvit.graph import GraphedStep
    calls = []
    real = ops.token_select_draw

    def recording(keep_idx, slot, B, shared, seed):
        calls.append((keep_idx, slot, B, seed))
        return real(keep_idx, slot, B, shared, seed)

    monkeypatch.setattr(ops, "token_select_draw", recording)
    cfg, sd, model = _model("tiny", patch_dropout=0.5)
    img4, lab4 = (t.to(dev()) for t in R.make_inputs(cfg, 4, seed=0))
    img3, lab3 = (t.to(dev()) for t in R.make_inputs(cfg, 3, seed=1))
    model.train()
    step = GraphedStep(model, img4, lab4)
    keep_idx, slot, B, seed = calls[-1]                               # the capture's own draw: these tensors are the graph's
    assert keep_idx.shape == (8, 8) and slot.shape == (8, 16) and B == 4
    assert model.last_token_keep.data_ptr() == keep_idx.data_ptr()

    def replay_and_check():
        logits, loss = step()
        torch.cuda.synchronize()
        ref_k, ref_s = T.draw(8, 4, 16, 8, False, seed, epoch=int(step._epoch))
        assert np.array_equal(keep_idx.cpu().numpy(), ref_k) and np.array_equal(slot.cpu().numpy(), ref_s)
        assert bool(torch.isfinite(logits).all()) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
        unkept = sorted(set(range(16)) - set(ref_k.reshape(-1).tolist()))
        assert bool((model.pos_embedding.grad[0, [1 + p for p in unkept]] == 0).all())      # the backward read THIS draw's slot
        return logits.clone(), ref_k

    l1, k1 = replay_and_check()
    n = len(calls)
    _, _, keep3 = _step(model, img3, lab3)                            # the ragged tail, eagerly
    assert len(calls) == n + 1 and calls[-1][0].shape == (6, 8) and calls[-1][0].data_ptr() != keep_idx.data_ptr()
    assert keep3.shape == (2, 3, 8)
    assert np.array_equal(keep3.reshape(6, 8).cpu().numpy(), T.draw(6, 3, 16, 8, False, calls[-1][3])[0])
    l2, k2 = replay_and_check()
    assert not np.array_equal(k1, k2) and not torch.equal(l1, l2)
    _step(model, img4, lab4)                                          # and an eager step at the captured batch
    assert calls[-1][0].data_ptr() != keep_idx.data_ptr()
    replay_and_check()

