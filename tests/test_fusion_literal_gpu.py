"""GPU: the fusion's literal-order K/V path ("dense": kv = hn Wkv^T + b, xvit_cls_xattn_fwd / _bwd, the K = 2 d dgrad, wgrad and column
sum) against the reference and the oracle, at the gates the low-rank form is held to.  It is a product path: the default for small eager
batches (XATTN_FORM = "auto" below 8192 token rows, e.g. the reference's own run shape at its batch of 8) and the only form above 16 heads,
captured steps included.

Every test that means the dense form proves it ran: the step is profiled (ops.PROFILE) and must have launched cls_xattn_fwd and
cls_xattn_bwd and none of the low-rank form's kernels (cls_softmax, head_linear, xattn_kv_dgrad).  The tests select the form in their
body; that runs after the suite's autouse fixture, so it wins."""
import pytest
import torch

import ref_cpu as R
from _util import dev, note, randn, rel
from test_modules_gpu import BLOCK_TOL, GRAD_TOL, _check_model_vs_golden, _check_unobserved_matches_observed, _run_model, _sub

pytestmark = pytest.mark.gpu

DENSE = {"cls_xattn_fwd", "cls_xattn_bwd"}
LOWRANK = {"cls_softmax", "head_linear", "xattn_kv_dgrad"}


def _profiled(monkeypatch, fn):
    """Run fn with the per-launch profile on; -> (fn's result, the set of kernel families it launched)."""
    from xvit import ops
    monkeypatch.setattr(ops, "PROFILE", [])
    try:
        out = fn()
        torch.cuda.synchronize()
        fam = {e[0] for e in ops.PROFILE}
    finally:
        monkeypatch.setattr(ops, "PROFILE", None)
    return out, fam


def _assert_form(fam, form):
    if form == "dense":
        assert DENSE <= fam and not fam & LOWRANK, f"the literal order did not run: {sorted(fam)}"
    else:
        assert LOWRANK <= fam and not fam & DENSE, f"the low-rank form did not run: {sorted(fam)}"


def _set_form(monkeypatch, form):
    import xvit.functional as XF
    monkeypatch.setattr(XF, "XATTN_FORM", form)


# ------------------------------------------------------------------------------------------ gate (2): the reference's own outputs
@pytest.mark.parametrize("name,batch,fixture,over", [("tiny", 4, None, {}), ("small", 2, None, {}), ("base", 2, None, {}), ("mist", 2, None, {}),
                                                      ("tiny", 3, "partial", dict(num_modalities=3, attn_order={"0": "1", "1": "2"}))],
                         ids=["tiny", "small", "base", "mist", "partial"])
def test_dense_model_cross_vs_reference_golden(monkeypatch, golden_dir, name, batch, fixture, over):
    """The goldens of test_modules_gpu.test_model_cross_vs_reference_golden (same gates) with the literal order forced."""
    _set_form(monkeypatch, "dense")
    _, fam = _profiled(monkeypatch, lambda: _check_model_vs_golden(golden_dir, name, batch, fixture=fixture, **over))
    _assert_form(fam, "dense")


def test_dense_model_cross_base_with_cls_peel_vs_reference_golden(monkeypatch, golden_dir):
    from xvit import ops
    _set_form(monkeypatch, "dense")
    ops.set_option("attn_peel", 2)
    try:
        _, fam = _profiled(monkeypatch, lambda: _check_model_vs_golden(golden_dir, "base", 2))
    finally:
        ops.set_option("attn_peel", 1)
    _assert_form(fam, "dense")


def test_auto_form_takes_the_literal_order_at_the_reference_run_shape(monkeypatch, golden_dir):
    """XATTN_FORM = "auto" (the default) at the reference's run shape and a small eager batch (mist, 2 x 513 = 1026 token rows): the step
    a main_mist.py user gets.  It must choose the literal order and meet the goldens."""
    _set_form(monkeypatch, "auto")
    _, fam = _profiled(monkeypatch, lambda: _check_model_vs_golden(golden_dir, "mist", 2))
    _assert_form(fam, "dense")


# ------------------------------------------------------------------------------------------ gate (1): the literal-order emulation
@pytest.mark.parametrize("name,batch", [("tiny", 4), ("small", 2), ("base", 2)])
def test_dense_model_cross_vs_literal_bf16_emulating_oracle(monkeypatch, name, batch):
    """The gates of test_modules_gpu.test_model_cross_vs_bf16_emulating_oracle against R.emulate_bf16(xattn="literal"), the rounding points
    of the dense form (k and v stored bf16; q, P and proj fp32).  base: every parameter gradient's norm against the emulating oracle's
    autograd at 1 %, as test_large_configs_vs_bf16_emulating_oracle."""
    _set_form(monkeypatch, "dense")
    (cfg, sd, img, labels, model, caps, logits, loss), fam = _profiled(monkeypatch, lambda: _run_model(name, batch))
    _assert_form(fam, "dense")
    cap = {}
    grads = name == "base"
    leaf = {k: v.detach().clone().requires_grad_(grads) for k, v in sd.items()}
    with R.emulate_bf16(xattn="literal"):
        ref_logits, ref_loss = R.model_cross_forward(leaf, img, labels, cfg, capture=cap)
        if grads:
            ref_loss.backward()
    e_blk = e_cls = 0.0
    for b in range(cfg.num_multi_blocks):
        for m in range(cfg.num_modalities):
            ref = cap[f"msb{b}"][m].detach()
            eb, ec = rel(caps[b][m], ref), rel(caps[b][m][:, 0], ref[:, 0])
            e_blk, e_cls = max(e_blk, eb), max(e_cls, ec)
            assert eb < 3e-3 and ec < 5.5e-3, (b, m, eb, ec)       # measured worst: blocks 1.9e-3, CLS rows 4.6e-3 (base)
    note(f"dense_vs_literal_emu.{name}.block", e_blk)
    note(f"dense_vs_literal_emu.{name}.cls", e_cls)
    assert note(f"dense_vs_literal_emu.{name}.logits", rel(logits, ref_logits)) < 1.5e-2, rel(logits, ref_logits)   # measured 2.4e-3 .. 8.4e-3
    assert abs(float(loss) - float(ref_loss)) < 2e-3
    if grads:
        worst = 0.0
        for k, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
            if k.endswith("wk.bias"):
                assert float(p.grad.abs().max()) < 1e-3          # analytically zero (softmax shift invariance)
                continue
            ref_n, got_n = float(leaf[k].grad.double().norm()), float(p.grad.double().norm())
            worst = max(worst, abs(got_n - ref_n) / (ref_n + 1e-12))
            assert abs(got_n - ref_n) <= 0.01 * ref_n + 1e-7, (k, got_n, ref_n)     # measured worst 3.2e-3
        note(f"dense_vs_literal_emu.{name}.worst_grad_norm_dev", worst)


@pytest.mark.parametrize("name,over", [("tiny", {}), ("small", {}),
                                       ("tiny", dict(num_modalities=4, attn_order={"0": "1", "1": "2", "2": "3", "3": "0"})),
                                       ("tiny", dict(num_modalities=3, attn_order={"0": "2"}))])
def test_dense_unobserved_last_block_cls_only_path_matches_full_path(monkeypatch, name, over):
    """test_modules_gpu.test_unobserved_last_block_cls_only_path_matches_full_path in the literal order: the CLS-only last block hands the
    fusion the CLS rows alone (a [B, 1, d] xi)."""
    _set_form(monkeypatch, "dense")
    _, fam = _profiled(monkeypatch, lambda: _check_unobserved_matches_observed(name, over))
    _assert_form(fam, "dense")


# ------------------------------------------------------------------------------------------ fusion dropout with the kernels' own masks
def _fusion_oracle(leaf, pfx, xcat, cls_res, H, masks):
    """model_cross.py:88-114 with the dropout sites of :97 (probabilities), :101 (proj output), :25 (after GELU), :27 (FFN output) as
    explicit masks (0 or 1 / (1 - p)); xcat = the fusion's input, cls_res = its un-normed row 0 (the residual)."""
    m_attn, m_proj, m_gelu, m_ffn = masks
    d = xcat.shape[-1]
    a = pfx + ".attn.fn"
    x = R.layer_norm(xcat, leaf[pfx + ".attn.norm.weight"], leaf[pfx + ".attn.norm.bias"])
    q = R._split_heads(R.linear(x[:, 0:1], leaf[a + ".wq.weight"], leaf[a + ".wq.bias"]), H)
    k = R._split_heads(R.linear(x, leaf[a + ".wk.weight"], leaf[a + ".wk.bias"]), H)
    v = R._split_heads(R.linear(x, leaf[a + ".wv.weight"], leaf[a + ".wv.bias"]), H)
    P = torch.softmax((q @ k.transpose(-1, -2)) * (d // H) ** -0.5, dim=-1)          # [B, H, 1, N]
    o = R._merge_heads((P * m_attn[:, :, None, :]) @ v)                              # [B, 1, d]
    y = R.linear(o, leaf[a + ".proj.weight"], leaf[a + ".proj.bias"]) * m_proj[:, None] + cls_res
    f = pfx + ".ffn"
    h = R.layer_norm(y, leaf[f + ".norm.weight"], leaf[f + ".norm.bias"])
    h = R.gelu(R.linear(h, leaf[f + ".fn.net.0.weight"], leaf[f + ".fn.net.0.bias"])) * m_gelu[:, None]
    return y + R.linear(h, leaf[f + ".fn.net.3.weight"], leaf[f + ".fn.net.3.bias"]) * m_ffn[:, None]


@pytest.mark.parametrize("form", ["lowrank", "dense"])
@pytest.mark.parametrize("site", ["cross_block", "msb_fusion"])
def test_fusion_training_dropout_matches_oracle_with_same_masks(monkeypatch, form, site):
    """The fusion at p = 0.25 on all four of its dropout sites, in both forms: the masks the kernels drew (a pure function of seed and element
    index) are regenerated with xvit_dropout on ones and fed to an fp32 oracle.  Output and input gradients at the block gates, every
    parameter gradient at GRAD_TOL.  site: a stand-alone CrossAttentionBlock (cls and tokens from one tensor) and the first fusion of a
    MultiScaleBlock as that block calls it (cls rows of modality 0, patch tokens of modality 1, the new CLS row spliced into a copy of
    modality 0's tokens)."""
    import xvit
    import xvit.functional as XF
    from xvit import ops
    from xvit.cross_vit import _fusion_args
    p = 0.25
    cfg = R.make_config("small", dropout=p)
    sd = R.make_state_dict(cfg, seed=3)
    pfx = "transformer.0.fusion.0"
    B, N, d, f, H = 2, 65, cfg.hidden_dim, cfg.mlp_dim, cfg.num_heads
    _set_form(monkeypatch, form)
    xi, xj, w = randn(B, N, d, seed=21), randn(B, N, d, seed=22), randn(B, N if site == "msb_fusion" else 1, d, seed=23)
    if site == "cross_block":
        mod = xvit.CrossAttentionBlock(cfg).to(dev())
        mod.load_state_dict(_sub(sd, pfx))
        mod.train()
    else:
        msb = xvit.MultiScaleBlock(cfg).to(dev())
        msb.load_state_dict(_sub(sd, "transformer.0"))
        msb.train()
        mod = msb.fusion[0]
    xri, xrj = xi.to(dev()).requires_grad_(), xj.to(dev()).requires_grad_()
    monkeypatch.setattr(XF, "_DROP_CALLS", 1000)

    def step():
        if site == "cross_block":
            y = mod(xri)
        else:        # MultiScaleBlock.forward's call for modality 0 (attn_order 0 <- 1), training mode
            y = XF.CrossFusionFn.apply(xri, xrj, *_fusion_args(mod), True, p, False)
        (y * w.to(dev())).sum().backward()
        return y.detach()

    y, fam = _profiled(monkeypatch, step)
    _assert_form(fam, form)
    monkeypatch.setattr(XF, "_DROP_CALLS", 1000)
    s_attn, s_proj, s_gelu, s_ffn = XF.drop_seeds(4)                # cross_forward's order: probabilities, proj, after GELU, FFN output
    mk = lambda shape, s: ops.dropout(torch.ones(*shape, device=dev()), p, s).cpu()     # noqa: E731
    masks = (mk((B, H, N), s_attn), mk((B, d), s_proj), mk((B, f), s_gelu), mk((B, d), s_ffn))
    assert all(0 < float((m == 0).float().mean()) < 0.5 for m in masks)
    leaf = {k: v.clone().requires_grad_() for k, v in sd.items() if k.startswith(pfx + ".")}
    xo_i, xo_j = xi.clone().requires_grad_(), xj.clone().requires_grad_()
    if site == "cross_block":
        yo = _fusion_oracle(leaf, pfx, xo_i, xo_i[:, 0:1], H, masks)
    else:        # model_cross.py:140-142
        yo = torch.cat((_fusion_oracle(leaf, pfx, torch.cat((xo_i[:, 0:1], xo_j[:, 1:]), dim=1), xo_i[:, 0:1], H, masks), xo_i[:, 1:]), dim=1)
    (yo * w).sum().backward()
    tag = f"fusion_dropout.{site}.{form}"
    if site == "msb_fusion":
        assert torch.equal(y[:, 1:].cpu(), xi[:, 1:]), "the patch rows of the spliced output are not modality 0's"
        assert note(f"{tag}.y_cls", rel(y[:, 0], yo[:, 0])) < BLOCK_TOL
        assert note(f"{tag}.dxj", rel(xrj.grad, xo_j.grad)) < GRAD_TOL, rel(xrj.grad, xo_j.grad)
    assert note(f"{tag}.y", rel(y, yo)) < BLOCK_TOL, rel(y, yo)
    assert note(f"{tag}.dx", rel(xri.grad, xo_i.grad)) < GRAD_TOL, rel(xri.grad, xo_i.grad)
    worst = (0.0, "")
    grads = dict(mod.named_parameters())
    for k, prm in grads.items():
        ref = leaf[pfx + "." + k].grad
        if k.endswith("wk.bias"):
            # analytically zero (softmax shift invariance): the low-rank form returns 0, the literal order the column sum of the bf16-rounded
            # dk rows, i.e. their rounding noise (measured at this loss scale: 0.2 % of wq.bias's gradient); harmless, bk does not enter the function
            assert float(ref.abs().max()) < 1e-4, k
            assert note(f"{tag}.wk_bias_vs_wq_bias", float(prm.grad.norm() / grads["attn.fn.wq.bias"].grad.norm())) < 0.05, k
            continue
        worst = max(worst, (rel(prm.grad, ref), k))
    note(f"{tag}.worst_param_grad", worst[0])      # measured: y 1.2e-3, dx 4.8e-3, dxj 8.1e-3, worst parameter 1.25e-2 (low-rank) / 6.5e-3 (dense)
    assert worst[0] < GRAD_TOL, worst


# ------------------------------------------------------------------------------------------ more than 16 heads: only the literal order
WIDE = {"H20": dict(hidden_dim=1280, num_heads=20, mlp_dim=2560),
        "H32": dict(hidden_dim=2048, num_heads=32, mlp_dim=4096, num_multi_blocks=1)}     # one MultiScaleBlock: 0.23 G parameters


@pytest.mark.parametrize("wide", sorted(WIDE))
def test_more_than_16_heads_vs_oracle(monkeypatch, wide):
    """small's geometry (N = 33, 3-ring) with 20 heads (d = 1280) and 32 heads (d = 2048): the low-rank kernels are built for H <= 16, so
    every XATTN_FORM runs the literal order here.  Forward against the fp32 oracle (gate (2)) and the bf16 emulation (gate (1); it takes
    its literal branch by itself above 16 heads), every parameter gradient's norm against the emulating oracle's autograd at 1 %."""
    _set_form(monkeypatch, "lowrank")                               # what the suite's fixture asks for: not available here
    (cfg, sd, img, labels, model, caps, logits, loss), fam = _profiled(monkeypatch, lambda: _run_model("small", 2, **WIDE[wide]))
    _assert_form(fam, "dense")
    cap32 = {}
    ref32_logits, ref32_loss = R.model_cross_forward(sd, img, labels, cfg, capture=cap32)
    cap = {}
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    with R.emulate_bf16():
        ref_logits, ref_loss = R.model_cross_forward(leaf, img, labels, cfg, capture=cap)
        ref_loss.backward()
    e = dict(blk32=0.0, cls32=0.0, blk=0.0, cls=0.0)
    for b in range(cfg.num_multi_blocks):
        for m in range(cfg.num_modalities):
            t, r32, r = caps[b][m], cap32[f"msb{b}"][m], cap[f"msb{b}"][m].detach()
            e["blk32"], e["cls32"] = max(e["blk32"], rel(t, r32)), max(e["cls32"], rel(t[:, 0], r32[:, 0]))
            e["blk"], e["cls"] = max(e["blk"], rel(t, r)), max(e["cls"], rel(t[:, 0], r[:, 0]))
    e["logits32"], e["logits"] = rel(logits, ref32_logits), rel(logits, ref_logits)
    for k, v in e.items():
        note(f"wide_heads.{wide}.{k}", v)
    # measured H20 | H32: blk32 4.0e-3 | 3.6e-3, cls32 6.7e-3 | 6.0e-3, logits32 6.0e-3 | 1.0e-2, blk 1.8e-3 | 1.3e-3, cls 2.9e-3 | 2.7e-3,
    # logits 7.3e-3 | 4.3e-3; worst gradient-norm deviation 2.0e-3 | 8.9e-4
    gates = dict(blk32=BLOCK_TOL, cls32=8e-3, logits32=1.8e-2, blk=3e-3, cls=5.5e-3, logits=1.5e-2)
    assert all(e[k] < gates[k] for k in gates), (e, gates)
    assert abs(float(loss) - float(ref32_loss)) < 5e-3 and abs(float(loss) - float(ref_loss)) < 2e-3
    worst = 0.0
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if k.endswith("wk.bias"):
            assert float(p.grad.abs().max()) < 1e-3
            continue
        ref_n, got_n = float(leaf[k].grad.double().norm()), float(p.grad.double().norm())
        worst = max(worst, abs(got_n - ref_n) / (ref_n + 1e-12))
        assert abs(got_n - ref_n) <= 0.01 * ref_n + 1e-7, (k, got_n, ref_n)
    note(f"wide_heads.{wide}.worst_grad_norm_dev", worst)


def test_graphed_step_with_20_heads_matches_eager(monkeypatch):
    """A captured training step (xvit.graph.GraphedStep) above 16 heads, where the capture cannot switch to the low-rank form: replays
    equal the eager step and follow new inputs, and the captured fusions are the literal order's kernels."""
    import xvit
    from xvit import ops
    from xvit.graph import GraphedStep
    _set_form(monkeypatch, "auto")
    cfg = R.make_config("small", **WIDE["H20"])
    model = xvit.ModelCross(cfg).to(dev())
    model.load_state_dict(R.make_state_dict(cfg, seed=0))
    model.train()
    img1, lab1 = (t.to(dev()) for t in R.make_inputs(cfg, 2, seed=0))
    img2, lab2 = (t.to(dev()) for t in R.make_inputs(cfg, 2, seed=9))

    def eager(img, lab):
        for p in model.parameters():
            p.grad = None
        logits, loss = model(img, lab)
        loss.backward()
        return logits.detach().clone(), float(loss.detach()), {k: p.grad.clone() for k, p in model.named_parameters()}

    e1, e2 = eager(img1, lab1), eager(img2, lab2)
    captured = []                                         # (family, launched while a capture was open)
    for name in ("cls_xattn_fwd", "cls_xattn_bwd", "cls_softmax_fwd", "cls_softmax_bwd", "xattn_kv_dgrad"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _fn=fn, _n=name, **k: (captured.append((_n, torch.cuda.is_current_stream_capturing())), _fn(*a, **k))[1])
    step = GraphedStep(model, img1, lab1)
    in_graph = {n for n, c in captured if c}
    assert in_graph == {"cls_xattn_fwd", "cls_xattn_bwd"}, captured
    for (img, lab), (el, eloss, eg) in (((img1, lab1), e1), ((img2, lab2), e2), ((img1, lab1), e1)):
        logits, loss = step(img, lab)
        torch.cuda.synchronize()
        assert torch.equal(logits, el) and float(loss.detach()) == eloss
        for k, p in model.named_parameters():
            assert rel(p.grad, eg[k]) < 1e-5 or float(eg[k].abs().max()) < 1e-6, k


# ------------------------------------------------------------------------------------------ head widths other than 64
@pytest.mark.parametrize("over", [dict(num_heads=4), dict(num_heads=4, num_self_blocks=0), dict(hidden_dim=256, mlp_dim=512, num_heads=2)],
                         ids=["dh48", "dh48_fusion_only", "dh128"])
def test_head_width_other_than_64_is_refused_on_the_first_forward(over):
    """The attention kernels and the fusion's (both forms) are built for 64-wide heads only: a model whose hidden_dim / num_heads is not
    64 must fail its first forward with an error that names the head dim, whichever kernel meets it first (with no self-attention blocks
    that is the fusion's)."""
    import xvit
    cfg = R.make_config("tiny", **over)
    dh = cfg.hidden_dim // cfg.num_heads
    model = xvit.ModelCross(cfg).to(dev())
    img, labels = R.make_inputs(cfg, 2, seed=0)
    with pytest.raises(RuntimeError, match=f"head dim {dh} unsupported"):
        model(img.to(dev()), labels.to(dev()))
