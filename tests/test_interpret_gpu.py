"""GPU: xvit.interpret.attention_maps against the bf16-emulating oracle, and its invariants.

Reference: R.softmax_attention is wrapped (monkeypatch, the oracle itself is unchanged) to record softmax(q k^T scale) in float64 at every
call site of R.model_cross_forward / R.model_vit_forward under R.emulate_bf16(xattn="literal") — the order in which the oracle calls it
names the site (per MultiScaleBlock: the branches' self-attention blocks, then the fusions).  The literal order is what calls
softmax_attention for the fusions; the low-rank GPU form is held to the same reference.  Rollout reference: float64 matrix products.

Gates, rel-L2 per map: 1.5 x the largest distance measured on an MI355X (XVIT_MEASURE_LOG), ceiling 1e-2.  Measured over tiny, small and
the ModelVIT config: self-attention maps <= 2.7e-3 (tiny), fusion maps <= 4.7e-3 in the low-rank form (its bf16 weights e, small) and
<= 4.0e-3 in the literal order (tiny), rollout <= 2.0e-4 (small, literal order).  The map rows are >= 0 and sum to one
within 1e-5: the self-attention and literal-order maps are fp32 softmax rows, and the low-rank maps are e rz with rz = 1 / sum of the
ROUNDED e (cls_softmax_kernel in csrc/head_linear.hip), so they too sum to one up to fp32 rounding."""
import pytest
import torch

import ref_cpu as R
from _util import dev, note, rel

pytestmark = pytest.mark.gpu

GATE = {"self": 4.1e-3, "fusion_lowrank": 7.1e-3, "fusion_dense": 6e-3, "rollout": 3e-4}


def _model(kind, name="tiny", batch=2, **over):
    import xvit
    if kind == "vit":
        cfg = R.make_config(name, num_layers=2, **over)
        sd = R.make_vit_state_dict(cfg, seed=0)
        model = xvit.ModelVIT(cfg).to(dev())
    else:
        cfg = R.make_config(name, **over)
        sd = R.make_state_dict(cfg, seed=0)
        model = xvit.ModelCross(cfg).to(dev())
    model.load_state_dict(sd)
    model.eval()
    img, labels = R.make_inputs(cfg, batch, seed=0)
    return cfg, sd, model, img, labels


def _site_names(kind, cfg):
    """Module names in the order the oracle reaches softmax_attention."""
    if kind == "vit":
        return [f"transformer.layers.{l}" for l in range(cfg.num_layers)]
    names = []
    for b in range(cfg.num_multi_blocks):
        names += [f"transformer.{b}.blocks.{m}.{s}" for m in range(cfg.num_modalities) for s in range(cfg.num_self_blocks)]
        names += [f"transformer.{b}.fusion.{k}" for k in range(len(cfg.attn_order))]
    return names


def _oracle_maps(kind, cfg, sd, img, labels, monkeypatch):
    probs = []
    inner = R.softmax_attention

    def recording(q, k, v, scale):
        probs.append(torch.softmax((q.double() @ k.double().transpose(-1, -2)) * scale, dim=-1))
        return inner(q, k, v, scale)

    monkeypatch.setattr(R, "softmax_attention", recording)
    with R.emulate_bf16(xattn="literal"):
        (R.model_vit_forward if kind == "vit" else R.model_cross_forward)(sd, img, labels, cfg)
    monkeypatch.setattr(R, "softmax_attention", inner)
    names = _site_names(kind, cfg)
    assert len(probs) == len(names)
    P = dict(zip(names, probs))
    cls = {n: p[:, :, 0, :] for n, p in P.items()}
    chains = {0: names} if kind == "vit" else {
        m: [f"transformer.{b}.blocks.{m}.{s}" for b in range(cfg.num_multi_blocks) for s in range(cfg.num_self_blocks)] for m in range(cfg.num_modalities)}
    roll = {}
    for key, chain in chains.items():
        if not chain:
            continue
        r = torch.zeros(img.shape[0], P[chain[0]].shape[-1], dtype=torch.float64)
        r[:, 0] = 1.0
        for n in reversed(chain):
            r = 0.5 * r + 0.5 * torch.einsum("bm,bhmn->bn", r, P[n]) / P[n].shape[1]
        roll[key] = r
    return cls, roll


def _check_rows(t, what):
    t = t.double().cpu()
    assert (t >= 0).all(), f"{what}: negative probabilities"
    dev_ = (t.sum(dim=-1) - 1.0).abs().max().item()
    assert dev_ <= 1e-5, f"{what}: rows sum to 1 +- {dev_:.2e}"


@pytest.mark.parametrize("kind,name,form", [("cross", "tiny", "lowrank"), ("cross", "tiny", "dense"), ("cross", "small", "lowrank"),
                                            ("cross", "small", "dense"), ("vit", "small", "lowrank")])
def test_maps_vs_bf16_emulating_oracle(kind, name, form, monkeypatch):
    import xvit
    import xvit.functional as XF
    monkeypatch.setattr(XF, "XATTN_FORM", form)
    cfg, sd, model, img, labels = _model(kind, name)
    maps = xvit.interpret.attention_maps(model, img.to(dev()), rollout=True)
    torch.cuda.synchronize()
    cls, roll = _oracle_maps(kind, cfg, sd, img, labels, monkeypatch)
    assert set(maps.self_attn) | set(maps.fusion) == set(cls)
    for n, ref in cls.items():
        fus = ".fusion." in n
        got = maps.fusion[n] if fus else maps.self_attn[n]
        assert got.shape == ref.shape and got.dtype == torch.float32
        _check_rows(got, n)
        e = note(f"maps_{kind}_{name}_{form}_{'fusion' if fus else 'self'}", rel(got, ref))
        g = GATE["fusion_" + form if fus else "self"]
        assert e <= g, f"{n}: rel-L2 {e:.3e} > {g:g}"
    assert set(maps.rollout) == set(roll)
    for key, ref in roll.items():
        _check_rows(maps.rollout[key], f"rollout {key}")
        e = note(f"maps_{kind}_{name}_{form}_rollout", rel(maps.rollout[key], ref))
        assert e <= GATE["rollout"], f"rollout {key}: rel-L2 {e:.3e} > {GATE['rollout']:g}"


@pytest.mark.parametrize("kind", ["cross", "vit"])
def test_recorded_pass_logits_and_repeatability(kind):
    """The recorded pass computes what a plain eval forward computes (bit for bit), two calls give identical maps, B = 1 works."""
    import xvit
    cfg, sd, model, img, labels = _model(kind, "small")
    x = img.to(dev())
    plain, _ = model(x, labels.to(dev()))
    a = xvit.interpret.attention_maps(model, x, rollout=True)
    b = xvit.interpret.attention_maps(model, x, rollout=True)
    torch.cuda.synchronize()
    assert torch.equal(a.logits, plain.detach()), "recorded pass changed the logits"
    for da, db in ((a.self_attn, b.self_attn), (a.fusion, b.fusion), (a.rollout, b.rollout)):
        assert da.keys() == db.keys() and all(torch.equal(da[k], db[k]) for k in da)
    one = xvit.interpret.attention_maps(model, x[:1], rollout=True)
    torch.cuda.synchronize()
    for k, v in one.self_attn.items():
        assert v.shape[0] == 1 and torch.isfinite(v).all()
        assert rel(v[0], a.self_attn[k][0]) < 1e-2      # the same sample at B = 1 (the GEMM tiling may differ with the batch)
    assert all(v.shape[0] == 1 for v in one.rollout.values())


def test_no_rollout_entry_without_self_blocks():
    import xvit
    _, _, model, img, _ = _model("cross", "tiny", num_self_blocks=0)
    maps = xvit.interpret.attention_maps(model, img.to(dev()), rollout=True)
    assert maps.rollout == {} and maps.self_attn == {} and len(maps.fusion) == 4


def test_refusals_and_state_reset(monkeypatch):
    import xvit
    import xvit.functional as XF
    from xvit.cross_vit import STREAM_MODE
    _, _, model, img, _ = _model("cross", "tiny")
    x = img.to(dev())
    xvit.interpret.attention_maps(model, x, rollout=True)
    assert STREAM_MODE.get() is None and XF.ATTN_RECORDER.get() is None
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        xvit.interpret.attention_maps(model, x)
    model.eval()
    monkeypatch.setenv("XVIT_ATTN_FP8", "1")
    with pytest.raises(RuntimeError, match="XVIT_ATTN_FP8"):
        xvit.interpret.attention_maps(model, x)
    monkeypatch.delenv("XVIT_ATTN_FP8")
    with pytest.raises(RuntimeError, match="GPU"):
        xvit.interpret.attention_maps(model, img)
    assert STREAM_MODE.get() is None and XF.ATTN_RECORDER.get() is None
