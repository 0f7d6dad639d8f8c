"""GPU: xvit.interpret.relevance_maps against the oracle's own autograd, and its invariants.

Reference: R.softmax_attention is wrapped (monkeypatch, the oracle itself is unchanged): the wrapper forms P = softmax(q k^T scale) in
float64, keeps its gradient (retain_grad) and returns P v.  R.model_cross_forward / R.model_vit_forward run under
R.emulate_bf16(xattn="literal") on leaf weights, and the sum over samples of logits[b, target_b] is backpropagated.  Per site,
A = mean_h relu(P * P.grad); relevance runs r <- r + r A from the last self-attention block of a branch to the first, starting from e_0;
the fusion maps are the CLS-query rows of A.

Gates, rel-L2 per map: 1.5 x the largest distance measured on an MI355X (XVIT_MEASURE_LOG), under the ceiling of 5e-2.  Measured over
tiny, small and the ModelVIT config, both targets: relevance <= 8.8e-4 (ModelVIT), fusion maps <= 1.3e-2 in the low-rank form (its bf16 Y
in dp, its bf16 weights e in p) and <= 1.1e-2 in the literal order.  The maps of class 0 and class 1 differ by >= 3.2e-2 (relevance,
small); B = 1 reproduces sample 0 of the batch to <= 7e-10."""
import pytest
import torch

import ref_cpu as R
from _util import dev, note, rel
from test_interpret_gpu import _model, _site_names

pytestmark = pytest.mark.gpu

GATE = {"relevance": 1.3e-3, "fusion_lowrank": 1.93e-2, "fusion_dense": 1.66e-2}


def _oracle(kind, cfg, sd, img, labels, target, monkeypatch):
    probs = []
    inner = R.softmax_attention

    def recording(q, k, v, scale):
        p = torch.softmax((q.double() @ k.double().transpose(-1, -2)) * scale, dim=-1)
        p.retain_grad()
        probs.append(p)
        _, lse = inner(q.detach(), k.detach(), v.detach(), scale)
        return (p @ v.double()).to(q.dtype), lse

    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    monkeypatch.setattr(R, "softmax_attention", recording)
    with R.emulate_bf16(xattn="literal"):
        logits, _ = (R.model_vit_forward if kind == "vit" else R.model_cross_forward)(leaf, img, labels, cfg)
    monkeypatch.setattr(R, "softmax_attention", inner)
    logits.gather(1, target[:, None]).sum().backward()
    names = _site_names(kind, cfg)
    assert len(probs) == len(names)
    A = {n: (p * p.grad).clamp_min(0).mean(dim=1) for n, p in zip(names, probs)}      # [B, Nq, N]
    fusion = {n: a[:, 0, :] for n, a in A.items() if ".fusion." in n}
    chains = {0: names} if kind == "vit" else {
        m: [f"transformer.{b}.blocks.{m}.{s}" for b in range(cfg.num_multi_blocks) for s in range(cfg.num_self_blocks)] for m in range(cfg.num_modalities)}
    relevance = {}
    for key, chain in chains.items():
        if not chain:
            continue
        r = torch.zeros(img.shape[0], A[chain[0]].shape[-1], dtype=torch.float64)
        r[:, 0] = 1.0
        for n in reversed(chain):
            r = r + torch.einsum("bm,bmn->bn", r, A[n])
        relevance[key] = r
    return relevance, fusion


@pytest.mark.parametrize("target", ["argmax", "explicit"])
@pytest.mark.parametrize("kind,name,form", [("cross", "tiny", "lowrank"), ("cross", "tiny", "dense"), ("cross", "small", "lowrank"),
                                            ("cross", "small", "dense"), ("vit", "small", "lowrank")])
def test_relevance_vs_oracle_autograd(kind, name, form, target, monkeypatch):
    import xvit
    import xvit.functional as XF
    monkeypatch.setattr(XF, "XATTN_FORM", form)
    cfg, sd, model, img, labels = _model(kind, name)
    tgt = None if target == "argmax" else torch.tensor([1, 0], dtype=torch.int64)
    out = xvit.interpret.relevance_maps(model, img.to(dev()), target=tgt)
    torch.cuda.synchronize()
    if tgt is None:
        assert torch.equal(out.target, out.logits.argmax(dim=1))
    else:
        assert torch.equal(out.target.cpu(), tgt)
    ref_rel, ref_fus = _oracle(kind, cfg, sd, img, labels, out.target.cpu(), monkeypatch)
    assert set(out.relevance) == set(ref_rel) and set(out.fusion) == set(ref_fus)
    for key, ref in ref_rel.items():
        got = out.relevance[key]
        assert got.shape == ref.shape and got.dtype == torch.float32
        assert (got.cpu() >= 0).all() and float(got[:, 0].min()) >= 1.0
        e = note(f"relevance_{kind}_{name}_{form}_{target}_chain", rel(got, ref))
        assert e <= GATE["relevance"], f"relevance {key}: rel-L2 {e:.3e} > {GATE['relevance']:g}"
    for n, ref in ref_fus.items():
        got = out.fusion[n]
        assert got.shape == ref.shape and got.dtype == torch.float32 and (got.cpu() >= 0).all()
        e = note(f"relevance_{kind}_{name}_{form}_{target}_fusion", rel(got, ref))
        assert e <= GATE["fusion_" + form], f"{n}: rel-L2 {e:.3e} > {GATE['fusion_' + form]:g}"


@pytest.mark.parametrize("kind", ["cross", "vit"])
def test_logits_repeatability_and_batch_one(kind):
    """The pass computes what a plain eval forward computes (bit for bit), two calls give identical maps, B = 1 matches sample 0."""
    import xvit
    cfg, sd, model, img, labels = _model(kind, "small")
    x = img.to(dev())
    with torch.no_grad():
        plain, _ = model(x, labels.to(dev()))
    a = xvit.interpret.relevance_maps(model, x)
    b = xvit.interpret.relevance_maps(model, x)
    torch.cuda.synchronize()
    assert torch.equal(a.logits, plain.detach()), "the relevance pass changed the logits"
    assert torch.equal(a.target, b.target)
    for da, db in ((a.relevance, b.relevance), (a.fusion, b.fusion)):
        assert da.keys() == db.keys() and all(torch.equal(da[k], db[k]) for k in da)
    one = xvit.interpret.relevance_maps(model, x[:1], target=a.target[:1])
    torch.cuda.synchronize()
    assert one.relevance.keys() == a.relevance.keys() and one.fusion.keys() == a.fusion.keys()
    for mine, batch in ((one.relevance, a.relevance), (one.fusion, a.fusion)):
        for k, v in mine.items():
            assert v.shape[0] == 1 and torch.isfinite(v).all()
            e = note(f"relevance_{kind}_b1_vs_batch", rel(v[0], batch[k][0]))
            assert e < 1e-2, f"{k}: B = 1 vs the batch's sample 0: rel-L2 {e:.3e}"


def test_the_two_classes_get_different_maps():
    import xvit
    _, _, model, img, _ = _model("cross", "small")
    x = img.to(dev())
    zero = xvit.interpret.relevance_maps(model, x, target=0)
    one = xvit.interpret.relevance_maps(model, x, target=1)
    torch.cuda.synchronize()
    assert torch.equal(zero.logits, one.logits)
    for maps0, maps1 in ((zero.relevance, one.relevance), (zero.fusion, one.fusion)):
        for k in maps0:
            e = note("relevance_class0_vs_class1", rel(maps0[k], maps1[k]))
            assert e > 1e-2, f"{k}: the maps of class 0 and class 1 agree to {e:.3e}"


class _Sink(dict):
    """A stand-in for a reducer's bucket registry that notes every lookup."""

    def __init__(self):
        super().__init__()
        self.lookups = 0

    def get(self, *a):
        self.lookups += 1
        return None


def test_training_state_is_untouched():
    import xvit
    import xvit.functional as XF
    from xvit.cross_vit import STREAM_MODE
    _, _, model, img, _ = _model("cross", "tiny")
    params = list(model.parameters())
    for i, p in enumerate(params):
        p.grad = torch.full_like(p, float(i)) if i % 2 == 0 else None
    before = [None if p.grad is None else p.grad.clone() for p in params]
    sink = _Sink()
    XF.GRAD_SINK = sink
    try:
        xvit.interpret.relevance_maps(model, img.to(dev()))
        torch.cuda.synchronize()
        assert XF.GRAD_SINK is sink and sink.lookups == 0, "a weight gradient looked for a reducer bucket"
    finally:
        XF.GRAD_SINK = None
    for p, g in zip(params, before):
        assert (p.grad is None) if g is None else torch.equal(p.grad, g)
    assert STREAM_MODE.get() is None and XF.ATTN_RECORDER.get() is None


def test_refusals_restore_state(monkeypatch):
    import xvit
    import xvit.functional as XF
    from xvit.cross_vit import STREAM_MODE
    _, _, model, img, _ = _model("cross", "tiny")
    x = img.to(dev())
    sink = _Sink()
    monkeypatch.setattr(XF, "GRAD_SINK", sink)

    def restored():
        return XF.GRAD_SINK is sink and STREAM_MODE.get() is None and XF.ATTN_RECORDER.get() is None

    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        xvit.interpret.relevance_maps(model, x)
    assert restored()
    model.eval()
    monkeypatch.setenv("XVIT_ATTN_FP8", "1")
    with pytest.raises(RuntimeError, match="XVIT_ATTN_FP8"):
        xvit.interpret.relevance_maps(model, x)
    monkeypatch.delenv("XVIT_ATTN_FP8")
    assert restored()
    with pytest.raises(RuntimeError, match="GPU"):
        xvit.interpret.relevance_maps(model, img)
    with pytest.raises(ValueError, match="target"):
        xvit.interpret.relevance_maps(model, x, target=torch.tensor([0, 1, 1]))
    with pytest.raises(ValueError, match="out of range"):
        xvit.interpret.relevance_maps(model, x, target=5)      # refused after the forward: the state is restored all the same
    assert restored() and sink.lookups == 0


def test_head_dim_refusal():
    import xvit
    _, _, model, img, _ = _model("cross", "tiny", num_heads=6)
    with pytest.raises(ValueError, match="head dim"):
        xvit.interpret.relevance_maps(model, img.to(dev()))


def test_no_relevance_entry_without_self_blocks():
    import xvit
    cfg, _, model, img, _ = _model("cross", "tiny", num_self_blocks=0)
    out = xvit.interpret.relevance_maps(model, img.to(dev()))
    assert out.relevance == {} and len(out.fusion) == 4
    assert all(v.shape == (img.shape[0], R.derived(cfg).N) for v in out.fusion.values())
