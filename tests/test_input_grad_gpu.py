"""GPU: the input-volume gradient of ModelCross / ModelVIT (PatchEmbedFn.backward) and xvit.interpret.input_attributions.

img.grad after loss.backward() is compared with torch.autograd through the oracle (R.model_cross_forward / R.model_vit_forward under
R.emulate_bf16()) on the same bf16-rounded volume.  Gates, rel-L2: 1.5 x the largest distance measured on an MI355X (note(),
XVIT_MEASURE_LOG), per case; the same dX feeds the patch_to_embedding.weight gradient, and the distances land near its gate.
Measured: img.grad 8.3e-3 .. 8.9e-3 (tiny, small, ModelVIT; both forms, fp32 and bf16 volumes), 1.02e-2 .. 1.04e-2 (base); unfused
against fused at base 0; IG |delta| / |logit_t(img) - logit_t(0)| at 64 steps 1.04e-2 (tiny) and 2.52e-2 (base, bf16 volume), at 8
steps 2.1e-2 and 0.40; batch_size 1 against 16: 3.6e-3, B = 3 against three B = 1 calls: 0."""
import pytest
import torch

import ref_cpu as R
from _util import dev, note, rel

pytestmark = pytest.mark.gpu

GATE = {"tiny": 1.34e-2, "small": 1.34e-2, "base": 1.56e-2, "ig_delta_tiny": 1.57e-2, "ig_delta_base": 3.78e-2, "ig_batch": 5.4e-3}


def _model(kind, name, batch=2, **over):
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
    img, labels = R.make_inputs(cfg, batch, seed=0)
    return cfg, sd, model, R.bf16_round(img), labels


_ORACLE = {}


def _oracle_img_grad(kind, cfg, sd, img, labels, xattn):
    key = (kind, tuple(cfg.img_size), cfg.hidden_dim, xattn)
    if key not in _ORACLE:
        x = img.clone().requires_grad_(True)
        with R.emulate_bf16(xattn=xattn):
            _, loss = (R.model_vit_forward if kind == "vit" else R.model_cross_forward)(sd, x, labels, cfg)
        loss.backward()
        _ORACLE[key] = x.grad
    return _ORACLE[key]


CASES = [("cross", "tiny", "lowrank"), ("cross", "tiny", "dense"), ("cross", "small", "lowrank"), ("cross", "base", "lowrank"),
         ("cross", "base", "dense"), ("vit", "small", "lowrank")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind,name,form", CASES, ids=["-".join(c) for c in CASES])
def test_img_grad_vs_oracle(kind, name, form, dtype, monkeypatch):
    import xvit.functional as XF
    monkeypatch.setattr(XF, "XATTN_FORM", form)
    cfg, sd, model, img, labels = _model(kind, name)
    model.train()
    x = img.to(dev(), dtype).requires_grad_(True)
    _, loss = model(x, labels.to(dev()))
    loss.backward()
    assert x.grad is not None and x.grad.dtype == dtype and x.grad.shape == x.shape
    ref = _oracle_img_grad(kind, cfg, sd, img, labels, "literal" if form == "dense" else "lowrank")
    e = note(f"input_grad.{kind}.{name}.{form}.{str(dtype)[6:]}", rel(x.grad, ref))
    assert torch.isfinite(x.grad).all() and e < GATE[name], e


def test_unfused_matches_fused_at_base(monkeypatch):
    """XVIT_PATCH_EMBED=unfused (patchify + GEMM forward, NN GEMM + unpatchify input gradient) against the fused kernels at base."""
    cfg, sd, model, img, labels = _model("cross", "base")
    model.train()
    grads = {}
    for mode in ("fused", "unfused"):
        monkeypatch.setenv("XVIT_PATCH_EMBED", mode)
        x = img.to(dev(), torch.bfloat16).requires_grad_(True)
        model(x, labels.to(dev()))[1].backward()
        grads[mode] = x.grad.float()
        model.zero_grad(set_to_none=True)
    e = note("input_grad.base.unfused_vs_fused", rel(grads["unfused"], grads["fused"]))
    assert e < GATE["base"], e


@pytest.mark.parametrize("kind,name", [("cross", "base"), ("vit", "small")])
def test_param_grads_unchanged_by_img_grad(kind, name):
    """Every parameter gradient is bit-identical with and without img.requires_grad (deterministic mode)."""
    from xvit import ops
    cfg, sd, model, img, labels = _model(kind, name)
    model.train()
    ops.set_deterministic(True)
    try:
        out = []
        for want in (False, True):
            model.zero_grad(set_to_none=True)
            x = img.to(dev(), torch.bfloat16).requires_grad_(want)
            model(x, labels.to(dev()))[1].backward()
            out.append({n: p.grad.clone() for n, p in model.named_parameters()})
            assert (x.grad is not None) == want
    finally:
        ops.set_deterministic(False)
    for n in out[0]:
        assert torch.equal(out[0][n], out[1][n]), n


# ---- input_attributions ---------------------------------------------------------------------------------------------------------

def test_gradient_method_is_autograd_bit_for_bit():
    import xvit
    from xvit import ops
    cfg, sd, model, img, labels = _model("cross", "base")
    model.eval()
    x = img.to(dev())
    ops.set_deterministic(True)
    try:
        out = xvit.interpret.input_attributions(model, x, method="gradient")
        xin = x.clone().requires_grad_(True)
        logits, _ = model(xin, torch.zeros(2, dtype=torch.long, device=dev()))
        g, = torch.autograd.grad(logits, xin, grad_outputs=torch.nn.functional.one_hot(out.target, logits.shape[1]).float())
        gx = xvit.interpret.input_attributions(model, x, method="grad_x_input", target=out.target)
    finally:
        ops.set_deterministic(False)
    assert torch.equal(out.target, logits.detach().argmax(dim=1)) and torch.equal(out.logits, logits.detach())
    assert out.attributions.shape == (2, cfg.num_modalities, *cfg.img_size) and out.attributions.dtype == torch.float32
    assert torch.equal(out.attributions, g[:, :, 0])
    assert torch.equal(gx.attributions, g[:, :, 0] * x[:, :, 0])      # the baseline defaults to zeros


@pytest.mark.parametrize("name,dtype", [("tiny", torch.float32), ("base", torch.bfloat16)])
def test_integrated_gradients_completeness(name, dtype):
    import xvit
    cfg, sd, model, img, labels = _model("cross", name, batch=1)
    model.eval()
    x = img.to(dev(), dtype)
    res = {}
    for steps in (8, 64):
        out = xvit.interpret.input_attributions(model, x, steps=steps)
        dlogit = out.attributions.reshape(1, -1).sum(dim=1) - out.delta          # logit_t(img) - logit_t(baseline)
        res[steps] = float((out.delta.abs() / dlogit.abs()).max())
        assert out.attributions.dtype == torch.float32 and torch.isfinite(out.attributions).all()
    e = note(f"ig_delta.{name}.64", res[64])
    note(f"ig_delta.{name}.8", res[8])
    assert e < GATE[f"ig_delta_{name}"], res
    assert res[64] <= res[8] + GATE[f"ig_delta_{name}"] / 2, res


def test_ig_batching_agrees():
    """batch_size=1 against batch_size=16, and B = 3 against three B = 1 calls (kernel choices depend on the batch: not bit-identical)."""
    import xvit
    cfg, sd, model, img, labels = _model("cross", "tiny", batch=3)
    model.eval()
    x = img.to(dev())
    full = xvit.interpret.input_attributions(model, x, steps=8, batch_size=16)
    one = xvit.interpret.input_attributions(model, x, steps=8, batch_size=1)
    e1 = note("ig_batch.bs1_vs_bs16", rel(one.attributions, full.attributions))
    singles = torch.cat([xvit.interpret.input_attributions(model, x[i:i + 1], steps=8, target=full.target[i:i + 1]).attributions for i in range(3)])
    e2 = note("ig_batch.B3_vs_B1", rel(singles, full.attributions))
    assert e1 < GATE["ig_batch"] and e2 < GATE["ig_batch"], (e1, e2)


@pytest.mark.parametrize("method", ["gradient", "grad_x_input", "integrated_gradients"])
def test_out_of_range_target_is_refused(method):
    """A class outside [0, C) raises the ValueError before any gradient is seeded (one_hot on the GPU does not bound-check), in every
    method; the state is restored and a valid call afterwards still works."""
    import xvit
    import xvit.functional as XF
    from xvit.cross_vit import STREAM_MODE
    _, _, model, img, _ = _model("cross", "tiny")
    model.eval()
    x = img.to(dev())
    for bad in (1000, 2, torch.tensor([0, 5]), torch.tensor([1, 2], device=dev())):
        with pytest.raises(ValueError, match="target out of range"):
            xvit.interpret.input_attributions(model, x, target=bad, method=method, steps=2)
        assert XF.GRAD_SINK is None and STREAM_MODE.get() is None and XF.ATTN_RECORDER.get() is None
    for bad in (-3, torch.tensor([0, -1])):
        with pytest.raises(ValueError, match="negative class"):
            xvit.interpret.input_attributions(model, x, target=bad, method=method, steps=2)
    torch.cuda.synchronize()
    out = xvit.interpret.input_attributions(model, x, target=1, method=method, steps=2)
    assert torch.isfinite(out.attributions).all() and out.target.tolist() == [1, 1]


class _Sink(dict):
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
    model.eval()
    params = list(model.parameters())
    for i, p in enumerate(params):
        p.grad = torch.full_like(p, float(i)) if i % 2 == 0 else None
    before = [None if p.grad is None else p.grad.clone() for p in params]
    arena = list(XF._ARENA)
    sink = _Sink()
    XF.GRAD_SINK = sink
    try:
        for method in ("gradient", "integrated_gradients"):
            xvit.interpret.input_attributions(model, img.to(dev()), method=method, steps=4)
        torch.cuda.synchronize()
        assert XF.GRAD_SINK is sink and sink.lookups == 0, "a weight gradient looked for a reducer bucket"
    finally:
        XF.GRAD_SINK = None
    for p, g in zip(params, before):
        assert (p.grad is None) if g is None else torch.equal(p.grad, g)
    assert STREAM_MODE.get() is None and XF.ATTN_RECORDER.get() is None and XF._ARENA == arena


def test_modelvit_and_frozen_model():
    """ModelVIT gives [B, M, D, H, W] too; a model whose parameters do not require grad still has an input gradient."""
    import xvit
    cfg, sd, model, img, labels = _model("vit", "small")
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    out = xvit.interpret.input_attributions(model, img.to(dev()), method="gradient")
    assert out.attributions.shape == (2, cfg.num_modalities, *cfg.img_size) and torch.isfinite(out.attributions).all()
    assert float(out.attributions.abs().sum()) > 0
