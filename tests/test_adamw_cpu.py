"""CPU: xvit.optim.FusedAdamW's refusals, layer_decay_groups on CPU-built models, and the xvit_adamw_extra layout."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import ref_cpu as R


def _params():
    return [torch.nn.Parameter(torch.zeros(3, 4)), torch.nn.Parameter(torch.zeros(5))]


def test_constructor_refusals():
    from xvit.optim import FusedAdam, FusedAdamW
    opt = FusedAdamW(_params(), lr=1e-3, ema_decay=0.99, ema_warmup=True)
    assert isinstance(opt, FusedAdam) and opt.decoupled and opt.param_groups[0]["lr_scale"] == 1.0 and opt.param_groups[0]["weight_decay"] == 1e-2
    assert opt.launch_sets == 1 and opt.scale_copies == 0 and opt.lr_copies == 0
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=math.nan), dict(ema_warmup=True), dict(weight_decay=-1.0), dict(lr=-1.0), dict(eps=-1.0),
                dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(max_grad_norm=0.0), dict(max_grad_norm=math.inf), dict(skip_nonfinite=True)):
        with pytest.raises(ValueError):
            FusedAdamW(_params(), **bad)
    for s in (-0.5, math.inf, math.nan):
        with pytest.raises(ValueError, match="lr_scale"):
            FusedAdamW([dict(params=_params(), lr_scale=s)])
    with pytest.raises(ValueError):
        FusedAdamW([dict(params=_params(), weight_decay=-0.1)])
    a, b = _params()
    opt = FusedAdamW([dict(params=[a], lr_scale=0.5), dict(params=[b], betas=(0.8, 0.9))], lr=1e-3)
    assert opt.launch_sets == 2                           # other betas: another launch set
    assert FusedAdamW([dict(params=[a], lr_scale=0.5, weight_decay=0.0), dict(params=[b], lr=5e-4)], lr=1e-3).launch_sets == 1
    with pytest.raises(RuntimeError, match="ema_decay=None"):
        FusedAdamW(_params()).ema_weights()
    with pytest.raises(RuntimeError, match="ema_decay=None"):
        FusedAdamW(_params()).ema_state_dict(torch.nn.Linear(2, 2))
    assert FusedAdamW._rates([dict(lr=1e-3, lr_scale=0.5), dict(lr=1e-3, lr_scale=0.25)]) == (1e-3, [0.5, 0.25])
    ref, sc = FusedAdamW._rates([dict(lr=2e-3, lr_scale=0.5), dict(lr=1e-3, lr_scale=1.0)])
    assert ref == 2e-3 and sc == [0.5, float(np.float32(1.0 * 1e-3 / 2e-3))]
    assert FusedAdamW._rates([dict(lr=0.0, lr_scale=0.5), dict(lr=0.0, lr_scale=1.0)]) == (0.0, [0.5, 1.0])


def _expected_layer(name, S, K):
    L = K * (S + 1) + 1
    if name in ("pos_embedding", "cls_token") or name.startswith("patch_to_embedding."):
        return 0
    m = re.fullmatch(r"transformer\.(\d+)\.blocks\.(\d+)\.(\d+)\..*", name)
    if m:
        return 1 + int(m.group(1)) * (S + 1) + int(m.group(3))
    m = re.fullmatch(r"transformer\.(\d+)\.fusion\.(\d+)\..*", name)
    if m:
        return 1 + int(m.group(1)) * (S + 1) + S
    assert name.startswith(("norm.", "mlp_head."))
    return L


def _check_groups(model, groups, L, layer_of, decay, wd, no_decay=("cls_token", "pos_embedding", "mask_token")):
    named = dict(model.named_parameters())
    seen = {}
    for g in groups:
        assert set(g) >= {"params", "param_names", "layer", "lr_scale", "weight_decay"} and len(g["params"]) == len(g["param_names"]) > 0
        assert g["lr_scale"] == pytest.approx(decay ** (L - g["layer"]), rel=1e-12) and g["weight_decay"] in (0.0, wd)
        for k, p in zip(g["param_names"], g["params"]):
            assert named[k] is p and k not in seen, k
            seen[k] = g
            assert g["layer"] == layer_of(k), (k, g["layer"], layer_of(k))
            plain = p.dim() <= 1 or k.endswith(".bias") or k.split(".")[-1] in no_decay
            assert g["weight_decay"] == (0.0 if plain else wd), k
    assert set(seen) == set(named)                                        # every parameter in exactly one group
    assert len({(g["layer"], g["weight_decay"] > 0) for g in groups}) == len(groups)


@pytest.mark.parametrize("over", [dict(), dict(num_modalities=3, num_multi_blocks=2, num_self_blocks=1, attn_order={"0": "1", "1": "2", "2": "0"})], ids=["tiny", "3 modalities"])
def test_layer_decay_groups_on_model_cross(over):
    import xvit
    from xvit.optim import FusedAdamW, layer_decay_groups
    cfg = R.make_config("tiny", **over)
    model = xvit.ModelCross(cfg)
    S, K = cfg.num_self_blocks, cfg.num_multi_blocks
    L = K * (S + 1) + 1
    groups = layer_decay_groups(model, 0.75, 0.05)
    _check_groups(model, groups, L, lambda k: _expected_layer(k, S, K), 0.75, 0.05)
    assert {g["layer"] for g in groups} == set(range(L + 1))
    for name in ("cls_token", "pos_embedding"):
        g = next(g for g in groups if name in g["param_names"])
        assert g["weight_decay"] == 0.0 and g["layer"] == 0 and getattr(model, name).dim() > 1        # by name, not by shape
    assert next(g for g in groups if "mlp_head.0.3.weight" in g["param_names"])["lr_scale"] == 1.0
    assert FusedAdamW(groups, lr=1e-3).launch_sets == 1
    groups = layer_decay_groups(model, 0.5, 0.1, no_decay_names=())
    assert next(g for g in groups if "cls_token" in g["param_names"])["weight_decay"] == 0.1


def test_layer_decay_groups_on_the_masked_volume_model_and_vit():
    import xvit
    from xvit.optim import layer_decay_groups
    cfg = R.make_config("tiny")
    S, K = cfg.num_self_blocks, cfg.num_multi_blocks
    L = K * (S + 1) + 1
    mae = xvit.MaskedVolumeModel(xvit.ModelCross(cfg), decoder_dim=64, decoder_depth=1)
    _check_groups(mae, layer_decay_groups(mae, 0.75, 0.05), L, lambda k: _expected_layer(k[8:], S, K) if k.startswith("encoder.") else L, 0.75, 0.05)
    g = next(g for g in layer_decay_groups(mae) if "mask_token" in g["param_names"])
    assert g["weight_decay"] == 0.0 and g["layer"] == L and mae.mask_token.dim() > 1
    cfgv = R.make_config("tiny", num_layers=3)
    vit = xvit.ModelVIT(cfgv)

    def vit_layer(k):
        m = re.fullmatch(r"transformer\.layers\.(\d+)\..*", k)
        return 1 + int(m.group(1)) if m else (0 if k in ("pos_embedding", "cls_token") or k.startswith("patch_to_embedding.") else 4)
    _check_groups(vit, layer_decay_groups(vit, 0.9, 0.01), 4, vit_layer, 0.9, 0.01)
    from types import SimpleNamespace
    enc = xvit.Encoder(SimpleNamespace(hidden_size=64, transformer=dict(num_heads=2, mlp_dim=128, dropout_rate=0.0, attention_dropout_rate=0.0, num_layers=2)))
    _check_groups(enc, layer_decay_groups(enc, 0.5, 0.1), 3, lambda k: 1 + int(k.split(".")[1]) if k.startswith("layers.") else 3, 0.5, 0.1)


def test_unknown_names_and_shared_parameters():
    from xvit.optim import layer_decay_groups

    class Odd(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.something = torch.nn.Linear(4, 4)
            self.again = torch.nn.Linear(4, 4)
    m = Odd()
    groups = layer_decay_groups(m, 0.75, 0.05)
    assert {g["layer"] for g in groups} == {1} and {g["lr_scale"] for g in groups} == {1.0}            # unknown names: layer L, scale 1
    m.again.weight = m.something.weight
    layer_decay_groups(m)                                      # named_parameters() lists a shared parameter once
    with pytest.raises(ValueError):
        layer_decay_groups(m, layer_decay=0.0)
    with pytest.raises(ValueError):
        layer_decay_groups(m, weight_decay=-1.0)


def test_extra_struct_layout():
    """xvit_adamw_extra { float* ema; float lr_scale; float weight_decay; }: 16 bytes, as the numpy mirrors that build the table lay it out."""
    import _adamw_check as W
    from xvit import optim

    class Extra(C.Structure):
        _fields_ = [("ema", C.c_void_p), ("lr_scale", C.c_float), ("weight_decay", C.c_float)]
    assert C.sizeof(Extra) == 16 and (Extra.ema.offset, Extra.lr_scale.offset, Extra.weight_decay.offset) == (0, 8, 12)
    for dt in (optim._EXTRA_DTYPE, W.EXTRA):
        assert dt.itemsize == 16 and [dt.fields[k][1] for k in ("ema", "lr_scale", "weight_decay")] == [0, 8, 12]
    x = np.zeros(2, dtype=optim._EXTRA_DTYPE)
    x["ema"], x["lr_scale"], x["weight_decay"] = [0x1122334455667788, 0], [0.5, 2.0], [0.25, 0.0]
    raw = (Extra * 2).from_buffer_copy(x.tobytes())
    assert (raw[0].ema, raw[0].lr_scale, raw[0].weight_decay, raw[1].ema, raw[1].lr_scale) == (0x1122334455667788, 0.5, 0.25, None, 2.0)
    header = open(__file__.rsplit("/tests/", 1)[0] + "/include/xvit.h").read()
    assert re.search(r"typedef struct xvit_adamw_extra \{\s*float\* ema;[^}]*float lr_scale;[^}]*float weight_decay;[^}]*\} xvit_adamw_extra;", header)
    from xvit import _lib
    assert _lib.load().xvit_version() >= 314


def test_a_wrapped_encoder_counts_its_blocks_and_a_loaded_state_keeps_lr_scale():
    import xvit
    from types import SimpleNamespace
    from xvit.optim import FusedAdamW, layer_decay_groups

    class Wrapped(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = xvit.Encoder(SimpleNamespace(hidden_size=64, transformer=dict(num_heads=2, mlp_dim=128, dropout_rate=0.0, attention_dropout_rate=0.0, num_layers=2)))
            self.head = torch.nn.Linear(64, 2)
    m = Wrapped()
    groups = layer_decay_groups(m, 0.5, 0.1)
    _check_groups(m, groups, 3, lambda k: 1 + int(k.split(".")[2]) if k.startswith("encoder.layers.") else 3, 0.5, 0.1)
    assert max(g["lr_scale"] for g in groups) == 1.0
    opt = FusedAdamW(groups, lr=1e-3)
    scales = [g["lr_scale"] for g in opt.param_groups]
    plain = torch.optim.AdamW([dict(params=g["params"], weight_decay=g["weight_decay"]) for g in groups], lr=2e-3)
    opt.load_state_dict(plain.state_dict())                   # no lr_scale in the saved groups: the constructed ones stay, lr is the saved one
    assert [g["lr_scale"] for g in opt.param_groups] == scales and {g["lr"] for g in opt.param_groups} == {2e-3}
    other = FusedAdamW(layer_decay_groups(m, 0.9, 0.1), lr=1e-3)
    opt.load_state_dict(other.state_dict())                   # saved scales replace the current ones, like every saved hyper-parameter
    assert [g["lr_scale"] for g in opt.param_groups] == [g["lr_scale"] for g in other.param_groups] != scales
