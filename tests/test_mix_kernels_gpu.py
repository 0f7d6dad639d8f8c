"""GPU: xvit_mix_apply, xvit_mix_draw and xvit_mean_ce_mix (csrc/mix.hip) against the restatements and gates of tests/_mix_check.py.

Apply: hand-made tables, independent of the draw.  Every launch writes into a window with sentinels on both sides.  Each table is run twice:
on finite volumes (the arithmetic), and with NaN in every voxel of the source that no record reads THROUGH ITS PARTNER INDEX — outside
the box of the CutMix records that name the sample, everywhere for a sample only copy records or nobody names — so that a partner voxel a
record must not read poisons its output (a sample's own record still carries its own NaN, as the restatement predicts).  The samples
between those of a batch-strided view are NaN as well.
Workgroups: a workgroup owns 1024 vectors of one volume, 16 bytes each on the wide path: (16, 16, 32) is one workgroup in bf16 and two in
fp32; (12, 16, 88) makes three in bf16 (the last one partial) and (9, 11, 13) two on the one-voxel path."""
import math

import numpy as np
import pytest
import torch

import _cls_check as X
import _mix_check as K
from _util import dev

pytestmark = pytest.mark.gpu

VOLUMES = [(8, 8, 16), (6, 10, 12), (5, 7, 9), (16, 16, 32), (12, 16, 88), (9, 11, 13)]
GUARD = 64                       # sentinel elements on each side of the destination (a multiple of 16 bytes in both dtypes)


# ---------------------------------------------------------------------------------------------------------------- apply
def _record_kinds(B, D, H, W):
    """(name, record without its partner) for sample b; the partner is filled in by the caller."""
    w8 = min(W, 8)
    kinds = [("mixup 0.3", dict(mode=K.MIXUP, lam=0.3)), ("mixup 0.9375 / oml 0.125 by hand", dict(mode=K.MIXUP, lam=0.9375, oml=0.125)),
             ("mixup lam 0", dict(mode=K.MIXUP, lam=0.0))]
    boxes = {"inner": (1, D - 1, 1, H - 1, 1, W - 1), "face d0": (0, 2, 1, H - 1, 1, W - 1), "face d1": (D - 2, D, 1, H - 1, 1, W - 1),
             "face h0": (1, D - 1, 0, 2, 1, W - 1), "face h1": (1, D - 1, H - 2, H, 1, W - 1), "face w0": (1, D - 1, 1, H - 1, 0, 3),
             "face w1": (1, D - 1, 1, H - 1, W - 3, W), "edges inside one vector": (0, D, 0, H, 2, w8 - 3), "one voxel wide": (2, 3, 3, 4, w8 - 1, w8),
             "across two vectors": (0, D, 1, H, w8 - 2, min(W, w8 + 2)), "empty": (2, 2, 0, H, 0, W), "reversed": (3, 1, 0, H, 0, W), "full": (0, D, 0, H, 0, W),
             "beyond the volume": (-3, D + 5, 0, H, 0, W + 9)}
    kinds += [(f"cutmix {n}", dict(mode=K.CUTMIX, lam=0.5, box=bx)) for n, bx in boxes.items()]
    kinds += [("mode 0", dict(mode=0, lam=0.25)), ("mode 3", dict(mode=3, lam=0.25)), ("mode 1.5", dict(mode=1.5, lam=0.25)),
              ("lam 1 mixup", dict(mode=K.MIXUP, lam=1.0, oml=0.5)), ("lam 1 cutmix", dict(mode=K.CUTMIX, lam=1.0, box=boxes["full"]))]
    kinds += [(f"partner {p}", dict(mode=m, lam=0.5, partner=p, box=boxes["full"])) for p, m in ((B, K.MIXUP), (-1, K.CUTMIX), (0.5, K.MIXUP), (math.nan, K.CUTMIX),
                                                                                              (1e9, K.MIXUP))]
    return kinds


def _tables(B, D, H, W):
    kinds = _record_kinds(B, D, H, W)
    n = -(-len(kinds) // B)
    for t in range(n):
        recs, names = [], []
        for b in range(B):
            name, kw = kinds[(t * B + b) % len(kinds)]
            kw = dict(kw)
            kw.setdefault("partner", (b + 1 + t) % B)
            recs.append(K.record(**kw))
            names.append(name)
        yield names, np.stack(recs)


def _unread_through_partners(table, B, D, H, W):
    """[B, D, H, W] bool: the voxels of sample s that no record reads through its partner index."""
    unread = np.ones((B, D, H, W), dtype=bool)
    for b in range(B):
        if not K.is_mixed(table[b], B):
            continue
        p = int(table[b, K.PARTNER])
        if int(table[b, K.MODE]) == K.MIXUP:
            unread[p] = False
        else:
            d0, d1, h0, h1, w0, w1 = K.box_of(table[b], D, H, W)
            unread[p, d0:d1, h0:h1, w0:w1] = False
    return unread


def _launch_apply(src_dev, table, shift=0):
    """src_dev [B, M, 1, D, H, W] on the GPU (any batch / modality strides) -> the destination as a CPU tensor [B, M, D, H, W], after the
    sentinels around it were checked.  shift: elements by which the destination is moved off its 16-byte alignment."""
    from xvit import ops
    B, M, _, D, H, W = src_dev.shape
    n = src_dev.numel()
    buf = torch.full((2 * GUARD + n + 8,), X.SENT, dtype=src_dev.dtype, device=dev())
    lo = GUARD + shift
    buf[lo:lo + n] = math.nan
    out = buf[lo:lo + n].view(src_dev.shape)
    got = ops.mix_apply(src_dev, torch.from_numpy(table).to(dev()), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu()
    sent = torch.full((1,), X.SENT, dtype=src_dev.dtype)
    assert bool((host[:lo] == sent).all()) and bool((host[lo + n:] == sent).all()), "sentinels around the destination were overwritten"
    return host[lo:lo + n].view(B, M, D, H, W)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("vol", VOLUMES, ids=lambda v: "x".join(map(str, v)))
def test_apply_against_the_restatement(vol, bf16):
    D, H, W = vol
    dtype = torch.bfloat16 if bf16 else torch.float32
    g = torch.Generator().manual_seed(1000 * D + 10 * H + W)
    launches = 0
    for B, M in ((1, 1), (2, 2), (3, 1), (5, 2)):
        base = torch.randn(2 * B, M, 1, D, H, W, generator=g).to(dtype)
        for t, (names, table) in enumerate(_tables(B, D, H, W)):
            layout = ("contiguous", "batch-strided", "misaligned source", "misaligned destination")[t % 4]
            for poison in (False, True):
                full = base.clone()
                full[1::2] = math.nan                                  # the samples a batch-strided view skips
                vals = full[0::2].clone()
                if poison:
                    unread = _unread_through_partners(table, B, D, H, W)
                    vals[torch.from_numpy(unread)[:, None, None].expand(B, M, 1, D, H, W)] = math.nan
                if layout == "batch-strided":
                    full[0::2] = vals
                    src = full.to(dev())[0::2]
                    assert src.stride(0) == 2 * M * D * H * W
                elif layout == "misaligned source":                    # one element off the allocation's alignment: the one-voxel path whatever W is
                    flat = torch.full((vals.numel() + 1,), math.nan, dtype=dtype)
                    flat[1:] = vals.reshape(-1)
                    src = flat.to(dev())[1:].view(vals.shape)
                else:
                    src = vals.to(dev())
                got = _launch_apply(src, table, shift=1 if layout == "misaligned destination" else 0)
                ref, bound, exact = K.apply(vals[:, :, 0].double().numpy(), table, bf16)
                K.check_apply(f"{vol} {dtype} B {B} M {M} {layout}{' poisoned' if poison else ''} records {names}", got, ref, bound, exact)
                launches += 1
    assert launches >= 8


def test_apply_at_the_model_shapes_matches_torch_on_a_strided_modality_view():
    """A modality-strided source (every second modality of a wider tensor), all three record kinds in one batch, against the torch
    composition on the GPU: CutMix and copies bit for bit, mixup within the bound."""
    from xvit import ops
    B, M, D, H, W = 4, 2, 16, 16, 16
    g = torch.Generator().manual_seed(3)
    wide = torch.randn(B, 2 * M, 1, D, H, W, generator=g).to(torch.bfloat16)
    table = np.stack([K.record(K.MIXUP, 2, 0.7), K.record(K.CUTMIX, 3, 0.5, box=(2, 9, 0, 16, 5, 11)), K.record(0, 1, 0.5), K.record(K.CUTMIX, 0, 0.9, box=(0, 16, 3, 4, 0, 16))])
    src = wide.to(dev())[:, ::2]
    assert src.stride(1) == 2 * D * H * W
    got = ops.mix_apply(src, torch.from_numpy(table).to(dev())).cpu()
    vals = wide[:, ::2, 0]
    ref, bound, exact = K.apply(vals.double().numpy(), table, True)
    K.check_apply("modality-strided", got[:, :, 0], ref, bound, exact)


# ---------------------------------------------------------------------------------------------------------------- draw
def _device_draw(cfg, B, vol, seed):
    from xvit import _lib, ops
    table = torch.full((B, K.NPARAM), math.nan, dtype=torch.float32, device=dev())
    c = _lib.MixConfig(cfg["mixup_alpha"], cfg["cutmix_alpha"], cfg["prob"], cfg["switch_prob"], int(cfg["per_sample"]))
    ops.mix_draw(c, table, vol, seed)
    torch.cuda.synchronize()
    return table.cpu().numpy()


@pytest.mark.parametrize("case", K.DRAW_CASES, ids=K.draw_case_id)
def test_draw_against_the_restatement(case):
    cfg, B, vol, seed = case
    got = _device_draw(cfg, B, vol, seed)
    ref, margin = K.draw(cfg, B, *vol, seed)
    skipped = K.check_draw(K.draw_case_id(case), got, ref, margin)
    print(f"{K.draw_case_id(case)}: {skipped:.2%} of the records left out")
    assert np.array_equal(got.view(np.uint32), _device_draw(cfg, B, vol, seed).view(np.uint32))       # same seed: the same table bit for bit


def test_draw_follows_the_device_epoch():
    from xvit import ops
    cfg, B, vol, seed = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, per_sample=True), 64, (6, 10, 12), 4242
    plain = _device_draw(cfg, B, vol, seed)
    epoch = torch.zeros(1, dtype=torch.int64, device=dev())
    ops.set_dropout_epoch(epoch)
    try:
        at0 = _device_draw(cfg, B, vol, seed)
        epoch.add_(1)
        at1 = _device_draw(cfg, B, vol, seed)
        epoch.add_(1)
        at2 = _device_draw(cfg, B, vol, seed)
    finally:
        ops.set_dropout_epoch(None)
    assert np.array_equal(plain.view(np.uint32), at0.view(np.uint32))                                  # epoch 0 is the plain seed
    assert not np.array_equal(at0, at1) and not np.array_equal(at1, at2)
    for e, got in ((1, at1), (2, at2)):
        ref, margin = K.draw(cfg, B, *vol, seed, epoch=e)
        K.check_draw(f"epoch {e}", got, ref, margin)


# ---------------------------------------------------------------------------------------------------------------- loss
def _loss_table(B, seed):
    """Per record: mixup / cutmix with a random partner and lam, or one of the copy kinds."""
    rng = np.random.RandomState(seed)
    recs = []
    for b in range(B):
        kind = rng.randint(6)
        lam = float(np.float32(rng.uniform(0.0, 1.0)))
        p = int(rng.randint(B))
        if kind <= 2:
            recs.append(K.record(K.MIXUP if kind < 2 else K.CUTMIX, p, lam, box=(0, 1, 0, 1, 0, 1)))
        elif kind == 3:
            recs.append(K.record(0, p, lam))
        elif kind == 4:
            recs.append(K.record(K.MIXUP, B + rng.randint(3), lam))
        else:
            recs.append(K.record(K.CUTMIX, p, 1.0, oml=0.5))
    return np.stack(recs)


@pytest.mark.parametrize("B", [1, 3, 64, 600])
def test_mean_ce_mix_against_float64(B):
    worst = 0.0
    for M in (1, 2, 3):
        for Cn in (2, 5):
            for eps in (0.0, 0.1):
                e32 = X.f32(eps)
                lm, labels = X.ce_inputs("usual", M, B, Cn)
                table = _loss_table(B, 7 * B + M + Cn)
                name = f"mean_ce_mix M {M} B {B} C {Cn} smoothing {eps:g}"
                rc, wins = K.ce_launch(lm, labels, table, e32)
                assert rc == 0, name
                ref = K.ce_ref(lm, labels, table, e32)
                worst = max(worst, X.ce_check(name, wins, ref, M, B, Cn))
                # sum_c dlogits = 0 per row: each element is within C_ce_dl 2^-24 S_dl of a float64 row that sums to 0 (up to 1e-16), so the
                # row sum is within the sum of those bounds
                dl = wins["dl"][0, :M * B * Cn].reshape(M, B, Cn).double()
                lim = (X.C["ce_dl"] * X.EPS32 * ref["S_dl"] * X.SLACK + X.UNDERFLOW).sum(-1) + 1e-15
                assert bool((dl.sum(-1).abs() <= lim).all()), name
                # lam = 1 in every record: xvit_mean_ce bit for bit
                ones = np.stack([K.record(K.MIXUP, (b + 1) % B, 1.0) for b in range(B)])
                rc1, w1 = K.ce_launch(lm, labels, ones, e32)
                rc0, w0 = X.ce_launch(lm, labels, e32)
                assert rc1 == 0 and rc0 == 0
                for k in w0:
                    assert torch.equal(X._bits(w1[k]), X._bits(w0[k])), (name, k)
    print(f"mean_ce_mix B {B}: worst share of the bound {worst:.3f}")


def test_mean_ce_mix_at_lam_one_is_mean_ce_on_the_hard_contents():
    """The contents that stress xvit_mean_ce (equal logits, +-80, one dominant class): bit-identity at lam = 1 and the bound under mixing."""
    M, B, Cn = 2, 7, 7
    for kind in X.CE_CONTENT:
        lm, labels = X.ce_inputs(kind, M, B, Cn)
        e32 = X.f32(0.1)
        ones = np.stack([K.record(K.CUTMIX, (b + 3) % B, 1.0) for b in range(B)])
        _, w1 = K.ce_launch(lm, labels, ones, e32)
        _, w0 = X.ce_launch(lm, labels, e32)
        for k in w0:
            assert torch.equal(X._bits(w1[k]), X._bits(w0[k])), (kind, k)
        table = _loss_table(B, 5)
        rc, wins = K.ce_launch(lm, labels, table, e32)
        assert rc == 0
        X.ce_check(f"mean_ce_mix {kind}", wins, K.ce_ref(lm, labels, table, e32), M, B, Cn)
