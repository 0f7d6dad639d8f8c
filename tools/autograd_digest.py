#!/usr/bin/env python3
"""One sha256 per case over the raw bytes of every output and every gradient (inputs and parameters included) of the autograd layer
(xvit/functional.py over xvit/ops.py): each Function on the smallest shapes that reach its paths, a training step of a small ModelCross
and ModelVIT, a captured step with two replays, and the interpret calls.  A second pass runs the same cases with ops.PROFILE = [] and
prints a sha256 of each case's sequence of (family, work, kind) records: the same launches in the same order.

The directory the xvit package is imported from is the first argument, so two trees of the Python layer are compared on ONE build of
the library:

    XVIT_LIB=$PWD/cross-attention-vit_amd/xvit/libxvit_hip.so python tools/autograd_digest.py /path/to/other/cross-attention-vit_amd > other.txt
    python tools/autograd_digest.py > this.txt && cmp other.txt this.txt

Only names that both trees have are used.  ops.set_deterministic(True): every gradient is bit-reproducible.  Every case starts from
torch.manual_seed(its number) and from the same dropout call counter, so its inputs and seeds do not depend on the cases in front.  The
captured step is left out of the second pass (timing events cannot be recorded into a capture).  The package and library in use are
named on stderr only."""
import hashlib
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "cross-attention-vit_amd"))
import ref_cpu as R  # noqa: E402
import xvit  # noqa: E402
import xvit.functional as XF  # noqa: E402
from xvit import _lib, interpret, ops  # noqa: E402
from xvit.graph import GraphedStep  # noqa: E402

DEV = torch.device("cuda:0")
B, D, H, F, EPS = 2, 128, 2, 256, 1e-5          # 64-wide heads; N = 65 is the 64 m + 1 CLS-peel form, N = 50 is not
CASES = []


def case(name, trace=True):
    def deco(fn):
        CASES.append((name, fn, trace))
        return fn
    return deco


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(b"-" if t is None else t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def rnd(*shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(tuple(shape)) * scale).to(DEV, dtype)


def leaf(*shape, scale=1.0, dtype=torch.float32):
    return rnd(*shape, scale=scale, dtype=dtype).requires_grad_(True)


def par(*shape, scale=0.05, shift=0.0):
    return torch.nn.Parameter(rnd(*shape, scale=scale) + shift)


def norm_par(d=D):
    return [par(d, scale=0.1, shift=1.0), par(d)]


def backprop(outs, leaves):
    """Random gradients into every floating-point output that has a graph -> the outputs, then the gradient of every leaf."""
    outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
    live = [o for o in outs if o.requires_grad]
    torch.autograd.backward(live, [rnd(*o.shape, dtype=o.dtype) for o in live])
    torch.cuda.synchronize()
    return outs + [t.grad for t in leaves]


def self_block_params():
    return [*norm_par(), par(3 * D, D), par(D, D), par(D), *norm_par(), par(F, D), par(F), par(D, F), par(D)]


def encoder_block_params():
    qkv = [t for _ in range(3) for t in (par(D, D), par(D))]
    return [*norm_par(), *qkv, par(D, D), par(D), *norm_par(), par(F, D), par(F), par(D, F), par(D)]


def fusion_params():
    proj = [t for _ in range(4) for t in (par(D, D), par(D))]          # wq, bq, wk, bk, wv, bv, wp, bp
    return [*norm_par(), *proj, *norm_par(), par(F, D), par(F), par(D, F), par(D)]


for p, N in itertools.product((0.0, 0.1), (65, 50)):
    @case(f"SelfAttentionBlockFn x2 p {p} N {N}")
    def _(p=p, N=N):
        x, w1, w2 = leaf(B, N, D), self_block_params(), self_block_params()
        y = XF.SelfAttentionBlockFn.apply(x, *w1, H, EPS, p, False)
        y = XF.SelfAttentionBlockFn.apply(y, *w2, H, EPS, p, True)                    # its dx goes to a block: the bf16 hand-off
        return backprop(y, [x, *w1, *w2])

for rates, N in (*(((r), 65) for r in ((0.0, 0.0, 0.0), (0.1, 0.0, 0.0), (0.0, 0.1, 0.0), (0.1, 0.1, 0.1))), ((0.1, 0.1, 0.1), 50)):
    @case(f"EncoderBlockFn (p_out, p_ffn, p_attn) {rates} N {N}")
    def _(rates=rates, N=N):
        x, w = leaf(B, N, D), encoder_block_params()
        return backprop(XF.EncoderBlockFn.apply(x, *w, H, 1e-6, *rates), [x, *w])

FUSION_SHAPES = (("concat", True, False, False), ("concat exclusive", True, True, False), ("cls", False, False, False), ("cls narrow xi", False, False, True))
for form, p, (tag, concat, exclusive, narrow), N in (*itertools.product(("dense", "lowrank"), (0.0, 0.1), FUSION_SHAPES, (65,)),
                                                     ("dense", 0.1, FUSION_SHAPES[0], 50), ("lowrank", 0.1, FUSION_SHAPES[2], 50)):
    @case(f"CrossFusionFn {form} p {p} {tag} N {N}")
    def _(form=form, p=p, concat=concat, exclusive=exclusive, narrow=narrow, N=N):
        xi, xj, w = leaf(B, 1 if narrow else N, D), leaf(B, N, D), fusion_params()
        prev, XF.XATTN_FORM = XF.XATTN_FORM, form
        try:
            # exclusive: x_i is produced inside the block (never a leaf) and its CLS rows are overwritten in place
            y = XF.CrossFusionFn.apply(xi.clone() if exclusive else xi, xj, *w, H, EPS, concat, p, exclusive)
            return backprop(y, [xi, xj, *w])
        finally:
            XF.XATTN_FORM = prev

VOL, PATCH = (2, 2, 1, 8, 8, 16), (4, 4, 8)                       # P = 8 patches of 128 voxels: the patchify path
VOL_FUSED, PATCH_FUSED, D_FUSED = (2, 2, 1, 64, 64, 32), (4, 8, 8), 256     # 2052 rows of 256 voxels: the fused gather / scatter GEMMs


def embed_params(vol, patch, d, concat):
    P, pd = ops._patch_counts(vol, patch)
    return [par(d, pd), par(d), par(1, 1, d), par(1, (vol[1] * P if concat else P) + 1, d)]


for (tag, vol, patch, d, dt), p, grad in itertools.product((("fp32 volume", VOL, PATCH, D, torch.float32), ("bf16 volume", VOL_FUSED, PATCH_FUSED, D_FUSED, torch.bfloat16)),
                                                           (0.0, 0.1), (False, True)):
    @case(f"PatchEmbedFn {tag} p {p} volume grad {int(grad)}")
    def _(vol=vol, patch=patch, d=d, dt=dt, p=p, grad=grad):
        img, w = rnd(*vol, dtype=dt).requires_grad_(grad), embed_params(vol, patch, d, False)
        fused = ops.patch_embed_supported(img, patch, d, cls_rows=1)
        return backprop(XF.PatchEmbedFn.apply(img, *w, patch, p, False, None), [img, *w]) + [torch.tensor([int(fused)])]

for p in (0.0, 0.1):
    @case(f"PatchEmbedFn concat p {p}")
    def _(p=p):
        img, w = leaf(*VOL), embed_params(VOL, PATCH, D, True)
        return backprop(XF.PatchEmbedFn.apply(img, *w, PATCH, p, True, None), [img, *w])

    @case(f"PatchEmbedFn keep p {p}")
    def _(p=p):
        img, w = rnd(*VOL), embed_params(VOL, PATCH, D, False)
        S, P, K = VOL[0] * VOL[1], ops._patch_counts(VOL, PATCH)[0], 5
        keep = ops.token_select_draw(torch.empty(S, K, dtype=torch.int32, device=DEV), torch.empty(S, P, dtype=torch.int32, device=DEV), VOL[0], False, 0x5EED)
        return backprop(XF.PatchEmbedFn.apply(img, *w, PATCH, p, False, keep), w) + list(keep)

for N, p in itertools.product((1, 65), (0.0, 0.1)):
    @case(f"HeadFn N {N} p {p}")
    def _(N=N, p=p):
        x, w = leaf(B, N, D), [*norm_par(), par(F, D), par(F), par(2, F), par(2)]
        return backprop(XF.HeadFn.apply(x, *w, EPS, p), [x, *w])

for smoothing in (0.0, 0.1):
    @case(f"MeanCrossEntropyFn smoothing {smoothing}")
    def _(smoothing=smoothing):
        lm, labels = leaf(2, 5, 3), torch.randint(0, 3, (5,)).to(DEV)
        return backprop(XF.MeanCrossEntropyFn.apply(lm, labels, smoothing), [lm])

    @case(f"MeanMixCrossEntropyFn smoothing {smoothing}")
    def _(smoothing=smoothing):
        Bn = 5
        lm, labels = leaf(2, Bn, 3), torch.randint(0, 3, (Bn,)).to(DEV)
        table, lam = torch.zeros(Bn, _lib.MIX_NPARAM), torch.rand(Bn) * 0.8 + 0.1
        table[:, _lib.MIX_PARTNER], table[:, _lib.MIX_LAM], table[:, _lib.MIX_LAM0] = torch.arange(Bn, dtype=torch.float32), 1.0, 1.0
        table[::2, _lib.MIX_MODE], table[::2, _lib.MIX_PARTNER] = _lib.MIX_MODE_MIXUP, ((torch.arange(Bn) + 1) % Bn)[::2].float()
        table[::2, _lib.MIX_LAM], table[::2, _lib.MIX_OML], table[::2, _lib.MIX_LAM0] = lam[::2], 1.0 - lam[::2], lam[::2]
        return backprop(XF.MeanMixCrossEntropyFn.apply(lm, labels, table.to(DEV), smoothing), [lm])


@case("LayerNormFn")
def _():
    x, w = leaf(B, 50, D), norm_par()
    return backprop(XF.LayerNormFn.apply(x, *w, EPS), [x, *w])


for bias, out_f32, p in itertools.product((True, False), (True, False), (0.0, 0.1)):
    @case(f"LinearFn bias {int(bias)} fp32 out {int(out_f32)} p {p}")
    def _(bias=bias, out_f32=out_f32, p=p):
        x, w, b = leaf(B, 50, D), par(F, D), par(F) if bias else None
        return backprop(XF.LinearFn.apply(x, w, b, out_f32, p), [x, w] + ([b] if bias else []))

for p in (0.0, 0.1):
    @case(f"FeedForwardFn p {p}")
    def _(p=p):
        x, w = leaf(B, 50, D), [par(F, D), par(F), par(D, F), par(D)]
        return backprop(XF.FeedForwardFn.apply(x, *w, p), [x, *w])

    for N in (65, 50):
        @case(f"AttentionCoreFn p {p} N {N}")
        def _(p=p, N=N):
            qkv = leaf(B, N, 3 * D, dtype=torch.bfloat16)
            return backprop(XF.AttentionCoreFn.apply(qkv, H, 0.125, p), [qkv])

    @case(f"ClsAttentionCoreFn p {p}")
    def _(p=p):
        q, kv = leaf(B, D), leaf(B, 50, 2 * D, dtype=torch.bfloat16)
        return backprop(XF.ClsAttentionCoreFn.apply(q, kv, H, 0.125, p), [q, kv])


def mae_draw(S, P, K, Bn):
    keep = ops.token_select_draw(torch.empty(S, K, dtype=torch.int32, device=DEV), torch.empty(S, P, dtype=torch.int32, device=DEV), Bn, False, 0xC0FFEE)
    return keep, ops.token_select_complement(keep[1], K)


@case("MaeUnshuffleFn")
def _():
    M, P, K, dd = 2, 8, 3, 68
    keep, _drop = mae_draw(M * B, P, K, B)
    t = [leaf(M * B, K + 1, dd), leaf(1, 1, dd), leaf(1, P + 1, dd), leaf(M, 1, dd)]
    return backprop(XF.MaeUnshuffleFn.apply(*t, keep), t)


@case("TokenRowsGatherFn")
def _():
    M, P, K, dd = 2, 8, 3, 68
    _keep, drop = mae_draw(M * B, P, K, B)
    x = leaf(M * B, P + 1, dd)
    return backprop(XF.TokenRowsGatherFn.apply(x, drop), [x])


for dt, norm_pix in itertools.product((torch.float32, torch.bfloat16), (True, False)):
    @case(f"MaskedPatchLossFn pred {dt} norm_pix {int(norm_pix)}")
    def _(dt=dt, norm_pix=norm_pix):
        P, pd = ops._patch_counts(VOL, PATCH)
        _keep, drop = mae_draw(VOL[0] * VOL[1], P, 3, VOL[0])
        pred, img = leaf(VOL[0] * VOL[1] * (P - 3), pd, dtype=dt), rnd(*VOL)
        return backprop(XF.MaskedPatchLossFn.apply(pred, img, drop[0], PATCH, norm_pix), [pred])


def small_config(**over):
    """A 2-modality model of the width of the cases above; 64 patches: N = 65, or 33 under patch dropout 0.5."""
    return R.make_config("tiny", hidden_dim=D, mlp_dim=F, num_heads=H, img_size=(32, 32, 8), patch_size=(8, 8, 2), **over)


def model_and_inputs(cls, cfg, batch=B):
    model = cls(cfg).to(DEV)
    img, labels = R.make_inputs(cfg, batch, seed=3)
    return model, img.to(DEV), labels.to(DEV)


def train_step(model, img, labels):
    model.train()
    logits, loss = model(img, labels)
    loss.backward()
    torch.cuda.synchronize()
    return [logits, loss] + [q.grad for q in model.parameters()]


@case("ModelCross training step, dropout and patch dropout")
def _():
    return train_step(*model_and_inputs(xvit.ModelCross, small_config(dropout=0.1, patch_dropout=0.5)))


@case("ModelCross training step, no dropout")
def _():
    return train_step(*model_and_inputs(xvit.ModelCross, small_config()))


@case("ModelVIT training step, dropout")
def _():
    return train_step(*model_and_inputs(xvit.ModelVIT, small_config(num_layers=2, dropout=0.1)))


@case("GraphedStep capture and two replays", trace=False)
def _():
    model, img, labels = model_and_inputs(xvit.ModelCross, small_config(dropout=0.1))
    model.train()
    step, out = GraphedStep(model, img, labels), []
    for _ in range(2):
        logits, loss = step(img, labels)
        torch.cuda.synchronize()
        out += [logits.clone(), loss.clone()] + [q.grad.clone() for q in model.parameters()]
    return out


@case("interpret.attention_maps with rollout, relevance_maps")
def _():
    model, img, _labels = model_and_inputs(xvit.ModelCross, small_config())
    model.eval()
    maps, rel = interpret.attention_maps(model, img, rollout=True), interpret.relevance_maps(model, img)
    torch.cuda.synchronize()
    out = [maps.logits, rel.logits, rel.target]
    for table in (maps.self_attn, maps.fusion, maps.rollout, rel.relevance, rel.fusion):
        out += [table[k] for k in sorted(table, key=str)]
    return out


def run(number, fn):
    torch.manual_seed(number)
    XF._DROP_CALLS = 1000 * number
    XF.arena_reset()
    return fn()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("autograd_digest: needs a GPU")
    print(f"autograd_digest: package {os.path.dirname(xvit.__file__)}, library {_lib.LIB_PATH}, version {_lib.load().xvit_version()}", file=sys.stderr)
    ops.set_deterministic(True)
    for number, (name, fn, _trace) in enumerate(CASES, 1):
        print(f"{name:<80s} {digest(run(number, fn))}")
    traced = [(number, name, fn) for number, (name, fn, trace) in enumerate(CASES, 1) if trace]
    for number, name, fn in traced:
        ops.PROFILE = []
        try:
            run(number, fn)
            records = repr([(family, work, kind) for family, work, kind, _s, _e in ops.PROFILE])
        finally:
            ops.PROFILE = None
        print(f"{'launches: ' + name:<80s} {hashlib.sha256(records.encode()).hexdigest()}")
    torch.cuda.synchronize()
    print(f"autograd_digest: {len(CASES)} cases, {len(traced)} launch traces", file=sys.stderr)
