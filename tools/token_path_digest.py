#!/usr/bin/env python3
"""One sha256 per case of the raw bytes the token-path kernels write (csrc/misc.hip's patchify / unpatchify / cls_row / embed_bwd,
token_select.hip, token_occupancy.hip, mae.hip, and the mean + cross-entropy tail of mix.hip), on the smallest inputs that reach each of their paths.  None of
these kernels uses atomics, so two builds of the library compute the same thing exactly when their printouts are equal:

    XVIT_LIB=/path/to/other/libxvit_hip.so python tools/token_path_digest.py > other.txt
    python tools/token_path_digest.py > this.txt && cmp other.txt this.txt

Every input comes from one fixed-seed generator; every volume and patch matrix carries -0.0, +inf, -inf, a quiet and a signalling NaN, so
that a run that is converted where it used to be copied shows.  Outputs that are accumulated into, or that a kernel may leave unwritten,
are pre-filled.  The library in use is named on stderr only."""
import hashlib
import itertools
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cross-attention-vit_amd"))
from xvit import _lib, ops  # noqa: E402

DEV = torch.device("cuda:0")
GEN = torch.Generator().manual_seed(20241020)
CASES = 0
SPECIAL = {torch.float32: (torch.int32, [-0x80000000, 0x7F800000, -0x00800000, 0x7FC00000, 0x7FA00001]),     # -0.0, +inf, -inf, qNaN, sNaN
           torch.bfloat16: (torch.int16, [-0x8000, 0x7F80, -0x0080, 0x7FC0, 0x7F81])}
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32


def say(name, *tensors):
    global CASES
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
    print(f"{name:<96s} {h.hexdigest()}")
    CASES += 1


def short(dt):
    return {F32: "fp32", BF16: "bf16"}[dt]


def rand(shape, dtype=F32, lo=-2.0, hi=2.0, off=0, special=False):
    """Uniform values in a fresh buffer whose first element sits `off` elements behind an allocation boundary; `special`: the first five
    elements are the special bit patterns."""
    n = int(torch.Size(shape).numel())
    buf = torch.empty(n + off, dtype=dtype, device=DEV)
    v = buf[off:]
    v.copy_((torch.rand(n, generator=GEN) * (hi - lo) + lo).to(dtype))
    if special:
        idt, bits = SPECIAL[dtype]
        v.view(idt)[:5] = torch.tensor(bits, dtype=idt, device=DEV)
    return v.view(shape)


def fill(shape, value, dtype=F32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def i32(rows):
    return torch.tensor(rows, dtype=I32, device=DEV)


VOL = (2, 2, 1, 8, 8, 16)
PATCHES = ((4, 4, 8), (4, 4, 4))
PLACEMENTS = (("plain", {}), ("pad_cls_row", {"pad_cls_row": True}), ("concat", {"concat": True}))


def patchifies():
    for patch, dt in itertools.product(PATCHES, (F32, BF16)):
        for pname, kw in PLACEMENTS:
            for off in (0, 1) if patch[2] == 8 else (0,):                  # one element off 32-byte alignment: the scalar path at wp = 8
                tag = f"{short(dt)} patch {patch} {pname} offset {off}"
                rows = ops.patchify(rand(VOL, dt, special=True, off=off), patch, **kw)
                say(f"patchify {tag}", rows)
                say(f"unpatchify {tag}", ops.unpatchify(rand(rows.shape, F32, special=True, off=off), fill(VOL, 7.0, dt), patch, **kw))


def patchify_selects():
    B, M = VOL[:2]
    for patch, dt in itertools.product(PATCHES, (F32, BF16)):
        P = ops._patch_counts(VOL, patch)[0]
        for off in (0, 16 // dt.itemsize, 1):                                # 32-byte aligned, 16-byte aligned only, element aligned only
            img = rand(VOL, dt, special=True, off=off)
            for K in (1, P):
                keep = (torch.arange(P, dtype=I32).repeat(M * B, 1) if K == P else i32([[0], [3], [P - 1], [2]])).to(DEV)
                keep[1, 0], keep[2, K - 1] = -1, P                          # outside the grid on both sides: zero rows
                say(f"patchify_select {short(dt)} patch {patch} offset {off} K {K}", ops.patchify_select(img, patch, keep, out=fill((M, B * (K + 1), patch[0] * patch[1] * patch[2]), 7.0, BF16)))


def draws():
    for (P, K), (S, B), shared, epoch in itertools.product(((1, 1), (64, 64), (65, 1), (1025, 512), (4096, 1024)), ((1, 1), (3, 2)), (False, True), (None, 5)):
        counter = None if epoch is None else fill((1,), epoch, torch.int64)
        ops.set_dropout_epoch(counter)
        try:
            keep, slot = ops.token_select_draw(fill((S, K), -7, I32), fill((S, P), -7, I32), B, shared, 0x5EED0123)
        finally:
            ops.set_dropout_epoch(None)
        say(f"token_select_draw P {P} K {K} S {S} B {B} shared {int(shared)} epoch {epoch}", keep, slot)


def complements():
    S = 3
    for P in (2, 64, 65, 1025, 8192):
        K = P // 2
        _, slot = ops.token_select_draw(fill((S, K), -7, I32), fill((S, P), -7, I32), S, False, 0xC0FFEE)
        kept1, dropped2 = int((slot[1] >= 0).nonzero()[0]), int((slot[2] < 0).nonzero()[-1])
        slot[1, kept1], slot[2, dropped2] = -1, 0                          # row 1: too few kept (positions past Rm unwritten); row 2: too many (-1 tail)
        say(f"token_select_complement P {P} K {K}", *ops.token_select_complement(slot, K, fill((S, P - K), -7, I32), fill((S, P), -7, I32)))


def unshuffles():
    M, B, P, K = 2, 2, 5, 2
    S, Rm = M * B, P - K
    keep = i32([[0, 1], [0, 2], [0, 3], [0, 1]])                            # patch 0: kept by everyone; patch 4: dropped by everyone
    slot = fill((S, P), -1, I32)
    slot.scatter_(1, keep.long(), torch.arange(K, dtype=I32, device=DEV).repeat(S, 1))
    drop, mslot = ops.token_select_complement(slot, K)
    keep[3, 1], drop[2, 1], mslot[1, 4] = 7, -3, Rm                        # outside the grid: zero rows
    for dd in (4, 68):
        xe, mask, dpos, dmod = rand((S, K + 1, dd)), rand((dd,)), rand((P + 1, dd)), rand((M, dd))
        say(f"mae_unshuffle_fwd dd {dd}", ops.mae_unshuffle_fwd(xe, mask, dpos, dmod, slot, out=fill((S, P + 1, dd), 7.0)))
        out = (fill((S, K + 1, dd), 7.0), fill((dd,), 7.0), fill((M, P + 1, dd), 7.0), fill((S, dd), 7.0))
        say(f"mae_unshuffle_bwd dd {dd}", *ops.mae_unshuffle_bwd(rand((S, P + 1, dd)), keep, slot, M, out=out))
        say(f"token_rows_gather dd {dd}", ops.token_rows_gather(rand((S, P + 1, dd)), drop, out=fill((S * Rm, dd), 7.0)))
        say(f"token_rows_scatter dd {dd}", ops.token_rows_scatter(rand((S * Rm, dd)), mslot, Rm, out=fill((S, P + 1, dd), 7.0)))


def losses():
    B, M, Rm = 2, 2, 3
    drop = i32([[0, 3, 7], [1, 2, 8], [4, 5, 6], [0, 2, 7]])                # P = 8; the 8 is outside the grid; sequence 0 holds the special values
    g = fill((1,), 0.7)
    for (patch, dhw), vdt, pdt, norm, off in itertools.product((((2, 2, 8), (4, 4, 16)), ((1, 1, 2), (2, 2, 4))), (F32, BF16), (F32, BF16), (True, False), (0, 1)):
        img = rand((B, M, 1) + dhw, vdt, special=True, off=off)             # off 1: element aligned only
        pred = rand((M * B * Rm, patch[0] * patch[1] * patch[2]), pdt)
        tag = f"volume {short(vdt)} pred {short(pdt)} patch {patch} norm_pix {int(norm)} offset {off}"
        out = (fill((1,), 7.0), fill((M * B,), 7.0), fill((M * B * Rm,), 7.0), fill((M * B * Rm, 2), 7.0))
        loss, loss_seq, row_loss, stats = ops.mae_loss_fwd(pred, drop, img, patch, norm, out=out)
        say(f"mae_loss_fwd {tag}", loss, loss_seq, row_loss, stats)
        say(f"mae_loss_bwd {tag}", ops.mae_loss_bwd(pred, drop, img, patch, stats, g, out=fill(pred.shape, 7.0, pdt)))


def embeds():
    S, P, K = 3, 5, 2
    keep = i32([[0, 4], [1, 2], [0, 3]])                                    # patch 0: two sequences; patches 1 .. 4: one
    slot = fill((S, P), -1, I32)
    slot.scatter_(1, keep.long(), torch.arange(K, dtype=I32, device=DEV).repeat(S, 1))
    slot[:, 1] = -1                                                        # nobody kept patch 1: its dpos row stays as it was
    for d in (4, 68):
        say(f"embed_select_fwd d {d}", ops.embed_select_fwd(rand((S * (K + 1), d)), rand((d,)), rand((P + 1, d)), keep))
        dpos, dcls = rand((P + 1, d)), rand((d,))
        ops.embed_select_bwd(rand((S * (K + 1), d)), slot, dpos, dcls, K)
        say(f"embed_select_bwd d {d}", dpos, dcls)
        dpos, dcls = rand((P + 1, d)), rand((d,))
        ops.embed_bwd(rand((S * (P + 1), d)), dpos, dcls, S, P + 1, d)
        say(f"embed_bwd d {d}", dpos, dcls)
        x = fill((S * (P + 1), d), 7.0)
        ops.cls_row_fwd(rand((d,)), rand((P + 1, d)), x, S, P + 1, d)
        say(f"cls_row_fwd d {d}", x)


def cross_entropies():
    for M, B, Cn, eps in itertools.product((1, 2), (1, 5, 257), (2, 7), (0.0, 0.1)):
        logits_m = rand((M, B, Cn), lo=-4.0, hi=4.0)
        labels = torch.randint(0, Cn, (B,), generator=GEN).to(DEV)
        tag = f"M {M} B {B} C {Cn} smoothing {eps}"
        say(f"mean_ce {tag}", *ops.mean_ce(logits_m, labels, eps))
        ones = torch.zeros(B, _lib.MIX_NPARAM)
        ones[:, _lib.MIX_PARTNER], ones[:, _lib.MIX_LAM], ones[:, _lib.MIX_LAM0] = torch.arange(B, dtype=F32), 1.0, 1.0
        mixed = ones.clone()                                               # every second record mixed with its right-hand neighbour
        lam = torch.rand(B, generator=GEN) * 0.8 + 0.1
        mixed[::2, _lib.MIX_MODE], mixed[::2, _lib.MIX_PARTNER] = _lib.MIX_MODE_MIXUP, ((torch.arange(B) + 1) % B)[::2].to(F32)
        mixed[::2, _lib.MIX_LAM], mixed[::2, _lib.MIX_OML], mixed[::2, _lib.MIX_LAM0] = lam[::2], 1.0 - lam[::2], lam[::2]
        for name, table in (("lam = 1", ones), ("mixed", mixed)):
            say(f"mean_ce_mix {name} {tag}", *ops.mean_ce_mix(logits_m, labels, table.to(DEV), eps))


def occupancies():
    B, M = VOL[:2]
    for patch, dt in itertools.product(PATCHES, (F32, BF16)):
        P = ops._patch_counts(VOL, patch)[0]
        for off, above in itertools.product((0, 16 // dt.itemsize, 1), (0.0, -0.5)):   # the special values against 0: -0.0, the NaNs and -inf are not counted
            say(f"patch_occupancy {short(dt)} patch {patch} offset {off} above {above}",
                ops.patch_occupancy(rand(VOL, dt, special=True, off=off), patch, above, out=fill((M * B, P), -7, I32)))


def rankeds():
    for (P, K), (S, B), shared, mode, epoch in itertools.product(((1, 1), (65, 1), (1025, 512), (4096, 1024)), ((1, 1), (6, 3)), (False, True),
                                                                 (_lib.TOKEN_RANK_RANDOM, _lib.TOKEN_RANK_TOP), (None, 5)):
        occ = torch.randint(0, 9, (S, P), generator=GEN).to(I32).to(DEV)       # few distinct counts: ties everywhere
        counter = None if epoch is None else fill((1,), epoch, torch.int64)
        ops.set_dropout_epoch(counter)
        try:
            n_fg = fill((S,), -7, I32)
            keep, slot = ops.token_select_ranked(occ, fill((S, K), -7, I32), fill((S, P), -7, I32), B, shared, mode, 5, 0x5EED0123, n_fg)
        finally:
            ops.set_dropout_epoch(None)
        say(f"token_select_ranked P {P} K {K} S {S} B {B} shared {int(shared)} mode {mode} epoch {epoch}", keep, slot, n_fg)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("token_path_digest: needs a GPU")
    print(f"token_path_digest: {_lib.LIB_PATH}, library version {_lib.load().xvit_version()}", file=sys.stderr)
    # new parts go at the end: every part draws from the one generator, so the cases in front keep their inputs
    for part in (patchifies, patchify_selects, draws, complements, unshuffles, losses, embeds, cross_entropies, occupancies, rankeds):
        part()
    torch.cuda.synchronize()
    print(f"token_path_digest: {CASES} cases", file=sys.stderr)
