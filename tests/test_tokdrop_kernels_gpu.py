"""GPU: patch dropout's four kernels (csrc/token_select.hip) against their NumPy restatement (tests/_tokdrop_check.py), bit for bit:
the draw is integer work, patchify_select moves (or converts once, as xvit_patchify does) values, and the two embed kernels make single
fp32 additions in a stated order.  Every destination sits between two sentinel-filled guard zones that must come back untouched, and is
pre-filled so that an element the kernel does not write shows."""
import numpy as np
import pytest
import torch

import _tokdrop_check as T
from _util import dev

TIE = T.TIE

pytestmark = pytest.mark.gpu

GUARD = 64      # elements on either side of a destination: 128 bytes or more, so the destination keeps its 16-byte alignment


class Guarded:
    """A contiguous tensor of `shape` inside a larger buffer whose margins hold a sentinel."""

    def __init__(self, shape, dtype, fill, sentinel):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=dev())
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.copy_(fill.to(dev()) if torch.is_tensor(fill) else torch.full(tuple(shape), fill, dtype=dtype, device=dev()))
        self.sentinel = sentinel

    def check(self, what):
        margins = torch.cat((self.buf[:GUARD], self.buf[-GUARD:]))
        assert bool((margins == self.sentinel).all()), f"{what}: wrote outside its destination"


def _bits(t):
    """Exact comparison that also tells -0 from 0 and any NaN payloads apart."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _draw_on_gpu(S, B, P, K, shared, seed):
    from xvit import ops
    keep_idx, slot = Guarded((S, K), torch.int32, -7, -99), Guarded((S, P), torch.int32, -7, -99)
    ops.token_select_draw(keep_idx.t, slot.t, B, shared, seed)
    torch.cuda.synchronize()
    keep_idx.check("keep_idx"), slot.check("slot")
    return keep_idx.t.cpu().numpy(), slot.t.cpu().numpy()


@pytest.mark.parametrize("P,K", [(1, 1), (2, 1), (63, 62), (64, 64), (65, 1), (257, 128), (512, 256), (513, 512), (4096, 1024), (4096, 4096)])
def test_draw_equals_the_restatement(P, K):
    for S, B in ((1, 1), (3, 2), (7, 2)):           # B = 2 does not divide 3 or 7: u = s mod B wraps inside a modality, too
        for shared in (False, True):
            for seed in (5, 0x7FFF_FFFF_FFFF_FFC1):
                got_k, got_s = _draw_on_gpu(S, B, P, K, shared, seed)
                ref_k, ref_s = T.draw(S, B, P, K, shared, seed)
                assert np.array_equal(got_k, ref_k), (S, shared, seed, "keep_idx")
                assert np.array_equal(got_s, ref_s), (S, shared, seed, "slot")


def test_draw_mixes_in_the_device_epoch():
    """With a registered epoch counter the kernel draws with seed + epoch * constant, read on the device at run time."""
    from xvit import ops
    S, B, P, K, seed = 6, 3, 257, 128, 31
    plain = _draw_on_gpu(S, B, P, K, False, seed)
    epoch = torch.zeros(1, dtype=torch.int64, device=dev())
    ops.set_dropout_epoch(epoch)
    try:
        for e in (3, 1 << 40):
            epoch.fill_(e)
            got_k, got_s = _draw_on_gpu(S, B, P, K, False, seed)
            ref_k, ref_s = T.draw(S, B, P, K, False, seed, epoch=e)
            assert np.array_equal(got_k, ref_k) and np.array_equal(got_s, ref_s), e
            assert not np.array_equal(got_k, plain[0])
    finally:
        ops.set_dropout_epoch(None)
    again = _draw_on_gpu(S, B, P, K, False, seed)
    assert np.array_equal(again[0], plain[0]) and np.array_equal(again[1], plain[1])       # unregistered: the plain seed again


def test_draw_breaks_a_key_tie_at_the_kth_place_towards_the_smaller_patch():
    """tests/test_tokdrop_cpu.py shows that this seed gives sequence 0 two equal 32-bit keys at places K and K + 1."""
    P, K, seed = TIE["P"], TIE["K"], TIE["seed"]
    got_k, got_s = _draw_on_gpu(2, 2, P, K, False, seed)
    ref_k, ref_s = T.draw(2, 2, P, K, False, seed)
    assert np.array_equal(got_k, ref_k) and np.array_equal(got_s, ref_s)


def _hand_keep(S, P, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(P, generator=g)[:K].sort().values for _ in range(S)]).to(torch.int32)


@pytest.mark.parametrize("vol,patch", [((32, 48, 16), (16, 16, 8)),      # grid 2 x 3 x 2: a swapped axis shows
                                       ((32, 32, 2), (8, 8, 2)),          # wp = 2: the scalar path
                                       ((32, 32, 16), (8, 8, 8))])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_patchify_select_equals_the_selected_rows_of_patchify(vol, patch, dtype):
    from xvit import ops
    P, pd = (vol[0] // patch[0]) * (vol[1] // patch[1]) * (vol[2] // patch[2]), patch[0] * patch[1] * patch[2]
    for M in (1, 3):
        for B in (1, 3):
            g = torch.Generator().manual_seed(M * 10 + B)
            img = torch.randn(B, M, 1, *vol, generator=g).to(dtype).to(dev())
            full = ops.patchify(img, patch, pad_cls_row=True).view(M * B, P + 1, pd)
            assert bool((full[:, 0] == 0).all())
            for K in sorted({1, max(1, P - 1), P}):
                keep_idx = _hand_keep(M * B, P, K, seed=K + 100 * M + B)
                rows = torch.cat((torch.zeros(M * B, 1, dtype=torch.int64), 1 + keep_idx.long()), dim=1).to(dev())
                ref = torch.gather(full, 1, rows[:, :, None].expand(-1, -1, pd)).reshape(M, B * (K + 1), pd)
                out = Guarded((M, B * (K + 1), pd), torch.bfloat16, 7.0, -3.0)
                ops.patchify_select(img, patch, keep_idx.to(dev()), out=out.t)
                torch.cuda.synchronize()
                out.check("patchify_select")
                assert torch.equal(_bits(out.t), _bits(ref)), (M, B, K)
                # and the restated index map says the same (on the values patchify wrote: conversion is patchify's, tested elsewhere)
                if M == 3 and B == 3:
                    vals = img.float().cpu().numpy()
                    mine = torch.from_numpy(T.patchify_select(vals, patch, keep_idx.numpy())).to(torch.bfloat16)
                    assert torch.equal(_bits(out.t), _bits(mine)), (M, B, K, "restated map")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_patchify_select_on_a_volume_that_is_16_byte_aligned_only(dtype):
    """A view 16 bytes into its buffer still takes the 8-voxel kernel (16-byte accesses); 2 bytes further in, the one-voxel kernel: the same rows."""
    from xvit import ops
    vol, patch, B, M, P, K, pd = (32, 32, 16), (8, 8, 8), 2, 2, 32, 5, 512
    n = B * M * vol[0] * vol[1] * vol[2]
    base = torch.randn(n + 64, generator=torch.Generator().manual_seed(7)).to(dtype).to(dev())
    keep_idx = _hand_keep(M * B, P, K, seed=3)
    rows = torch.cat((torch.zeros(M * B, 1, dtype=torch.int64), 1 + keep_idx.long()), dim=1).to(dev())
    for off in (16 // base.element_size(), 16 // base.element_size() + 1):
        img = base[off:off + n].view(B, M, 1, *vol)
        assert img.data_ptr() % 32 != 0 and img.is_contiguous()
        full = ops.patchify(img.clone(), patch, pad_cls_row=True).view(M * B, P + 1, pd)
        ref = torch.gather(full, 1, rows[:, :, None].expand(-1, -1, pd)).reshape(M, B * (K + 1), pd)
        out = Guarded((M, B * (K + 1), pd), torch.bfloat16, 7.0, -3.0)
        ops.patchify_select(img, patch, keep_idx.to(dev()), out=out.t)
        torch.cuda.synchronize()
        out.check("patchify_select")
        assert torch.equal(_bits(out.t), _bits(ref)), off


def _embed_case(S, d, seed):
    """P = 37, K = 9: patch 0 is kept by nobody, patch 36 by every sequence, the rest at random."""
    P, K = 37, 9
    g = torch.Generator().manual_seed(seed)
    keep_idx = torch.stack([torch.cat(((1 + torch.randperm(P - 2, generator=g)[:K - 1]).sort().values, torch.tensor([P - 1]))) for _ in range(S)]).to(torch.int32)
    assert int(keep_idx.min()) >= 1 and bool((keep_idx[:, -1] == P - 1).all())
    return P, K, keep_idx, g


@pytest.mark.parametrize("d", [4, 192, 768, 1024])
@pytest.mark.parametrize("S", [1, 6])
def test_embed_select_fwd_equals_the_restatement(S, d):
    from xvit import ops
    P, K, keep_idx, g = _embed_case(S, d, seed=S * 1000 + d)
    x0 = torch.randn(S * (K + 1), d, generator=g)
    cls, pos = torch.randn(d, generator=g), torch.randn(P + 1, d, generator=g)
    x = Guarded((S * (K + 1), d), torch.float32, x0, -77.0)
    ops.embed_select_fwd(x.t, cls.to(dev()), pos.to(dev()), keep_idx.to(dev()))
    torch.cuda.synchronize()
    x.check("embed_select_fwd")
    ref = torch.from_numpy(T.embed_select_fwd(x0.numpy(), cls.numpy(), pos.numpy(), keep_idx.numpy()))
    assert torch.equal(_bits(x.t), _bits(ref))


@pytest.mark.parametrize("d", [4, 192, 768, 1024])
@pytest.mark.parametrize("S", [1, 6])
def test_embed_select_bwd_equals_the_restatement(S, d):
    from xvit import ops
    P, K, keep_idx, g = _embed_case(S, d, seed=S * 2000 + d)
    slot = torch.from_numpy(T.slot_of(keep_idx.numpy(), P))
    dx = torch.randn(S * (K + 1), d, generator=g)
    dpos0, dcls0 = torch.randn(P + 1, d, generator=g), torch.randn(d, generator=g)      # the kernel accumulates: non-zero prior values
    dpos0[5] = -0.0                                                                      # a signed zero as prior value (kept or not, the bits must follow the restatement)
    dpos, dcls = Guarded((P + 1, d), torch.float32, dpos0, -55.0), Guarded((d,), torch.float32, dcls0, -55.0)
    ops.embed_select_bwd(dx.to(dev()), slot.to(dev()), dpos.t, dcls.t, K)
    torch.cuda.synchronize()
    dpos.check("dpos"), dcls.check("dcls")
    ref_pos, ref_cls = T.embed_select_bwd(dx.numpy(), slot.numpy(), dpos0.numpy(), dcls0.numpy(), K)
    assert torch.equal(_bits(dpos.t), _bits(torch.from_numpy(ref_pos)))
    assert torch.equal(_bits(dcls.t), _bits(torch.from_numpy(ref_cls)))
    assert torch.equal(_bits(dpos.t[1]), _bits(dpos0[1]))                                # patch 0: nobody kept it, its row keeps its bits
    assert not torch.equal(dpos.t[P].cpu(), dpos0[P])                                    # patch 36: everybody kept it
    # a second launch accumulates on top, in the same order: the same bits as the restatement applied twice
    ops.embed_select_bwd(dx.to(dev()), slot.to(dev()), dpos.t, dcls.t, K)
    torch.cuda.synchronize()
    ref_pos2, ref_cls2 = T.embed_select_bwd(dx.numpy(), slot.numpy(), ref_pos, ref_cls, K)
    assert torch.equal(_bits(dpos.t), _bits(torch.from_numpy(ref_pos2))) and torch.equal(_bits(dcls.t), _bits(torch.from_numpy(ref_cls2)))
