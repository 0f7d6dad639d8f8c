"""GPU: the masked-pretraining kernels (csrc/mae.hip) element-wise.

Every destination sits between sentinels that are checked afterwards, and NaN sits behind every input row a kernel must not read (the
kept patches of the volume for the loss, the CLS and kept rows for the row gather).  The complement, the unshuffle pair and the row
gather / scatter are compared bit for bit with the NumPy restatements of tests/_mae_check.py; every element of the loss kernels' outputs
is compared with float64 under the bounds derived there, and a second call must give the same bits."""
import numpy as np
import pytest
import torch

import _mae_check as C
import _tokdrop_check as T
from _util import dev

pytestmark = pytest.mark.gpu

PAD = 64                  # sentinel elements on either side of a destination (a multiple of 16 bytes: the destination stays aligned)


class Guarded:
    """A destination tensor inside a larger buffer of sentinels."""

    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.value = -777 if dtype == torch.int32 else -12345.0
        self.buf = torch.full((PAD + n + PAD,), self.value, dtype=dtype, device=dev())
        self.t = self.buf[PAD:PAD + n].view(*shape)

    def intact(self):
        edge = torch.cat((self.buf[:PAD], self.buf[-PAD:]))
        return bool((edge == torch.full_like(edge, self.value)).all())

    def untouched_inside(self):
        return bool((self.t == torch.full_like(self.t, self.value)).any())


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


def _keep(S, P, K, seed):
    rng = np.random.default_rng(seed)
    keep_idx = np.stack([np.sort(rng.choice(P, size=K, replace=False)) for _ in range(S)]).astype(np.int32)
    return keep_idx, T.slot_of(keep_idx, P)


# ---- complement ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("P", [2, 63, 64, 65, 1024, 1025, 8192])
def test_complement_bit_for_bit(P):
    from xvit import ops
    S = 3
    for K in sorted({1, max(1, P // 2), P - 1}):
        keep_idx, slot = _keep(S, P, K, seed=P + K)
        drop, ms = Guarded((S, P - K), torch.int32), Guarded((S, P), torch.int32)
        ops.token_select_complement(torch.from_numpy(slot).to(dev()), K, drop.t, ms.t)
        torch.cuda.synchronize()
        want_drop, want_ms = C.complement(slot, K)
        assert drop.intact() and ms.intact() and not drop.untouched_inside() and not ms.untouched_inside()
        assert same_bits(drop.t, want_drop) and same_bits(ms.t, want_ms), (P, K)
        assert all(np.array_equal(want_drop[s], np.flatnonzero(slot[s] < 0)) for s in range(S))


def test_complement_of_a_row_with_the_wrong_count_writes_inside_its_destinations():
    """The caller's error (include/xvit.h): the first Rm dropped patches are listed, the rest read as kept; a short row ends in -1."""
    from xvit import ops
    P, K = 130, 65
    slot = T.slot_of(_keep(3, P, K, seed=1)[0], P)
    slot[0, np.flatnonzero(slot[0] >= 0)[:7]] = -1          # 7 more dropped than Rm
    slot[2, np.flatnonzero(slot[2] < 0)[:9]] = 0            # 9 fewer
    drop, ms = Guarded((3, P - K), torch.int32), Guarded((3, P), torch.int32)
    ops.token_select_complement(torch.from_numpy(slot).to(dev()), K, drop.t, ms.t)
    torch.cuda.synchronize()
    want_drop, want_ms = C.complement(slot, K)
    assert drop.intact() and ms.intact()
    assert same_bits(drop.t, want_drop) and same_bits(ms.t, want_ms)
    assert int((want_drop[2] == -1).sum()) == 9 and int(want_ms[0].max()) == P - K - 1


# ---- unshuffle, gather, scatter -------------------------------------------------------------------------------------------------------------


def _unshuffle_case(K, dd, keep_idx=None, M=3, B=2, P=32, seed=0):
    S = M * B
    rng = np.random.default_rng(100 * K + dd + seed)
    if keep_idx is None:
        keep_idx, slot = _keep(S, P, K, seed=K + dd)
    else:
        slot = T.slot_of(keep_idx, P)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)      # noqa: E731
    return dict(S=S, M=M, B=B, P=P, K=K, dd=dd, keep_idx=keep_idx, slot=slot, xe=f(S, K + 1, dd), mask=f(dd), dpos=f(P + 1, dd), dmod=f(M, dd), dy=f(S, P + 1, dd))


def _check_unshuffle_gather_scatter(c):
    from xvit import ops
    g = lambda a: torch.from_numpy(a).to(dev())                           # noqa: E731
    S, M, B, P, K, dd = (c[k] for k in ("S", "M", "B", "P", "K", "dd"))
    Rm = P - K
    slot_t, keep_t = g(c["slot"]), g(c["keep_idx"])
    # forward
    y = Guarded((S, P + 1, dd))
    ops.mae_unshuffle_fwd(g(c["xe"]), g(c["mask"]), g(c["dpos"]), g(c["dmod"]), slot_t, out=y.t)
    torch.cuda.synchronize()
    assert y.intact() and same_bits(y.t, C.unshuffle_fwd(c["xe"], c["mask"], c["dpos"], c["dmod"], c["slot"], B))
    # backward
    outs = [Guarded(shape) for shape in ((S, K + 1, dd), (dd,), (M, P + 1, dd), (S, dd))]
    ops.mae_unshuffle_bwd(g(c["dy"]), keep_t, slot_t, M, out=tuple(o.t for o in outs))
    torch.cuda.synchronize()
    want = C.unshuffle_bwd(c["dy"], c["keep_idx"], c["slot"], M)
    assert all(o.intact() and not o.untouched_inside() for o in outs)
    for name, o, w in zip(("dxe", "dmask_token", "ddpos_m"), outs, want):
        assert same_bits(o.t, w), (name, K, dd)
    # gather: NaN behind the CLS rows and the kept patches, which only the dropped rows' readers must not touch
    drop_idx, mslot = C.complement(c["slot"], K)
    x = c["dy"].copy()
    x[:, 0] = np.nan
    for s in range(S):
        x[s, 1 + c["keep_idx"][s]] = np.nan
    rows = Guarded((S * Rm, dd))
    ops.token_rows_gather(g(x), g(drop_idx), out=rows.t)
    torch.cuda.synchronize()
    assert rows.intact() and same_bits(rows.t, C.rows_gather(c["dy"], drop_idx)) and not bool(torch.isnan(rows.t).any())
    # scatter
    dg = np.random.default_rng(K + dd).standard_normal((S * Rm, dd)).astype(np.float32)
    dx = Guarded((S, P + 1, dd))
    ops.token_rows_scatter(g(dg), g(mslot), Rm, out=dx.t)
    torch.cuda.synchronize()
    want_dx = C.rows_scatter(dg, mslot, Rm)
    assert dx.intact() and not dx.untouched_inside() and same_bits(dx.t, want_dx)
    assert bool((dx.t[:, 0] == 0).all())


@pytest.mark.parametrize("dd", [64, 192])
@pytest.mark.parametrize("K", [1, 16, 31])
def test_unshuffle_gather_scatter_bit_for_bit(K, dd):
    _check_unshuffle_gather_scatter(_unshuffle_case(K, dd))


def test_unshuffle_with_a_patch_everyone_keeps_and_a_patch_everyone_drops():
    P, K, S = 32, 16, 6
    rng = np.random.default_rng(5)
    rows = []
    for _ in range(S):                                                    # patch 7 kept by every sequence, patch 20 dropped by every sequence
        others = rng.choice([p for p in range(P) if p not in (7, 20)], size=K - 1, replace=False)
        rows.append(np.sort(np.append(others, 7)))
    keep_idx = np.stack(rows).astype(np.int32)
    c = _unshuffle_case(K, 64, keep_idx=keep_idx)
    assert (c["slot"][:, 7] >= 0).all() and (c["slot"][:, 20] < 0).all()
    _check_unshuffle_gather_scatter(c)
    # the mask token's gradient sees patch 20 of every sequence and patch 7 of none: move dy there and look at the restatement's answer
    dy2 = c["dy"].copy()
    dy2[:, 1 + 7] += 100.0
    assert same_bits(C.unshuffle_bwd(dy2, keep_idx, c["slot"], 3)[1], C.unshuffle_bwd(c["dy"], keep_idx, c["slot"], 3)[1])


# ---- the loss --------------------------------------------------------------------------------------------------------------------------------


def _run_loss(case, vol_bf16, pred_bf16, norm, misalign=False):
    """-> (got dict of numpy arrays, everything intact?) from two calls that must agree bit for bit."""
    from xvit import ops
    vdt, pdt = (torch.bfloat16 if vol_bf16 else torch.float32), (torch.bfloat16 if pred_bf16 else torch.float32)
    img = torch.from_numpy(case["img"]).to(vdt)
    if misalign:                                                          # the volume's base 2 bytes past a 16-byte boundary
        assert vol_bf16
        buf = torch.full((img.numel() + 16,), float("nan"), dtype=vdt, device=dev())
        buf[1:1 + img.numel()] = img.reshape(-1).to(dev())
        img_t = buf[1:1 + img.numel()].view(img.shape)
        assert img_t.data_ptr() % 16 == 2 and img_t.is_contiguous()
    else:
        img_t = img.to(dev())
        assert img_t.data_ptr() % 16 == 0
    pred_t = torch.from_numpy(case["pred"]).to(pdt).to(dev())
    drop_t = torch.from_numpy(case["drop_idx"]).to(dev())
    S, Rm, pd = case["S"], case["Rm"], case["pd"]
    g_t = torch.tensor([C.LOSS_G], dtype=torch.float32, device=dev())
    runs = []
    for _ in range(2):
        outs = [Guarded(shape) for shape in ((1,), (S,), (S * Rm,), (S * Rm, 2))]
        loss, loss_seq, row_loss, stats = ops.mae_loss_fwd(pred_t, drop_t, img_t, case["patch"], norm, out=tuple(o.t for o in outs))
        dp = Guarded((S * Rm, pd), pdt)
        ops.mae_loss_bwd(pred_t, drop_t, img_t, case["patch"], stats, g_t, out=dp.t)
        torch.cuda.synchronize()
        assert all(o.intact() and not o.untouched_inside() for o in outs) and dp.intact()
        runs.append(dict(mean=stats[:, 0].cpu().numpy(), rstd=stats[:, 1].cpu().numpy(), row_loss=row_loss.cpu().numpy(), loss_seq=loss_seq.cpu().numpy(),
                         loss=loss.cpu().numpy(), dpred=dp.t.float().cpu().numpy()))
    for k in C.BOUNDED:
        assert same_bits(runs[0][k], runs[1][k]), k                      # no atomics, fixed orders: the same bits at every run
    return runs[0]


def _check_loss(shape, vol_bf16, pred_bf16, norm, misalign=False):
    case = C.loss_case(shape, vol_bf16, pred_bf16)
    got = _run_loss(case, vol_bf16, pred_bf16, norm, misalign)
    ref = C.loss_ref64(case["pred"], np.nan_to_num(case["img"], nan=0.0), case["patch"], case["drop_idx"], norm, C.LOSS_G)
    bounds = C.loss_bounds(ref, pred_bf16)
    res = C.violations(got, ref, bounds)
    for k, (bad, worst) in res.items():
        print(f"mae loss {shape} vol_bf16={vol_bf16} pred_bf16={pred_bf16} norm={norm} misalign={misalign} {k}: worst |err| / bound = {worst:.3e}")
    for k, (bad, worst) in res.items():
        assert bad == 0, (k, bad, worst)
    if not norm:
        assert bool((got["mean"] == 0).all()) and bool((got["rstd"] == 1).all())
    else:
        r = case["special"]["constant"]
        assert ref["_var"][r] == 0.0 and abs(got["mean"][r] - 0.75) <= bounds["mean"][r]
        if case["special"]["offset"] is not None:
            r = case["special"]["offset"]
            assert abs(ref["mean"][r]) >= 1000 * np.sqrt(ref["_var"][r])
    return res


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("pred_bf16", [False, True])
@pytest.mark.parametrize("vol_bf16", [False, True])
@pytest.mark.parametrize("shape", list(C.LOSS_SHAPES))
def test_loss_forward_and_backward_against_float64(shape, vol_bf16, pred_bf16, norm):
    _check_loss(shape, vol_bf16, pred_bf16, norm)


@pytest.mark.parametrize("pred_bf16", [False, True])
def test_loss_with_a_volume_two_bytes_off_alignment_takes_the_scalar_path(pred_bf16):
    """wp = 8 would take the 16-byte loads; a bf16 volume whose base sits 2 bytes past a 16-byte boundary cannot: same results, one voxel per
    access.  NaN sits right in front of and behind the volume."""
    _check_loss("pd512", True, pred_bf16, True, misalign=True)
