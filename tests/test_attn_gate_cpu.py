"""The element-wise attention gate (tests/_attn_check.py) has teeth, on the CPU.

Not too tight: the bf16-emulating oracle (R.softmax_attention under R.emulate_bf16(), attn_bwd_emulated) and an fp32 emulation of the
forward kernel's online softmax (P rounded relative to the RUNNING max, tile by tile), each rounded to bf16, pass on every element.
Not too loose: each planted defect, a mistake a kernel could make at a tile edge, exceeds the bound by at least 4x at its worst element,
so kernel noise that is itself inside the bound cannot hide it."""
import pytest
import torch

import ref_cpu as R
from _attn_check import (attn_bwd_emulated, attn_ref, check_bwd, check_fwd, online_softmax_emulated, ratio_of)
from _util import randn, rt

MARGIN = 4.0


def _operands(B, H, N, seed, spikes=False):
    q, k, v, do = (rt(randn(B, H, N, 64, seed=seed + i)) for i in range(4))
    if spikes:
        plant_spikes(q, k, [N - 1])
    return q, k, v, do


def plant_spikes(q, k, keys):
    """k[j] = 6 q[i] (bf16-rounded) in every (b, h): one dominant key per query wave of each 128-query workgroup, key j taken from
    `keys` in turn.  Queries i = 32 w + 5 of each wave w; a key already used as a spike is not reused."""
    B, H, N, _ = q.shape
    placed = []
    for i, j in zip(range(5, N, 32), keys * N):
        if j in [p[1] for p in placed]:
            continue
        k[:, :, j] = rt(q[:, :, i] * 6.0)
        placed.append((i, j))
    return placed


def _emulated(q, k, v, do, scale, mask=None):
    """bf16-emulating oracle: o, lse and the gradients as the kernels round them, and the DEVICE-like o (bf16) for delta."""
    if mask is None:
        with R.emulate_bf16():
            o, lse = R.softmax_attention(q, k, v, scale)
    else:
        o, lse = online_softmax_emulated(q, k, v, scale, mask=mask)
    o = rt(o)
    dq, dk, dv = attn_bwd_emulated(q, k, v, o, do, lse, scale, mask=mask)
    return o, lse, rt(dq), rt(dk), rt(dv)


SHAPES = [(2, 3, 1), (2, 3, 2), (2, 3, 33), (2, 3, 65), (2, 3, 129), (2, 3, 193), (1, 2, 513), (1, 1, 4097)]


@pytest.mark.parametrize("scale", [0.125, 4.0])
@pytest.mark.parametrize("B,H,N", SHAPES)
def test_bf16_emulating_oracle_passes(B, H, N, scale):
    q, k, v, do = _operands(B, H, N, seed=N)
    o, lse, dq, dk, dv = _emulated(q, k, v, do, scale)
    ref = attn_ref(q, k, v, scale, o_dev=o, dO=do)
    assert check_fwd(ref, o, lse) <= 1.0
    assert check_bwd(ref, dq, dk, dv) <= 1.0


@pytest.mark.parametrize("scale", [0.125, 4.0])
@pytest.mark.parametrize("B,H,N", SHAPES)
def test_online_softmax_emulation_passes(B, H, N, scale):
    q, k, v, _ = _operands(B, H, N, seed=N + 50, spikes=N > 64)
    o, lse = online_softmax_emulated(q, k, v, scale)
    check_fwd(attn_ref(q, k, v, scale), rt(o), lse)


@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("B,H,N", [(2, 3, 33), (2, 3, 129)])
def test_dropout_emulation_passes(B, H, N, p):
    q, k, v, do = _operands(B, H, N, seed=N + 70)
    g = torch.Generator().manual_seed(N)
    mask = (torch.rand(B, H, N, N, generator=g) >= p).float() / (1 - p)
    o, lse, dq, dk, dv = _emulated(q, k, v, do, 0.125, mask=mask)
    ref = attn_ref(q, k, v, 0.125, mask=mask, o_dev=o, dO=do)
    check_fwd(ref, o, lse)
    check_bwd(ref, dq, dk, dv)


# ------------------------------------------------------------------------------------------------------------ planted defects
def _ratios(ref, got):
    """Worst ratio to the bound of each defective output (bf16-rounded like the kernels' outputs, lse fp32)."""
    r = {}
    for name, t in got.items():
        if name == "lse":
            r[name] = ratio_of(t.float(), ref["lse"], S=ref["S_lse"], lse=True)
        else:
            r[name] = ratio_of(rt(t.float()), ref[name], ref["T_" + name], ref["S_" + name])
    return r


def _assert_caught(ref, got, what):
    r = _ratios(ref, got)
    weak = {n: round(x, 2) for n, x in r.items() if not x >= MARGIN}
    assert not weak, f"{what}: the gate misses by less than {MARGIN}x on {weak} (all: { {n: round(x, 1) for n, x in r.items()} })"


def _case(B, H, N, scale=0.125, spikes=False):
    q, k, v, do = _operands(B, H, N, seed=3 * N + 1, spikes=spikes)
    o_dev = rt(attn_ref(q, k, v, scale)["o"].float())
    return q, k, v, do, o_dev, attn_ref(q, k, v, scale, o_dev=o_dev, dO=do)


def _with_keys(q, k, v, do, o_dev, scale, keep, extra=None):
    """The reference over keys `keep` (+ keys `extra` a second time): dk / dv of each original key summed over its copies, 0 when
    the key was dropped."""
    idx = torch.tensor(list(keep) + list(extra or []))
    r = attn_ref(q, k[:, :, idx], v[:, :, idx], scale, o_dev=o_dev, dO=do)
    dk, dv = torch.zeros(k.shape, dtype=torch.float64), torch.zeros(v.shape, dtype=torch.float64)
    dk.index_add_(2, idx, r["dk"])
    dv.index_add_(2, idx, r["dv"])
    return {"o": r["o"], "lse": r["lse"], "dq": r["dq"], "dk": dk, "dv": dv}


DEFECT_SHAPES = [(1, 2, 129), (1, 1, 4097)]


@pytest.mark.parametrize("which", ["last", "63", "64", "32", "0"])
@pytest.mark.parametrize("B,H,N", DEFECT_SHAPES)
def test_dropped_key_is_caught(B, H, N, which):
    """One key left out of the softmax, lse and every backward sum: the tail key, the keys on either side of the first 64-key tile
    boundary, the first key of the second 32-key block, and key 0 (the peel's initial state)."""
    j = N - 1 if which == "last" else int(which)
    q, k, v, do, o_dev, ref = _case(B, H, N)
    got = _with_keys(q, k, v, do, o_dev, 0.125, [i for i in range(N) if i != j])
    _assert_caught(ref, got, f"key {j} dropped")


@pytest.mark.parametrize("B,H,N", [(1, 2, 97), (1, 2, 129), (1, 1, 4097)])
def test_tail_block_counted_twice_is_caught(B, H, N):
    """The first 32-key block of the tail tile (keys 64 t .. 64 t + 31, fewer at the end) summed twice."""
    t0 = (N - 1) // 64 * 64
    q, k, v, do, o_dev, ref = _case(B, H, N)
    got = _with_keys(q, k, v, do, o_dev, 0.125, range(N), extra=range(t0, min(t0 + 32, N)))
    _assert_caught(ref, got, f"keys {t0}.. counted twice")


@pytest.mark.parametrize("src", ["row", "head"])
@pytest.mark.parametrize("n", [0, 64, 127])
def test_row_from_the_wrong_place_is_caught(n, src):
    """One query row of o and dq taken from row n + 1 of the same head, or from the same row of head h + 1."""
    B, H, N = 1, 2, 129
    *_, ref = _case(B, H, N)
    got = {}
    for name in ("o", "dq"):
        t = ref[name].clone()
        t[0, 0, n] = ref[name][0, 0, n + 1] if src == "row" else ref[name][0, 1, n]
        got[name] = t
    _assert_caught(ref, got, f"row {n} from the {src} next to it")


@pytest.mark.parametrize("B,H,N", [(1, 1, 200), (1, 1, 513), (1, 1, 4097)])
def test_skipped_rescale_is_caught(B, H, N):
    """The running-max rescale skipped for one row at the tile where its spike key (k[j] = 6 q[i], section 3e of the GPU tests)
    makes the max jump."""
    q, k, v, _ = _operands(B, H, N, seed=N + 9)
    placed = plant_spikes(q, k, [N - 1])
    i, j = placed[0]
    ref = attn_ref(q, k, v, 0.125)
    o, lse = online_softmax_emulated(q, k, v, 0.125, skip_rescale=(0, 0, i, j // 64))
    _assert_caught(ref, {"o": o.double(), "lse": lse}, f"rescale skipped at row {i}, tile {j // 64}")


@pytest.mark.parametrize("B,H,N", DEFECT_SHAPES)
@pytest.mark.parametrize("row", [0, 64, -1])
def test_query_missing_from_dkdv_is_caught(B, H, N, row):
    """One query row left out of the dK / dV sums over the queries."""
    i = row % N
    q, k, v, do, o_dev, ref = _case(B, H, N)
    keep = torch.tensor([n for n in range(N) if n != i])
    r = attn_ref(q[:, :, keep], k, v, 0.125, o_dev=o_dev[:, :, keep], dO=do[:, :, keep])
    _assert_caught(ref, {"dk": r["dk"], "dv": r["dv"]}, f"query {i} missing from dK/dV")


@pytest.mark.parametrize("B,H,N", DEFECT_SHAPES)
def test_lse_without_its_last_key_is_caught(B, H, N):
    """One row's lse summed without the last key (the row whose last-key probability is largest: where the defect shows most)."""
    q, k, v, do, o_dev, ref = _case(B, H, N)
    P_last = torch.exp((q[0, 0].double() @ k[0, 0, -1].double()) * 0.125 - ref["lse"][0, 0])
    i = int(P_last.argmax())
    short = attn_ref(q[:, :, i:i + 1], k[:, :, :-1], v[:, :, :-1], 0.125)["lse"]
    lse = ref["lse"].clone()
    lse[:, :, i] = short[:, :, 0]
    _assert_caught(ref, {"lse": lse.float()}, f"lse of row {i} without key {N - 1}")
