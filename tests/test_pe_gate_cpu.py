"""The element-wise check of the fused patch embedding (tests/_pe_check.py) has teeth, on the CPU.

For a few cases of tests/test_patch_embed_edges_gpu.py the destinations are built as a faultless kernel would leave them (_pe_check.ideal)
and pass the check.  Then one fault at a time is planted, each a mistake the gather paths of csrc/gemm.hip could make: the check must
fail and name the place.  The last test pins the classes the case table reaches, by the Python restatement of the host logic, so that
a later edit of the table cannot silently drop a branch."""
import re

import pytest
import torch

import _pe_check as P
from _util import gemm_coords

RAGGED = P.BY_NAME["m3-9tok-M1"]          # mode 3, K % 64 = 53, rows % 256 = 2
PAIRS = P.BY_NAME["dn32-pairs"]           # mode 2, nw = 2
UNEVEN = P.BY_NAME["dn8-uneven"]          # mode 2, nw = 8, rows % 256 = 97
EMPTY = P.BY_NAME["m3-1tok-empty"]        # splits with nk = 0, -4, -9


def _case(case):
    """(reference, fresh ideal destinations)."""
    ref = P.reference(case)
    return ref, P.ideal(case, ref)


def _fails_at(case, ref, out, shape, r, c, what):
    """compare fails on `what` (x | dW) and names element (r, c) as the first wrong one."""
    where = gemm_coords(shape, r * shape[1] + c)
    with pytest.raises(AssertionError, match=re.escape(f"{case.tag}: {what}: ") + r"\d+ of \d+ elements wrong; first at " + re.escape(where)):
        P.compare(case, ref, out)


def _first_diff(a, b):
    return (a != b).nonzero()[0].tolist()


@pytest.mark.parametrize("case", [RAGGED, PAIRS, UNEVEN, EMPTY, P.BY_NAME["m3-cls0"]], ids=lambda c: c.name)
def test_faultless_output_passes(case):
    ref, out = _case(case)
    P.compare(case, ref, out)
    for bias, pos in ((False, False), (True, False), (False, True)):
        P.compare(case, ref, {"x": P.ideal(case, ref, bias, pos)["x"]}, bias, pos)
    with pytest.raises(AssertionError, match="x: .* elements wrong"):          # and the variants differ from one another
        P.compare(case, ref, {"x": out["x"]}, True, False)


def test_ragged_last_k_step_left_out_of_dw():
    """Mode 3: the 53 tokens of the last, partial K-step never reach dW."""
    c = RAGGED
    ref, out = _case(c)
    k0 = c.K // 64 * 64
    assert c.K - k0 == 53
    wrong = ref["dW"] - ref["dxp"][k0:].T @ ref["patches"][k0:]
    r, col = _first_diff(wrong, ref["dW"])
    assert int((wrong != ref["dW"]).sum()) > c.d * c.pd // 2
    P.dw_body(c, out["dW"])[:c.d, :c.pd] = wrong
    _fails_at(c, ref, out, (c.d, c.pd), r, col, "dW")


def test_one_samples_dx_rows_shifted_onto_its_cls_row():
    """The dx rows of sample 3 are read from its CLS row on (not skipped): the CLS row's NaN reaches every element of dW."""
    c = PAIRS
    ref, out = _case(c)
    s = 3
    pt = ref["patches"][s * c.P:(s + 1) * c.P]
    shifted = ref["dx"][s * c.ntok:s * c.ntok + c.P]
    assert torch.isnan(shifted[0]).all() and torch.equal(shifted[1:], ref["dxp"][s * c.P:(s + 1) * c.P - 1])
    P.dw_body(c, out["dW"])[:c.d, :c.pd] = ref["dW"] - ref["dxp"][s * c.P:(s + 1) * c.P].T @ pt + shifted.T @ pt
    _fails_at(c, ref, out, (c.d, c.pd), 0, 0, "dW")


def test_empty_splits_slab_left_unwritten():
    """A split without K-steps returns without storing its zero slab: the workspace's NaN prefill is summed into dW."""
    c = EMPTY
    assert [n for n in P.split_steps(c) if n <= 0] == [0, -4, -9]
    ref, out = _case(c)
    slab = torch.full((c.d, c.pd), P.NAN)
    P.dw_body(c, out["dW"])[:c.d, :c.pd] = ref["dW"] + slab
    _fails_at(c, ref, out, (c.d, c.pd), 0, 0, "dW")


@pytest.mark.parametrize("case", [PAIRS, UNEVEN], ids=lambda c: c.name)
def test_pairing_applied_to_the_volume_only(case):
    """Mode 2: in one 64-token group the volume's k-rows are in the paired order (gather_krow_token), those of dx are not."""
    c = case
    ref, out = _case(c)
    perm = torch.tensor([P.krow_token(c, kr) for kr in range(64)])
    assert sorted(perm.tolist()) == list(range(64)) and perm.tolist() != list(range(64))
    k0 = 5 * 64
    dxg, pg = ref["dxp"][k0:k0 + 64], ref["patches"][k0:k0 + 64]
    wrong = ref["dW"] - dxg.T @ pg + dxg.T @ pg[perm]
    r, col = _first_diff(wrong, ref["dW"])
    P.dw_body(c, out["dW"])[:c.d, :c.pd] = wrong
    _fails_at(c, ref, out, (c.d, c.pd), r, col, "dW")


def test_two_rows_of_one_dma_group_swapped_in_the_last_row_tile():
    """Forward: tile rows 2 and 10 of the ragged last row tile (LDS rows 8 and 9, the first two of wave 0's second DMA instruction:
    init_gather_rows) come out in each other's place."""
    c = UNEVEN
    ref, out = _case(c)
    m0 = c.rows // 256 * 256
    r1, r2 = m0 + 2, m0 + 10
    assert r2 < c.rows and r1 % c.ntok >= c.cls and r2 % c.ntok >= c.cls
    x = P.x_body(c, out["x"])
    want = P.x_ref(c, ref)
    x[r1, :c.d], x[r2, :c.d] = want[r2], want[r1]
    col = _first_diff(want[r2], want[r1])[0]
    _fails_at(c, ref, out, (c.rows, c.d), r1, col, "x")


def test_cls_row_that_received_a_patch():
    """The CLS row of sample 2 holds the sample's first patch (times W) instead of bias + pos[0] alone."""
    c = UNEVEN
    ref, out = _case(c)
    r = 2 * c.ntok
    want = P.x_ref(c, ref)
    assert torch.equal(want[r], ref["bias"] + ref["pos"][0])
    wrong = want[r] + ref["acc"][2 * c.P]
    P.x_body(c, out["x"])[r, :c.d] = wrong
    _fails_at(c, ref, out, (c.rows, c.d), r, _first_diff(wrong, want[r])[0], "x")


def test_element_written_in_a_padding_column_of_x():
    c = RAGGED
    ref, out = _case(c)
    P.x_body(c, out["x"])[700, c.d + 1] = 0.0
    with pytest.raises(AssertionError, match=re.escape(f"{c.tag}: x: 1 elements outside the output were overwritten (padding columns); first at destination (row 700, col {c.d + 1})")):
        P.compare(c, ref, out)
    ref, out = _case(c)
    P.x_body(c, out["x"])[c.rows, 3] = 0.0            # the row behind the last one
    with pytest.raises(AssertionError, match=re.escape(f"(padding rows); first at destination (row {c.rows}, col 3)")):
        P.compare(c, ref, out)


def test_margin_behind_dw_changed():
    c = RAGGED
    ref, out = _case(c)
    out["dW"][-P.MARGIN + 17] = 0.0
    with pytest.raises(AssertionError, match=re.escape(f"{c.tag}: dW: 1 elements outside the output were overwritten (the margin behind); first at element 17 behind the buffer's end")):
        P.compare(c, ref, out)
    ref, out = _case(c)
    out["ws"][P.MARGIN - 1] = 0.0                     # the element in front of the workspace
    with pytest.raises(AssertionError, match=re.escape("workspace: 1 elements outside the output were overwritten (the margin in front); first at element -1 of the output")):
        P.compare(c, ref, out)


def test_unwritten_element_is_found():
    """An output element the kernel never stores keeps its NaN prefill and fails."""
    c = RAGGED
    ref, _ = _case(c)
    out = P.ideal(c, ref)
    P.x_body(c, out["x"])[c.rows - 1, c.d - 1] = P.NAN
    _fails_at(c, ref, out, (c.rows, c.d), c.rows - 1, c.d - 1, "x")


def test_restatement_counts_k_steps_as_c_does():
    assert P.k_per_split(8256, 16) == 576 and P.k_per_split(1845, 4) == 512 and P.k_per_split(64, 4) == 64
    assert P.split_steps(P.BY_NAME["m2-empty-split"]) == [9] * 14 + [3, -5]        # (8256 - 8640 + 63) / 64 truncates to -5
    assert P.split_steps(EMPTY) == [5] * 13 + [0, -4, -9]
    assert P.split_steps(UNEVEN) == [9, 9, 9, 6]
    assert P.split_steps(RAGGED) == [8, 8, 8, 5]


def test_case_table_reaches_every_class():
    """Every case is one the fused kernels take, and the table holds every class of the gather paths' branches."""
    assert len({c.name for c in P.CASES}) == len(P.CASES)
    for c in P.CASES:
        assert P.supported(c), c.name
        assert P.wgrad_split(c) > 1, f"{c.name}: the slab-free path is out of this check's reach (its reference would be too large)"
        assert c.B * c.M * c.vol[0] * c.vol[1] * c.vol[2] <= 2.2e6 and c.K <= 8256, f"{c.name}: too large for a quick test / the exactness argument"
    K = {c.name: P.classify(c) for c in P.CASES}
    m2 = [k for k in K.values() if k["mode"] == 2]
    m3 = [k for k in K.values() if k["mode"] == 3]

    def some(ks, pred):
        return any(pred(k) for k in ks)

    # mode 2: gather_krow_token's identity branch and every pairing, gather_soff_wgrad's h / w steps
    assert {k["nw"] for k in m2} >= {1, 2, 4, 8, 16, 32, 64}
    assert some(m2, lambda k: k["grid"][0] == 1) and some(m2, lambda k: k["grid"][2] == 1)
    assert some(m2, lambda k: k["grid"][1] > 1 and k["wsteps"] == 2) and some(m2, lambda k: k["grid"][1] == 3)
    assert some(m2, lambda k: len(set(k["steps"])) > 1 and min(k["steps"]) > 0), "mode 2 with uneven splits"
    assert some(m2, lambda k: min(k["steps"]) < 0), "mode 2 with a split behind K"
    assert some(m2, lambda k: k["cls"] == 0)
    # mode 3: fast_div by 1, K-steps over several samples and modalities, P around 64, K % 64
    assert some(m3, lambda k: set(k["div1"]) == {"Dn", "Wn", "pcount"})
    assert some(m3, lambda k: k["div1"] == ("Dn",)) and some(m3, lambda k: k["div1"] == ("Wn",))
    assert some(m3, lambda k: k["P"] <= 9 and k["modalities"] == 1) and some(m3, lambda k: k["P"] <= 9 and k["modalities"] > 1)
    assert {63, 65, 1} <= {k["P"] for k in m3} and some(m3, lambda k: k["P"] < 64)
    assert some(m3, lambda k: k["k_mod_64"] == 0 and k["P"] > 64) and some(m3, lambda k: k["k_mod_64"] % 64 not in (0, 32))
    assert some(m3, lambda k: k["grid"][0] > 64)
    assert some(m3, lambda k: 0 in k["steps"]) and some(m3, lambda k: min(k["steps"]) < 0), "mode 3 with an empty split and one behind K"
    assert some(m3, lambda k: k["cls"] == 0)
    assert {k["P"] + k["cls"] for k in m3} >= {1, 2, 3}, "pos tables of 1, 2 and 3 rows: shorter than the epilogue's 4-row step"
    # both: row tiles of the forward, output tiles of dW, run lengths
    allk = list(K.values())
    assert some(allk, lambda k: k["rows_mod_256"] == 0) and some(allk, lambda k: k["rows_mod_256"] not in (0, 128))
    assert {k["wp"] for k in allk} >= {8, 16, 32, 64}
    assert some(allk, lambda k: k["tiles"] == (3, 4)) and some(m3, lambda k: k["tiles"][0] == 3)
    assert some(allk, lambda k: k["fwd_ksteps"] == 16)
