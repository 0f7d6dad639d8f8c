"""The element-wise GEMM check (tests/_gemm_check.py) has teeth, on the CPU.

For a few cases of tests/test_gemm_small_gpu.py the destinations are built as a faultless kernel would leave them (_gemm_check.ideal)
and pass the check.  Then one fault at a time is planted, each a mistake the 128x128 kernel or the split-K reduce could make: the
check must fail and name the 128x128 tile, the wave's 64x64 sub-tile and the 16x16 fragment of the fault -- and, where the fault is
small against the whole tensor, the rel-L2 gate of _util.assert_close (all that tests/test_gemm_gpu.py asks) must let it through."""
import re

import pytest
import torch

import _gemm_check as G
from _util import assert_close

# the example of a local fault: bf16 output, K = 3072 (48 K-steps)
DEEP = G.Spec("nt-deep", "NT", 2052, 768, 3072, tile=128, force=True)
OUT_PROJ_DROP = G.Spec("out-proj-drop", "NT", 1026, 768, 768, f32=True, bias=True, res=True, drop=True, tile=128)
REMAP = G.Spec("patch-embed-remap", "NT", 3 * 16, 192, 128, f32=True, bias=True, res=True, res_mod=16, res_off=1, seg=(16, 1, 1), tile=128)
GELU = G.Spec("ffn1", "NT", 513, 768, 768, bias=True, act="gelu", aux_mode=1, ldc_pad=8, ldaux_pad=4, tile=128)
DGELU = G.Spec("ffn2-dgrad", "NN", 130, 192, 768, act="dgelu", aux_mode=0, colsum=True, split=3, tile=128, force=True)
# a contraction long enough for sums of 11 and more significant bits (std 1000 units): what a second rounding needs to show
LONG = G.Spec("tn-long", "TN", 200, 136, 64638, tile=128, force=True)
BATCHED = G.Spec("lowrank-S", "TN", 16, 192, 130, f32=True, batch=3, accumulate="again", tile=128)


def _cpu_mask(spec, seed=3):
    if not spec.drop:
        return None
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2, spec.bt + (spec.M, spec.N), generator=g).float() * 2.0


_CACHE = {}


def _case(spec):
    """(reference, ideal destinations): the reference is computed once per case, the destinations are fresh copies."""
    if spec not in _CACHE:
        R = G.reference(spec, _cpu_mask(spec))
        _CACHE[spec] = (R, G.ideal(spec, R))
    R, out = _CACHE[spec]
    return R, {k: v.clone() for k, v in out.items()}


def _where(r, c):
    """The coordinates the check must name for output element (r, c) of the 128x128 kernel."""
    return (f"(row {r}, col {c}): 128x128 tile ({r // 128}, {c // 128}), wave sub-tile ({(r % 128) // 64}, {(c % 128) // 64}), "
            f"16x16 fragment ({(r % 64) // 16}, {(c % 64) // 16})")


def _fails_at(spec, R, out, r, c):
    with pytest.raises(AssertionError, match=re.escape(_where(r, c))):
        G.compare(spec, R, out)


def _old_gate_passes(spec, R, out):
    """What tests/test_gemm_gpu.py asks of the same output: one rel-L2 number per tensor."""
    assert_close(out["C"][..., spec.out_rows(), :spec.N], G.stored(spec, R), spec.name)


@pytest.mark.parametrize("spec", [DEEP, LONG, OUT_PROJ_DROP, REMAP, GELU, DGELU, BATCHED], ids=lambda s: s.name)
def test_faultless_output_passes(spec):
    R, out = _case(spec)
    G.compare(spec, R, out)


def test_one_wrong_element():
    """One element one bf16 ulp off, in the last ragged row tile."""
    R, out = _case(DEEP)
    r, c = 2050, 701
    bits = out["C"].view(torch.int16)
    bits[r, c] += 1
    _fails_at(DEEP, R, out, r, c)
    _old_gate_passes(DEEP, R, out)


def test_one_fragment_misses_one_k_step():
    """The example of the issue: one 16x16 fragment without one 64-deep K-step of 48 (each element ~14 % off, the tensor's rel-L2 1.8e-3)."""
    R, out = _case(DEEP)
    r0, c0, k0 = 1168, 464, 1984
    part = R["a"][r0:r0 + 16, k0:k0 + 64] @ R["b"][c0:c0 + 16, k0:k0 + 64].T
    frag = (R["acc"][r0:r0 + 16, c0:c0 + 16] - part).to(torch.bfloat16)
    wrong = frag != out["C"][r0:r0 + 16, c0:c0 + 16]
    assert int(wrong.sum()) > 200
    out["C"][r0:r0 + 16, c0:c0 + 16] = frag
    first = wrong.nonzero()[0].tolist()
    _fails_at(DEEP, R, out, r0 + first[0], c0 + first[1])
    with pytest.raises(AssertionError, match=r"^nt-deep .*: (\d+) of 1575936 elements wrong"):
        G.compare(DEEP, R, out)
    _old_gate_passes(DEEP, R, out)


def test_one_residual_row_from_its_neighbour():
    """Row 16 (the first row of the second segment) takes the position row of row 15 instead of wrapping to the first."""
    R, out = _case(REMAP)
    s = REMAP
    r = 16
    wrong = R["v"][r] - R["res"][s.res_off + r % s.res_mod] + R["res"][s.res_off + (r - 1) % s.res_mod]
    c = int((wrong != R["v"][r]).nonzero()[0])
    out["C"][int(s.out_rows()[r])] = wrong
    _fails_at(s, R, out, r, c)


def test_one_dropout_decision_flipped():
    R, out = _case(OUT_PROJ_DROP)
    s = OUT_PROJ_DROP
    r = 700
    zr = R["acc"][r] + R["bias"]
    c = int(torch.where(zr == 0, torch.inf, zr.abs()).argmin())      # the flip that moves the norm least: 2 |z| on one element
    z = zr[c]
    out["C"][r, c] = (0.0 if R["mask"][r, c] else 2.0 * z) + R["res"][r, c]
    _fails_at(s, R, out, r, c)
    _old_gate_passes(s, R, out)


def _round_to_9_bits(x):
    """fp32 -> nearest-even at one bit more than bf16 keeps (an intermediate rounding a kernel could slip in before the bf16 store)."""
    b = x.contiguous().view(torch.int32)
    b = (b + 0x3FFF + ((b >> 15) & 1)) & ~0x7FFF
    return b.view(torch.float32)


def test_one_value_rounded_twice():
    """fp32 -> 9 significant bits -> bf16 differs from fp32 -> bf16 where the first rounding lands on a tie (that takes a sum of at
    least 11 significant bits)."""
    R, out = _case(LONG)
    twice = _round_to_9_bits(R["v"]).to(torch.bfloat16)
    diff = (twice != R["v"].to(torch.bfloat16)).nonzero()
    assert len(diff), "no element of this case shows the double rounding"
    r, c = diff[len(diff) // 2].tolist()
    out["C"][r, c] = twice[r, c]
    _fails_at(LONG, R, out, r, c)
    _old_gate_passes(LONG, R, out)


def test_a_sentinel_row_of_a_remapped_output_overwritten():
    """The CLS row of the second sample (destination row 17) is written although no GEMM row maps to it."""
    R, out = _case(REMAP)
    out["C"][17, 40:44] = 0.0
    with pytest.raises(AssertionError, match=re.escape("4 elements outside the output were overwritten (a row outside the output's row map); first at destination (row 17, col 40)")):
        G.compare(REMAP, R, out)
    _old_gate_passes(REMAP, R, out)      # the old test never looks there


def test_padding_columns_of_a_strided_destination_overwritten():
    R, out = _case(GELU)
    out["C"][5, GELU.N + 1] = 0.0
    with pytest.raises(AssertionError, match=re.escape("ffn1 NT 513x768x768 split 1: C: 1 elements outside the output were overwritten (columns >= N); first at destination (row 5, col 769)")):
        G.compare(GELU, R, out)
    R, out = _case(GELU)
    out["aux"][GELU.M, 3] = 1.0          # the row behind the last one
    with pytest.raises(AssertionError, match="aux: 1 elements outside the output"):
        G.compare(GELU, R, out)


def test_activation_error_beyond_the_tolerance():
    """GELU one bf16 ulp and a half off; the saved derivative of one element taken from its neighbour; an unwritten element."""
    R, out = _case(GELU)
    r = 300
    c = int(R["v"][r].abs().argmax())
    ref = float(R["v"][r, c])
    out["C"][r, c] = ref + 2.5 * float(G.bf16_ulp(R["v"][r, c]))
    _fails_at(GELU, R, out, r, c)
    R, out = _case(GELU)
    out["aux"][r, c] = float("nan")
    _fails_at(GELU, R, out, r, c)


def test_colsum_misses_one_row_or_the_start_value():
    R, out = _case(DGELU)
    pre = G.colsum_pre(DGELU, R).double()
    c = int(pre[7].abs().argmax())
    out["cs"][c] -= float(pre[7, c])
    with pytest.raises(AssertionError, match=rf"colsum: 1 of 192 elements wrong; first at \(col {c}\): 128x128 tile column {c // 128}"):
        G.compare(DGELU, R, out)
    R, out = _case(DGELU)
    out["cs"] -= G.COLSUM_START
    with pytest.raises(AssertionError, match="colsum: 192 of 192"):
        G.compare(DGELU, R, out)


def test_batch_and_accumulate_faults_are_named():
    """The second batch's result written over the third's; accumulate that overwrites instead of adding."""
    R, out = _case(BATCHED)
    out["C"][2] = out["C"][1]
    with pytest.raises(AssertionError, match=r"first at batch 2, \(row 0, col \d+\): 128x128 tile \(0, 0\)"):
        G.compare(BATCHED, R, out)
    R, out = _case(BATCHED)
    out["C2"] = out["C"].clone()
    with pytest.raises(AssertionError, match="accumulate"):
        G.compare(BATCHED, R, out)


def test_256_coordinates_are_unchanged():
    """The production test's messages (256x256 tile, 128x64 wave sub-tile) stay as they were."""
    from _util import gemm_coords
    assert gemm_coords((600, 520), 300 * 520 + 270) == "(row 300, col 270): 256x256 tile (1, 1), wave sub-tile (0, 0), 16x16 fragment (2, 0)"
    assert gemm_coords((600, 520), 300 * 520 + 270, tile=128) == "(row 300, col 270): " + _where(300, 270).split(": ", 1)[1]
    assert gemm_coords((2, 600, 520), 600 * 520 + 5).startswith("batch 1, (row 0, col 5): 256x256 tile (0, 0)")
