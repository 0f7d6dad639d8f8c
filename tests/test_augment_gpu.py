"""GPU: the augmenting input stage (csrc/augment.hip, xvit/augment.py) element by element against the float64 restatement of
tests/_augment_check.py.  Every destination element is compared; exact-path volumes must be EQUAL to the reference.

Shapes (source -> destination): (9, 10, 11) -> (8, 8, 16) crop and pad mixed per axis, one full 16-byte run; (4, 20, 16) -> (8, 8, 16)
pad, crop and equal; (7, 6, 5) -> (5, 6, 7) scalar tail only, odd everything; (20, 20, 20) -> (16, 16, 24) run plus tail;
(40, 40, 40) -> (32, 32, 32) several bricks per volume; B = 2, M = 2, and B = 3, M = 1 for an odd volume count.

Noise and draw gates: K.NOISE_GATE, K.MATRIX_GATE, K.OFFSET_GATE of tests/_augment_check.py.  They are to be 8 x the first MI355X
measurement; until such a run exists they are the format-derived bounds written out there (NOT measured).  The tests print what they measure
and record it under XVIT_MEASURE_LOG."""
import functools

import numpy as np
import pytest
import torch

import _augment_check as K
from _util import dev, note

pytestmark = pytest.mark.gpu

SHAPES = [((9, 10, 11), (8, 8, 16)), ((4, 20, 16), (8, 8, 16)), ((7, 6, 5), (5, 6, 7)), ((20, 20, 20), (16, 16, 24)), ((40, 40, 40), (32, 32, 32))]
CASES = [(2, 2, s, d) for s, d in SHAPES] + [(3, 1, (20, 20, 20), (16, 16, 24))]
IDS = ["%dx%d-%s-%s" % (b, m, "x".join(map(str, s)), "x".join(map(str, d))) for b, m, s, d in CASES]
PAD = -1.0
OFF = dict(flip_prob=(0, 0, 0), rotate_prob=0, zoom_prob=0, translate_prob=0, scale_intensity_prob=0, shift_intensity_prob=0, noise_prob=0)
TORCH_DT = {"i16": torch.int16, "bf16": torch.bfloat16, "f32": torch.float32}


@functools.lru_cache(maxsize=None)
def source(B, M, shape, seed=0):
    """Uniform in [-1000, 3000], on the bf16 grid (integers there), so that ONE tensor is exact as int16, bf16 and fp32: float32 CPU."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-1000, 3001, (B, M) + tuple(shape), generator=g).float()
    return v.to(torch.bfloat16).float()


def on_gpu(src, dt):
    return src.to(TORCH_DT[dt]).to(dev())


def general_matrices(kind, s, d):
    """Four hand-written transforms, one per volume."""
    if kind == "rotations":       # about each axis, and combined
        draws = [((0, 0, 0), (0.3, 0, 0), (1, 1, 1), (0, 0, 0)), ((0, 0, 0), (0, -0.25, 0), (1, 1, 1), (0, 0, 0)),
                 ((0, 0, 0), (0, 0, 0.35), (1, 1, 1), (0, 0, 0)), ((1, 0, 1), (0.2, -0.15, 0.1), (1, 1, 1), (0, 0, 0))]
    else:                         # zoom 0.8 and 1.25, a fractional translation, half of the volume pushed out of the source
        draws = [((0, 0, 0), (0, 0, 0), (0.8, 0.8, 0.8), (0, 0, 0)), ((0, 0, 0), (0, 0, 0), (1.25, 1.25, 1.25), (0, 0, 0)),
                 ((0, 0, 0), (0, 0, 0), (1, 1, 1), (0.37, -1.62, 2.5)), ((0, 0, 0), (0.1, 0, 0), (1, 1, 1), (0.5 * s[0], 0.25, -0.5 * s[2]))]
    return np.stack([K.compose(*dr, s, d) for dr in draws])


@functools.lru_cache(maxsize=None)
def general_case(kind, s, d, intensity=False):
    """(source fp32 CPU [2, 2, ...], table fp32 [4, 32], ref, R, exact) — computed once, shared by every dtype combination."""
    src = source(2, 2, s)
    a, b = (np.array([1.1, 0.9, -0.5, 2.0]), np.array([0.3, -0.2, 10.0, 0.0])) if intensity else (1.0, 0.0)
    table = K.table_from(4, general_matrices(kind, s, d), a=a, b=b)
    return (src, table) + K.apply_ref(src.reshape((4,) + s).numpy(), table, d, PAD)


def run_apply(src_gpu, table, d, out_dtype):
    from xvit.augment import VolumeAugment
    B, M = src_gpu.shape[:2]
    aug = VolumeAugment(d, pad_value=PAD, out_dtype=out_dtype)
    out = aug.apply(src_gpu, torch.from_numpy(table).reshape(B, M, K.NPARAM).to(dev()))
    assert out.shape == (B, M, 1) + tuple(d) and out.dtype == out_dtype and out.is_contiguous()
    return out


def as64(out):
    return out.float().cpu().double().numpy().reshape((-1,) + tuple(out.shape[3:]))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------- exact path
@pytest.mark.parametrize("B,M,s,d", CASES, ids=IDS)
def test_identity_is_resize_pad_crop_bit_for_bit(B, M, s, d):
    from xvit import ops
    from xvit.augment import VolumeAugment
    src = on_gpu(source(B, M, s), "i16")
    aug = VolumeAugment(d, pad_value=PAD, **OFF)
    out = aug(src)
    want = ops.resize_pad_crop_i16(src, d, PAD)
    assert out.dtype == torch.bfloat16 and out.shape == want.shape and torch.equal(bits(out), bits(want))
    assert bool(aug.last_params.exact.all())
    assert torch.equal(bits(aug(src.unsqueeze(2))), bits(want))            # [B, M, 1, Ds, Hs, Ws] is accepted too


@pytest.mark.parametrize("axes", [(0,), (1,), (2,), (0, 1, 2)], ids=["z", "y", "x", "zyx"])
@pytest.mark.parametrize("B,M,s,d", CASES, ids=IDS)
def test_flips_are_torch_flip_of_the_identity(B, M, s, d, axes):
    from xvit import ops
    from xvit.augment import VolumeAugment
    src = on_gpu(source(B, M, s), "i16")
    kw = dict(OFF, flip_prob=tuple(1.0 if i in axes else 0.0 for i in range(3)))
    aug = VolumeAugment(d, pad_value=PAD, **kw)
    out = aug(src)
    want = torch.flip(ops.resize_pad_crop_i16(src, d, PAD), dims=[3 + i for i in axes])
    assert torch.equal(bits(out), bits(want))
    p = aug.last_params
    assert bool(p.exact.all()) and p.flips.cpu().tolist() == [[[1.0 if i in axes else 0.0 for i in range(3)]] * M] * B


@pytest.mark.parametrize("shift", [(2, -3, 5), (-1, 0, -9), (0, 7, 1)], ids=str)
@pytest.mark.parametrize("B,M,s,d", CASES, ids=IDS)
def test_integer_translation_is_the_shifted_identity(B, M, s, d, shift):
    from xvit import ops
    src_cpu = source(B, M, s)
    src = on_gpu(src_cpu, "i16")
    m = K.identity_matrix(s, d)
    m[:, 3] += shift
    table = K.table_from(B * M, m, exact=True)
    out = run_apply(src, table, d, torch.bfloat16)
    ref, R, exact = K.apply_ref(src_cpu.reshape((B * M,) + s).numpy(), table, d, PAD)
    assert exact.all() and K.check("translation", as64(out), ref, R, exact, table, "bf16") == 0.0
    # ... which is the identity output moved by `shift` wherever the shifted index stays inside the destination
    ident = ops.resize_pad_crop_i16(src, d, PAD)
    lo = [max(0, -sh) for sh in shift]
    hi = [min(n, n - sh) for n, sh in zip(d, shift)]
    if all(h > l for l, h in zip(lo, hi)):
        a = out[..., lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        b = ident[..., lo[0] + shift[0]:hi[0] + shift[0], lo[1] + shift[1]:hi[1] + shift[1], lo[2] + shift[2]:hi[2] + shift[2]]
        assert torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------- general path
@pytest.mark.parametrize("dst_dt", ["bf16", "f32"])
@pytest.mark.parametrize("src_dt", ["i16", "bf16", "f32"])
@pytest.mark.parametrize("kind", ["rotations", "zoom_translate"])
@pytest.mark.parametrize("s,d", SHAPES, ids=IDS[:5])
def test_general_path_against_float64(s, d, kind, src_dt, dst_dt):
    src, table, ref, R, exact = general_case(kind, s, d)
    assert not exact.any()
    out = run_apply(on_gpu(src, src_dt), table, d, TORCH_DT[dst_dt])
    note(f"augment:general:{kind}:{src_dt}:{dst_dt}:ratio", K.check(f"general {kind}", as64(out), ref, R, exact, table, dst_dt))


def test_general_path_odd_volume_count():
    s, d = (20, 20, 20), (16, 16, 24)
    src = source(3, 1, s, seed=1)
    table = K.table_from(3, general_matrices("rotations", s, d)[[3, 0, 2]])
    ref, R, exact = K.apply_ref(src.reshape((3,) + s).numpy(), table, d, PAD)
    K.check("general 3x1", as64(run_apply(on_gpu(src, "i16"), table, d, torch.bfloat16)), ref, R, exact, table, "bf16")


@pytest.mark.parametrize("dst_dt", ["bf16", "f32"])
@pytest.mark.parametrize("path", ["exact", "general"])
def test_intensity_differs_per_volume(path, dst_dt):
    s, d = (20, 20, 20), (16, 16, 24)
    if path == "general":
        src, table, ref, R, exact = general_case("rotations", s, d, True)
    else:
        src = source(2, 2, s)
        table = K.table_from(4, K.identity_matrix(s, d), a=np.array([1.1, 0.9, -0.5, 2.0]), b=np.array([0.3, -0.2, 10.0, 0.0]), exact=True)
        ref, R, exact = K.apply_ref(src.reshape((4,) + s).numpy(), table, d, PAD)
        assert exact.all()
    out = run_apply(on_gpu(src, "i16"), table, d, TORCH_DT[dst_dt])
    K.check(f"intensity {path}", as64(out), ref, R, exact, table, dst_dt)


# ---------------------------------------------------------------------------------------------------------------- noise
NOISE_SEEDS = np.array([12345, 7, 99, 2 ** 32 - 5], dtype=np.uint32)
NOISE_SIGMA = np.array([0.5, 0.0, 0.0625, 2.0])      # powers of two: out / sigma is exact, what is left is the fp32 Box-Muller


def test_noise_field_against_the_restatement():
    """A zero source with a = 1, b = 0 and an fp32 destination: out = sigma n, so out / sigma IS the kernel's noise field.  Gate: K.NOISE_GATE
    (tests/_augment_check.py: a derived 2^-18 until the first MI355X measurement replaces it by 8 x the measured value; never above 1e-3).
    Not yet measured on a GPU."""
    s = d = (32, 32, 32)
    n = 32 ** 3
    src = torch.zeros(2, 2, *s, dtype=torch.float32, device=dev())
    table = K.table_from(4, K.identity_matrix(s, d), sigma=NOISE_SIGMA, noise_seed=NOISE_SEEDS, exact=True)
    out = as64(run_apply(src, table, d, torch.float32)).reshape(4, n)
    quiet = K.table_from(4, K.identity_matrix(s, d), noise_seed=NOISE_SEEDS, exact=True)
    base = as64(run_apply(src, quiet, d, torch.float32)).reshape(4, n)
    assert (base == 0).all() and (out[1] == 0).all()                      # sigma = 0: bit-equal to the no-noise output
    worst = 0.0
    for v in (0, 2, 3):
        ref = K.normal_field(int(NOISE_SEEDS[v]), n)
        assert abs(ref.mean()) <= 5 / np.sqrt(n) and abs(ref.std() - 1) <= 5 / np.sqrt(2 * n), "the restatement's own field"
        got = (out[v] - base[v]) / NOISE_SIGMA[v]
        assert np.isfinite(got).all()
        worst = max(worst, float(np.abs(got - ref).max()))
        assert abs(got.mean()) <= 5 / np.sqrt(n) and abs(got.std() - 1) <= 5 / np.sqrt(2 * n), f"volume {v}: mean {got.mean():.4g}, std {got.std():.4g}"
    print(f"augment noise: max |got - ref| / sigma = {worst:.4e}")
    note("augment:noise:max_err_over_sigma", worst)
    assert worst <= K.NOISE_GATE, f"noise field off the float64 Box-Muller by {worst:.3e} > {K.NOISE_GATE:.3e}"


@pytest.mark.parametrize("dst_dt", ["bf16", "f32"])
def test_noise_on_top_of_a_resample(dst_dt):
    """Noise on the general and the exact path, voxel indices with a tail (W = 24): the gate with its noise allowance."""
    s, d = (20, 20, 20), (16, 16, 24)
    src = source(2, 2, s)
    m = general_matrices("rotations", s, d)
    m[1], m[2] = K.identity_matrix(s, d), K.identity_matrix(s, d)
    table = K.table_from(4, m, a=0.001, b=0.1, sigma=np.array([0.05, 0.02, 0.0, 0.1]), noise_seed=NOISE_SEEDS, exact=np.array([False, True, True, False]))
    ref, R, exact = K.apply_ref(src.reshape((4,) + s).numpy(), table, d, PAD)
    K.check("noise on a resample", as64(run_apply(on_gpu(src, "i16"), table, d, TORCH_DT[dst_dt])), ref, R, exact, table, dst_dt)


# ---------------------------------------------------------------------------------------------------------------- draw
ALL_ON = dict(flip_prob=(1, 1, 1), rotate_prob=1, zoom_prob=1, translate_prob=1, scale_intensity_prob=1, shift_intensity_prob=1, noise_prob=1)


def test_draw_with_every_probability_one_stays_inside_its_ranges():
    from xvit.augment import VolumeAugment
    s, d = (20, 20, 20), (16, 16, 24)
    aug = VolumeAugment(d, rotate_range=(0.26, 0.1, 0.4), zoom_range=(0.9, 1.1), translate_range=(8, 2, 0.5), scale_intensity_range=(0.9, 1.1),
                        shift_intensity_range=(-0.1, 0.2), noise_std=0.05, intensity_scale=0.001, intensity_shift=0.5, **ALL_ON)
    aug(on_gpu(source(4, 2, s), "i16"))
    p = aug.last_params
    t = p.table.cpu()
    assert not bool(p.exact.any()) and bool((p.flips == 1).all())
    for k, r in enumerate((0.26, 0.1, 0.4)):
        assert bool((t[..., K.ANGLES + k].abs() <= np.float32(r)).all())
    assert bool(((t[..., K.ZOOMS:K.ZOOMS + 3] >= np.float32(0.9)) & (t[..., K.ZOOMS:K.ZOOMS + 3] <= np.float32(1.1))).all())
    for k, r in enumerate((8, 2, 0.5)):
        assert bool((t[..., K.TRANSLATION + k].abs() <= r).all())
    fac = t[..., K.SCALE].double() / float(np.float32(0.001))
    assert bool(((fac >= 0.9 - 1e-6) & (fac <= 1.1 + 1e-6)).all())
    shift = t[..., K.SHIFT].double() - fac * 0.5
    assert bool(((shift >= -0.1 - 1e-6) & (shift <= 0.2 + 1e-6)).all())
    assert bool(((t[..., K.SIGMA] > 0) & (t[..., K.SIGMA] <= np.float32(0.05))).all())
    assert bool((t[..., 29:] == 0).all())
    # one spatial transform per sample, shared by its modalities and different between samples; intensity per volume
    sp = t[..., list(range(0, 12)) + list(range(K.FLIPS, 29))]
    assert torch.equal(sp[:, 0], sp[:, 1])
    for i in range(4):
        for j in range(i + 1, 4):
            assert not torch.equal(t[i, 0, K.ANGLES:29], t[j, 0, K.ANGLES:29])
    for k in (K.SCALE, K.SHIFT, K.SIGMA):
        assert bool((t[:, 0, k] != t[:, 1, k]).all())
    assert len(set(p.noise_seed.cpu().reshape(-1).tolist())) == 8


def test_draw_with_every_probability_zero_is_the_pure_pad_crop_record():
    from xvit.augment import AugmentParams, VolumeAugment
    for B, M, s, d in CASES:
        aug = VolumeAugment(d, **OFF)
        aug(on_gpu(source(B, M, s), "i16"))
        got, want = aug.last_params.table.cpu().clone(), AugmentParams.identity(B, M, s, d).table
        got[..., K.NOISE_SEED] = 0
        assert torch.equal(got, want), (s, d)


def test_drawn_matrix_is_the_float64_composition_of_the_recorded_draws():
    """The kernel composes in double from the fp32 draws and rounds once.  Gates: K.MATRIX_GATE on the linear part (never above 1e-4) and
    K.OFFSET_GATE relative on the offsets (tests/_augment_check.py: derived 2^-23 each until the first MI355X measurement replaces them by
    8 x the measured values).  Not yet measured on a GPU."""
    from xvit.augment import VolumeAugment
    worst_a = worst_t = 0.0
    for (s, d), seed in zip(SHAPES, range(5)):
        aug = VolumeAugment(d, seed=seed, flip_prob=(0.5, 0.5, 0.5), rotate_prob=0.7, zoom_prob=0.7, translate_prob=0.7)
        for _ in range(2):
            aug(on_gpu(source(2, 2, s), "i16"))
            t = aug.last_params.table.cpu().double().numpy().reshape(4, K.NPARAM)
            for row in t:
                m64 = K.compose(row[K.FLIPS:K.FLIPS + 3], row[K.ANGLES:K.ANGLES + 3], row[K.ZOOMS:K.ZOOMS + 3], row[K.TRANSLATION:K.TRANSLATION + 3], s, d)
                got = row[:12].reshape(3, 4)
                worst_a = max(worst_a, float(np.abs(got[:, :3] - m64[:, :3]).max()))
                worst_t = max(worst_t, float((np.abs(got[:, 3] - m64[:, 3]) / np.maximum(1.0, np.abs(m64[:, 3]))).max()))
                is_exact = bool(np.all(got[:, :3] == np.diag(np.sign(np.diag(got[:, :3])))) and np.all(got[:, 3] == np.rint(got[:, 3])))
                assert bool(int(row[K.FLAGS]) & 1) == is_exact
    print(f"augment draw: max |A - A64| = {worst_a:.4e}, max rel |t - t64| = {worst_t:.4e}")
    note("augment:draw:matrix_abs", worst_a)
    note("augment:draw:offset_rel", worst_t)
    assert worst_a <= K.MATRIX_GATE <= 1e-4 and worst_t <= K.OFFSET_GATE


def test_same_seed_and_call_index_reproduce_table_and_output():
    from xvit.augment import VolumeAugment
    s, d = (20, 20, 20), (16, 16, 24)
    src = on_gpu(source(2, 2, s), "i16")

    def calls(aug, n):
        """(table copy, output) of n successive calls (a capturable stage reuses one table: hence the copy)."""
        res = []
        for _ in range(n):
            out = aug(src)
            res.append((aug.last_params.table.clone(), out))
        return res

    a, b, c = VolumeAugment(d, seed=5), VolumeAugment(d, seed=5), VolumeAugment(d, seed=5, capturable=True)
    (ta0, oa0), (ta1, oa1) = calls(a, 2)
    (tb0, ob0), = calls(b, 1)
    assert torch.equal(bits(ta0), bits(tb0)) and torch.equal(bits(oa0), bits(ob0))
    assert not torch.equal(bits(ta0), bits(ta1)) and not torch.equal(bits(oa0), bits(oa1))
    assert a.call_index == 2 and b.call_index == 1
    # the capturable stage keeps its call index on the device and draws the same numbers
    (tc0, oc0), (tc1, oc1) = calls(c, 2)
    assert torch.equal(bits(tc0), bits(ta0)) and torch.equal(bits(tc1), bits(ta1)) and torch.equal(bits(oc0), bits(oa0)) and torch.equal(bits(oc1), bits(oa1))
    assert c.call_index == 2
    assert not torch.equal(bits(VolumeAugment(d, seed=6)(src)), bits(oa0))


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_under_the_gate_with_its_own_table():
    from xvit.augment import VolumeAugment
    s, d = (40, 40, 40), (32, 32, 32)
    src = source(2, 2, s)
    aug = VolumeAugment(d, pad_value=PAD, noise_prob=0.5, intensity_scale=0.001, seed=3)
    for dt in ("i16", "f32"):
        out = aug(on_gpu(src, dt))
        table = aug.last_params.table.cpu().numpy().reshape(4, K.NPARAM)
        ref, R, exact = K.apply_ref(src.reshape((4,) + s).numpy(), table, d, PAD)
        K.check("end to end", as64(out), ref, R, exact, table, "bf16")
    aug.eval()
    out = aug(on_gpu(src, "i16"))
    assert bool(aug.last_params.exact.all()) and aug.call_index == 2
    table = aug.last_params.table.cpu().numpy().reshape(4, K.NPARAM)
    assert np.all(table[:, K.SCALE] == np.float32(0.001)) and np.all(table[:, K.SIGMA] == 0)
    ref, R, exact = K.apply_ref(src.reshape((4,) + s).numpy(), table, d, PAD)
    assert K.check("eval", as64(out), ref, R, exact, table, "bf16") == 0.0


def test_eval_is_the_identity_and_the_output_feeds_model_cross():
    import ref_cpu as Rf
    import xvit
    from xvit import ops
    cfg = Rf.make_config("tiny")
    d = tuple(cfg.img_size)                                   # (32, 32, 2)
    s = (36, 30, 3)
    src = on_gpu(source(4, cfg.num_modalities, s), "i16")
    aug = xvit.VolumeAugment(d, pad_value=PAD, translate_range=(3, 3, 0.5), intensity_scale=0.001, seed=1)
    img = aug(src)
    assert img.shape == (4, cfg.num_modalities, 1) + d and bool(torch.isfinite(img.float()).all())
    model = xvit.ModelCross(cfg).to(dev())
    model.load_state_dict(Rf.make_state_dict(cfg, seed=0))
    model.train()
    labels = torch.tensor([0, 1, 1, 0], device=dev())
    logits, loss = model(img, labels)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    plain = xvit.VolumeAugment(d, pad_value=PAD).eval()
    assert torch.equal(bits(plain(src)), bits(ops.resize_pad_crop_i16(src, d, PAD))) and plain.call_index == 0


# ---------------------------------------------------------------------------------------------------------------- capture
def test_capturable_stage_draws_anew_at_every_replay():
    from xvit.augment import VolumeAugment
    s, d = (20, 20, 20), (16, 16, 24)
    src_cpu = source(2, 2, s)
    static = on_gpu(src_cpu, "i16")
    aug = VolumeAugment(d, pad_value=PAD, noise_prob=0.5, seed=11, capturable=True)
    aug(static)                                                # allocates the table and the counter; call index 0 -> 1
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = aug(static)
    assert aug.call_index == 1, "a capture executes nothing"
    tables = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        table = aug.last_params.table.cpu().numpy().reshape(4, K.NPARAM).copy()
        ref, R, exact = K.apply_ref(src_cpu.reshape((4,) + s).numpy(), table, d, PAD)
        K.check("replay", as64(out), ref, R, exact, table, "bf16")
        tables.append(table)
    assert not np.array_equal(tables[0], tables[1])
    assert aug.call_index == 3
    # the replays drew what a plain stage draws at call indices 1 and 2
    plain = VolumeAugment(d, pad_value=PAD, noise_prob=0.5, seed=11)
    plain(static)
    for want in tables:
        plain(static)
        assert np.array_equal(plain.last_params.table.cpu().numpy().reshape(4, K.NPARAM).view(np.uint32), want.view(np.uint32))
