"""GPU: xvit_augment_apply_elastic and xvit_elastic_draw (csrc/elastic.hip) against the float64 restatement and the gate of
tests/_elastic_check.py: every destination element, nothing excluded.  tests/test_elastic_gate_cpu.py shows on the same cases that the
gate rejects a wrong kernel.

Cases (K.SHAPES; B = 3, M = 2, flags (1, 0, 1), hand-written fields and tables): "lx3" (14, 23, 37) -> (12, 20, 40) on 7^3 control points, a
W tail; "lx4" (8, 12, 64) -> (6, 10, 72) on the single cell (4, 4, 4); "lx2" (11, 9, 20) -> (9, 7, 24) on (16, 5, 4), odd H and D;
"thin" (6, 3, 12) -> (5, 1, 9) on (4, 4, 16): an axis of length 1 and runs that cross several control cells.  Flag-0 samples carry NaN in
their field on the device, so that a read of it shows.  The worst error-to-bound ratios are printed and recorded under XVIT_MEASURE_LOG
(profiles/elastic_measured.txt)."""
import numpy as np
import pytest
import torch

import _augment_check as A
import _elastic_check as K
from _util import dev, note

pytestmark = pytest.mark.gpu

TORCH_DT = {"i16": torch.int16, "bf16": torch.bfloat16, "f32": torch.float32}
OUT_NAME = {torch.bfloat16: "bf16", torch.float32: "f32"}
SHAPE_IDS = tuple(K.SHAPES)
GUARD = 4096      # sentinel elements behind the destination and the field


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def as64(out):
    return out.float().cpu().double().numpy().reshape((-1,) + tuple(out.shape[-3:]))


def gpu_src(src, dt):
    s = torch.from_numpy(src).float().reshape((K.B, K.M) + src.shape[1:])
    return s.to(TORCH_DT[dt]).to(dev())


def gpu_tables(table, field, erec, nan_inactive=True):
    """The tables on the device; the field of every flag-0 sample filled with NaN."""
    f = torch.from_numpy(field).clone()
    if nan_inactive:
        f[torch.from_numpy(erec[:, K.FLAG] == 0)] = float("nan")
    nb = field.shape[0]
    return torch.from_numpy(table).reshape(nb, -1, A.NPARAM).to(dev()), f.to(dev()), torch.from_numpy(erec).to(dev())


def run(src_gpu, table, field, erec, d, out_dtype, pad=K.PAD):
    from xvit import ops
    out = ops.augment_apply_elastic(src_gpu, table, field, erec, d, pad, out_dtype)
    assert out.shape == src_gpu.shape[:2] + (1,) + tuple(d) and out.dtype == out_dtype and out.is_contiguous()
    return out


def run_case(shape, kind, m, src_dt, out_dtype):
    src, table, field, erec, (ref, R, exact, deformed, cell) = K.case(shape, kind, m)
    out = run(gpu_src(src, src_dt), *gpu_tables(table, field, erec), K.SHAPES[shape][1], out_dtype)
    name = f"elastic_{shape}_{kind}_m{m:g}_{src_dt}_{OUT_NAME[out_dtype]}"
    ratio = note(name, K.check(name, as64(out), ref, R, exact, deformed, cell, table, OUT_NAME[out_dtype]))
    need = note(name + ":c_needed_over_c", K.MEASURED["c_needed"] / K.C_ELASTIC)
    print(f"{name}: worst error / bound {ratio:.4f}; the smallest c that passes is {need:.4f} of C_ELASTIC")
    return out


# ---------------------------------------------------------------------------------------------------------------- against apply_ref
@pytest.mark.parametrize("m", [3.0, 12.0], ids=["m3", "m12"])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_random_field_against_float64(shape, out_dtype, m):
    run_case(shape, "plain", m, "i16", out_dtype)


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("src_dt", ["i16", "bf16", "f32"])
def test_all_six_dtype_pairs(src_dt, out_dtype):
    run_case("lx3", "plain", 3.0, src_dt, out_dtype)


@pytest.mark.parametrize("kind", ["clamp", "noise"])
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_clamp_window_and_noise(shape, kind):
    run_case(shape, kind, 3.0, "i16", torch.float32)
    run_case(shape, kind, 3.0, "bf16", torch.bfloat16)


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_partition_of_unity(shape):
    """A constant field (dz, dy, dx) is plain apply with t + A d, under the gate: the reference here is _augment_check.apply_ref itself."""
    s, d, grid = K.SHAPES[shape]
    src, table = K.source(s), K.tables(s, d)
    disp = np.array([1.25, -2.5, 0.75])
    field = np.broadcast_to(disp.astype(np.float32)[None, :, None, None, None], (K.B, 3) + grid).copy()
    erec = np.zeros((K.B, K.NREC), dtype=np.float32)
    erec[:, K.FLAG] = 1.0
    moved = table.copy().astype(np.float64)
    for v in range(K.NVOL):
        At = moved[v, :12].reshape(3, 4)
        At[:, 3] += At[:, :3] @ disp
    ref, _, _ = A.apply_ref(src, moved, d, K.PAD)                        # float64 rows: t + A d is not rounded to fp32
    _, R, exact, deformed, cell = K.apply_ref(src, table, field, erec, K.M, d, K.PAD)
    assert deformed.all()
    out = run(gpu_src(src, "i16"), *gpu_tables(table, field, erec), d, torch.float32)
    ratio = note(f"elastic_unity_{shape}", K.check(f"unity {shape}", as64(out), ref, R, exact, deformed, cell, table, "f32"))
    print(f"partition of unity {shape}: worst error / bound {ratio:.4f}")


# ---------------------------------------------------------------------------------------------------------------- bit for bit
def _plain(src_gpu, table, d, out_dtype):
    from xvit import ops
    return ops.augment_apply(src_gpu, table, d, K.PAD, out_dtype)


@pytest.mark.parametrize("kind", ["plain", "clamp", "noise"])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_zero_field_with_flag_1_is_augment_apply(shape, out_dtype, kind):
    s, d, grid = K.SHAPES[shape]
    src = gpu_src(K.source(s), "i16")
    table = torch.from_numpy(K.tables(s, d, kind)).reshape(K.B, K.M, A.NPARAM).to(dev())
    field = torch.zeros((K.B, 3) + grid, device=dev())
    erec = torch.zeros(K.B, K.NREC, device=dev())
    erec[:, K.FLAG] = 1.0
    assert torch.equal(bits(run(src, table, field, erec, d, out_dtype)), bits(_plain(src, table, d, out_dtype)))


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_zero_field_with_flag_1_on_exact_records(shape):
    """Records carrying FLAG_EXACT (flips and integer shifts): the general path at integral coordinates has weights 0 and 1."""
    s, d, grid = K.SHAPES[shape]
    src = gpu_src(K.source(s), "i16")
    mats = []
    for v, (flips, shift) in enumerate([((0, 0, 0), (0, 0, 0)), ((1, 0, 0), (1, -2, 3)), ((0, 1, 0), (0, 0, -5)), ((0, 0, 1), (-1, 0, 0)),
                                        ((1, 1, 1), (2, 1, 1)), ((0, 1, 1), (0, 0, 0))]):
        m = A.compose(flips, (0, 0, 0), (1, 1, 1), shift, s, d)
        assert np.array_equal(m, np.rint(m))
        mats.append(m)
    t = A.table_from(K.NVOL, np.stack(mats), a=np.array([1.0, 0.9, -0.5, 2.0, 1.0, 0.7]), b=np.array([0.0, -0.2, 10.0, 0.0, 1.5, -4.0]), exact=True)
    table = torch.from_numpy(t).reshape(K.B, K.M, A.NPARAM).to(dev())
    field = torch.zeros((K.B, 3) + grid, device=dev())
    erec = torch.zeros(K.B, K.NREC, device=dev())
    erec[:, K.FLAG] = torch.tensor(K.FLAGS_ON)
    field[1] = float("nan")
    for out_dtype in (torch.bfloat16, torch.float32):
        assert torch.equal(bits(run(src, table, field, erec, d, out_dtype)), bits(_plain(src, table, d, out_dtype)))


@pytest.mark.parametrize("kind", ["plain", "noise"])
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_flag_0_samples_are_augment_apply_and_their_field_is_not_read(shape, kind):
    src, table, field, erec, _ = K.case(shape, kind, 3.0)
    d = K.SHAPES[shape][1]
    g = gpu_src(src, "bf16")
    t, f, e = gpu_tables(table, field, erec)
    assert torch.isnan(f[1]).all() and not torch.isnan(f[0]).any()
    for out_dtype in (torch.bfloat16, torch.float32):
        out, want = run(g, t, f, e, d, out_dtype), _plain(g, t, d, out_dtype)
        assert torch.equal(bits(out[1]), bits(want[1])) and not torch.equal(bits(out[0]), bits(want[0]))
        assert torch.isfinite(out.float()).all()
    e0 = torch.zeros_like(e)                                       # every flag 0, every field NaN: the whole call is xvit_augment_apply
    out = run(g, t, torch.full_like(f, float("nan")), e0, d, torch.bfloat16)
    assert torch.equal(bits(out), bits(_plain(g, t, d, torch.bfloat16)))


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_two_runs_are_identical_and_sentinels_stay(shape):
    from xvit import _lib, ops
    src, table, field, erec, _ = K.case(shape, "noise", 12.0)
    s, d, grid = K.SHAPES[shape]
    g = gpu_src(src, "i16")
    t, f, e = gpu_tables(table, field, erec)
    first = run(g, t, f, e, d, torch.bfloat16)
    assert torch.equal(bits(first), bits(run(g, t, f, e, d, torch.bfloat16)))
    # the entry point itself, into a destination and from a field with sentinels behind them
    n_out, n_f = K.NVOL * d[0] * d[1] * d[2], f.numel()
    dst = torch.full((n_out + GUARD,), -12345.0, dtype=torch.bfloat16, device=dev())
    fbuf = torch.full((n_f + GUARD,), 777.0, dtype=torch.float32, device=dev())
    fbuf[:n_f] = f.reshape(-1)
    rc = _lib.load().xvit_augment_apply_elastic(g.data_ptr(), ops.I16, dst.data_ptr(), ops.BF16, t.data_ptr(), fbuf.data_ptr(), e.data_ptr(), K.NVOL, K.M, *grid,
                                                *s, *d, K.PAD, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(dst[:n_out]), bits(first).reshape(-1)) and bool((dst[n_out:] == -12345.0).all()) and bool((fbuf[n_f:] == 777.0).all())
    assert torch.equal(bits(fbuf[:n_f]), bits(f.reshape(-1)))       # NaN included: the field is read only


# ---------------------------------------------------------------------------------------------------------------- draw
def _draw(cfg, nb, grid, seed, counter=None, advance=False, guard=False):
    from xvit import _lib, ops
    c = _lib.ElasticConfig()
    c.prob, c.locked_borders = float(cfg["prob"]), cfg["locked_borders"]
    c.max_displacement[:] = [float(v) for v in cfg["max_displacement"]]
    n_f = nb * 3 * grid[0] * grid[1] * grid[2]
    fbuf = torch.full((n_f + GUARD,), 777.0, dtype=torch.float32, device=dev())
    ebuf = torch.full((nb * K.NREC + GUARD,), 777.0, dtype=torch.float32, device=dev())
    field, erec = fbuf[:n_f].view((nb, 3) + tuple(grid)), ebuf[:nb * K.NREC].view(nb, K.NREC)
    ops.elastic_draw(c, field, erec, seed, counter, advance)
    torch.cuda.synchronize()
    assert bool((fbuf[n_f:] == 777.0).all()) and bool((ebuf[nb * K.NREC:] == 777.0).all())
    return field.cpu().numpy(), erec.cpu().numpy()


def _same(got, want):
    for g, w, what in zip(got, want, ("field", "record")):
        assert g.shape == w.shape and g.dtype == w.dtype == np.float32
        bad = np.nonzero(g.view(np.uint32) != w.view(np.uint32))
        assert bad[0].size == 0, f"{what}: {bad[0].size} slots differ, first at {tuple(int(i[0]) for i in bad)}: {g[tuple(i[0] for i in bad)]!r} != {w[tuple(i[0] for i in bad)]!r}"


@pytest.mark.parametrize("L", [0, 1, 2, 3])
@pytest.mark.parametrize("grid", [(4, 4, 4), (7, 7, 7), (16, 5, 4), (16, 16, 16)], ids=str)
def test_draw_slot_for_slot(grid, L):
    cfg = K.config(prob=0.6, max_displacement=(3.0, 7.5, 0.37), locked_borders=L)
    _same(_draw(cfg, 5, grid, seed=1234 + L), K.field_ref(cfg, 5, grid, seed=1234 + L))


@pytest.mark.parametrize("prob", [0.0, 1.0])
def test_draw_prob_0_and_1(prob):
    cfg = K.config(prob=prob, max_displacement=2.0, locked_borders=1)
    field, erec = _draw(cfg, 7, (6, 5, 7), seed=9)
    _same((field, erec), K.field_ref(cfg, 7, (6, 5, 7), seed=9))
    assert (erec[:, K.FLAG] == prob).all() and (np.abs(field).max() > 0) == (prob == 1.0)
    assert bool((erec[:, K.MAX_ABS:K.MAX_ABS + 3] <= 2.0).all())


def test_draw_counter_and_advance():
    cfg = K.config(prob=0.5, max_displacement=4.0, locked_borders=2)
    grid, seed = (7, 6, 8), 0xFEDCBA9876543210
    counter = torch.tensor([3], dtype=torch.int64, device=dev())
    _same(_draw(cfg, 4, grid, seed, counter, advance=False), K.field_ref(cfg, 4, grid, seed, call=3))
    assert int(counter.item()) == 3
    _same(_draw(cfg, 4, grid, seed, counter, advance=True), K.field_ref(cfg, 4, grid, seed, call=3))
    assert int(counter.item()) == 4                                  # advance leaves the counter at + 1
    _same(_draw(cfg, 4, grid, seed, counter, advance=True), K.field_ref(cfg, 4, grid, seed, call=4))
    assert int(counter.item()) == 5
    _same(_draw(cfg, 4, grid, seed), K.field_ref(cfg, 4, grid, seed, call=0))          # without a counter
    a, b = K.field_ref(cfg, 4, grid, seed, call=3), K.field_ref(cfg, 4, grid, seed, call=4)
    assert not np.array_equal(a[0], b[0])


def test_drawn_field_through_the_apply():
    """Draw and apply together, on the drawn tables read back: the reference takes the device's field, which the draw tests hold to equality."""
    s, d, grid = K.SHAPES["lx3"]
    cfg = K.config(prob=0.7, max_displacement=(1.0, 1.5, 2.5), locked_borders=2)
    field, erec = K.field_ref(cfg, K.B, grid, seed=21)
    assert 0 < erec[:, K.FLAG].sum() < K.B
    got = _draw(cfg, K.B, grid, seed=21)
    _same(got, (field, erec))
    src, table = K.source(s), K.tables(s, d)
    ref, R, exact, deformed, cell = K.apply_ref(src, table, field, erec, K.M, d, K.PAD)
    out = run(gpu_src(src, "i16"), *gpu_tables(table, field, erec, nan_inactive=False), d, torch.float32)
    ratio = note("elastic_drawn_lx3", K.check("drawn field", as64(out), ref, R, exact, deformed, cell, table, "f32"))
    print(f"drawn field: worst error / bound {ratio:.4f}")
