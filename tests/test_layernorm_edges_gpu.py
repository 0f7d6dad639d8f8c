"""GPU: LayerNorm forward / backward (csrc/layernorm.hip) and xvit_colsum (csrc/misc.hip) element by element against float64, under the
gate of tests/_ln_check.py: every width either side of a 64-lane boundary and of each template instance, every row count where a grid
or a row loop changes shape (the production call included), the contents where a variance goes wrong, and every option of the C entry
points that the wrappers of xvit.ops never pass (row strides, x_alt forms, NULL outputs, prefilled sums, the workspace form).

Outputs are prefilled with NaN, padding and a guard row included; the backward is fed float32(mu_ref), float32(rs_ref)."""
import math

import pytest
import torch

import _ln_check as L
from _util import dev, rt

pytestmark = pytest.mark.gpu

EPS = L.f32(1e-5)
COLS = ("dgamma", "dbeta", "dxsum", "dressum")


def _lib():
    from xvit import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _err():
    return _lib().xvit_last_error_string().decode(errors="replace")


def _strided(t, ld, dtype=None):
    """Device copy of the CPU [rows, d] tensor with row stride ld; the padding is NaN, so a kernel that reads it shows."""
    rows, d = t.shape
    buf = torch.full((rows, ld), math.nan, dtype=dtype or t.dtype, device=dev())
    buf[:, :d] = t.to(dev())
    return buf


def _alt(x_alt, seq_len, ldx, packed):
    """x_alt on the device in its packed form ([sequences, d], ld_alt = d) or as row k * seq_len of a tensor laid out like x
    (ld_alt = seq_len * ldx; every other row NaN).  -> (tensor, ld_alt)"""
    if x_alt is None:
        return None, 0
    n, d = x_alt.shape
    if packed:
        return x_alt.to(dev()).contiguous(), d
    full = torch.full((n * seq_len, ldx), math.nan, dtype=torch.float32, device=dev())
    full[::seq_len, :d] = x_alt.to(dev())
    return full, seq_len * ldx


def _case(rows, d, seed, kind="usual", seq_len=0):
    x = L.content(kind, rows, d, seed=seed)
    g, b = L.affine(d, seed=seed + 1)
    gen = torch.Generator().manual_seed(seed + 2)
    dy, dres = rt(torch.randn(rows, d, generator=gen)), torch.randn(rows, d, generator=gen)
    x_alt = L.content(kind, -(-rows // seq_len), d, seed=seed + 3) if seq_len else None
    return x, g, b, dy, dres, x_alt


def _prefill(d, seed):
    gen = torch.Generator().manual_seed(seed)
    return {n: torch.randn(d, generator=gen) for n in COLS}


def raw_fwd(x, g, b, eps, *, x_alt=None, seq_len=0, packed=True, ldx=None, ldy=None, ldyf=None, want_f32=True, want_bf16=True, log=None):
    """xvit_layernorm_fwd through the C ABI into NaN-prefilled strided outputs, checked against float64.  -> ln_ref's dict"""
    rows, d = x.shape
    ldx, ldy, ldyf = ldx or d, ldy or d, ldyf or d
    xd = _strided(x, ldx)
    alt, ld_alt = _alt(x_alt, seq_len, ldx, packed)
    gd, bd = g.to(dev()), b.to(dev())
    yb = L.nan_buffer(rows, ldy, torch.bfloat16, dev()) if want_bf16 else None
    yf = L.nan_buffer(rows, ldyf, torch.float32, dev()) if want_f32 else None
    mean, rstd = (torch.full((rows + 1,), math.nan, device=dev()) for _ in range(2))
    rc = _lib().xvit_layernorm_fwd(_p(xd), _p(alt), ldx, seq_len, ld_alt, _p(gd), _p(bd), eps, _p(yb), ldy, _p(yf), ldyf, _p(mean), _p(rstd), rows, d, _stream())
    assert rc == 0, f"xvit_layernorm_fwd rc = {rc}: {_err()}"
    torch.cuda.synchronize()
    ref = L.ln_ref(x, x_alt, seq_len, g, b, eps)
    L.check_fwd(ref, d, rows, mean[:rows], rstd[:rows], None if yf is None else yf[:rows, :d], None if yb is None else yb[:rows, :d],
                seq_len=seq_len if x_alt is not None else 0, log=log)
    assert math.isnan(float(mean[rows])) and math.isnan(float(rstd[rows])), "mean / rstd written behind the last row"
    if yf is not None:
        L.check_padding("y_f32", yf, rows, d)
    if yb is not None:
        L.check_padding("y_bf16", yb, rows, d)
    return ref


def raw_bwd(x, g, dy, ref_f, *, dres=None, x_alt=None, seq_len=0, packed=True, want_bf16=True, dxsum=True, dressum=True, prefill=None, workspace=False,
            ldx=None, lddy=None, lddres=None, lddx=None, lddxb=None, log=None):
    """xvit_layernorm_bwd through the C ABI, fed float32(mu_ref) / float32(rs_ref), into NaN-prefilled strided dx / dx_bf16 and
    prefilled sums, checked against float64.  workspace: the deterministic form, called twice and compared bit for bit."""
    rows, d = x.shape
    ldx, lddy, lddres, lddx, lddxb = ldx or d, lddy or d, lddres or d, lddx or d, lddxb or d
    xd, dyd = _strided(x, ldx), _strided(dy, lddy, torch.bfloat16)
    dresd = _strided(dres, lddres) if dres is not None else None
    alt, ld_alt = _alt(x_alt, seq_len, ldx, packed)
    mu32, rs32 = ref_f["mu"].float(), ref_f["rs"].float()
    mud, rsd, gd = mu32.to(dev()), rs32.to(dev()), g.to(dev())
    names = ["dgamma", "dbeta"] + (["dxsum"] if dxsum else []) + (["dressum"] if dressum else [])
    pre = prefill if prefill is not None else {n: torch.zeros(d) for n in COLS}
    ws_bytes = _lib().xvit_layernorm_bwd_workspace_bytes(rows, d) if workspace else 0
    assert ws_bytes == (L.ln_bwd_grid(rows) * 4 * d * 4 if workspace else 0)
    runs = []
    for _ in range(2 if workspace else 1):
        ws = torch.full((ws_bytes // 4,), math.nan, device=dev()) if workspace else None
        dx = L.nan_buffer(rows, lddx, torch.float32, dev())
        dxb = L.nan_buffer(rows, lddxb, torch.bfloat16, dev()) if want_bf16 else None
        cols = {n: pre[n].to(dev()).clone() for n in names}
        rc = _lib().xvit_layernorm_bwd(_p(dyd), lddy, _p(xd), _p(alt), ldx, seq_len, ld_alt, _p(mud), _p(rsd), _p(gd), _p(dresd), lddres if dres is not None else 0,
                                       _p(dx), lddx, _p(dxb), lddxb, _p(cols["dgamma"]), _p(cols["dbeta"]), _p(cols.get("dxsum")), _p(cols.get("dressum")),
                                       rows, d, _p(ws), ws_bytes, _stream())
        assert rc == 0, f"xvit_layernorm_bwd rc = {rc}: {_err()}"
        torch.cuda.synchronize()
        runs.append((dx, dxb, cols))
    dx, dxb, cols = runs[0]
    ref = L.ln_bwd_ref(dy, ref_f["rows"], mu32, rs32, g, dres)
    sl = seq_len if x_alt is not None else 0
    L.check_dx(ref, d, rows, dx[:rows, :d], None if dxb is None else dxb[:rows, :d], seq_len=sl, log=log)
    L.check_cols(ref, d, rows, cols, pre, log=log)
    L.check_padding("dx", dx, rows, d)
    if dxb is not None:
        L.check_padding("dx_bf16", dxb, rows, d)
    if workspace:
        dx2, dxb2, cols2 = runs[1]
        same = lambda a, b: torch.equal(a[:rows, :d], b[:rows, :d])   # noqa: E731
        assert same(dx, dx2) and (dxb is None or same(dxb, dxb2)), "workspace form: dx differs between two calls"
        for n in names:
            assert torch.equal(cols[n], cols2[n]), f"workspace form: {n} differs between two calls"
    return ref


# ------------------------------------------------------------------------------------------------------------------ widths
@pytest.mark.parametrize("d", L.WIDTHS)
def test_widths_forward(d):
    """Every width through its template instance (V = 3: d <= 768, V = 4: d <= 1024, V = 16 above); 67 rows = 8 blocks and 3 rows."""
    x, g, b, *_ = _case(67, d, seed=d)
    raw_fwd(x, g, b, EPS, log=f"ln:width{d}")
    raw_fwd(x, g, b, EPS, want_f32=False)
    raw_fwd(x, g, b, EPS, want_bf16=False)


@pytest.mark.parametrize("workspace", [False, True], ids=["atomic", "workspace"])
@pytest.mark.parametrize("d", L.WIDTHS)
def test_widths_backward(d, workspace):
    """67 rows = 5 blocks of 4 waves: rows 0 .. 59 in pairs (d <= 1024), rows 60 .. 66 a third trip on 7 of the 20 waves.  d > 2048
    asks for more than 64 KiB of dynamic LDS (32 d bytes)."""
    x, g, b, dy, dres, _ = _case(67, d, seed=d)
    ref_f = L.ln_ref(x, None, 0, g, b, EPS)
    raw_bwd(x, g, dy, ref_f, dres=dres, prefill=_prefill(d, d), workspace=workspace, log=f"ln:width{d}:{'ws' if workspace else 'atomic'}")


# ------------------------------------------------------------------------------------------------------------------ row counts
ROW_COUNTS = [(r, 768) for r in (1, 7, 8, 9, 15, 16, 17, 31, 33, 12288, 12289, 16384, 16393)] + [(33, 1024), (12289, 1024)]


def _ops_fwd_bwd(x, g, b, dy, dres, eps, log, content_kind=None):
    """Forward (fp32 + bf16, and bf16 only) and backward through xvit.ops, against float64."""
    from xvit import ops
    rows, d = x.shape
    xd, gd, bd = x.to(dev()), g.to(dev()), b.to(dev())
    ref = L.ln_ref(x, None, 0, g, b, eps)
    yf, yb, mean, rstd = ops.layernorm_fwd_f32(xd, gd, bd, eps)
    L.check_fwd(ref, d, rows, mean, rstd, yf, yb, log=log)
    yb2, mean2, rstd2 = ops.layernorm_fwd(xd, gd, bd, eps)
    L.check_fwd(ref, d, rows, mean2, rstd2, None, yb2)
    assert torch.equal(yb2, yb) and torch.equal(mean2, mean) and torch.equal(rstd2, rstd)
    mu32, rs32 = ref["mu"].float(), ref["rs"].float()
    pre = _prefill(d, rows + d)
    cols = {n: pre[n].to(dev()).clone() for n in COLS}
    dx, dxb = ops.layernorm_bwd(dy.to(dev(), torch.bfloat16), xd, mu32.to(dev()), rs32.to(dev()), gd, cols["dgamma"], cols["dbeta"], dres=dres.to(dev()),
                                want_bf16=True, dxsum=cols["dxsum"], dressum=cols["dressum"])
    rb = L.ln_bwd_ref(dy, ref["rows"], mu32, rs32, g, dres)
    L.check_dx(rb, d, rows, dx, dxb, log=log)
    L.check_cols(rb, d, rows, cols, pre, log=log)


@pytest.mark.parametrize("rows,d", ROW_COUNTS)
def test_row_counts(rows, d):
    """Forward: a block of 8 waves either side of full, and the grid-stride loop past 2048 x 8 rows.  Backward: 16 rows per block, the
    second row of a pair present or not, and the grid at its cap of 768 (12 288 rows) and one row past it."""
    x, g, b, dy, dres, _ = _case(rows, d, seed=rows)
    _ops_fwd_bwd(x, g, b, dy, dres, EPS, f"ln:rows{rows}x{d}")


def test_production_rows():
    """126 x 513 = 64 638 rows of 768: the forward's grid-stride loop runs four times, the backward's two-rows-in-flight loop eleven
    times with a one-row tail on some waves.  The float64 reference is built in slabs of 8 sequences."""
    from xvit import ops
    rows, d, seq = 126 * 513, 768, 513
    x, g, b, dy, dres, x_alt = _case(rows, d, seed=5, seq_len=seq)
    xd, gd, bd, altd = x.to(dev()), g.to(dev()), b.to(dev()), x_alt.to(dev())
    yb, mean, rstd = ops.layernorm_fwd(xd, gd, bd, EPS, x_alt=altd, seq_len=seq)
    yf, yb2, mean2, rstd2 = ops.layernorm_fwd_f32(xd, gd, bd, EPS)          # no x_alt: the sequence heads are checked against x here
    pre = _prefill(d, 11)
    cols = {n: pre[n].to(dev()).clone() for n in COLS}
    slab = 8 * seq
    mu32, rs32 = torch.empty(rows), torch.empty(rows)
    for r0 in range(0, rows, slab):
        r1 = min(rows, r0 + slab)
        ref = L.ln_ref(x[r0:r1], x_alt[r0 // seq:], seq, g, b, EPS)
        L.check_fwd(ref, d, rows, mean[r0:r1], rstd[r0:r1], None, yb[r0:r1], row0=r0, seq_len=seq, log="ln:production")
        mu32[r0:r1], rs32[r0:r1] = ref["mu"].float(), ref["rs"].float()
        ref = L.ln_ref(x[r0:r1], None, 0, g, b, EPS)
        L.check_fwd(ref, d, rows, mean2[r0:r1], rstd2[r0:r1], yf[r0:r1], yb2[r0:r1], row0=r0, log="ln:production")
    del yf, yb, yb2
    dx, dxb = ops.layernorm_bwd(dy.to(dev(), torch.bfloat16), xd, mu32.to(dev()), rs32.to(dev()), gd, cols["dgamma"], cols["dbeta"], x_alt=altd, seq_len=seq,
                                dres=dres.to(dev()), want_bf16=True, dxsum=cols["dxsum"], dressum=cols["dressum"])
    total = None
    for r0 in range(0, rows, slab):
        r1 = min(rows, r0 + slab)
        rr = L.rows_read(x[r0:r1], x_alt[r0 // seq:], seq)
        ref = L.ln_bwd_ref(dy[r0:r1], rr, mu32[r0:r1], rs32[r0:r1], g, dres[r0:r1])
        L.check_dx(ref, d, rows, dx[r0:r1], dxb[r0:r1], row0=r0, seq_len=seq, log="ln:production")
        part = {k: v for k, v in ref.items() if v.dim() == 1}
        total = part if total is None else {k: total[k] + v for k, v in part.items()}
    L.check_cols(total, d, rows, cols, pre, log="ln:production")


# ------------------------------------------------------------------------------------------------------------------ contents
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("d", [768, 1024])
@pytest.mark.parametrize("kind", L.CONTENT)
def test_row_contents(kind, d, eps):
    """Rows whose variance cancels (mean 100 / std 0.5, mean -1000 / std 1), sits at or below eps (std 1e-2, 1e-3: eps decides the
    result), is exactly 0 (constant rows), or belongs to one row of 3e4 spikes; eps = 1e-5 and the encoder's 1e-6."""
    x, g, b, dy, dres, _ = _case(257, d, seed=d + 17, kind=kind)
    _ops_fwd_bwd(x, g, b, dy, dres, L.f32(eps), f"ln:{kind}:d{d}:eps{eps:.0e}")


# ------------------------------------------------------------------------------------------------------------------ options
SHAPES = [(130, 256), (1026, 768), (65, 1024)]


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("rows,d", SHAPES)
def test_row_strides(rows, d, flip):
    """Every leading dimension d + 4 and d + 64, neighbours in the argument list taking different ones (a stride used for the wrong
    tensor shows); the padding of the inputs is NaN, that of the outputs must stay NaN."""
    a, c = (d + 4, d + 64) if flip == 0 else (d + 64, d + 4)
    x, g, b, dy, dres, _ = _case(rows, d, seed=rows + flip)
    ref_f = raw_fwd(x, g, b, EPS, ldx=a, ldy=c, ldyf=a)
    raw_fwd(x, g, b, EPS, ldx=c, ldy=a, want_f32=False)
    raw_fwd(x, g, b, EPS, ldx=a, ldyf=c, want_bf16=False)
    for workspace in (False, True):
        raw_bwd(x, g, dy, ref_f, dres=dres, prefill=_prefill(d, rows), workspace=workspace, ldx=a, lddy=c, lddres=a + 8, lddx=c + 8, lddxb=a)


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "strided"])
@pytest.mark.parametrize("seq_len", [1, 17, 513])
@pytest.mark.parametrize("rows,d", SHAPES)
def test_x_alt_forms(rows, d, seq_len, packed):
    """Row 0 of every sequence from x_alt, as a packed [sequences, d] tensor (ld_alt = d) or as the rows of a tensor laid out like x
    (ld_alt = seq_len * ldx); seq_len = 1 takes every row from x_alt; the last sequence is cut short where rows % seq_len != 0."""
    x, g, b, dy, dres, x_alt = _case(rows, d, seed=rows + seq_len, seq_len=seq_len)
    ldx = d + 4 if not packed else d
    ref_f = raw_fwd(x, g, b, EPS, x_alt=x_alt, seq_len=seq_len, packed=packed, ldx=ldx)
    for workspace in (False, True):
        raw_bwd(x, g, dy, ref_f, dres=dres, x_alt=x_alt, seq_len=seq_len, packed=packed, ldx=ldx, prefill=_prefill(d, seq_len), workspace=workspace)


@pytest.mark.parametrize("workspace", [False, True], ids=["atomic", "workspace"])
@pytest.mark.parametrize("rows,d", SHAPES)
def test_backward_option_sets(rows, d, workspace):
    """dres NULL / given x dx_bf16 NULL / given x dxsum NULL / given x dressum NULL / given, the sums prefilled with non-zero values
    (the kernel adds), each in the atomic and in the workspace form (bit-identical on a second call)."""
    x, g, b, dy, dres, _ = _case(rows, d, seed=rows + 31)
    ref_f = L.ln_ref(x, None, 0, g, b, EPS)
    for with_dres in (False, True):
        for want_bf16 in (False, True):
            for dxsum in (False, True):
                for dressum in ((False, True) if with_dres else (False,)):
                    raw_bwd(x, g, dy, ref_f, dres=dres if with_dres else None, want_bf16=want_bf16, dxsum=dxsum, dressum=dressum,
                            prefill=_prefill(d, rows + dxsum), workspace=workspace)


def test_refusals_launch_nothing():
    """dressum without dres, and an undersized workspace, are refused with a negative status before anything is launched."""
    rows, d = 65, 1024
    x, g, b, dy, _, _ = _case(rows, d, seed=3)
    ref_f = L.ln_ref(x, None, 0, g, b, EPS)
    xd, dyd, gd = x.to(dev()), dy.to(dev(), torch.bfloat16), g.to(dev())
    mud, rsd = ref_f["mu"].float().to(dev()), ref_f["rs"].float().to(dev())
    dx = L.nan_buffer(rows, d, torch.float32, dev())
    dg, db, sx, sr = (torch.full((d,), 0.5, device=dev()) for _ in range(4))
    need = _lib().xvit_layernorm_bwd_workspace_bytes(rows, d)
    ws = torch.full((need // 4,), math.nan, device=dev())

    def call(dressum, ws_bytes):
        return _lib().xvit_layernorm_bwd(_p(dyd), d, _p(xd), None, d, 0, 0, _p(mud), _p(rsd), _p(gd), None, 0, _p(dx), d, None, 0, _p(dg), _p(db), _p(sx),
                                         _p(dressum), rows, d, _p(ws) if ws_bytes else None, ws_bytes, _stream())
    rc = call(sr, 0)
    assert rc < 0 and "dressum needs dres" in _err(), (rc, _err())
    rc = call(None, need - 4)
    assert rc < 0 and "workspace too small" in _err(), (rc, _err())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(ws).all()), "a refused call wrote dx or the workspace"
    for t in (dg, db, sx, sr):
        assert bool((t == 0.5).all()), "a refused call touched a sum"
    for bad_d in (4100, 6):
        rc = _lib().xvit_layernorm_bwd(_p(dyd), d, _p(xd), None, d, 0, 0, _p(mud), _p(rsd), _p(gd), None, 0, _p(dx), d, None, 0, _p(dg), _p(db), None, None, 1,
                                       bad_d, None, 0, _stream())
        assert rc < 0 and "d <= 4096" in _err(), (rc, _err())


# ------------------------------------------------------------------------------------------------------------------ column sums
COLSUM_ROWS = (1, 3, 4, 5, 13, 16, 17, 63, 64, 65, 77, 1026)


def _colsum(x, *, ldx, accumulate, workspace, seed, log=None):
    """xvit_colsum through the C ABI: accumulate on a prefilled vector or off on a NaN-prefilled one; atomic or workspace form (the
    latter twice, bit-identical)."""
    rows, n = x.shape
    xd = _strided(x, ldx)
    pre = _prefill(n, seed)["dgamma"] if accumulate else None
    from xvit import ops
    dt = ops.F32 if x.dtype == torch.float32 else ops.BF16
    ws_bytes = _lib().xvit_colsum_workspace_bytes(rows, n) if workspace else 0
    outs = []
    for _ in range(2 if workspace else 1):
        out = pre.to(dev()).clone() if accumulate else torch.full((n + 4,), math.nan, device=dev())
        ws = torch.full((ws_bytes // 4,), math.nan, device=dev()) if workspace else None
        rc = _lib().xvit_colsum(_p(xd), dt, ldx, _p(out), rows, n, int(accumulate), _p(ws), ws_bytes, _stream())
        assert rc == 0, f"xvit_colsum rc = {rc}: {_err()}"
        torch.cuda.synchronize()
        outs.append(out)
    L.check_colsum(outs[0][:n], x, n, rows, pre, log=log)
    if not accumulate:
        assert bool(torch.isnan(outs[0][n:]).all()), "xvit_colsum wrote past column n"
    if workspace:
        assert torch.equal(outs[0][:n], outs[1][:n]), "xvit_colsum, workspace form: two calls differ"


@pytest.mark.parametrize("n", [4, 252, 256, 260, 768, 3072])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_colsum(dtype, n):
    """Every remainder class of the 16-row main loop and the 4-row tail, one and several 64-row chunks; row stride n and n + 4;
    accumulate on and off; the atomic and the workspace form."""
    for rows in COLSUM_ROWS:
        x = L.content("usual", rows, n, seed=rows + n).to(dtype)
        for ldx, accumulate, workspace in ((n, False, False), (n + 4, True, False), (n + 4, False, True), (n, True, True)):
            _colsum(x, ldx=ldx, accumulate=accumulate, workspace=workspace, seed=rows, log=f"colsum:{dtype}:n{n}:rows{rows}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_colsum_where_the_chunk_doubles(dtype):
    """64 x 171 + 1 rows at n = 3072: 12 column blocks x 172 chunks would pass 2048 blocks, so a chunk takes 128 rows."""
    rows, n = 64 * 171 + 1, 3072
    assert L.colsum_rows_per_block(rows, n) == 128
    x = L.content("usual", rows, n, seed=9).to(dtype)
    for ldx, accumulate, workspace in ((n + 4, True, False), (n, False, True)):
        _colsum(x, ldx=ldx, accumulate=accumulate, workspace=workspace, seed=1, log=f"colsum:{dtype}:n{n}:rows{rows}")
    need = _lib().xvit_colsum_workspace_bytes(rows, n)
    assert need == -(-rows // 128) * n * 4
    out, ws = torch.zeros(n, device=dev()), torch.zeros(need // 4, device=dev())
    from xvit import ops
    rc = _lib().xvit_colsum(_p(x.to(dev())), ops.F32 if dtype == torch.float32 else ops.BF16, n, _p(out), rows, n, 0, _p(ws), need - 4, _stream())
    assert rc < 0 and "workspace too small" in _err(), (rc, _err())
