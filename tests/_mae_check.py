"""Restatements and gates of the masked-pretraining kernels (include/xvit.h "Masked-volume pretraining", csrc/mae.hip), shared by the mae tests.

Bit-exact (integer work, or single fp32 additions in the order the header states), NumPy fp32:
  complement           xvit_token_select_complement
  unshuffle_fwd / bwd  xvit_mae_unshuffle_fwd / _bwd
  rows_gather/scatter  xvit_token_rows_gather / _scatter

Bounded (float64 reference, bounds below):
  loss_ref64           xvit_mae_loss_fwd / _bwd: mean, rstd, row_loss, loss_seq, loss, dpred
  loss_bounds          the bound of every element of those, from the reference's own tensors
  loss_fp32_alt        the same formulas in fp32 NumPy with every sum taken sequentially from the far end (another order than the kernel's)

The bounds.  u = 2^-24 (fp32 unit round-off), ub = 2^-8 (bf16), gamma(n) = n u / (1 - n u) (Higham): a sum of n fp32 terms taken in ANY
order and divided once is within gamma(n) sum|x_i| of the exact sum.  The inputs (bf16 or fp32 voxels v_i and predictions p_i) are exact
in float64.  Per row, with pd voxels, A = sum|v_i| / pd, c_i = v_i - mean, var = sum c_i^2 / (pd - 1), w = var + 1e-6:
  mean      |mean~ - mean| <= E_mean = gamma(pd) A
  rstd      c~_i = (c_i - e)(1 + eta), |e| <= E_mean, |eta| <= u; sum_i (c_i - e)^2 = sum c_i^2 + pd e^2 because sum c_i = 0: the mean's
            error enters the variance in second order only (this is what the two-pass form buys; a one-pass sum v^2 - pd mean^2 has
            the error u (mean / std)^2 relative to var).  So |var~ - var| <= pd E_mean^2 / (pd - 1) (1 + g) + g var, g = gamma(pd + 4),
            |w~ - w| <= dw = |var~ - var| + u (w + 1e-6 + |var~ - var|), w~ >= 1e-6 (1 - 2u) as var~ >= 0, and with sqrt and the division within 2 ulp
            each: E_rstd = max(1/sqrt(w_lo) - rstd, rstd - 1/sqrt(w + dw)) (1 + 4u) + 4u rstd, w_lo = max(w - dw, 1e-6 (1 - 2u)).
  target    t_i = c_i rstd: |t~_i - t_i| <= dt_i = |c_i| E_rstd + (rstd + E_rstd) E_mean + 2u (|t_i| + the two terms before)
            (|mean| rstd enters through E_mean rstd = gamma(pd) A rstd).  Without norm_pix mean = 0, rstd = 1 and t~ = v exactly: dt = 0.
  row_loss  e_i = p_i - t_i, |e~_i - e_i| <= de_i = dt_i + u (|e_i| + dt_i);  sum e~^2 - sum e^2 <= 2 sum|e_i| de_i + sum de_i^2 =: D;
            E_row = (D + gamma(pd + 2) (sum e_i^2 + D)) / pd
  loss_seq  E_seq = mean_j E_row + gamma(Rm + 1) mean_j (row_loss + E_row)
  loss      E_loss = mean_r E_row + gamma(S Rm + 2) mean_r (row_loss + E_row)     (any order over all S Rm rows covers the kernel's two levels)
  dpred     coef = g 2 / (pd S Rm) carries 3 roundings: E_dpred = |coef| (de_i + 4u (|e_i| + de_i)), and for a bf16 dpred + ub (|dpred_i| + that)
A tiny absolute 1e-37 covers results in the denormal range."""
import numpy as np
import torch

U32 = 2.0 ** -24
UB16 = 2.0 ** -8
EPS = 1e-6
TINY = 1e-37


def gamma(n):
    return n * U32 / (1.0 - n * U32)


# ---- bit-exact restatements ------------------------------------------------------------------------------------------------------------


def complement(slot, K):
    """slot int32 [S, P] -> (drop_idx int32 [S, P - K], mslot int32 [S, P]) as the kernel writes them, a row with another count of kept
    entries than K included: the first P - K dropped patches are listed, the tail of drop_idx is -1."""
    S, P = slot.shape
    Rm = P - K
    dropped = slot < 0
    pos = np.cumsum(dropped, axis=1) - 1                               # position among the dropped patches of the row
    place = dropped & (pos < Rm)
    mslot = np.where(place, pos, -1).astype(np.int32)
    drop_idx = np.full((S, Rm), -1, dtype=np.int32)
    s_i, p_i = np.nonzero(place)
    drop_idx[s_i, pos[s_i, p_i]] = p_i
    return drop_idx, mslot


def unshuffle_fwd(xe, mask_token, dpos, dmod, slot, B):
    """y[s, 0] = (xe[s, 0] + dpos[0]) + dmod[m]; y[s, 1 + p] = ((kept ? xe[s, 1 + slot] : mask_token) + dpos[1 + p]) + dmod[m], fp32."""
    S, K1, dd = xe.shape
    P = slot.shape[1]
    xe, mask_token, dpos, dmod = (np.asarray(a, dtype=np.float32) for a in (xe, mask_token, dpos, dmod))
    src = np.empty((S, P + 1, dd), dtype=np.float32)
    src[:, 0] = xe[:, 0]
    kept = slot >= 0
    gathered = np.take_along_axis(xe[:, 1:], np.where(kept, slot, 0).astype(np.int64)[:, :, None], axis=1) if K1 > 1 else np.zeros((S, P, dd), np.float32)
    src[:, 1:] = np.where(kept[:, :, None], gathered, mask_token.reshape(1, 1, dd))
    m = np.arange(S) // B
    return (src + dpos.reshape(1, P + 1, dd)) + dmod.reshape(-1, dd)[m][:, None, :]


def unshuffle_bwd(dy, keep_idx, slot, M):
    """-> (dxe [S, K+1, dd], dmask_token [dd], ddpos_m [M, P+1, dd]): the gather, and the sums in the header's order (sequential fp32, from 0)."""
    S, P1, dd = dy.shape
    B = S // M
    dy = np.asarray(dy, dtype=np.float32)
    rows = np.concatenate((np.zeros((S, 1), dtype=np.int64), 1 + keep_idx.astype(np.int64)), axis=1)
    dxe = np.take_along_axis(dy, rows[:, :, None], axis=1)
    ddpos_m = np.zeros((M, P1, dd), dtype=np.float32)
    for m in range(M):
        for b in range(B):
            ddpos_m[m] = ddpos_m[m] + dy[m * B + b]
    dmask = np.zeros(dd, dtype=np.float32)
    for s in range(S):
        part = np.zeros(dd, dtype=np.float32)
        for p in range(P1 - 1):
            if slot[s, p] < 0:
                part = part + dy[s, 1 + p]
        dmask = dmask + part
    return dxe, dmask, ddpos_m


def rows_gather(x, drop_idx):
    S, P1, dd = x.shape
    return np.take_along_axis(np.asarray(x), 1 + drop_idx.astype(np.int64)[:, :, None], axis=1).reshape(-1, dd)


def rows_scatter(dg, mslot, Rm):
    S, P = mslot.shape
    dd = dg.shape[1]
    dx = np.zeros((S, P + 1, dd), dtype=dg.dtype)
    s_i, p_i = np.nonzero(mslot >= 0)
    dx[s_i, 1 + p_i] = dg.reshape(S, Rm, dd)[s_i, mslot[s_i, p_i]]
    return dx


# ---- the loss: reference, bounds, another fp32 order --------------------------------------------------------------------------------------


def patch_rows(img, patch, idx):
    """img [B, M, 1, D, H, W] (values copied), idx [M*B, R] -> [M*B*R, pd]: patch idx[m B + b][j] of volume (b, m); token t = (h Wn + w) Dn + d,
    feature f = (p1 hp + p2) wp + p3 (xvit_patchify)."""
    B, M, _, D, H, W = img.shape
    dp, hp, wp = patch
    Dn, Wn = D // dp, W // wp
    out = np.empty((idx.shape[0] * idx.shape[1], dp * hp * wp), dtype=img.dtype)
    r = 0
    for s in range(M * B):
        m, b = divmod(s, B)
        for t in idx[s]:
            d, w, h = int(t) % Dn, (int(t) // Dn) % Wn, int(t) // (Dn * Wn)
            out[r] = img[b, m, 0, d * dp:(d + 1) * dp, h * hp:(h + 1) * hp, w * wp:(w + 1) * wp].reshape(-1)
            r += 1
    return out


def loss_ref64(pred, img, patch, drop_idx, norm_pix, g):
    """float64: dict(mean, rstd [rows], row_loss [rows], loss_seq [S], loss [1], dpred [rows, pd]) and the tensors the bounds need."""
    S, Rm = drop_idx.shape
    v = patch_rows(np.asarray(img, dtype=np.float64), patch, drop_idx)
    p = np.asarray(pred, dtype=np.float64)
    rows, pd = v.shape
    if norm_pix:
        mean = v.mean(axis=1)
        c = v - mean[:, None]
        var = (c * c).sum(axis=1) / (pd - 1)
        rstd = 1.0 / np.sqrt(var + EPS)
    else:
        mean, rstd, c, var = np.zeros(rows), np.ones(rows), v, None
    e = p - c * rstd[:, None]
    row_loss = (e * e).sum(axis=1) / pd
    coef = float(g) * 2.0 / (pd * rows)
    return dict(mean=mean, rstd=rstd, row_loss=row_loss, loss_seq=row_loss.reshape(S, Rm).mean(axis=1), loss=np.array([row_loss.mean()]), dpred=coef * e,
                _v=v, _c=c, _var=var, _e=e, _coef=coef, _norm=bool(norm_pix), _shape=(S, Rm, pd))


BOUNDED = ("mean", "rstd", "row_loss", "loss_seq", "loss", "dpred")


def loss_bounds(ref, dpred_bf16):
    """The module docstring's bounds, evaluated on the reference's own tensors -> dict over BOUNDED, each shaped like its quantity."""
    S, Rm, pd = ref["_shape"]
    v, c, e, rstd = ref["_v"], ref["_c"], ref["_e"], ref["rstd"]
    rows = S * Rm
    if ref["_norm"]:
        var = ref["_var"]
        E_mean = gamma(pd) * np.abs(v).sum(axis=1) / pd
        g4 = gamma(pd + 4)
        dvar = pd * E_mean ** 2 / (pd - 1) * (1 + g4) + g4 * var
        w = var + EPS
        dw = dvar + U32 * (w + EPS + dvar)
        w_lo = np.maximum(w - dw, EPS * (1 - 2 * U32))
        E_rstd = np.maximum(1.0 / np.sqrt(w_lo) - rstd, rstd - 1.0 / np.sqrt(w + dw)) * (1 + 4 * U32) + 4 * U32 * rstd
        first = np.abs(c) * E_rstd[:, None] + ((rstd + E_rstd) * E_mean)[:, None]
        dt = first + 2 * U32 * (np.abs(c * rstd[:, None]) + first)
    else:
        E_mean, E_rstd, dt = np.zeros(rows), np.zeros(rows), np.zeros_like(e)
    de = dt + U32 * (np.abs(e) + dt)
    D = 2 * (np.abs(e) * de).sum(axis=1) + (de * de).sum(axis=1)
    E_row = (D + gamma(pd + 2) * ((e * e).sum(axis=1) + D)) / pd
    up = ref["row_loss"] + E_row
    E_seq = E_row.reshape(S, Rm).mean(axis=1) + gamma(Rm + 1) * up.reshape(S, Rm).mean(axis=1)
    E_loss = np.array([E_row.mean() + gamma(rows + 2) * up.mean()])
    coef = abs(ref["_coef"])
    E_d = coef * (de + 4 * U32 * (np.abs(e) + de))
    if dpred_bf16:
        E_d = E_d + UB16 * (np.abs(ref["dpred"]) + E_d)
    out = dict(mean=E_mean, rstd=E_rstd, row_loss=E_row, loss_seq=E_seq, loss=E_loss, dpred=E_d)
    return {k: b + TINY for k, b in out.items()}


def violations(got, ref, bounds):
    """{quantity: (number of elements outside their bound, largest |got - ref| / bound)}; NaN counts as outside."""
    out = {}
    for k in BOUNDED:
        err = np.abs(np.asarray(got[k], dtype=np.float64).reshape(ref[k].shape) - ref[k])
        bad = ~(err <= bounds[k])
        out[k] = (int(bad.sum()), float(np.nanmax(err / bounds[k])) if err.size else 0.0)
    return out


def _seq_sum_f32(a):
    """fp32 sum along the last axis taken sequentially from the FAR end (np.cumsum keeps fp32 and adds in order)."""
    return np.cumsum(np.asarray(a, dtype=np.float32)[..., ::-1], axis=-1, dtype=np.float32)[..., -1]


def loss_fp32_alt(pred, img, patch, drop_idx, norm_pix, g, dpred_bf16):
    """The kernel's formulas in fp32 NumPy, every sum sequential from the far end -> the quantities of BOUNDED."""
    S, Rm = drop_idx.shape
    f = np.float32
    v = patch_rows(np.asarray(img, dtype=f), patch, drop_idx)
    p = np.asarray(pred, dtype=f)
    rows, pd = v.shape
    if norm_pix:
        mean = _seq_sum_f32(v) / f(pd)
        c = v - mean[:, None]
        var = _seq_sum_f32(c * c) / f(pd - 1)
        rstd = f(1.0) / np.sqrt(var + f(EPS), dtype=f)
    else:
        mean, rstd, c = np.zeros(rows, f), np.ones(rows, f), v
    e = p - c * rstd[:, None]
    row_loss = _seq_sum_f32(e * e) / f(pd)
    loss_seq = _seq_sum_f32(row_loss.reshape(S, Rm)) / f(Rm)
    loss = np.array([_seq_sum_f32(row_loss) / f(rows)], dtype=f)
    coef = f(g) * (f(2.0) / (f(pd) * f(rows)))
    dpred = coef * e
    if dpred_bf16:
        dpred = torch.from_numpy(dpred).to(torch.bfloat16).float().numpy()
    return dict(mean=mean, rstd=rstd, row_loss=row_loss, loss_seq=loss_seq, loss=loss, dpred=dpred)


# ---- the cases of the loss tests (tests/test_mae_kernels_gpu.py runs them on the GPU, tests/test_mae_gate_cpu.py the reference arithmetic) ----

LOSS_SHAPES = {"pd64": ((8, 8, 16), (4, 4, 4)),        # scalar path (wp = 4)
               "pd512": ((32, 32, 16), (8, 8, 8)),     # vector path
               "pd4096": ((32, 32, 32), (16, 16, 16))}
LOSS_M, LOSS_B = 3, 2
LOSS_G = 0.375                                         # the upstream scalar (exact in fp32)


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def loss_case(shape, vol_bf16, pred_bf16, seed=0):
    """-> dict(img fp32 array [B, M, 1, D, H, W] holding exactly representable values of the volume dtype, NaN in every patch that is not
    dropped; patch; drop_idx int32 [S, Rm] (hand-made: ascending, different per sequence); pred fp32 array [S*Rm, pd] of values of the
    prediction dtype; special = {"constant": row, "offset": row | None}).  Row `constant` is a patch of one value (var = 0); on an fp32
    volume row `offset` has mean 1000 and standard deviation 0.5 (mean / std = 2000)."""
    vol, patch = LOSS_SHAPES[shape]
    M, B = LOSS_M, LOSS_B
    S = M * B
    D, H, W = vol
    dp, hp, wp = patch
    Dn, Hn, Wn = D // dp, H // hp, W // wp
    P, pd = Dn * Hn * Wn, dp * hp * wp
    Rm = max(2, P // 3)
    rng = np.random.default_rng(1234 + seed + pd)
    drop_idx = np.stack([np.sort(rng.choice(P, size=Rm, replace=False)) for _ in range(S)]).astype(np.int32)
    drop_idx[0, 0], drop_idx[S - 1, Rm - 1] = 0, P - 1                   # the first and the last patch of the grid are scored somewhere
    drop_idx[0], drop_idx[S - 1] = np.sort(_distinct(drop_idx[0], P, rng)), np.sort(_distinct(drop_idx[S - 1], P, rng))
    img = (rng.standard_normal((B, M, 1, D, H, W)) * 1.5 + 0.8).astype(np.float32)       # MRI-like: away from zero

    def region(s, t):
        m, b = divmod(s, B)
        d, w, h = int(t) % Dn, (int(t) // Dn) % Wn, int(t) // (Dn * Wn)
        return (b, m, 0, slice(d * dp, (d + 1) * dp), slice(h * hp, (h + 1) * hp), slice(w * wp, (w + 1) * wp))

    img[region(0, drop_idx[0, 1])] = 0.75                                # row 1: a constant patch
    offset = None
    if not vol_bf16:
        offset = Rm                                                       # row Rm: the first row of sequence 1
        img[region(1, drop_idx[1, 0])] = (1000.0 + 0.5 * rng.standard_normal((dp, hp, wp))).astype(np.float32)
    if vol_bf16:
        img = bf16_round(img)
    for s in range(S):                                                    # NaN behind everything the kernel must not read
        for t in sorted(set(range(P)) - set(drop_idx[s].tolist())):
            img[region(s, t)] = np.nan
    pred = rng.standard_normal((S * Rm, pd)).astype(np.float32)
    if pred_bf16:
        pred = bf16_round(pred)
    return dict(img=img, patch=patch, drop_idx=drop_idx, pred=pred, special=dict(constant=1, offset=offset), P=P, pd=pd, Rm=Rm, S=S)


def _distinct(row, P, rng):
    """A row of distinct indices: repeated entries (after the forced first / last patch) are replaced by unused ones."""
    seen, out = set(), []
    free = [p for p in range(P) if p not in set(row.tolist())]
    for t in row.tolist():
        if t in seen:
            t = free.pop()
        seen.add(t)
        out.append(t)
    return np.array(out, dtype=np.int32)


# ---- the model, restated on the oracle's blocks (torch: autograd and the bf16 emulation run through it) -------------------------------------


def model_forward(sd, img, cfg, keep, norm_pix=True):
    """MaskedVolumeModel.forward on the tokens it kept.  sd: the model's state_dict (keys "encoder.*", "decoder_*", "mask_token"); keep int64
    [M, B, K] -> dict(unshuffled, decoded [S, P+1, dd], pred, target [S*Rm, pd], loss_seq [M, B], loss, drop_idx [S, Rm]).  Composed from
    ref_cpu's patchify / linear / layer_norm / multi_scale_block / self_block, so R.emulate_bf16() rounds where the HIP path does."""
    import ref_cpu as R
    enc = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    B, M = img.shape[0], img.shape[1]
    K = keep.shape[-1]
    pos = enc["pos_embedding"]
    P, S = pos.shape[1] - 1, M * B
    patches = [R.patchify(img[:, m, 0], cfg.patch_size) for m in range(M)]                     # M x [B, P, pd]
    xs = []
    for m in range(M):
        p = torch.gather(patches[m], 1, keep[m][:, :, None].expand(-1, -1, patches[m].shape[2]))
        x = R.linear(p, enc["patch_to_embedding.weight"], enc["patch_to_embedding.bias"])
        x = torch.cat((enc["cls_token"].expand(B, -1, -1), x), dim=1)
        idx = torch.cat((torch.zeros(B, 1, dtype=torch.int64), 1 + keep[m]), dim=1)
        xs.append(x + pos[0][idx])
    for b in range(cfg.num_multi_blocks):
        xs = R.multi_scale_block(enc, f"transformer.{b}", xs, cfg)
    normed = torch.cat([R.layer_norm(xs[m], enc[f"norm.{m}.weight"], enc[f"norm.{m}.bias"]) for m in range(M)], dim=0)      # [S, K + 1, d]
    xe = R.linear(normed, sd["decoder_embed.weight"], sd["decoder_embed.bias"])
    dd = xe.shape[-1]
    keep_s = keep.reshape(S, K)
    full = sd["mask_token"].expand(S, P, dd).scatter(1, keep_s[:, :, None].expand(-1, -1, dd), xe[:, 1:])
    y = (torch.cat((xe[:, :1], full), dim=1) + sd["decoder_pos_embed"]) + sd["decoder_modality_embed"].repeat_interleave(B, dim=0)
    out = dict(unshuffled=y)
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("decoder_blocks."))
    for i in range(depth):
        y = R.self_block(sd, f"decoder_blocks.{i}", y, dd // 64)
    out["decoded"] = y
    slot = np.full((S, P), -1, dtype=np.int32)
    np.put_along_axis(slot, keep_s.numpy(), np.broadcast_to(np.arange(K, dtype=np.int32), (S, K)), axis=1)
    drop_idx = torch.from_numpy(complement(slot, K)[0]).long()                               # [S, Rm]
    Rm = P - K
    rows = torch.gather(y[:, 1:], 1, drop_idx[:, :, None].expand(-1, -1, dd)).reshape(S * Rm, dd)
    rows = R.layer_norm(rows, sd["decoder_norm.weight"], sd["decoder_norm.bias"])
    pred = R.linear(rows, sd["decoder_pred.weight"], sd["decoder_pred.bias"], store=True)
    target = torch.gather(torch.cat(patches, dim=0), 1, drop_idx[:, :, None].expand(-1, -1, patches[0].shape[2])).reshape(S * Rm, -1)
    if norm_pix:
        mean = target.mean(dim=1, keepdim=True)
        target = (target - mean) / torch.sqrt(target.var(dim=1, unbiased=True, keepdim=True) + EPS)
    row_loss = ((pred - target) ** 2).mean(dim=1)
    out.update(pred=pred, target=target, loss_seq=row_loss.reshape(S, Rm).mean(dim=1).reshape(M, B), loss=row_loss.mean(), drop_idx=drop_idx)
    return out


def loss_gate(ref, eps):
    """What a relative L2 distance eps of the predicted rows allows on the losses, by Cauchy-Schwarz on sum (p~ - t)^2 - sum (p - t)^2 =
    sum (p~ - p)(p~ + p - 2t) with ||p~ - p|| <= eps ||p||: (2 eps ||p|| ||p - t|| + eps^2 ||p||^2) / (pd rows), on the reference's own
    tensors; for a sequence ||p - t|| and rows are the sequence's, ||p~ - p|| stays the whole tensor's.  -> (bound of loss, of loss_seq [M, B])."""
    p, t = ref["pred"].detach().double(), ref["target"].detach().double()
    rows, pd = p.shape
    M, B = ref["loss_seq"].shape
    pn = float(p.norm())
    whole = (2 * eps * pn * float((p - t).norm()) + eps ** 2 * pn ** 2) / (pd * rows)
    Rm = rows // (M * B)
    en = (p - t).reshape(M * B, Rm * pd).norm(dim=1)
    return whole, ((2 * eps * pn * en + eps ** 2 * pn ** 2) / (pd * Rm)).reshape(M, B)
