"""NumPy restatement of patch dropout's kernels (include/xvit.h, csrc/token_select.hip), shared by the tokdrop tests.

  hash32               the project's counter hash (xvit_common.h), as tests/_augment_check.py restates it
  draw                 xvit_token_select_draw: the K smallest (key, p) of every sequence, ascending, and the inverse map
  patchify_select      xvit_patchify_select's index map: which voxels make row 1 + j of sequence s (values untouched)
  embed_select_fwd     + pos of the kept patch on the patch rows, cls + pos[0] on the CLS rows: one fp32 add per element
  embed_select_bwd     the same sequential fp32 sum the kernel makes: per pos row, over the sequences in ascending order
  TIE                  the (P, K, seed) of the draw tests' tie case

Everything the kernels compute is either integer work or single fp32 additions in a stated order, so every comparison against these
functions is bit-exact."""
import numpy as np

_M64 = (1 << 64) - 1
EPOCH_STRIDE = 0xD1B54A32D192ED03          # drop_seed_at: seed + epoch * this (mod 2^64)
TIE = dict(P=4096, K=20, seed=109)         # under this seed the 20th and 21st smallest keys of sequence 0 are equal (tests/test_tokdrop_cpu.py shows it)


def hash32(seed, idx):
    """xvit_common.h hash32 on arrays of indices -> uint32 values (as uint64 arrays)."""
    with np.errstate(over="ignore"):
        z = np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(int(seed) & _M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((z ^ (z >> np.uint64(31))) >> np.uint64(16)) & np.uint64(0xFFFFFFFF)


def seed_at(seed, epoch=None):
    return int(seed) & _M64 if epoch is None else (int(seed) + int(epoch) * EPOCH_STRIDE) & _M64


def keys(S, B, P, shared, seed, epoch=None):
    """[S, P] keys: hash32(seed', u P + p), u = s (or s mod B when shared)."""
    s = np.arange(S, dtype=np.uint64)
    u = s % np.uint64(B) if shared else s
    return hash32(seed_at(seed, epoch), u[:, None] * np.uint64(P) + np.arange(P, dtype=np.uint64)[None, :])


def draw(S, B, P, K, shared, seed, epoch=None):
    """-> keep_idx int32 [S, K] (ascending), slot int32 [S, P] (position in keep_idx, -1 = dropped)."""
    k = keys(S, B, P, shared, seed, epoch)
    order = np.argsort(k, axis=1, kind="stable")          # by (key, p): a stable sort leaves equal keys in ascending p
    keep_idx = np.sort(order[:, :K], axis=1).astype(np.int32)
    slot = np.full((S, P), -1, dtype=np.int32)
    np.put_along_axis(slot, keep_idx.astype(np.int64), np.broadcast_to(np.arange(K, dtype=np.int32), (S, K)), axis=1)
    return keep_idx, slot


def slot_of(keep_idx, P):
    """The inverse map of a hand-made keep_idx [S, K]."""
    S, K = keep_idx.shape
    slot = np.full((S, P), -1, dtype=np.int32)
    np.put_along_axis(slot, keep_idx.astype(np.int64), np.broadcast_to(np.arange(K, dtype=np.int32), (S, K)), axis=1)
    return slot


def patchify_select(img, patch, keep_idx):
    """img [B, M, 1, D, H, W] (any dtype, values copied) -> [M, B (K + 1), pd]: row 0 of every sequence zero, row 1 + j = patch
    keep_idx[m B + b][j]; token t = (h Wn + w) Dn + d, feature f = (p1 hp + p2) wp + p3."""
    B, M, _, D, H, W = img.shape
    dp, hp, wp = patch
    Dn, Hn, Wn = D // dp, H // hp, W // wp
    K = keep_idx.shape[1]
    out = np.zeros((M, B, K + 1, dp * hp * wp), dtype=img.dtype)
    for m in range(M):
        for b in range(B):
            for j, t in enumerate(keep_idx[m * B + b]):
                d, w, h = int(t) % Dn, (int(t) // Dn) % Wn, int(t) // (Dn * Wn)
                out[m, b, 1 + j] = img[b, m, 0, d * dp:(d + 1) * dp, h * hp:(h + 1) * hp, w * wp:(w + 1) * wp].reshape(-1)
    return out.reshape(M, B * (K + 1), -1)


def embed_select_fwd(x, cls, pos, keep_idx):
    """x fp32 [S (K + 1), d] -> a new array: patch rows + pos[1 + kept patch], CLS rows = cls + pos[0]."""
    S, K = keep_idx.shape
    d = x.shape[1]
    y = x.astype(np.float32).reshape(S, K + 1, d).copy()
    pos = pos.astype(np.float32).reshape(-1, d)
    y[:, 1:] = y[:, 1:] + pos[1 + keep_idx.astype(np.int64)]
    y[:, 0] = cls.astype(np.float32).reshape(d) + pos[0]
    return y.reshape(S * (K + 1), d)


def embed_select_bwd(dx, slot, dpos, dcls, K):
    """-> (dpos, dcls) after the kernel: for pos row 1 + p, acc = 0; acc += dx[s, 1 + slot[s][p]] for s ascending where slot >= 0;
    dpos[1 + p] += acc.  Row 0 and dcls += the sum of the CLS rows in the same order.  A row nobody kept keeps its bits."""
    S, P = slot.shape
    d = dx.shape[1]
    dx = dx.astype(np.float32).reshape(S, K + 1, d)
    dpos, dcls = dpos.astype(np.float32).copy(), dcls.astype(np.float32).copy()
    acc = np.zeros(d, dtype=np.float32)
    for s in range(S):
        acc = acc + dx[s, 0]
    dpos[0] = dpos[0] + acc
    dcls = dcls + acc
    for p in range(P):
        acc = np.zeros(d, dtype=np.float32)
        kept = False
        for s in range(S):
            if slot[s, p] >= 0:
                acc = acc + dx[s, 1 + slot[s, p]]
                kept = True
        if kept:
            dpos[1 + p] = dpos[1 + p] + acc
    return dpos, dcls
