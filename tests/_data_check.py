"""NumPy restatement of the device-resident volume store's two kernels (include/xvit.h, "Device-resident volume store"): the hash, the
global ordinals, the weighted draw, the keyed Feistel permutation, the sequential mode and the gather.  Integer and fp64 arithmetic only,
so the kernels are compared with it bit for bit."""
import numpy as np

_M64 = (1 << 64) - 1
SEED_STRIDE = 0xD1B54A32D192ED03          # kSeedStride of xvit_common.h
TAG = 0x5356444154415354                   # keeps this stream apart from the other draw streams under one seed
WEIGHTED, SHUFFLE, SEQUENTIAL = 0, 1, 2    # XVIT_BATCH_*
MODES = {"weighted": WEIGHTED, "shuffle": SHUFFLE, "sequential": SEQUENTIAL}
GATHER_THREADS, GATHER_ITEMS = 256, 8      # a workgroup of xvit_batch_gather owns 256 * 8 accesses of one case:
WIDE_CHUNK = GATHER_THREADS * GATHER_ITEMS * 16     # ... 32 KiB where case_bytes % 16 == 0
NARROW_CHUNK = GATHER_THREADS * GATHER_ITEMS * 2    # ... 4 KiB otherwise


def hash32(seed, idx):
    """xvit_common.h hash32 on arrays of indices -> uint32 values (as uint64 arrays).  seed: one integer, or a uint64 array (one per index)."""
    seed = seed if isinstance(seed, np.ndarray) else np.uint64(int(seed) & _M64)
    with np.errstate(over="ignore"):
        z = np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + seed
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((z ^ (z >> np.uint64(31))) >> np.uint64(16)) & np.uint64(0xFFFFFFFF)


def draw24(seed, idx):
    return hash32(seed, idx) & np.uint64(0xFFFFFF)


def ordinals(B, rank=0, world=1, call=0):
    """k = (call * world + rank) * B + i for i < B, modulo 2^64 (Python integers: exact)."""
    base = ((int(call) * world + rank) * B) & _M64
    return [(base + i) & _M64 for i in range(B)]


def make_cdf(weights):
    """The inclusive fp64 prefix of the normalised weights; every entry from the last positive weight on is exactly 1."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.size == 0 or not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
        raise ValueError("weights: a non-empty vector of finite, non-negative numbers with a positive sum")
    cdf = np.cumsum(w) / w.sum()
    cdf[int(np.nonzero(w > 0)[0][-1]):] = 1.0
    return np.minimum(cdf, 1.0)


def weighted_ref(cdf, ks, seed):
    s = (int(seed) & _M64) ^ TAG
    k = np.array(ks, dtype=np.uint64)
    with np.errstate(over="ignore"):
        hi, lo = draw24(s, k * np.uint64(2)), draw24(s, k * np.uint64(2) + np.uint64(1))
    u = (hi * np.uint64(1 << 24) + lo).astype(np.float64) * 2.0 ** -48           # < 2^48: exact
    return np.minimum(np.searchsorted(np.asarray(cdf, dtype=np.float64), u, side="right"), len(cdf) - 1).astype(np.int32)


def feistel_bits(n):
    return max(2, ((int(n) - 1).bit_length() + 1) // 2 * 2)


def permute(n, e, q, seed):
    """pi_e(q) for arrays e, q (uint64, q < n): four balanced Feistel rounds on feistel_bits(n) bits, cycle-walked into [0, n)."""
    s = (int(seed) & _M64) ^ TAG
    half = np.uint64(feistel_bits(n) // 2)
    mask = np.uint64((1 << int(half)) - 1)
    e = np.asarray(e, dtype=np.uint64)
    x = np.array(q, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = np.uint64(s) + e * np.uint64(SEED_STRIDE)
    key = np.broadcast_to(key, x.shape)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        L, R = x[todo] >> half, x[todo] & mask
        for r in range(4):
            L, R = R, L ^ (hash32(key[todo], (np.uint64(r) << np.uint64(32)) | R) & mask)
        x[todo] = (L << half) | R
        todo = x >= np.uint64(n)
    return x


def shuffle_ref(n, ks, seed):
    q = np.array([k % n for k in ks], dtype=np.uint64)
    e = np.array([k // n for k in ks], dtype=np.uint64)
    return permute(n, e, q, seed).astype(np.int32)


def sequential_ref(n, ks):
    return np.array([k % n for k in ks], dtype=np.int32)


def draw_ref(mode, n, B, seed=0, rank=0, world=1, call=0, cdf=None):
    """What xvit_batch_draw writes: int32 [B]."""
    ks = ordinals(B, rank, world, call)
    mode = MODES.get(mode, mode)
    if mode == WEIGHTED:
        assert cdf is not None and len(cdf) == n
        return weighted_ref(cdf, ks, seed)
    if mode == SHUFFLE:
        return shuffle_ref(n, ks, seed)
    assert mode == SEQUENTIAL
    return sequential_ref(n, ks)


def gather_ref(store, idx, labels=None):
    """store uint8 [n, case_bytes], idx int [B] -> (dst uint8 [B, case_bytes], labels int64 [B] or None, status int32 [B])."""
    n = store.shape[0]
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < n)
    dst = np.zeros((len(idx), store.shape[1]), dtype=np.uint8)
    dst[ok] = store[idx[ok]]
    lab = None
    if labels is not None:
        lab = np.full(len(idx), -1, dtype=np.int64)
        lab[ok] = np.asarray(labels, dtype=np.int64)[idx[ok]]
    return dst, lab, (~ok).astype(np.int32)


def chunks(case_bytes):
    """Workgroups per case of xvit_batch_gather."""
    c = WIDE_CHUNK if case_bytes % 16 == 0 else NARROW_CHUNK
    return (case_bytes + c - 1) // c


def chi_square(counts, expected):
    counts, expected = np.asarray(counts, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    return float(((counts - expected) ** 2 / expected).sum())
