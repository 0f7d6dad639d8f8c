"""CPU: patch dropout's host side — the keep count, the argument refusals of the C entry points (nothing is launched), the NumPy
restatement of the draw that the GPU tests compare against (tests/_tokdrop_check.py), and the model's attributes."""
import math

import numpy as np
import pytest

import ref_cpu as R
import _tokdrop_check as T

TIE = T.TIE


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 127, 128, 512, 4096])
@pytest.mark.parametrize("p", [0.01, 0.25, 0.5, 0.75, 0.99])
def test_patch_keep_count_edges(P, p):
    from xvit.functional import patch_keep_count
    K = patch_keep_count(P, p)
    raw = max(1, math.floor(P * (1.0 - p)))
    assert 1 <= K <= P and K <= raw
    if raw >= 64:
        assert K % 64 == 0 and raw - K < 64 and K >= 64     # rounded down to the CLS-peel shape N - 1 = 64 m
    else:
        assert K == raw


def test_patch_keep_count_values_and_bad_rates():
    from xvit.functional import patch_keep_count
    assert [patch_keep_count(512, p) for p in (0.0, 0.25, 0.5, 0.75)] == [512, 384, 256, 128]
    assert patch_keep_count(4096, 0.5) == 2048 and patch_keep_count(65, 0.01) == 64 and patch_keep_count(63, 0.5) == 31
    assert patch_keep_count(1, 0.99) == 1 and patch_keep_count(2, 0.75) == 1
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            patch_keep_count(64, bad)


def test_argument_refusals_do_not_launch():
    """K = 0, K > P and a P beyond the LDS layout are refused on the host with a text; dummy non-null addresses, never dereferenced."""
    from xvit import _lib
    lib = _lib.load()
    A = 256
    assert _lib.TOKEN_SELECT_MAX_P >= 4096
    draw = lambda P, K: lib.xvit_token_select_draw(A, A, 4, 2, P, K, 0, 1, None)   # noqa: E731
    assert draw(64, 0) < 0 and b"xvit_token_select_draw" in lib.xvit_last_error_string() and b"K=0" in lib.xvit_last_error_string()
    assert draw(64, 65) < 0 and b"K=65" in lib.xvit_last_error_string()
    assert draw(_lib.TOKEN_SELECT_MAX_P + 1, 64) < 0 and b"too long" in lib.xvit_last_error_string()
    assert lib.xvit_token_select_draw(None, A, 4, 2, 64, 16, 0, 1, None) < 0
    sel = lambda K: lib.xvit_patchify_select(A, 1, A, A, 2, 2, 32, 32, 16, 8, 8, 8, K, None)   # noqa: E731   (P = 32)
    assert sel(0) < 0 and b"xvit_patchify_select" in lib.xvit_last_error_string()
    assert sel(33) < 0
    assert lib.xvit_patchify_select(A, 1, A, A, 2, 2, 32, 30, 16, 8, 8, 8, 4, None) < 0 and b"divisible" in lib.xvit_last_error_string()
    assert lib.xvit_patchify_select(A, 7, A, A, 2, 2, 32, 32, 16, 8, 8, 8, 4, None) < 0          # unknown dtype
    assert lib.xvit_embed_select_fwd(A, A, A, A, 4, 0, 64, None) < 0 and b"xvit_embed_select_fwd" in lib.xvit_last_error_string()
    assert lib.xvit_embed_select_fwd(A, A, A, A, 4, 8, 66, None) < 0                              # d not a multiple of 4
    assert lib.xvit_embed_select_bwd(A, A, A, A, 4, 32, 0, 64, None) < 0 and b"xvit_embed_select_bwd" in lib.xvit_last_error_string()
    assert lib.xvit_embed_select_bwd(A, A, A, A, 4, 32, 33, 64, None) < 0                         # K > P
    assert lib.xvit_embed_select_bwd(A, A, A + 4, A, 4, 32, 8, 64, None) < 0 and b"aligned" in lib.xvit_last_error_string()


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("P,K", [(1, 1), (2, 1), (63, 62), (64, 64), (65, 1), (257, 128), (513, 512)])
def test_restated_draw_is_a_sorted_subset_with_its_inverse(P, K, shared):
    M, B = 3, 4
    keep_idx, slot = T.draw(M * B, B, P, K, shared, seed=77)
    assert keep_idx.shape == (M * B, K) and slot.shape == (M * B, P)
    assert keep_idx.min() >= 0 and keep_idx.max() < P
    assert (np.diff(keep_idx, axis=1) > 0).all()                      # ascending, hence distinct
    for s in range(M * B):
        assert (slot[s, keep_idx[s]] == np.arange(K)).all()           # slot inverts keep_idx ...
        assert (slot[s] >= 0).sum() == K and ((slot[s] == -1) | (slot[s] >= 0)).all()   # ... and marks everything else dropped
    assert (T.slot_of(keep_idx, P) == slot).all()
    k3 = keep_idx.reshape(M, B, K)
    if shared:
        assert (k3 == k3[0]).all()                                    # every modality of a sample keeps the same patches
    elif 1 < K < P and P > 8:
        assert not (k3 == k3[0]).all()
    if K < P:                                                         # another epoch is another draw
        assert not np.array_equal(T.draw(M * B, B, P, K, shared, seed=77, epoch=1)[0], keep_idx) or P <= 2
    assert np.array_equal(T.draw(M * B, B, P, K, shared, seed=77 + T.EPOCH_STRIDE)[0], T.draw(M * B, B, P, K, shared, seed=77, epoch=1)[0])


def test_restated_draw_breaks_key_ties_towards_the_smaller_patch():
    """The seed the GPU test uses for its tie case really holds a tie at the K-th place, and the restatement resolves it by patch index."""
    P, K, seed = TIE["P"], TIE["K"], TIE["seed"]
    k = T.keys(1, 1, P, False, seed)[0]
    order = np.argsort(k, kind="stable")
    a, b = int(order[K - 1]), int(order[K])
    assert k[a] == k[b] and a < b
    keep_idx, slot = T.draw(1, 1, P, K, False, seed)
    assert a in keep_idx[0] and b not in keep_idx[0] and slot[0, a] >= 0 and slot[0, b] == -1


def test_restated_draw_is_uniform():
    """P = 64, K = 16 over 16 384 sequences: each patch's keep count is Binomial(16384, 1/4), sd = sqrt(16384 * 3/16) = 55.4; gate 6 sd."""
    S, P, K = 16384, 64, 16
    keep_idx, _ = T.draw(S, S, P, K, False, seed=2023)
    count = np.bincount(keep_idx.reshape(-1), minlength=P)
    sd = math.sqrt(S * 0.25 * 0.75)
    assert count.sum() == S * K and np.abs(count - S * K / P).max() <= 6 * sd, (count.min(), count.max())


def test_restated_embed_kernels_on_a_hand_example():
    keep_idx = np.array([[0, 2], [1, 2]], dtype=np.int32)             # P = 4: patch 3 kept by nobody, patch 2 by both
    slot = T.slot_of(keep_idx, 4)
    assert slot.tolist() == [[0, -1, 1, -1], [-1, 0, 1, -1]]
    pos = np.arange(5 * 4, dtype=np.float32).reshape(5, 4)
    cls = np.full(4, 100.0, dtype=np.float32)
    x = np.ones((2 * 3, 4), dtype=np.float32)
    y = T.embed_select_fwd(x, cls, pos, keep_idx).reshape(2, 3, 4)
    assert (y[:, 0] == cls + pos[0]).all() and (y[0, 1] == 1 + pos[1]).all() and (y[0, 2] == 1 + pos[3]).all() and (y[1, 1] == 1 + pos[2]).all()
    dx = np.arange(2 * 3 * 4, dtype=np.float32).reshape(6, 4)
    dpos, dcls = T.embed_select_bwd(dx, slot, np.full((5, 4), 0.5, np.float32), np.full(4, 0.25, np.float32), 2)
    d3 = dx.reshape(2, 3, 4)
    assert (dpos[0] == 0.5 + d3[0, 0] + d3[1, 0]).all() and (dcls == 0.25 + d3[0, 0] + d3[1, 0]).all()
    assert (dpos[1] == 0.5 + d3[0, 1]).all() and (dpos[2] == 0.5 + d3[1, 1]).all() and (dpos[3] == 0.5 + d3[0, 2] + d3[1, 2]).all()
    assert (dpos[4] == 0.5).all()
    img = np.arange(1 * 1 * 4 * 4 * 2, dtype=np.float32).reshape(1, 1, 1, 4, 4, 2)
    sel = T.patchify_select(img, (2, 2, 2), np.array([[1, 2]], dtype=np.int32))          # grid Dn = 2, Hn = 2, Wn = 1: t = h * 2 + d
    ref = R.patchify(__import__("torch").from_numpy(img[:, 0, 0]), (2, 2, 2)).numpy()    # the oracle's own index map
    assert (sel[0, 0] == 0).all() and (sel[0, 1] == ref[0, 1]).all() and (sel[0, 2] == ref[0, 2]).all()


def test_model_attributes():
    """A config without the new fields constructs as before (rate 0); with patch_dropout the attribute is None until a training forward."""
    import xvit
    cfg = R.make_config("tiny")
    assert not hasattr(cfg, "patch_dropout")
    plain = xvit.ModelCross(cfg)
    assert plain.patch_dropout == 0.0 and plain.patch_dropout_shared is False and plain.last_token_keep is None
    model = xvit.ModelCross(R.make_config("tiny", patch_dropout=0.5, patch_dropout_shared=True))
    assert model.patch_dropout == 0.5 and model.patch_dropout_shared is True
    assert set(model.state_dict()) == set(plain.state_dict())                     # no new parameters or buffers
    model.eval()
    assert model.last_token_keep is None
    from xvit.graph import _has_dropout
    assert _has_dropout(model) and not _has_dropout(plain)
    import torch
    assert _has_dropout(torch.nn.ModuleList([model])) and not _has_dropout(torch.nn.ModuleList([plain]))     # found inside a container, too
    with pytest.raises(ValueError):
        xvit.ModelCross(R.make_config("tiny", patch_dropout=1.0))
