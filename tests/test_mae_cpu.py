"""CPU: masked-volume pretraining without a GPU: the constructor's refusals, the parameter names, the encoder hand-off, the host-side
argument errors of every new entry point (nothing is launched: dummy aligned addresses are never dereferenced), and the restated
complement against a brute-force np.flatnonzero."""
import numpy as np
import pytest
import torch

import ref_cpu as R
import _mae_check as C
import _tokdrop_check as T


def _cfg(**over):
    return R.make_config("small", **over)          # (32, 32, 16) / (8, 8, 8): P = 32, pd = 512, d = 256, M = 3


def test_constructor_refusals():
    import xvit
    for ratio in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="mask_ratio"):
            xvit.MaskedVolumeModel(_cfg(), decoder_dim=128, mask_ratio=ratio)
    with pytest.raises(ValueError, match="multiple of 64"):
        xvit.MaskedVolumeModel(_cfg(), decoder_dim=96)
    with pytest.raises(ValueError, match="decoder_heads"):
        xvit.MaskedVolumeModel(_cfg(), decoder_dim=128, decoder_heads=4)
    big = _cfg(img_size=(64, 64, 40), patch_size=(2, 2, 2))                          # 32 * 32 * 20 = 20480 patches
    with pytest.raises(ValueError, match="8192"):
        xvit.MaskedVolumeModel(big, decoder_dim=128)


def test_k_equals_p_is_refused():
    import xvit
    import xvit.functional as XF
    assert XF.patch_keep_count(32, 0.01) == 31 and XF.patch_keep_count(1, 0.5) == 1      # the floor drops a patch wherever there are two
    one = _cfg(img_size=(8, 8, 8), patch_size=(8, 8, 8))                             # P = 1: K = max(1, floor(0.5)) = 1 == P
    with pytest.raises(ValueError, match="K == P"):
        xvit.MaskedVolumeModel(one, decoder_dim=128, mask_ratio=0.5)


def test_parameter_names_and_the_encoder_hand_off():
    import xvit
    cfg = _cfg()
    mae = xvit.MaskedVolumeModel(cfg, decoder_dim=128, decoder_depth=2, mask_ratio=0.5)
    assert isinstance(mae.encoder, xvit.ModelCross) and mae.num_kept == 16 and mae.num_dropped == 16
    own = {n: tuple(p.shape) for n, p in mae.named_parameters() if not n.startswith("encoder.")}
    block = {"attn.norm.weight": (128,), "attn.norm.bias": (128,), "attn.fn.to_qkv.weight": (384, 128), "attn.fn.to_out.0.weight": (128, 128),
             "attn.fn.to_out.0.bias": (128,), "ffn.norm.weight": (128,), "ffn.norm.bias": (128,), "ffn.fn.net.0.weight": (512, 128),
             "ffn.fn.net.0.bias": (512,), "ffn.fn.net.3.weight": (128, 512), "ffn.fn.net.3.bias": (128,)}
    want = {"mask_token": (1, 1, 128), "decoder_pos_embed": (1, 33, 128), "decoder_modality_embed": (3, 1, 128), "decoder_embed.weight": (128, 256),
            "decoder_embed.bias": (128,), "decoder_norm.weight": (128,), "decoder_norm.bias": (128,), "decoder_pred.weight": (512, 128),
            "decoder_pred.bias": (512,)}
    want.update({f"decoder_blocks.{i}.{k}": v for i in range(2) for k, v in block.items()})
    assert own == want
    assert mae.decoder_blocks[0].attn.fn.heads == 2
    assert xvit.MaskedVolumeModel(cfg, decoder_dim=128, decoder_mlp_dim=256).decoder_blocks[0].ffn.fn.net[0].weight.shape == (256, 128)
    fresh = xvit.ModelCross(cfg)
    assert set(mae.encoder.state_dict()) == set(fresh.state_dict()) == set(R.make_state_dict(cfg))
    res = fresh.load_state_dict(mae.encoder.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), mae.encoder.state_dict().values()))
    # an existing encoder is taken as it is
    assert xvit.MaskedVolumeModel(fresh, decoder_dim=64).encoder is fresh
    # the graph's predicate sees the mask ratio: every replay of a captured step draws a new mask
    from xvit.graph import _has_dropout
    assert _has_dropout(mae) and not _has_dropout(fresh)


def test_forward_refuses_a_volume_that_requires_grad_and_a_wrong_modality_count():
    import xvit
    mae = xvit.MaskedVolumeModel(_cfg(), decoder_dim=128, mask_ratio=0.5)
    with pytest.raises(RuntimeError, match="requires grad|require grad"):
        mae(torch.zeros(1, 3, 1, 32, 32, 16, requires_grad=True))
    with pytest.raises(ValueError, match="expected"):
        mae(torch.zeros(1, 2, 1, 32, 32, 16))


def test_argument_errors_do_not_launch():
    """Every call below fails a host-side check: callable without a GPU, and on a machine with one nothing is launched."""
    from xvit import _lib
    lib = _lib.load()
    A = 256                                            # any non-null, 16-byte aligned "address"
    err = lib.xvit_last_error_string

    def refused(rc, *words):
        assert rc < 0, rc
        msg = err()
        assert all(w in msg for w in words), msg

    comp = lib.xvit_token_select_complement
    refused(comp(None, A, A, 3, 32, 16, None), b"xvit_token_select_complement", b"null")
    refused(comp(A, A, A, 0, 32, 16, None), b"bad sizes")
    refused(comp(A, A, A, 3, 32, 0, None), b"K=0")
    refused(comp(A, A, A, 3, 32, 32, None), b"K=32")                    # nothing dropped
    refused(comp(A, A, A, 3, 8193, 16, None), b"P=8193 too long")
    fwd = lib.xvit_mae_unshuffle_fwd
    refused(fwd(A, A, A, A, A, None, 6, 2, 32, 16, 128, None), b"xvit_mae_unshuffle_fwd", b"null")
    refused(fwd(A, A, A, A, A, A, 6, 2, 32, 16, 130, None), b"dd %")
    refused(fwd(A, A, A, A, A, A, 7, 2, 32, 16, 128, None), b"S % B")
    refused(fwd(A, A, A, A, A, A, 6, 2, 32, 32, 128, None), b"K < P")
    refused(fwd(A + 4, A, A, A, A, A, 6, 2, 32, 16, 128, None), b"16-byte aligned")
    bwd = lib.xvit_mae_unshuffle_bwd
    refused(bwd(A, A, A, A, A, A, None, 6, 2, 32, 16, 128, None), b"xvit_mae_unshuffle_bwd", b"null")
    refused(bwd(A, A, A, A, A, A, A, 6, 2, 32, 16, 126, None), b"dd %")
    refused(bwd(A, A, A, A, A + 8, A, A, 6, 2, 32, 16, 128, None), b"16-byte aligned")
    for fn, name in ((lib.xvit_token_rows_gather, b"xvit_token_rows_gather"), (lib.xvit_token_rows_scatter, b"xvit_token_rows_scatter")):
        refused(fn(A, None, A, 6, 32, 16, 128, None), name, b"null")
        refused(fn(A, A, A, 6, 32, 32, 128, None), name, b"Rm < P")
        refused(fn(A, A, A, 6, 32, 0, 128, None), name, b"Rm < P")
        refused(fn(A, A, A, 6, 32, 16, 6, None), name, b"dd %")
        refused(fn(A, A, A + 4, 6, 32, 16, 128, None), name, b"16-byte aligned")
    lf = lambda pred, pdt, img, idt, norm, geom, Rm, stats=A: lib.xvit_mae_loss_fwd(pred, pdt, A, img, idt, norm, stats, A, A, A, 2, 3, *geom, Rm, None)   # noqa: E731
    lb = lambda pred, pdt, img, idt, geom, Rm, g=A, dpred=A: lib.xvit_mae_loss_bwd(pred, pdt, A, img, idt, A, g, dpred, 2, 3, *geom, Rm, None)         # noqa: E731
    ok = (32, 32, 16, 8, 8, 8)
    refused(lf(None, 0, A, 0, 1, ok, 16), b"xvit_mae_loss_fwd", b"null")
    refused(lf(A, 0, A, 0, 1, ok, 16, stats=None), b"null")
    refused(lf(A, 7, A, 0, 1, ok, 16), b"dtype")
    refused(lf(A, 0, A, 2, 1, ok, 16), b"dtype")                        # int16 volumes are not scored
    refused(lf(A, 0, A, 0, 1, (32, 32, 15, 8, 8, 8), 16), b"divisible")
    refused(lf(A, 0, A, 0, 1, ok, 32), b"Rm=32")
    refused(lf(A, 0, A, 0, 1, ok, 0), b"Rm=0")
    refused(lf(A, 0, A, 0, 1, (64, 64, 64, 32, 32, 32), 1), b"too large", b"8192")
    refused(lf(A, 0, A, 0, 1, (2, 1, 1, 1, 1, 1), 1), b"norm_pix")      # one voxel per patch has no unbiased variance
    refused(lf(A + 1, 0, A, 0, 1, ok, 16), b"element size")
    refused(lf(A, 1, A + 2, 1, 1, ok, 16), b"element size")             # an fp32 volume at a 2-byte offset
    refused(lb(A, 0, A, 0, ok, 16, g=None), b"xvit_mae_loss_bwd", b"null")
    refused(lb(A, 0, A, 0, ok, 16, dpred=None), b"null")
    refused(lb(A, 1, A, 0, ok, 16, dpred=A + 2), b"element size")
    refused(lb(A, 0, A, 0, ok, 32), b"Rm=32")
    refused(lb(A, 3, A, 0, ok, 16), b"dtype")


@pytest.mark.parametrize("P", [2, 63, 64, 65, 1024, 1025])
def test_restated_complement_against_brute_force(P):
    rng = np.random.default_rng(P)
    for K in sorted({1, max(1, P // 2), P - 1}):
        S = 5
        keep_idx = np.stack([np.sort(rng.choice(P, size=K, replace=False)) for _ in range(S)]).astype(np.int32)
        slot = T.slot_of(keep_idx, P)
        drop_idx, mslot = C.complement(slot, K)
        assert drop_idx.shape == (S, P - K) and drop_idx.dtype == np.int32 and mslot.dtype == np.int32
        for s in range(S):
            want = np.flatnonzero(slot[s] < 0)
            assert np.array_equal(drop_idx[s], want)
            assert np.array_equal(np.flatnonzero(mslot[s] >= 0), want) and np.array_equal(mslot[s][want], np.arange(P - K))
            assert set(drop_idx[s].tolist()) | set(keep_idx[s].tolist()) == set(range(P))
    # a draw of the project's own (xvit_token_select_draw restated) gives the same through both
    keep_idx, slot = T.draw(4, 2, P, max(1, P // 2), False, seed=11)
    drop_idx, _ = C.complement(slot, max(1, P // 2))
    assert all(np.array_equal(drop_idx[s], np.flatnonzero(slot[s] < 0)) for s in range(4))


def test_restated_complement_on_a_row_with_the_wrong_count():
    """The caller's error, with the behaviour the header states: the first Rm dropped patches are listed, the rest read as kept; a short row
    leaves -1 at the end of drop_idx."""
    slot = np.array([[0, -1, -1, -1, 1, -1], [0, 1, 2, 3, -1, 4]], dtype=np.int32)     # K = 3 claimed: 4 and 1 dropped
    drop_idx, mslot = C.complement(slot, 3)
    assert drop_idx.tolist() == [[1, 2, 3], [4, -1, -1]]
    assert mslot.tolist() == [[-1, 0, 1, 2, -1, -1], [-1, -1, -1, -1, 0, -1]]
