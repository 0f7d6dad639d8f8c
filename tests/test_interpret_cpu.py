"""CPU: host-side refusals of xvit_attn_rollout_step (no launch: callable without a GPU) and xvit.interpret.patch_grid, which inverts the
reference's patch-token order (oracle/ref_cpu.py:patchify, model_cross.py:193)."""
import ctypes as C

import pytest
import torch

import ref_cpu as R


def _rollout(lib, q=64, k=64, sb=3 * 768 * 513, sn=3 * 768, lse=64, r_in=4096, r_out=1 << 20, B=2, H=12, N=513, dh=64):
    return lib.xvit_attn_rollout_step(q, k, sb, sn, lse, r_in, r_out, B, H, N, dh, 0.125, None)


def test_rollout_step_argument_errors_do_not_launch():
    """Dummy non-null addresses (never dereferenced): each call is refused on the host, with its reason."""
    from xvit import _lib
    lib = _lib.load()
    err = lambda: lib.xvit_last_error_string()   # noqa: E731
    for dh in (32, 128):
        assert _rollout(lib, dh=dh) < 0
        assert b"xvit_attn_rollout_step" in err() and b"head dim %d unsupported (only 64)" % dh in err(), err()
    for arg in ("q", "k", "lse", "r_in", "r_out"):
        assert _rollout(lib, **{arg: None}) < 0 and b"null pointer" in err(), (arg, err())
    assert _rollout(lib, r_in=4096, r_out=4096) < 0 and b"alias" in err(), err()
    assert _rollout(lib, r_in=4096, r_out=4096 + 4 * 513) < 0 and b"alias" in err(), err()     # overlapping [B, N] ranges
    assert _rollout(lib, sn=3 * 768 + 4) < 0 and b"multiples of 8" in err(), err()
    assert _rollout(lib, sb=3 * 768 * 513 + 2) < 0 and b"multiples of 8" in err(), err()
    for bad in (dict(B=0), dict(H=0), dict(N=0), dict(B=-1)):
        assert _rollout(lib, **bad) < 0 and b"bad B/H/N" in err(), (bad, err())


def test_rollout_step_in_the_ctypes_table():
    from xvit import _lib
    fn = _lib.load().xvit_attn_rollout_step
    assert fn.restype is C.c_int and len(fn.argtypes) == 13


def _id_volume(img_size, patch, seed):
    """A [1, D, H, W] volume whose voxels hold an id of their patch (a random permutation of 0 .. P-1 over the patch grid), and that
    id grid [Dn, Hn, Wn]."""
    grid = [s // p for s, p in zip(img_size, patch)]
    ids = torch.randperm(grid[0] * grid[1] * grid[2], generator=torch.Generator().manual_seed(seed)).to(torch.int32).reshape(grid)
    vol = ids.repeat_interleave(patch[0], 0).repeat_interleave(patch[1], 1).repeat_interleave(patch[2], 2)
    return vol[None], ids


@pytest.mark.parametrize("img_size,patch", [((32, 32, 16), (8, 8, 8)), (R.make_config("ucsf").img_size, R.make_config("ucsf").patch_size)],
                         ids=["32x32x16", "configs2"])
def test_patch_grid_inverts_patchify(img_size, patch):
    from xvit.interpret import patch_grid
    vol, ids = _id_volume(img_size, patch, seed=0)
    tok = R.patchify(vol, patch)                                  # [1, P, pd]: every row holds its patch's id
    assert (tok == tok[:, :, :1]).all()
    back = patch_grid(tok[:, :, 0], img_size, patch)
    assert back.shape == (1, *ids.shape) and torch.equal(back[0], ids)


def test_patch_grid_modalities_and_errors():
    """ModelVIT's N - 1 patch tokens are the M modalities' grids concatenated in order."""
    from xvit.interpret import patch_grid
    img_size, patch = (32, 32, 16), (8, 8, 8)
    vols = [_id_volume(img_size, patch, seed=s) for s in range(3)]
    tok = torch.cat([R.patchify(v, patch)[:, :, 0] for v, _ in vols], dim=1)       # [1, 3 P]
    back = patch_grid(tok, img_size, patch, num_modalities=3)
    assert back.shape == (1, 3, 4, 4, 2)                                            # [.., M, D/8, H/8, W/8]
    for m, (_, ids) in enumerate(vols):
        assert torch.equal(back[0, m], ids)
    with pytest.raises(ValueError, match="patch tokens"):
        patch_grid(torch.zeros(2, 33), img_size, patch)                             # CLS token not dropped
