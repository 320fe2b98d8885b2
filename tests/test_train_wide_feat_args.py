"""CPU-only: the argument checks of the MLP training entries after feat_dim 36 / 40 (7 / 8 source views) joined them.  Validation happens
before any launch, so the codes can be read without a GPU: F = 42 and odd F stay MVSNERF_EUNSUPPORTED, null pointers stay MVSNERF_EINVAL and
are looked at before F, and an empty batch at F = 34 / 36 / 40 is accepted without a launch (it was MVSNERF_EUNSUPPORTED while the training
kernels stopped at F = 32)."""
import ctypes

import pytest

from mvsnerf_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2
BAD_F = [42, 44, 41, 37, 33, 21, 1, 0]
WIDE_F = [34, 36, 40]


def _host():
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    return buf, p, (ctypes.c_void_p * 11)(*[p] * 11)


@pytest.mark.parametrize("entry", ["mvsnerf_mlp_pack_bwd", "mvsnerf_mlp_pack_bwd_bf16"])
def test_pack_bwd_refuses_unsupported_feat_dims_after_the_null_checks(entry):
    fn = getattr(_lib.lib(), entry)
    buf, p, wp = _host()
    for F in BAD_F:
        assert fn(wp, F, p, 0) == EUNSUPPORTED, F
        assert fn(None, F, p, 0) == EINVAL, F                      # null pointer table: before the F check
        assert fn(wp, F, 0, 0) == EINVAL, F                        # null destination: before the F check
    holes = (ctypes.c_void_p * 11)(*([p] * 5 + [None] + [p] * 5))
    for F in (20, 36, 40):
        assert fn(holes, F, p, 0) == EINVAL, F                     # a null tensor in the table (a supported F: nothing is launched before it is seen)
        assert fn(None, F, p, 0) == EINVAL and fn(wp, F, 0, 0) == EINVAL


@pytest.mark.parametrize("entry", ["mvsnerf_mlp_fwd_train", "mvsnerf_mlp_fwd_bf16_train"])
def test_training_forward_refuses_unsupported_feat_dims_after_the_null_checks(entry):
    fn = getattr(_lib.lib(), entry)
    buf, p, _ = _host()
    lead = (p, p) if entry.endswith("bf16_train") else (p,)         # (packed_bf16, packed_f32) | (packed)
    call = lambda F, N=1, raw=p, saved=p, feat_stride=None: fn(*lead, F, p, 3, p, F if feat_stride is None else feat_stride, p, 3, N, 1, raw, saved, 0)
    for F in BAD_F:
        assert call(F) == EUNSUPPORTED, F
        assert call(F, N=0) == EUNSUPPORTED, F                     # ... for an empty batch too
        assert call(F, raw=0) == EINVAL and call(F, saved=0) == EINVAL, F
        assert fn(*((0,) * len(lead)), F, p, 3, p, F, p, 3, 1, 1, p, p, 0) == EINVAL, F
    for F in WIDE_F + [2, 20, 32]:
        assert call(F, N=0) == 0, F                                # supported: an empty batch is a no-op, nothing is launched
        assert call(F, N=0, feat_stride=F - 1) == EINVAL, F
        assert call(F, N=-1) == EINVAL, F


def test_backward_entry_takes_wide_feature_rows():
    l = _lib.lib()
    buf, p, gp = _host()
    for fn in (l.mvsnerf_mlp_bwd, l.mvsnerf_mlp_bwd_bf16):
        call = lambda F, n_out, N=0: fn(p, p, F, p, p, p, N, 1, p, p, n_out, gp, gp, p, p, 0)
        for F in WIDE_F + [20, 32]:
            assert call(F, 8) == 0, F                                # empty batch
        assert call(36, 36) == 0 and call(40, 40) == 0              # every column of a colour volume
        assert call(36, 40) == EINVAL and call(36, 34) == EINVAL    # more columns than features; not a multiple of four
        for F in (42, 37):
            assert call(F, 8) == EUNSUPPORTED, F
        # F is judged before n_feat_out, and the backward starts at F = 4 (d_feat rows are written four columns at a time): F = 0 was MVSNERF_EINVAL
        # through n_feat_out > F, and F = 2, which the forward and the packs take, had no n_feat_out at all
        for F in (0, 2):
            assert call(F, 8) == EUNSUPPORTED and call(F, 4) == EUNSUPPORTED, F
        assert call(4, 4) == 0 and call(4, 8) == EINVAL
        assert fn(p, p, 20, p, p, p, 0, 0, p, p, 8, gp, gp, p, p, 0) == EUNSUPPORTED and call(20, 8, N=-1) == EUNSUPPORTED     # S = 0, N < 0
        assert fn(0, p, 42, p, p, p, 0, 1, p, p, 8, gp, gp, p, p, 0) == EINVAL


def test_sizes_hold_the_second_block_of_pts_bias():
    """the F-independent size queries cover the wide case: pts_bias^T is two blocks of 32 columns, its weight gradient a 128 x 64 product"""
    l = _lib.lib()
    seg = lambda steps, nb: steps * nb * 64
    assert l.mvsnerf_mlp_packed_bwd_floats() == seg(32, 4) + 6 * seg(64, 4) + 2 * seg(64, 1)
    assert l.mvsnerf_mlp_packed_bwd_bf16_elems() == 8 * (seg(4, 4) + 6 * seg(8, 4) + 2 * seg(8, 1))
    n_out = 128 * 65 + 4 * 128 * 129 + 128 * 193 + 128 * 65 + 128 * 129 + 64 * 161 + 32 * 193
    assert l.mvsnerf_mlp_bwd_workspace_floats() >= 257 * n_out
    assert l.mvsnerf_mlp_saved_floats(128) == 4 * 608 * 64          # the saved-activation format keeps its size: the extra feature slots fill unused ones
    assert l.mvsnerf_abi_version() == 12


def test_wide_column_table():
    """ops._mlp_bwd_maps: the 64-entry table behind the others sends every feature column to exactly one row of [S_FV | S_DR block]"""
    import numpy as np
    from mvsnerf_amd import ops
    for F in (20, 32, 34, 36, 40):
        ops._maps_cache.pop((F, "cpu"), None)
        t = ops._mlp_bwd_maps(F, "cpu").numpy()
        assert t.shape == (1376,)
        narrow, wide = t[320:352], t[1312:1376]
        assert np.array_equal(wide[:32], narrow)
        cols = wide[wide >= 0]
        assert sorted(cols.tolist()) == list(range(F))
        assert (wide[32:36] == -1).all() and (wide[44:] == -1).all()            # the direction slots and the unused ones
        for r in range(32, 64):
            s, h = (r - 32) >> 1, r & 1
            want = h * (F // 2) + 14 + s if 2 <= s < 6 and 14 + s < F // 2 else -1
            assert wide[r] == want, (F, r)
