"""CPU-only: the argument checks of the two deterministic gradient scatters (mvsnerf_volume_sample_bwd_det, mvsnerf_planesweep_costvar_bwd_det) and their
workspace formulas.  Validation happens before any launch, so host buffers are enough (as tests/test_error_behaviour.py does for the forward entries)."""
import ctypes

from mvsnerf_amd import _lib

EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
MAX_POINTS = 1 << 22


def _buf():
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert p % 16 == 0
    return buf, p


def test_volume_scatter_refuses_more_points_than_an_accumulator_word_holds():
    """A voxel channel receives at most one contribution of at most 2^40 per point: 2^22 points keep |sum| <= 2^62, one more is refused before any launch."""
    l = _lib.lib()
    buf, p = _buf()
    assert l.mvsnerf_volume_sample_bwd_det(4, 4, 4, 8, p, MAX_POINTS + 1, p, 8, p, p, 0) == EUNSUPPORTED
    assert l.mvsnerf_volume_sample_bwd_det(4, 4, 4, 8, p, 1 << 40, p, 8, p, p, 0) == EUNSUPPORTED
    assert l.mvsnerf_volume_sample_bwd_det(4, 4, 4, 8, p, 0, p, 8, p, p, 0) == 0                       # an empty input is a no-op
    # the float-atomic entry has no accumulator word to protect: the same count passes its checks (EALIGN is a later check than the count's)
    assert l.mvsnerf_volume_sample_bwd(4, 4, 4, 8, p, MAX_POINTS + 1, p + 4, 8, p, 0) == EALIGN
    # an invalid argument is still reported as such at that size
    assert l.mvsnerf_volume_sample_bwd_det(4, 4, 4, 8, 0, MAX_POINTS + 1, p, 8, p, p, 0) == EINVAL


def test_volume_scatter_rejects_bad_arguments_without_launching():
    l = _lib.lib()
    buf, p = _buf()
    det = l.mvsnerf_volume_sample_bwd_det
    for null in (4, 6, 8, 9):                                                                         # ndc, g, gvol, workspace
        a = [4, 4, 4, 8, p, 1, p, 8, p, p, 0]
        a[null] = 0
        assert det(*a) == EINVAL, null
    assert det(0, 4, 4, 8, p, 1, p, 8, p, p, 0) == EINVAL and det(4, 0, 4, 8, p, 1, p, 8, p, p, 0) == EINVAL and det(4, 4, 0, 8, p, 1, p, 8, p, p, 0) == EINVAL
    assert det(4, 4, 4, 8, p, -1, p, 8, p, p, 0) == EINVAL                                            # negative count
    assert det(4, 4, 4, 8, p, 1, p, 4, p, p, 0) == EINVAL                                             # rows narrower than C
    assert det(4, 4, 4, 0, p, 1, p, 8, p, p, 0) == EUNSUPPORTED and det(4, 4, 4, 6, p, 1, p, 8, p, p, 0) == EUNSUPPORTED      # C: a multiple of 4, >= 4
    assert det(4, 4, 4, 8, p, 1, p, 10, p, p, 0) == EALIGN                                            # row stride: whole 16-byte channel quads
    assert det(4, 4, 4, 8, p, 1, p + 4, 8, p, p, 0) == EALIGN                                         # misaligned g
    assert det(4, 4, 4, 8, p, 1, p, 8, p, p + 4, 0) == EALIGN                                         # workspace: 8-byte words
    assert det(4, 4, 4, 8, p + 4, 0, p, 8, p + 4, p + 8, 0) == 0                                      # ndc, gvol: floats; the workspace: 8 bytes
    # the float-atomic entry: the same checks, no workspace
    atomic = l.mvsnerf_volume_sample_bwd
    assert atomic(4, 4, 4, 8, 0, 1, p, 8, p, 0) == EINVAL and atomic(4, 4, 4, 8, p, 1, p, 4, p, 0) == EINVAL
    assert atomic(4, 4, 4, 6, p, 1, p, 8, p, 0) == EUNSUPPORTED and atomic(4, 4, 4, 8, p, 1, p + 4, 8, p, 0) == EALIGN
    assert atomic(4, 4, 4, 8, p, 0, p, 8, p, 0) == 0


def test_planesweep_scatter_rejects_bad_arguments_without_launching():
    l = _lib.lib()
    buf, p = _buf()
    det = l.mvsnerf_planesweep_costvar_bwd_det
    good = [p, p, p, 3, 32, 8, 8, 4, 1, p, 32, 0, p, p, 0]        # feats, proj, depth, V, C, H, W, D, pad, g_cost, CP, with_img, g_feats, workspace, stream
    assert det(*good[:13], 0, 0) == EINVAL                                                            # no workspace
    assert det(*good[:13], p + 4, 0) == EALIGN                                                        # workspace: 8-byte words
    for null in (0, 1, 2, 9, 12):                                                                     # feats, proj, depth, g_cost, g_feats
        a = list(good)
        a[null] = 0
        assert det(*a) == EINVAL, null
    for at, bad in ((3, 0), (3, 9), (5, 1), (6, 1), (7, 0), (8, -1)):                                  # V in 1..8, H >= 2, W >= 2, D >= 1, pad >= 0
        a = list(good)
        a[at] = bad
        assert det(*a) == EINVAL, (at, bad)
    a = list(good)
    a[4] = 16
    assert det(*a) == EUNSUPPORTED                                                                    # C != 32
    a[0] = 0
    assert det(*a) == EINVAL                                                                          # ... reported after an invalid argument
    atomic = l.mvsnerf_planesweep_costvar_bwd
    assert atomic(0, *good[1:13], 0) == EINVAL and atomic(*good[:5], 1, *good[6:13], 0) == EINVAL
    assert atomic(p, p, p, 3, 16, 8, 8, 4, 1, p, 32, 0, p, 0) == EUNSUPPORTED


def test_workspace_word_formulas():
    l = _lib.lib()
    vol = l.mvsnerf_volume_sample_bwd_det_workspace_words
    assert vol(6, 7, 9, 8) == 8 + 6 * 7 * 9 * 8 and vol(5, 6, 7, 20) == 8 + 5 * 6 * 7 * 20 and vol(1, 1, 1, 4) == 12
    assert vol(128, 176, 208, 8) == 8 + 128 * 176 * 208 * 8
    assert vol(2048, 2048, 2048, 8) == 8 + 2048 ** 3 * 8                                              # past 2^32 words: size_t arithmetic
    assert vol(0, 7, 9, 8) == 0 and vol(6, 0, 9, 8) == 0 and vol(6, 7, 0, 8) == 0                     # 0: no such shape
    assert vol(6, 7, 9, 0) == 0 and vol(6, 7, 9, 6) == 0 and vol(6, 7, 9, 2) == 0
    psw = l.mvsnerf_planesweep_costvar_bwd_det_workspace_words
    assert psw(3, 32, 30, 41) == 2 * 30 * 41 * 32 + 1 and psw(4, 32, 128, 160) == 3 * 128 * 160 * 32 + 1
    assert psw(1, 32, 8, 8) == 1                                                                      # one view: no source views, the two max words only
    assert psw(0, 32, 8, 8) == 0 and psw(3, 16, 8, 8) == 0 and psw(3, 32, 0, 8) == 0 and psw(3, 32, 8, 0) == 0
