"""CPU-only: tests/resample_refs.py, the yardstick of tests/test_gpu_resample.py, is Pillow's 8-bit resampler - equal to the bytes Pillow wrote into
tests/golden/caseG_resample.npz, and to live Pillow where it is importable - and the tables mvsnerf_amd.ops builds for the kernels are the restatement's."""
import numpy as np
import pytest

from tests import resample_refs as R

CHANNELS = (3, 4)


@pytest.fixture(scope="module")
def golden():
    return R.golden()


def test_the_cases_are_the_agreed_ones():
    assert len(R.CASES) == 10 and ((20, 126), (20, 30)) in R.CASES and ((5, 1100), (3, 300)) in R.CASES and ((1100, 5), (300, 3)) in R.CASES
    assert ((9, 9), (9, 9)) in R.CASES
    assert R.tables(126, 30, "lanczos")[2] == 27                                 # the factor-4.2 window
    # Pillow 12 resizes only the 1100 x 5 image vertically first (R.pillow_order_differs): every other case is in the golden
    assert [c for c in R.CASES if c not in R.GOLDEN_CASES] == [((1100, 5), (300, 3))]
    for hw, _ in R.CASES:                                                        # the alpha planes hold the values the unpremultiply branches on
        assert set(np.unique(R.case_image(hw, 4)[..., 3])) <= set(R.ALPHAS)
    assert set(np.unique(R.case_image((37, 53), 4)[..., 3])) == set(R.ALPHAS)


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("flt", R.FILTERS)
@pytest.mark.parametrize("case", R.GOLDEN_CASES, ids=lambda c: R.case_name(*c, 0)[:-3])
def test_restatement_equals_the_golden_bytes(golden, case, flt, channels):
    hw, out_hw = case
    name = R.case_name(hw, out_hw, channels)
    img = golden["in_" + name]
    assert np.array_equal(img, R.case_image(hw, channels))                       # the stored input is the generator's
    want = golden[f"{flt}_{name}"]
    assert want.shape == out_hw + (channels,) and want.dtype == np.uint8
    assert np.array_equal(R.resize(img, out_hw, flt), want)


def test_restatement_equals_live_pillow(golden):
    PIL = pytest.importorskip("PIL")
    from tests.gen_golden_resample import pillow_resize
    n = 0
    for hw, out_hw in R.GOLDEN_CASES + (((33, 21), (40, 8)), ((6, 6), (19, 19))):
        for channels in CHANNELS:
            img = R.case_image(hw, channels, seed=1)
            for flt in R.FILTERS:
                assert np.array_equal(R.resize(img, out_hw, flt), pillow_resize(img, out_hw, flt)), (PIL.__version__, hw, out_hw, channels, flt)
                n += 1
    assert n == 44


def test_premultiply_round_trip_branches():
    px = np.array([[[200, 100, 7, a] for a in R.ALPHAS]], dtype=np.uint8)
    pre = R.premultiply(px)
    assert np.array_equal(pre[0, 0], [0, 0, 0, 0]) and np.array_equal(pre[0, 1], [200, 100, 7, 255]) and np.array_equal(pre[0, 2], [1, 0, 0, 1])
    un = R.unpremultiply(np.array([[[9, 3, 0, 0], [9, 3, 0, 255], [200, 100, 7, 128], [5, 1, 0, 1]]], dtype=np.uint8))
    assert np.array_equal(un[0, 0], [9, 3, 0, 0]) and np.array_equal(un[0, 1], [9, 3, 0, 255])        # copies
    assert np.array_equal(un[0, 2], [255, 199, 13, 128]) and np.array_equal(un[0, 3], [255, 255, 0, 1])   # 255 c // a, clamped


@pytest.mark.parametrize("flt", R.FILTERS)
def test_ops_tables_are_the_restatements(flt):
    from mvsnerf_amd import ops
    sizes = {(n_in, n_out) for (h, w), (ho, wo) in R.CASES for n_in, n_out in ((h, ho), (w, wo)) if n_in != n_out}
    sizes |= {(1600, 640), (1200, 512), (800, 400), (3, 1), (1, 5)}
    for n_in, n_out in sorted(sizes):
        win, kk, ks = ops._resample_tables(n_in, n_out, flt)
        e_win, e_kk, e_ks = R.tables(n_in, n_out, flt)
        assert ks == e_ks and win.dtype == np.int32 and kk.dtype == np.int32
        assert np.array_equal(win, e_win) and np.array_equal(kk, e_kk), (n_in, n_out)
        assert ops._resample_tables(n_in, n_out, flt)[1] is kk                   # cached
        # what the kernels' guard asks of a window, and Pillow's int32 accumulator
        assert (win[:, 0] >= 0).all() and (win[:, 1] >= 1).all() and (win[:, 1] <= ks).all() and (win.sum(1) <= n_in).all()
        assert int(np.abs(kk.astype(np.int64)).sum(1).max()) * 255 + 2 ** 21 < 2 ** 31
