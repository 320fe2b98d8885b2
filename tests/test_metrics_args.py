"""CPU-only: the surface and argument handling of the frame-metrics entries (mvsnerf_frame_metrics_fwd, mvsnerf_frame_metrics_workspace_bytes)
and of their Python faces.  Every call here is rejected before the first launch: there is no GPU, and the pointers are made-up addresses that
nothing may dereference."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from mvsnerf_amd import _lib

OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
PTR = 0x10000        # non-NULL, 16-byte aligned, never dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mvsnerf_frame_metrics_fwd", "mvsnerf_frame_metrics_workspace_bytes")
TILE_H, TILE_W = 16, 32    # window origins per workgroup (csrc/metrics.hip)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _row():
    src = open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read()
    return int(re.search(r"#define\s+MVSNERF_METRICS_ROW\s+(\d+)", src).group(1))


def test_new_exports_are_bound_and_exported(lib):
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    for n in NEW:
        assert n in names and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.mvsnerf_abi_version() == 12                      # internal tier: no ABI bump
    from mvsnerf_amd import ops
    assert ops.METRICS_ROW == _row() == 15
    assert [ops.M_SSE, ops.M_N, ops.M_SSE_CROP, ops.M_N_CROP, ops.M_SSE_MASK, ops.M_N_MASK, ops.M_SSIM0, ops.M_SSIM1, ops.M_SSIM2, ops.M_N_SSIM,
            ops.M_ABS_ERR, ops.M_ACC0, ops.M_ACC1, ops.M_ACC2, ops.M_N_DEPTH] == list(range(15))


def _tiles(H, W):
    return -(-H // TILE_H) * -(-W // TILE_W)


@pytest.mark.parametrize("K,H,W,win", [(1, 7, 7, 7), (1, 16, 32, 3), (1, 17, 33, 7), (3, 38, 45, 11), (8, 512, 640, 7), (2, 70, 33, 5), (1, 11, 4000, 9)])
def test_workspace_is_one_row_per_frame_and_tile(lib, K, H, W, win):
    n = lib.mvsnerf_frame_metrics_workspace_bytes(K, H, W, win)
    row_bytes = _row() * 8
    assert n > 0 and n % row_bytes == 0
    assert n == K * _tiles(H, W) * row_bytes


def test_workspace_grows_with_the_tile_count(lib):
    f = lib.mvsnerf_frame_metrics_workspace_bytes
    assert f(1, 16, 32, 7) < f(1, 17, 32, 7) == f(1, 16, 33, 7) < f(1, 17, 33, 7) < f(2, 17, 33, 7)
    assert f(1, 16, 32, 3) == f(1, 16, 32, 11)                  # the window changes the halo, not the tiling


def test_workspace_query_refuses_what_the_entry_refuses(lib):
    for bad in ((0, 64, 64, 7), (1, 0, 64, 7), (1, 64, 0, 7), (1, 64, 64, 6), (1, 64, 64, 1), (1, 64, 64, 13), (1, 6, 64, 7), (1, 64, 10, 11), (-1, 64, 64, 7)):
        assert lib.mvsnerf_frame_metrics_workspace_bytes(*bad) == 0, bad


THR = (ctypes.c_double * 3)(0.01, 0.05, 0.1)


def _call(lib, pred=PTR, gt=PTR, dp=PTR, dg=PTR, K=2, H=64, W=96, win=7, thr=THR, out=PTR, ws=PTR):
    return lib.mvsnerf_frame_metrics_fwd(pred, gt, dp, dg, K, H, W, win, 2.0, 0.01, 0.03, 1.0 / 200.0, thr, out, ws, None)


def test_argument_codes(lib):
    for f in ("pred", "gt", "out", "ws"):
        assert _call(lib, **{f: 0}) == EINVAL, f
    assert _call(lib, thr=None) == EINVAL
    assert _call(lib, dp=0) == EINVAL and _call(lib, dg=0) == EINVAL          # the depth maps come together (both NULL is the no-depth call)
    for K in (0, -1):
        assert _call(lib, K=K) == EINVAL
    assert _call(lib, H=0) == EINVAL and _call(lib, W=-3) == EINVAL
    for win in (4, 6, 8, 10, 2, 0):                                             # even
        assert _call(lib, win=win) == EINVAL, win
    for win in (1, 13, 15, -7):                                                 # odd, outside 3..11
        assert _call(lib, win=win) == EINVAL, win
    # min(H, W) < win_size: an unsupported shape, not an invalid argument
    assert _call(lib, H=6, W=96, win=7) == EUNSUPPORTED
    assert _call(lib, H=64, W=10, win=11) == EUNSUPPORTED
    assert _call(lib, H=2, W=2, win=3) == EUNSUPPORTED
    # an invalid window is reported before the shape it does not fit
    assert _call(lib, H=2, W=2, win=4) == EINVAL
    # alignment: floats on 4 bytes (a frame of a batch of odd-sized frames is a valid input), doubles on 8
    for f in ("pred", "gt", "dp", "dg"):
        assert _call(lib, **{f: PTR + 2}) == EALIGN, f
    assert _call(lib, out=PTR + 4) == EALIGN and _call(lib, ws=PTR + 4) == EALIGN
    # more workgroups than a grid holds
    assert _call(lib, K=1 << 20, H=1 << 14, W=1 << 14) == EUNSUPPORTED


def test_python_faces_refuse_cpu_tensors_and_bad_shapes():
    from mvsnerf_amd import evaluate, ops
    a = torch.rand((20, 24, 3))
    for fn in (ops.frame_metrics, evaluate.frame_metrics, evaluate.ssim_hip):
        with pytest.raises(RuntimeError, match="frame_metrics"):
            fn(a, a)
    with pytest.raises(RuntimeError, match="frame_metrics"):
        ops.frame_metrics(a, torch.rand((20, 25, 3)))
    with pytest.raises(RuntimeError, match="frame_metrics"):
        ops.frame_metrics(a.permute(2, 0, 1), a.permute(2, 0, 1))
    with pytest.raises(RuntimeError, match="frame_metrics"):
        ops.frame_metrics(a, a, depth_gt=torch.rand((20, 24)))
    # the centre crop of a frame under 10 pixels is empty: the same ValueError as psnr_center_crop, known from the shape alone
    small = torch.rand((7, 7, 3))
    with pytest.raises(ValueError) as e1:
        evaluate.psnr_center_crop(small, small)
    with pytest.raises(ValueError) as e2:
        evaluate.frame_metrics(small, small)
    assert str(e1.value) == str(e2.value)
