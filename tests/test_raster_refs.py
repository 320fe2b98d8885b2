"""CPU-only: the restatement of the rasteriser's definition (tests/raster_refs.py) held to itself - its float32 run against its float64 run, a
second per-pixel formulation, the winding of the library's own meshes, the fill rule, and the figure the GPU chain test takes its margin from.

Measured here (printed by the tests):
    fp32 against fp64, face maps of 5 views: 0 of 3 840 pixels differ at grid (9,11,13) / image 24 x 32, 1 of 15 360 at (17,19,23) / 48 x 64
    chain (tsdf_refs.Case((24,32),(9,11,13)) -> masked_mesh -> render, float64): the median |mesh depth - analytic depth| over jointly valid pixels is
    CHAIN_MEDIAN below
"""
import functools

import numpy as np
import pytest
import torch

import raster_refs as R
import tsdf_refs as T

CHAIN_MEDIAN = R.CHAIN_MEDIAN


@functools.lru_cache(maxsize=None)
def _sphere(shape):
    return R.sphere_mesh(shape)


@pytest.mark.parametrize("shape,hw", [((9, 11, 13), (24, 32)), ((17, 19, 23), (48, 64))])
def test_float32_run_against_float64_run(shape, hw):
    V, F, C = _sphere(shape)
    H, W = hw
    _, _, w2c, K, _ = R.rig(H, W, 5, True)
    a = R.render_views(V, F, C, w2c, K, H, W, dtype=np.float32)
    b = R.render_views(V, F, C, w2c, K, H, W, dtype=np.float64)
    differ = int((a["face"] != b["face"]).sum())
    same = (a["face"] == b["face"]) & (a["face"] >= 0)
    derr = float(np.abs(a["depth"][same].astype(np.float64) - b["depth"][same]).max())
    cerr = int(np.abs(a["colors"][same].astype(int) - b["colors"][same].astype(int)).max())
    print(f"\n{shape} {hw}: V {len(V)} T {len(F)}, covered {float((b['face'] >= 0).mean()):.3f}, face maps differ on {differ} of {a['face'].size} pixels "
          f"({100 * differ / a['face'].size:.4f} %), max |d32 - d64| {derr:.2e}, max colour difference {cerr}")
    assert (b["face"] >= 0).mean() > 0.1 and differ <= 0.001 * a["face"].size
    # where the two runs pick the same face they may still have snapped a corner one sub-pixel step (1/256 pixel) apart: a face spans at least about a
    # pixel and at most the sphere's radius (120) in depth and 255 colour levels, so the step moves z by < 120 / 256 and a byte by < 1 level (+ 1 rounding)
    assert derr < 120.0 / 256.0 and cerr <= 2
    assert a["depth"].dtype == np.float32 and ((a["face"] < 0) == (a["depth"] == 0)).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_per_pixel_formulation_equals_the_per_face_one(dtype):
    V, F, C = _sphere((9, 11, 13))
    H, W = 24, 32
    _, _, w2c, K, _ = R.rig(H, W, 5, True)
    for m in (0, 3):
        for cull in (0, 1, -1):
            a = R.render(V, F, C, w2c[m], K[m], H, W, dtype=dtype, cull=cull)
            b = R.render_pixels(V, F, C, w2c[m], K[m], H, W, dtype=dtype, cull=cull)
            assert (a["face"] == b["face"]).all() and (a["depth"] == b["depth"]).all() and (a["colors"] == b["colors"]).all()
            assert (a["face"] >= 0).any()


def test_a_closed_sphere_seen_from_outside_wins_with_negative_areas():
    V, F, C = _sphere((9, 11, 13))
    H, W = 24, 32
    _, _, w2c, K, _ = R.rig(H, W, 5, True)
    both = R.render_views(V, F, C, w2c, K, H, W, dtype=np.float32)
    back = R.render_views(V, F, C, w2c, K, H, W, dtype=np.float32, cull=1)
    for m in range(5):
        win = np.unique(both["face"][m][both["face"][m] >= 0])
        assert len(win) > 20 and (both["area"][m][win] < 0).all()                        # the front faces of the library's own meshes: A < 0
        assert (both["area"][m] > 0).any()                                              # (the far side is there, and loses)
    for k in ("depth", "face", "colors"):
        assert both[k].tobytes() == back[k].tobytes()                                   # cull=+1 is back-face culling: the same bytes
    front = R.render_views(V, F, C, w2c, K, H, W, dtype=np.float32, cull=-1)
    assert (front["face"] != both["face"]).any() and ((front["face"] >= 0) == (both["face"] >= 0)).mean() > 0.95


@pytest.mark.parametrize("flip", [False, True])
def test_fill_rule_on_a_quad(flip):
    V, F = R.quad()
    if flip:
        F = F[:, ::-1].copy()                               # the other winding: the setup swaps it back
    H, W = 14, 16
    w2c, K = np.linalg.inv(R.EYE_C2W)[:, :3, :4], R.EYE_K
    for dtype in (np.float32, np.float64):
        o = R.render(V, F, None, w2c[0], K[0], H, W, dtype=dtype)
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        inside = (x >= 2) & (x <= 9) & (y >= 2) & (y <= 9)  # the left and top borders belong to the quad, the right and bottom ones do not
        assert (o["hits"] == inside).all()                  # every pixel once: no hole and no double hit along the diagonal
        # the diagonal runs up-left for face 0 (its interior lies to the right): a left edge, which owns its pixels
        want = np.where(inside, np.where(x >= y, 0, 1), -1)
        assert (o["face"] == want).all()
        assert (o["depth"][inside] == 4.0).all() and (o["depth"][~inside] == 0).all()


def test_chain_figure():
    """tsdf_refs.Case((24,32),(9,11,13)) -> masked_mesh of its float64 volume -> render into the case's own cameras, float64: the median |mesh depth - analytic
    depth| over the pixels both cover.  Measured: 1.1783 world units (the grid's voxels are 25 to 39 units wide and the truncation is 30) with 22.7 % of the
    pixels jointly valid, 527 vertices and 757 faces.  CHAIN_MEDIAN is that figure; the GPU chain test allows 2 x CHAIN_MEDIAN."""
    c = T.Case((24, 32), (9, 11, 13))
    o = c.o64
    m = T.masked_mesh(torch.from_numpy(-o["tsdf"]), 0.0, o["weight"] >= 1, box=torch.from_numpy(c.box), dtype=torch.float64)
    V, F = m["vertices"].numpy(), m["faces"].numpy()
    assert len(F) > 100
    r = R.render_views(V, F, None, c.w2c32, c.K32, 24, 32, dtype=np.float64)
    both = (r["face"] >= 0) & (c.g["label"] >= 0)
    med = float(np.median(np.abs(r["depth"][both] - c.g["depth"][both])))
    print(f"\nchain: V {len(V)} T {len(F)}, jointly valid {float(both.mean()):.3f}, median |mesh depth - analytic depth| {med:.4f}")
    assert both.mean() > 0.2 and abs(med - CHAIN_MEDIAN) < 1e-3
