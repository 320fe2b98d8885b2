"""CPU-only: the float64 yardstick of the depth-fusion kernels (tests/depth_fusion_refs.py) behaves as the definition says on the analytic rig - consistent
where the surfaces are visible, inconsistent where a depth is off by 3 %, exact on the fronto-parallel plane - and its compaction walks the pixels in
np.nonzero's order."""
import numpy as np
import pytest

import depth_fusion_refs as R

H, W, M = 24, 40, 5


@pytest.fixture(scope="module")
def rig():
    g = R.make_rig(H, W, M)
    w2c = np.linalg.inv(g["c2w"])[:, :3, :4]
    return g, w2c


def _interior(label, r=2):
    """pixels whose (2r+1)^2 neighbourhood (clipped at the border) carries one label: away from the sphere's silhouette"""
    Hh, Ww = label.shape
    out = np.ones(label.shape, bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            yy, xx = np.clip(np.arange(Hh) + dy, 0, Hh - 1), np.clip(np.arange(Ww) + dx, 0, Ww - 1)
            out &= label[yy][:, xx] == label
    return out


def _one_surface(label, x0, y0):
    return (label[y0, x0] == label[y0, x0 + 1]) & (label[y0, x0] == label[y0 + 1, x0]) & (label[y0, x0] == label[y0 + 1, x0 + 1])


def _pure(ref, g, src, seen):
    """pixels all of whose agreeing sources were read from a cell on the pixel's own surface (a cell that straddles the silhouette interpolates between
    the sphere's depth and the plane's: it can agree within rel_thr and still pull the average)"""
    out = np.ones(seen.shape, bool)
    for r in range(M):
        for j, s in enumerate(src[r]):
            if s < 0:
                continue
            p = ref.pairs(r, int(s))
            own = _one_surface(g["label"][s], p["x0"], p["y0"]) & (g["label"][s][p["y0"], p["x0"]] == g["label"][r])
            out[r] &= own | (((seen[r] >> np.uint32(j)) & 1) == 0)
    return out


def test_clean_rig_is_consistent_away_from_the_silhouette(rig):
    g, w2c = rig
    ref = R.Reference(g["depth"], g["c2w"][:, :3], w2c, g["K"])
    n = 0
    for r in range(M):
        for s in range(M):
            if s == r:
                continue
            p = ref.pairs(r, s)
            c = ref.consistent(p, 1.0, 0.01)
            # the four taps and the pixel itself lie on one surface, none of them within two pixels of the silhouette
            inter_s, lab_s = _interior(g["label"][s]), g["label"][s]
            x0, y0 = p["x0"], p["y0"]
            clean = p["taps_ok"] & _interior(g["label"][r])
            for dy in (0, 1):
                for dx in (0, 1):
                    clean &= inter_s[y0 + dy, x0 + dx] & (lab_s[y0 + dy, x0 + dx] == g["label"][r])
            assert clean.sum() > 0
            assert c[clean].all(), (r, s, float(p["err"][clean & ~c].max()), float(p["rel"][clean & ~c].max()))
            n += int(clean.sum())
    assert n > 0.5 * M * (M - 1) * H * W * 0.5          # the statement covers most pairs, not a corner of the rig


def test_scaled_block_agrees_with_nothing(rig):
    g, w2c = rig
    depth = g["depth"].copy()
    blk = (slice(6, 16), slice(8, 24))
    depth[2][blk] *= 1.03
    ref = R.Reference(depth, g["c2w"][:, :3], w2c, g["K"])
    inblk = np.zeros((H, W), bool)
    inblk[blk] = True
    for s in (0, 1, 3, 4):
        # (a cell that straddles the silhouette interpolates between the sphere's depth and the plane's and can meet any depth by accident, and at the
        #  sphere's limb the surface runs along the ray: the statement is about pixels away from the silhouette and cells whose four taps lie on one surface)
        p = ref.pairs(2, s)
        one = inblk & _interior(g["label"][2]) & ~(p["taps_ok"] & ~_one_surface(g["label"][s], p["x0"], p["y0"]))
        assert one.sum() > 0.5 * inblk.sum()
        assert not ref.consistent(p, 1.0, 0.01)[one].any()                         # the block agrees with no view
        p = ref.pairs(s, 2)
        x0, y0 = p["x0"], p["y0"]
        all_in = p["inside"] & inblk[y0, x0] & inblk[y0, x0 + 1] & inblk[y0 + 1, x0] & inblk[y0 + 1, x0 + 1] & _one_surface(g["label"][2], x0, y0)
        assert all_in.sum() > 0
        assert not ref.consistent(p, 1.0, 0.01)[all_in].any()                      # and no view agrees with it


def test_fused_depth_of_a_clean_plane_pixel_is_its_ray_cast_depth(rig):
    g, w2c = rig
    ref = R.Reference(g["depth"], g["c2w"][:, :3], w2c, g["K"])
    src = R.default_src_ids(M, 4)
    seen, fused, mask = ref.consistency(src, 1.0, 0.01, 3)
    clean = (g["label"] == 0) & (R.popcount(seen) >= 1) & _pure(ref, g, src, seen)
    assert clean.sum() > 0.3 * M * H * W
    assert np.abs(fused[clean] / g["depth"][clean] - 1.0).max() < 1e-9
    assert (mask == ((R.popcount(seen) >= 3) & ref.usable)).all()


def test_compaction_order_and_counts_are_those_of_nonzero(rig):
    g, w2c = rig
    ref = R.Reference(g["depth"], g["c2w"][:, :3], w2c, g["K"])
    src = R.default_src_ids(M, 4)
    seen, fused, mask = ref.consistency(src, 1.0, 0.01, 3)
    pts, col, nv, idx = ref.compact(mask, fused, seen, g["images"])
    want = np.nonzero(mask.reshape(-1))[0]
    assert 0 < len(want) < mask.size
    assert (idx == want).all() and len(pts) == len(col) == len(nv) == len(want)
    assert (col == g["images"].reshape(-1, 3)[want]).all()
    assert (nv == R.popcount(seen).reshape(-1)[want]).all()
    # points: o + d * fused of the pixel, and so on the plane where the pixel sees the plane
    on_plane = ((g["label"] == 0) & _pure(ref, g, src, seen)).reshape(-1)[want]
    assert on_plane.sum() > 0.3 * len(want)
    assert np.abs(pts[on_plane, 2] - R.PLANE_Z).max() < 1e-6
    e = ref.compact(np.zeros_like(mask), fused, seen, g["images"])
    assert e[0].shape == (0, 3) and e[3].shape == (0,)


def test_float32_restatement_is_close_to_float64(rig):
    """the switch the GPU tests take their margins from: same statements, single precision"""
    g, _ = rig
    c2w32, w2c32 = R.rounded_cameras(g["c2w"])
    K32, d32 = g["K"].astype(np.float32), g["depth"].astype(np.float32)
    r64, r32 = R.Reference(d32, c2w32, w2c32, K32), R.Reference(d32, c2w32, w2c32, K32, dtype=np.float32)
    p64, p32 = r64.pairs(0, 3), r32.pairs(0, 3)
    assert p32["err"].dtype == np.float32 and p32["zp"].dtype == np.float32
    both = p64["taps_ok"] & p32["taps_ok"] & (p64["x0"] == p32["x0"]) & (p64["y0"] == p32["y0"])
    assert both.sum() > 100
    assert np.abs(p32["err"][both] - p64["err"][both]).max() < 1e-2 and np.abs(p32["rel"][both] - p64["rel"][both]).max() < 1e-4
