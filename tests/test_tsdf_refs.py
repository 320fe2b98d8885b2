"""CPU-only: the yardstick of the TSDF kernels (tests/tsdf_refs.py) held to its own claims - the fp32 noise floor of the definition on the
rigs the GPU tests use, the sign and scale of the distance on a fronto-parallel plane, what a hole, a mask, a view list and z_min remove, the integer
colour rounding, and the mesher's node mask stated as a post-filter.

Measured here (box (-160,-150,-140)..(160,150,170), trunc 30, 5 views, corrupted inputs):
    rig, grid                          uv noise (px)   z noise    undecided   max |tsdf32 - tsdf64| on decided   weight32 == weight64 on decided
    24 x 32, (9,11,13), look-at        3.2e-06         4.7e-05    0.00 %      9.9e-07                            yes
    40 x 56, (17,19,23), look-at       6.8e-06         4.8e-05    0.05 %      1.5e-06                            yes
    48 x 64, (20,24,28), look-at       7.3e-06         5.5e-05    0.13 %      1.6e-06                            yes
    48 x 64, (20,24,28), fronto        1.2e-05         4.5e-05    0.34 %      1.4e-06                            yes
    48 x 64, (33,37,41), look-at       8.7e-06         4.7e-05    0.13 %      1.6e-06                            yes
"""
import functools

import numpy as np
import pytest
import torch

import depth_fusion_refs as F
import mesh_refs as MR
import tsdf_refs as T

RIGS = {"24x32": ((24, 32), (9, 11, 13), True), "40x56": ((40, 56), (17, 19, 23), True), "48x64": ((48, 64), (20, 24, 28), True),
        "48x64_fronto": ((48, 64), (20, 24, 28), False), "48x64_fine": ((48, 64), (33, 37, 41), True)}
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _case(name):
    hw, dims, look_at = RIGS[name]
    return T.Case(hw, dims, look_at=look_at)


@pytest.mark.parametrize("name", list(RIGS))
def test_the_fp32_restatement_agrees_with_float64_on_decided_nodes(name):
    c = _case(name)
    print(c.describe())
    assert c.undecided_fraction() <= 0.01
    assert c.weights_agree
    dec = c.decided
    assert (c.o32["colors"][dec] == c.o64["colors"][dec]).all() and (c.o32["cw"][dec] == c.o64["cw"][dec]).all()
    # a term of the mean is sdf / trunc: the noise of q.z over trunc, twice for the rounding of d - q.z at depths of several hundred, and a few roundings of
    # numbers <= 1 for the quotient, the sum and the mean
    assert 0 < c.tsdf_noise <= 2 * c.n_z / c.trunc + 16 * U, (c.tsdf_noise, c.n_z)
    o = c.o64
    assert 0.5 < float((o["weight"] > 0).mean()) < 0.9 and 0.03 < float((o["tsdf"] < 0).mean()) < 0.2        # the rig exercises both sides of the surface
    assert (o["tsdf"][o["weight"] == 0] == 1).all() and (o["tsdf"] <= 1).all() and (o["tsdf"] >= -1).all()
    assert o["weight"].dtype == np.int32 and o["weight"].max() <= c.M


def test_sign_and_scale_on_the_fronto_parallel_plane():
    """Unrounded float64 inputs: every camera's optical axis is the world's z axis, so q.z = Z - camera z and a plane pixel's depth is 150 - camera z; a node
    all of whose taps hit the plane has tsdf = min((150 - Z) / trunc, 1), and none further behind the plane than trunc."""
    hw, dims = (48, 64), (20, 24, 28)
    g = F.make_rig(hw[0], hw[1], 5, look_at=False)
    w2c = np.linalg.inv(g["c2w"])[:, :3, :4]
    o = T.integrate(g["depth"], w2c, g["K"], g["images"], T.BOX, dims, T.TRUNC, dtype=np.float64)
    Z = T.node_positions(T.BOX, dims)[2]
    on_plane = np.stack([g["label"][m][o["y"][a], o["x"][a]] == 0 for a, m in enumerate(o["views"])])
    sel = (o["weight"] > 0) & (~o["hit"] | on_plane).all(0)
    assert sel.sum() > 0.3 * sel.size
    want = np.minimum((F.PLANE_Z - Z) / T.TRUNC, 1.0)
    assert (want[sel] >= -1 - 1e-12).all()                                              # nothing past the truncation band
    assert np.abs(o["tsdf"][sel] - want[sel]).max() < 1e-12
    assert (o["tsdf"][sel] > 0).any() and (o["tsdf"][sel] < 0).any()
    assert (Z[sel & (o["tsdf"] < 0)] > F.PLANE_Z).all()                                   # negative behind the plane, seen from the cameras


def test_holes_masks_view_lists_and_z_min_remove_exactly_their_contributions():
    hw, dims = (40, 56), (17, 19, 23)
    g = F.make_rig(hw[0], hw[1], 5, look_at=True)
    c2w32, w2c32 = F.rounded_cameras(g["c2w"])
    K32 = g["K"].astype(np.float32)
    clean = g["depth"].astype(np.float32)
    d32, valid, rgba = T.corrupt(g)
    run = lambda depth, **kw: T.integrate(depth, w2c32, K32, rgba, T.BOX, dims, T.TRUNC, **kw)
    base = run(clean)
    taps = lambda plane: np.stack([plane[m][base["y"][m], base["x"][m]] for m in range(5)])
    with np.errstate(invalid="ignore"):
        bad_depth = ~(np.isfinite(d32) & (d32 > 0))
    for name, o, hole in (("depth", run(d32), bad_depth), ("valid", run(clean, valid=valid), valid == 0),
                          ("alpha", run(clean, alpha=rgba[..., 3]), rgba[..., 3] == 0),
                          ("all", run(d32, valid=valid, alpha=rgba[..., 3]), bad_depth | (valid == 0) | (rgba[..., 3] == 0))):
        gone = base["hit"] & taps(hole)
        assert gone.sum() > 0, name
        assert (o["hit"] == (base["hit"] & ~gone)).all() and (o["near"] == (base["near"] & ~gone)).all(), name
        assert (o["weight"] == (base["hit"] & ~gone).sum(0)).all(), name
        assert (o["x"] == base["x"]).all() and (o["y"] == base["y"]).all()
        assert (o["csum"] == np.where((base["near"] & ~gone)[..., None], np.stack([rgba[m][base["y"][m], base["x"][m], :3] for m in range(5)]), 0).sum(0)).all()
    sub = run(clean, views=[3, 1])                                                      # a list out of order: integrated in ascending order
    assert sub["views"] == [1, 3] and (sub["weight"] == base["hit"][1].astype(np.int32) + base["hit"][3]).all()
    t = np.where(base["hit"][1], np.minimum(base["sdf"][1] / T.TRUNC, 1.0), 0.0) + np.where(base["hit"][3], np.minimum(base["sdf"][3] / T.TRUNC, 1.0), 0.0)
    assert (sub["tsum"] == t).all()
    far = run(clean, z_min=700.0)
    assert (far["hit"] == (base["hit"] & (base["qz"] > 700.0))).all() and 0 < far["hit"].sum() < base["hit"].sum()


def test_colour_rounding_is_exact_integer_rounding():
    o = _case("40x56").o64
    has = o["cw"] > 0
    assert has.any() and (~has).any()
    c, cw, cs = o["colors"].astype(np.int64), o["cw"][..., None], o["csum"]
    assert (o["colors"][~has] == 0).all() and (o["colors"][has][:, 3] == 255).all()
    lo, hi = 2 * c[..., :3] * cw, 2 * (c[..., :3] + 1) * cw                              # c <= csum / cw + 1/2 < c + 1, in integers; a tie rounds up
    assert ((lo <= 2 * cs + cw) & (2 * cs + cw < hi))[has].all()
    # a hand-made node: 3 views, sums 10, 11, 766 -> 3.33 -> 3, 3.67 -> 4, 255.33 -> 255; and a tie 1 / 2 -> 1
    for s, n, want in ((10, 3, 3), (11, 3, 4), (766, 3, 255), (1, 2, 1), (3, 2, 2), (0, 5, 0)):
        assert (2 * s + n) // (2 * n) == want


@pytest.mark.parametrize("mode", ["grid", "box", "table"])
def test_masked_mesh_with_every_node_valid_is_the_plain_extraction(mode):
    f = MR.sphere_field()
    kw = {"box": MR.BOX} if mode == "box" else {"positions": MR.node_table(*f.shape)} if mode == "table" else {}
    a = MR.extract(torch.from_numpy(f), 0.0, dtype=torch.float32, **kw)
    b = T.masked_mesh(torch.from_numpy(f), 0.0, np.ones(f.shape, np.uint8), dtype=torch.float32, **kw)
    for k in ("vertices", "ndc", "vertex_edge", "faces", "count"):
        assert torch.equal(a[k], b[k]), k


def test_masked_mesh_drops_what_touches_an_invalid_node():
    f = MR.sphere_field()
    valid = np.ones(f.shape, np.uint8)
    valid[:, :, 7:] = 0
    a = MR.extract(torch.from_numpy(f), 0.0)
    b = T.masked_mesh(torch.from_numpy(f), 0.0, valid)
    V, Tn = b["count"].tolist()
    assert 0 < V < int(a["count"][0]) and 0 < Tn < int(a["count"][1])
    ok = torch.from_numpy(valid.reshape(-1) != 0)
    assert bool(ok[b["node"]].all()) and bool(ok[b["upper"]].all()) and int(b["faces"].max()) < V and int(b["faces"].min()) >= 0
    assert bool((b["vertex_edge"][1:] > b["vertex_edge"][:-1]).all())
    # the faces that survive are the old faces, renumbered: the same positions
    keep = (ok[a["node"]] & ok[a["upper"]])[a["faces"].long()].all(1)
    assert torch.equal(a["vertices"][a["faces"].long()[keep]], b["vertices"][b["faces"].long()])


def test_vertex_colour_statement():
    tsdf = np.array([[[0.5, -0.5], [0.25, -0.75]], [[1.0, 1.0], [np.nan, -1.0]]], np.float32)
    col = np.zeros((2, 2, 2, 4), np.uint8)
    col[0, 0, 0], col[0, 0, 1], col[0, 1, 0] = (10, 20, 255, 255), (20, 0, 0, 255), (100, 100, 100, 255)
    col[1, 1, 0], col[1, 1, 1] = (0, 0, 0, 255), (200, 100, 51, 255)
    # both ends (t = 0.5) | one end | the other end | a NaN end (t = 0.5) | t = 2, clamped | neither
    key = np.array([0 * 8 + 0, 2 * 8 + 0, 3 * 8 + 2, 6 * 8 + 0, 0 * 8 + 1, 4 * 8 + 0], np.int64)
    got = T.vertex_colors(tsdf, col, key, count=6)
    assert got.tolist() == [[15, 10, 128], [100, 100, 100], [200, 100, 51], [100, 50, 26], [190, 180, 0], [0, 0, 0]]
    cut = T.vertex_colors(tsdf, col, key, count=2)
    assert (cut[2:] == 0).all() and (cut[:2] == got[:2]).all() and cut.shape == (6, 3)
