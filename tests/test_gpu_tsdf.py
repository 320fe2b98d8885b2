"""GPU: the TSDF kernels (csrc/tsdf.hip) and the mesher's node mask (csrc/mesh.hip) against the restatements of their definitions (tests/tsdf_refs.py,
DESIGN.md 4o and 4n).

A node whose projection lies within single-precision noise of a pixel boundary, or whose distance lies within it of the truncation band's ends, may take
either verdict, so the volume is compared on DECIDED nodes (tsdf_refs.decided), with margins measured on the very rig under test: m_px = 8 x the largest
|uv32 - uv64| and m_z = 8 x the largest |z32 - z64| of the float32 run of the restatement against its float64 run (test_gpu_depth_fusion.py's convention).
On decided nodes weight and colours equal the float64 restatement exactly and |tsdf - tsdf64| <= 4 x the restatement's own largest |tsdf32 - tsdf64|;
undecided nodes are at most 1 %.  tests/test_tsdf_refs.py lists the measured figures.  The (2,2,2) grid has eight nodes, too few to measure a noise floor on:
it takes the (9,11,13) grid's figures as a floor (the same rig, the same box).  The masked mesher, the vertex colours and the chain are compared exactly.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mesh_refs as MR
import tsdf_refs as T
from mvsnerf_amd import _lib, geometry, ops
from mvsnerf_amd.rays import SceneRays

pytestmark = pytest.mark.gpu
DEV = "cuda"

# name -> (image (H,W), grid (D,H,W), look_at, M, views)
CASES = {
    "9x11x13": ((24, 32), (9, 11, 13), True, 5, None),
    "17x19x23": ((40, 56), (17, 19, 23), True, 5, None),
    "fronto": ((48, 64), (20, 24, 28), False, 5, None),
    "one_cell": ((24, 32), (2, 2, 2), True, 5, None),
    "long_row": ((24, 32), (3, 5, 300), True, 5, None),                  # a row longer than a workgroup, odd sizes everywhere
    "one_view": ((24, 32), (9, 11, 13), True, 1, None),
    "subset": ((24, 32), (9, 11, 13), True, 5, (3, 0, 2)),               # out of order in the bank: integrated in ascending order
}


@functools.lru_cache(maxsize=None)
def _case(name):
    hw, dims, look_at, M, views = CASES[name]
    return T.Case(hw, dims, M=M, look_at=look_at, views=views)


@functools.lru_cache(maxsize=None)
def _volume(name):
    c = _case(name)
    scene = SceneRays(c.rgba, c.g["c2w"], c.g["K"], (300.0, 1000.0), device=DEV)
    assert (c.c2w32 == scene.c2ws.cpu().numpy()).all() and (c.K32 == scene.intrinsics.cpu().numpy()).all() and scene.has_alpha
    args = (scene, torch.from_numpy(c.d32).to(DEV), c.box, c.dims)
    kw = dict(trunc=c.trunc, valid=torch.from_numpy(c.valid).to(DEV), views=None if c.views is None else list(c.views))
    return geometry.fuse_tsdf(*args, **kw), args, kw


@pytest.mark.parametrize("name", list(CASES))
def test_volume_matches_the_float64_definition_on_decided_nodes(name):
    c = _case(name)
    vol, args, kw = _volume(name)
    D, H, W = c.dims
    assert tuple(vol.tsdf.shape) == (D, H, W) and vol.tsdf.dtype == torch.float32 and tuple(vol.weight.shape) == (D, H, W) and vol.weight.dtype == torch.int32
    assert tuple(vol.colors.shape) == (D, H, W, 4) and vol.colors.dtype == torch.uint8 and vol.trunc == c.trunc
    assert torch.equal(vol.box, torch.from_numpy(c.box))
    tsdf, weight, colors = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.colors.cpu().numpy()
    like = _case("9x11x13") if name == "one_cell" else c
    noise = max(c.tsdf_noise, like.tsdf_noise)
    dec = c.decided if like is c else T.decided(c.o64, c.trunc, max(c.m_px, like.m_px), max(c.m_z, like.m_z), c.hw)
    und = 1.0 - float(dec.mean())
    err = float(np.abs(tsdf[dec].astype(np.float64) - c.o64["tsdf"][dec]).max())
    print(f"\n{c.describe()}\n[{name}] GPU: undecided {100 * und:.2f} %, |tsdf - tsdf64| {err:.2e}, tolerance 4 x {noise:.2e}")
    assert und <= 0.01
    assert (weight[dec] == c.o64["weight"][dec]).all()
    assert (colors[dec] == c.o64["colors"][dec]).all()
    assert noise > 0 and err <= 4 * noise, (err, noise)
    assert np.isfinite(tsdf).all() and (tsdf <= 1).all() and (tsdf >= -1).all() and (tsdf[weight == 0] == 1).all()
    assert (colors[..., 3][colors[..., 3] != 0] == 255).all() and (colors[colors[..., 3] == 0] == 0).all()
    assert (weight > 0).any() and (colors[..., 3] == 255).any()
    again = geometry.fuse_tsdf(*args, **kw)                                             # two runs, the same bytes
    assert torch.equal(again.tsdf.view(torch.int32), vol.tsdf.view(torch.int32)) and torch.equal(again.weight, vol.weight)
    assert torch.equal(again.colors, vol.colors)


def test_view_lists_defaults_and_masks():
    c = _case("9x11x13")
    vol, args, kw = _volume("subset")
    bits = lambda v: v.tsdf.view(torch.int32)
    for views in ([0, 2, 3], torch.tensor([2, 3, 0]), np.array([3, 2, 0])):            # any order, any container: the same bytes
        v = geometry.fuse_tsdf(*args, **{**kw, "views": views})
        assert torch.equal(bits(v), bits(vol)) and torch.equal(v.weight, vol.weight) and torch.equal(v.colors, vol.colors)
    full, fargs, fkw = _volume("9x11x13")
    every = geometry.fuse_tsdf(*fargs, **{**fkw, "views": list(range(5))})
    assert torch.equal(bits(every), bits(full)) and torch.equal(every.weight, full.weight)
    assert not torch.equal(vol.weight, full.weight)
    # trunc=None: 3 x the longest voxel edge; a bool mask is the uint8 mask
    auto = geometry.fuse_tsdf(*fargs, valid=fkw["valid"] != 0)
    size = c.box[1].astype(np.float64) - c.box[0]
    assert abs(auto.trunc - 3.0 * max(size[0] / 12, size[1] / 10, size[2] / 8)) < 1e-9
    same = geometry.fuse_tsdf(*fargs, trunc=auto.trunc, valid=fkw["valid"])
    assert torch.equal(bits(auto), bits(same)) and torch.equal(auto.colors, same.colors)
    # z_min: no node nearer than it contributes
    far = geometry.fuse_tsdf(*fargs, **{**fkw, "z_min": 700.0})
    want = (c.o64["hit"] & (c.o64["qz"] > 700.0)).sum(0)
    sure = (np.abs(c.o64["qz"] - 700.0) > 1e-2).all(0) & c.decided
    assert (far.weight.cpu().numpy()[sure] == want[sure]).all() and 0 < int(far.weight.sum()) < int(full.weight.sum())


# ------------------------------------------------------------------ the mesher's node mask
SPHERES = [(30.2, 30.1, 19.7, 12.3), (88.8, 40.4, 18.1, 15.2), (60.5, 33.3, 22.2, 9.1), (110.3, 60.6, 30.9, 6.7), (14.1, 55.2, 13.3, 10.4)]
FIELDS = {
    "odd": ((5, 37, 67), [(20.3, 15.4, 2.3, 6.7), (50.2, 22.2, 1.8, 9.1), (66.0, 36.0, 4.0, 3.3)]),
    "big": ((40, 70, 130), SPHERES),
}
MODES = ("grid", "box", "table")


@functools.lru_cache(maxsize=None)
def _field(name):
    shape, spheres = FIELDS[name]
    f = MR.spheres_field(shape, spheres)
    valid = (np.random.default_rng(7).random(shape) >= 0.1).astype(np.uint8)            # a seeded 10 % of the nodes invalid ...
    valid[:, shape[1] // 2, :] = 0                                                      # ... and one slab
    valid[valid != 0] = np.random.default_rng(8).integers(1, 256, int((valid != 0).sum()))       # any non-zero byte is valid
    return f, valid


def _kw(mode, shape, dev=None):
    if mode == "box":
        return {"box": MR.BOX}
    if mode == "table":
        P = MR.node_table(*shape)
        return {"positions": torch.from_numpy(P).to(dev) if dev else P}
    return {}


@functools.lru_cache(maxsize=None)
def _ref(name, mode):
    f, valid = _field(name)
    return T.masked_mesh(torch.from_numpy(f), 0.0, valid, dtype=torch.float32, **_kw(mode, f.shape))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def _check(mesh, ref):
    V, Tn = ref["count"].tolist()
    assert mesh.count.tolist() == [V, Tn]
    assert tuple(mesh.vertices.shape) == (V, 3) and tuple(mesh.faces.shape) == (Tn, 3)
    assert torch.equal(mesh.vertex_edge.cpu(), ref["vertex_edge"]) and torch.equal(mesh.faces.cpu(), ref["faces"])
    assert _same_bits(mesh.ndc, ref["ndc"]) and _same_bits(mesh.vertices, ref["vertices"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(FIELDS))
def test_masked_mesh_is_the_filtered_restatement_exactly(name, mode):
    f, valid = _field(name)
    ref = _ref(name, mode)
    plain = MR.extract(torch.from_numpy(f), 0.0, dtype=torch.float32)["count"]
    assert 0 < ref["count"][0] < plain[0] and 0 < ref["count"][1] < plain[1]
    d, v = torch.from_numpy(f).to(DEV), torch.from_numpy(valid).to(DEV)
    mesh = geometry.extract_mesh(d, 0.0, valid=v, **_kw(mode, f.shape, DEV))
    _check(mesh, ref)
    _check(geometry.extract_mesh(d, 0.0, valid=v != 0, **_kw(mode, f.shape, DEV)), ref)  # a bool mask


@pytest.mark.parametrize("mode", ["box", "table"])
def test_no_mask_a_full_mask_and_the_old_entry_give_the_same_bytes(mode):
    f, _ = _field("odd")
    D, H, W = f.shape
    d = torch.from_numpy(f).to(DEV)
    kw = _kw(mode, f.shape, DEV)
    a = geometry.extract_mesh(d, 0.0, **kw)
    b = geometry.extract_mesh(d, 0.0, valid=torch.ones((D, H, W), dtype=torch.uint8, device=DEV), **kw)
    V, Tn = a.count.tolist()
    assert V > 0 and Tn > 0
    lib = _lib.lib()
    out = (torch.empty((V, 3), device=DEV), torch.empty((V, 3), device=DEV), torch.empty((V,), device=DEV, dtype=torch.int64),
           torch.empty((Tn, 3), device=DEV, dtype=torch.int32))
    count = torch.zeros((2,), device=DEV, dtype=torch.int64)
    ws = torch.empty((lib.mvsnerf_mesh_workspace_bytes(D, H, W) // 4 + 1,), device=DEV, dtype=torch.int32)
    box = (ctypes.c_float * 6)(*MR.BOX.reshape(-1).tolist()) if mode == "box" else None
    rc = lib.mvsnerf_mesh_extract_fwd(d.data_ptr(), D, H, W, 0.0, kw["positions"].data_ptr() if mode == "table" else 0, box, V, Tn,
                                      *[t.data_ptr() for t in out], count.data_ptr(), ws.data_ptr(), ops.stream_ptr())
    assert rc == 0
    old = geometry.TriangleMesh(out[0], out[1], out[3], out[2], count)
    ref = MR.extract(torch.from_numpy(f), 0.0, dtype=torch.float32, **_kw(mode, f.shape))
    for m in (a, b, old):
        _check(m, ref)


@pytest.mark.parametrize("caps", [(100, 150), (0, 40), (257, 0), "exact", "roomy"])
def test_capacities_of_the_masked_mesher(caps):
    f, valid = _field("big")
    ref = _ref("big", "table")
    V, Tn = ref["count"].tolist()
    cv, cf = (V, Tn) if caps == "exact" else (V + 9, Tn + 11) if caps == "roomy" else caps
    D, H, W = f.shape
    d, v = torch.from_numpy(f).to(DEV), torch.from_numpy(valid).to(DEV)
    P = torch.from_numpy(MR.node_table(D, H, W)).to(DEV)
    lib = _lib.lib()
    pad = 128
    vertices = torch.full((cv + pad, 3), -7.5, device=DEV)
    ndc = torch.full((cv + pad, 3), -7.5, device=DEV)
    vedge = torch.full((cv + pad,), -99, device=DEV, dtype=torch.int64)
    faces = torch.full((cf + pad, 3), -99, device=DEV, dtype=torch.int32)
    count = torch.full((2,), -1, device=DEV, dtype=torch.int64)
    ws = torch.empty((lib.mvsnerf_mesh_workspace_bytes(D, H, W) // 4 + 1,), device=DEV, dtype=torch.int32)
    rc = lib.mvsnerf_mesh_extract_masked_fwd(d.data_ptr(), v.data_ptr(), D, H, W, 0.0, P.data_ptr(), None, cv, cf, vertices.data_ptr() if cv else 0,
                                             ndc.data_ptr() if cv else 0, vedge.data_ptr() if cv else 0, faces.data_ptr() if cf else 0, count.data_ptr(),
                                             ws.data_ptr(), ops.stream_ptr())
    assert rc == 0
    assert count.tolist() == [V, Tn]                                                    # the true totals, whatever the capacity
    nv, nf = min(cv, V), min(cf, Tn)
    assert _same_bits(vertices[:nv], ref["vertices"][:nv]) and _same_bits(ndc[:nv], ref["ndc"][:nv])
    assert torch.equal(vedge[:nv].cpu(), ref["vertex_edge"][:nv]) and torch.equal(faces[:nf].cpu(), ref["faces"][:nf])
    assert bool((vertices[nv:] == -7.5).all()) and bool((ndc[nv:] == -7.5).all()) and bool((vedge[nv:] == -99).all()) and bool((faces[nf:] == -99).all())
    mesh = geometry.extract_mesh(d, 0.0, positions=P, valid=v, capacity=(cv, cf))
    assert mesh.count.tolist() == [V, Tn] and torch.equal(mesh.faces[:nf].cpu(), ref["faces"][:nf]) and _same_bits(mesh.vertices[:nv], ref["vertices"][:nv])
    assert tuple(mesh.vertices.shape) == (cv, 3) and tuple(mesh.faces.shape) == (cf, 3)


# ------------------------------------------------------------------ vertex colours and the chain
def test_vertex_colours_are_their_numpy_statement():
    vol, _, _ = _volume("17x19x23")
    mesh = geometry.tsdf_mesh(vol, colors=False)
    V = int(mesh.count[0])
    assert V > 200 and mesh.colors is None
    tsdf, key = vol.tsdf.cpu().numpy(), mesh.vertex_edge.cpu().numpy()
    got = ops.tsdf_vertex_colors(vol.tsdf, vol.colors, mesh.vertex_edge, mesh.count)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (V, 3)
    assert (got.cpu().numpy() == T.vertex_colors(tsdf, vol.colors.cpu().numpy(), key, V)).all() and int(got.max()) > int(got.min())
    # colours knocked out of a seeded third of the nodes: both ends, one end and neither all occur
    col = vol.colors.clone()
    col[torch.from_numpy(np.random.default_rng(3).random(tuple(vol.tsdf.shape)) < 0.33).to(DEV)] = 0
    D, H, W = vol.tsdf.shape
    d = np.array(MR.EDGES, np.int64)[key & 7]
    up = (key >> 3) + d[:, 0] + d[:, 1] * W + d[:, 2] * H * W
    has = (col.cpu().numpy().reshape(-1, 4)[:, 3] == 255)
    ends = has[key >> 3].astype(int) + has[up]
    assert all((ends == k).sum() > 10 for k in (0, 1, 2))
    got = ops.tsdf_vertex_colors(vol.tsdf, col, mesh.vertex_edge, mesh.count).cpu().numpy()
    assert (got == T.vertex_colors(tsdf, col.cpu().numpy(), key, V)).all() and (got[ends == 0] == 0).all()
    # rows past the count are left 0: a smaller count, and a mesh with spare rows
    short = torch.tensor([V // 3, 0], device=DEV)
    got = ops.tsdf_vertex_colors(vol.tsdf, vol.colors, mesh.vertex_edge, short).cpu().numpy()
    assert (got == T.vertex_colors(tsdf, vol.colors.cpu().numpy(), key, V // 3)).all() and (got[V // 3:] == 0).all() and got[:V // 3].any()
    roomy = geometry.tsdf_mesh(vol, capacity=(V + 37, int(mesh.count[1]) + 5))
    assert tuple(roomy.colors.shape) == (V + 37, 3) and (roomy.colors[V:] == 0).all()
    assert (roomy.colors[:V].cpu().numpy() == T.vertex_colors(tsdf, vol.colors.cpu().numpy(), key, V)).all()
    assert tuple(ops.tsdf_vertex_colors(vol.tsdf, vol.colors, mesh.vertex_edge[:0], mesh.count).shape) == (0, 3)


@pytest.mark.parametrize("min_weight", [1, 3])
def test_fuse_then_mesh_end_to_end(tmp_path, min_weight):
    vol, _, _ = _volume("17x19x23")
    mesh = geometry.tsdf_mesh(vol, min_weight=min_weight)
    weight = vol.weight.cpu().numpy()
    ok = weight >= min_weight
    ref = T.masked_mesh(-vol.tsdf.cpu(), 0.0, ok, box=vol.box, dtype=torch.float32)     # the mesh of the GPU's own volume
    _check(mesh, ref)
    V, Tn = mesh.count.tolist()
    assert V > 200 and Tn > 200 and int(mesh.faces.max()) < V and int(mesh.faces.min()) >= 0
    key = mesh.vertex_edge.cpu().numpy()
    D, H, W = weight.shape
    d = np.array(MR.EDGES, np.int64)[key & 7]
    up = (key >> 3) + d[:, 0] + d[:, 1] * W + d[:, 2] * H * W
    assert ok.reshape(-1)[key >> 3].all() and ok.reshape(-1)[up].all()                   # no vertex on an edge with an unobserved end
    unmasked = geometry.extract_mesh(-vol.tsdf, 0.0, box=vol.box)
    assert int(unmasked.count[0]) > V                                                   # the back of the truncation band is gone
    assert tuple(mesh.colors.shape) == (V, 3)
    assert (mesh.colors.cpu().numpy() == T.vertex_colors(vol.tsdf.cpu().numpy(), vol.colors.cpu().numpy(), key, V)).all()
    # the surface lies in the box and faces the cameras (z < 0 side): the mean normal has a negative z
    v, f = mesh.vertices.cpu().numpy().astype(np.float64), mesh.faces.cpu().numpy()
    lo, hi = vol.box.numpy()
    assert (v >= lo - 1e-3).all() and (v <= hi + 1e-3).all()
    normal = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).sum(0)
    assert normal[2] < 0 and abs(normal[2]) > 5 * max(abs(normal[0]), abs(normal[1]))
    assert geometry.save_ply(str(tmp_path / "tsdf.ply"), mesh) == (V, Tn)
    raw = open(str(tmp_path / "tsdf.ply"), "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert f"element vertex {V}\n".encode() in head and f"element face {Tn}\n".encode() in head and len(body) == 15 * V + 13 * Tn


def test_entries_check_their_arguments():
    c = _case("9x11x13")
    vol, args, kw = _volume("9x11x13")
    scene, depths = args[0], args[1]
    w2c = torch.from_numpy(c.w2c32).to(DEV)
    D, H, W = c.dims
    out = dict(tsdf=torch.full((D, H, W), -5.0, device=DEV), weight=torch.full((D, H, W), -5, device=DEV, dtype=torch.int32),
               colors=torch.full((D, H, W, 4), 9, device=DEV, dtype=torch.uint8))
    lib = _lib.lib()
    box = (ctypes.c_float * 6)(*c.box.reshape(-1).tolist())
    base = dict(depth=depths.data_ptr(), valid=0, images=scene.images.data_ptr(), alpha=1, w2c=w2c.data_ptr(), K=scene.intrinsics.data_ptr(), view_ids=0,
                n_views=0, M=5, H_img=24, W_img=32, box=box, D=D, H=H, W=W, trunc=30.0, z_min=0.0, **{k: v.data_ptr() for k, v in out.items()})
    order = ("depth", "valid", "images", "alpha", "w2c", "K", "view_ids", "n_views", "M", "H_img", "W_img", "box", "D", "H", "W", "trunc", "z_min", "tsdf",
             "weight", "colors")
    call = lambda **k: lib.mvsnerf_tsdf_integrate_fwd(*[{**base, **k}[n] for n in order], ops.stream_ptr())
    for k in ({"depth": 0}, {"images": 0}, {"w2c": 0}, {"K": 0}, {"box": None}, {"tsdf": 0}, {"weight": 0}, {"colors": 0}):
        assert call(**k) == -1, k
    for k in ({"D": 1}, {"W": 1}, {"D": 513, "H": 512, "W": 512}, {"trunc": 0.0}, {"trunc": float("nan")}, {"z_min": -1.0}, {"M": 0}, {"H_img": 0},
              {"view_ids": base["depth"], "n_views": 0}):
        assert call(**k) == -2, k
    for k in ({"depth": base["depth"] + 2}, {"images": base["images"] + 1}, {"w2c": base["w2c"] + 2}, {"tsdf": base["tsdf"] + 2}, {"colors": base["colors"] + 2}):
        assert call(**k) == -3, k
    torch.cuda.synchronize()
    assert bool((out["tsdf"] == -5.0).all()) and bool((out["weight"] == -5).all()) and bool((out["colors"] == 9).all())       # nothing was launched
    assert call() == 0                                                                  # valid = NULL and alpha on: the corrupted rig without its mask
    ref = T.integrate(c.d32, c.w2c32, c.K32, c.rgba, c.box, c.dims, c.trunc, alpha=c.rgba[..., 3])
    assert (out["weight"].cpu().numpy()[c.decided] == ref["weight"][c.decided]).all()
    # an id outside the bank is skipped and reads nothing
    ids = torch.tensor([0, 7, -1, 2, 3], device=DEV, dtype=torch.int32)
    assert call(view_ids=ids.data_ptr(), n_views=5, valid=kw["valid"].data_ptr()) == 0
    sub = _volume("subset")[0]
    assert torch.equal(out["weight"], sub.weight) and torch.equal(out["colors"], sub.colors) and torch.equal(out["tsdf"].view(torch.int32), sub.tsdf.view(torch.int32))
    mesh = geometry.tsdf_mesh(vol, colors=False)
    V = int(mesh.count[0])
    col = torch.full((V, 3), 9, device=DEV, dtype=torch.uint8)
    vc = lambda **k: lib.mvsnerf_tsdf_vertex_colors_fwd(*[{**dict(tsdf=vol.tsdf.data_ptr(), node_colors=vol.colors.data_ptr(), D=D, H=H, W=W,
                                                                   vertex_edge=mesh.vertex_edge.data_ptr(), count=mesh.count.data_ptr(), rows=V,
                                                                   colors=col.data_ptr()), **k}[n]
                                                          for n in ("tsdf", "node_colors", "D", "H", "W", "vertex_edge", "count", "rows", "colors")], ops.stream_ptr())
    assert vc(tsdf=0) == -1 and vc(count=0) == -1 and vc(colors=0) == -1 and vc(rows=-1) == -1 and vc(D=1) == -2 and vc(rows=1 << 31) == -2
    assert vc(tsdf=vol.tsdf.data_ptr() + 2) == -3 and vc(vertex_edge=mesh.vertex_edge.data_ptr() + 4) == -3 and vc(rows=0, vertex_edge=0, colors=0) == 0
    torch.cuda.synchronize()
    assert bool((col == 9).all())
    with pytest.raises(RuntimeError, match="float32"):
        ops.tsdf_vertex_colors(vol.tsdf.double(), vol.colors, mesh.vertex_edge, mesh.count)
    with pytest.raises(RuntimeError, match="valid"):
        ops.mesh_extract(vol.tsdf, 0.0, valid=torch.ones((D, H, W), device=DEV))
