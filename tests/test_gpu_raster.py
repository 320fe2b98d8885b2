"""GPU: the mesh rasteriser, the face visibility and the mesh filter (csrc/raster.hip) against the restatement of their definition
(tests/raster_refs.py).  Everything is compared EXACTLY with the float32 run of the restatement: face numbers, the bits of the depths, the colour bytes.
tests/test_raster_refs.py holds the restatement to its own float64 run and records the figure the chain test takes its margin from."""
import functools

import numpy as np
import pytest
import torch

import raster_refs as R
import tsdf_refs as T
from mvsnerf_amd import geometry, ops
from mvsnerf_amd.rays import SceneRays

pytestmark = pytest.mark.gpu
DEV = "cuda"

# name -> (grid of the sphere mesh, image (H,W), look_at, M)
RIGS = {
    "9x11x13": ((9, 11, 13), (24, 32), True, 5),
    "17x19x23": ((17, 19, 23), (48, 64), True, 5),
    "fronto": ((9, 11, 13), (24, 32), False, 5),
    "one_view": ((9, 11, 13), (24, 32), True, 1),
}


def _mesh(V, F, C=None, count=None):
    """A TriangleMesh on the device from numpy arrays; ndc and vertex_edge carry recognisable rows"""
    v = torch.from_numpy(np.ascontiguousarray(V, np.float32).reshape(-1, 3)).to(DEV)
    f = torch.from_numpy(np.ascontiguousarray(F, np.int32).reshape(-1, 3)).to(DEV)
    n = torch.tensor([v.shape[0], f.shape[0]] if count is None else list(count), dtype=torch.int64, device=DEV)
    c = None if C is None else torch.from_numpy(np.ascontiguousarray(C, np.uint8)).to(DEV)
    return geometry.TriangleMesh(v, v * 0.5 + 1.0, f, torch.arange(v.shape[0], device=DEV) * 8 + 3, n, c)


@functools.lru_cache(maxsize=None)
def _rig(name):
    shape, (H, W), look_at, M = RIGS[name]
    V, F, C = R.sphere_mesh(shape)
    c2w, K, w2c32, K32, g = R.rig(H, W, M, look_at)
    scene = SceneRays(np.zeros((M, H, W, 3), np.uint8), c2w, K, (300.0, 1000.0), device=DEV)
    assert (K32 == scene.intrinsics.cpu().numpy()).all()
    return V, F, C, w2c32, K32, (H, W), scene, _mesh(V, F, C)


@functools.lru_cache(maxsize=None)
def _ref(name, cull=0, views=None):
    V, F, C, w2c, K, (H, W), _, _ = _rig(name)
    return R.render_views(V, F, C, w2c, K, H, W, views=views, dtype=np.float32, cull=cull)


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t, np.float32)).view(np.int32)


def _same(img, ref):
    """face numbers, depth bits and colour bytes of a MeshImage equal a restatement's"""
    assert img.depth.dtype == torch.float32 and img.face.dtype == torch.int32 and tuple(img.depth.shape) == ref["depth"].shape == tuple(img.face.shape)
    assert (img.face.cpu().numpy() == ref["face"]).all()
    assert (_bits(img.depth) == _bits(ref["depth"])).all()
    if ref["colors"] is None:
        assert img.colors is None
    else:
        assert img.colors.dtype == torch.uint8 and (img.colors.cpu().numpy() == ref["colors"]).all()
    assert torch.equal(img.mask, img.face >= 0) and torch.equal(img.mask, img.depth > 0)


# ------------------------------------------------------------------ (a) the rigs
@pytest.mark.parametrize("cull", [0, 1, -1])
@pytest.mark.parametrize("name", list(RIGS))
def test_rigs_equal_the_float32_restatement(name, cull):
    _, _, _, _, _, _, scene, mesh = _rig(name)
    ref = _ref(name, cull)
    assert (ref["face"] >= 0).mean() > 0.1
    _same(geometry.render_mesh(mesh, scene, cull=cull), ref)


def test_view_lists_and_novel_cameras():
    V, F, C, w2c, K, (H, W), scene, mesh = _rig("9x11x13")
    full = _ref("9x11x13")
    img = geometry.render_mesh(mesh, scene, views=(3, 0, 2))
    assert img.views == [3, 0, 2] and tuple(img.depth.shape) == (3, H, W)
    _same(img, {k: full[k][[3, 0, 2]] for k in ("depth", "face", "colors")})
    _same(geometry.render_mesh(mesh, scene, views=torch.tensor([4])), {k: full[k][[4]] for k in ("depth", "face", "colors")})
    # cameras= instead of a bank: the same cameras give the same bytes; a (3,3) K serves every pose
    g = R.rig(H, W, 5, True)
    _same(geometry.render_mesh(mesh, cameras=(g[0], g[1], (H, W))), full)
    one = geometry.render_mesh(mesh, cameras=(g[0][:, :3], g[1][2], (H, W)))
    ref = R.render_views(V, F, C, w2c, np.repeat(K[2:3], 5, 0), H, W, dtype=np.float32)
    _same(one, ref)
    # a mesh without colours has no colour map; the background fills the holes of one that has
    mesh_nc = _mesh(V, F)
    assert geometry.render_mesh(mesh_nc, scene).colors is None
    bg = geometry.render_mesh(mesh, scene, background=(1, 2, 250))
    hole = ~bg.mask.cpu().numpy()
    assert hole.any() and (bg.colors.cpu().numpy()[hole] == np.array([1, 2, 250], np.uint8)).all()
    # the ops tier skips a view id outside the bank: its slot is empty
    ids = torch.tensor([0, 7, -1, 2], dtype=torch.int32, device=DEV)
    d, f, c = ops.mesh_raster(mesh.vertices, mesh.faces, torch.from_numpy(w2c).to(DEV), scene.intrinsics, (H, W), colors=mesh.colors, views=ids)
    assert (f[1] == -1).all() and (f[2] == -1).all() and (d[1] == 0).all() and (c[2] == 255).all()
    assert (f[0].cpu().numpy() == full["face"][0]).all() and (f[3].cpu().numpy() == full["face"][2]).all()
    n, seen = ops.mesh_face_views(f, len(F), views=ids, n_bank=5)
    want_n, want_seen = R.face_views(f.cpu().numpy(), len(F), views=[0, 7, -1, 2], n_bank=5)
    assert (n.cpu().numpy() == want_n).all() and (seen.cpu().numpy() == want_seen).all() and int(n.max()) == 2


# ------------------------------------------------------------------ (b) hand-made meshes at 40 x 56
HH, HW = 40, 56


def _tri(*corners):
    return [R.at(*c) for c in corners]


def _hand(name):
    """(vertices, faces) of a hand-made mesh in front of the camera at the origin (raster_refs.EYE_*)"""
    if name == "larger_than_the_image":                       # the big-face path and the clipped box; a small face in front of a part of it
        V = _tri((-100, -50, 8.0), (300, -50, 8.0), (-100, 400, 8.0)) + _tri((10.25, 10.5, 4.0), (20.75, 11.0, 4.0), (12.0, 19.5, 4.0))
    elif name == "threshold":                                 # clipped boxes of 15, 16 and 17 pixels in either direction: both kernels, and the border
        V = []
        for k, (w, h) in enumerate(((15, 15), (16, 16), (17, 17), (17, 5), (5, 17), (16, 17), (15, 16))):
            x0, y0 = 1 + 7 * k, 2 + 3 * k
            V += _tri((x0, y0, 4.0 + k % 2 * 4), (x0 + w - 1, y0 + 0.5, 8.0), (x0 + 0.5, y0 + h - 1, 4.0))
    elif name == "quad":
        return R.quad()
    elif name == "coplanar_duplicates":                       # the lower face number wins
        V = _tri((5.5, 3.25, 4.0), (40.0, 8.0, 8.0), (12.0, 30.0, 16.0)) * 2
    elif name == "interpenetrating":
        V = _tri((4.0, 4.0, 2.0), (50.0, 6.0, 16.0), (20.0, 36.0, 8.0)) + _tri((6.0, 30.0, 4.0), (45.0, 2.0, 4.0), (48.0, 38.0, 4.0))
    V = np.array(V, np.float32)
    return V, np.arange(len(V), dtype=np.int32).reshape(-1, 3)


@pytest.mark.parametrize("name", ["larger_than_the_image", "threshold", "quad", "coplanar_duplicates", "interpenetrating"])
def test_hand_made_meshes(name):
    V, F = _hand(name)
    C = np.random.default_rng(5).integers(0, 256, (len(V), 3)).astype(np.uint8)
    w2c = np.linalg.inv(R.EYE_C2W)[:, :3, :4].astype(np.float32)
    for cull in (0, 1, -1):
        ref = R.render_views(V, F, C, w2c, R.EYE_K.astype(np.float32), HH, HW, dtype=np.float32, cull=cull)
        img = geometry.render_mesh(_mesh(V, F, C), cameras=(R.EYE_C2W, R.EYE_K, (HH, HW)), cull=cull)
        _same(img, ref)
    face = geometry.render_mesh(_mesh(V, F, C), cameras=(R.EYE_C2W, R.EYE_K, (HH, HW))).face.cpu().numpy()[0]
    if name == "larger_than_the_image":
        assert (face >= 0).all() and (face == 1).sum() > 20 and (face == 0).sum() > 1000
    elif name == "threshold":
        assert set(np.unique(face)) == {-1, 0, 1, 2, 3, 4, 5, 6}
    elif name == "coplanar_duplicates":
        assert set(np.unique(face)) == {-1, 0}
    elif name == "interpenetrating":
        assert (face == 0).sum() > 50 and (face == 1).sum() > 50
    elif name == "quad":
        assert (face >= 0).sum() == 64


# ------------------------------------------------------------------ (c) bad faces change no pixel
def test_bad_faces_change_no_pixel():
    V, F, C, w2c, K, (H, W), scene, mesh = _rig("9x11x13")
    nv = len(V)
    extra = np.array([[np.nan, 0.0, 0.0],             # nv: a NaN vertex
                      [0.0, 0.0, -2000.0],            # nv + 1: behind every camera (they sit at distance 600 on the z < 0 side, looking at the origin)
                      [0.0, 0.0, -350.0]], np.float32)  # nv + 2: in front of every camera, but nearer than z_min = 300
    V2 = np.concatenate([V, extra])
    C2 = np.concatenate([C, np.full((3, 3), 77, np.uint8)])
    a, b, c = (int(i) for i in F[len(F) // 2])
    bad = np.array([[a, a, b], [a, b, b],                                 # zero area
                    [a, b, nv], [nv, a, b],                               # a NaN vertex
                    [a, b, nv + 1], [nv + 1, c, b],                       # a vertex behind the camera
                    [a, b, nv + 2],                                       # a face straddling z_min (with z_min = 300)
                    [a, b, nv + 3], [-1, a, b], [a, 0x7fffffff, b]], np.int32)       # an index out of range
    F2 = np.concatenate([F, bad])
    for m in range(5):
        assert not R.project(extra, w2c[m], K[m], np.float32, 300.0)[0].any()
        assert R.project(extra, w2c[m], K[m], np.float32, 0.0)[0].tolist() == [False, False, True]   # (the z_min vertex is a good one without z_min)
    for z_min in (300.0,):
        good = geometry.render_mesh(mesh, scene, z_min=z_min)
        both = geometry.render_mesh(_mesh(V2, F2, C2), scene, z_min=z_min)
        assert torch.equal(good.face, both.face) and torch.equal(good.depth.view(torch.int32), both.depth.view(torch.int32)) and torch.equal(good.colors, both.colors)
        ref = R.render_views(V2, F2, C2, w2c, K, H, W, dtype=np.float32, z_min=z_min)
        _same(both, ref)
        assert (ref["area"][:, len(F):] == 0).all() and int(ref["face"].max()) < len(F)   # the restatement dropped every added face whole
    _same(good, _ref("9x11x13"))                                                        # z_min = 300 lies in front of the whole sphere
    # a vertex beyond 2^23 sub-pixels, in front of the camera at the origin: u = 64 x / z + 8 = 65 544 pixels.  At u = 32 768 exactly the vertex is usable.
    Vh, Fh = _hand("interpenetrating")
    Ch = np.random.default_rng(6).integers(0, 256, (len(Vh) + 2, 3)).astype(np.uint8)
    Vb = np.concatenate([Vh, np.array([[4096.0, 0.0, 4.0], R.at(32768.0, 20.0, 4.0)], np.float32)])
    assert R.project(Vb[6:], np.eye(4)[:3], R.EYE_K[0], np.float32)[0].tolist() == [False, True]
    assert R.project(Vb[7:], np.eye(4)[:3], R.EYE_K[0], np.float32)[1].tolist() == [2 ** 23]
    cam = (R.EYE_C2W, R.EYE_K, (HH, HW))
    w2ch = np.linalg.inv(R.EYE_C2W)[:, :3, :4].astype(np.float32)
    good = geometry.render_mesh(_mesh(Vh, Fh, Ch[:6]), cameras=cam)
    far = geometry.render_mesh(_mesh(Vb, np.concatenate([Fh, np.array([[0, 2, 6], [6, 1, 0]], np.int32)]), Ch), cameras=cam)
    assert torch.equal(good.face, far.face) and torch.equal(good.depth.view(torch.int32), far.depth.view(torch.int32)) and torch.equal(good.colors, far.colors)
    Fe = np.concatenate([Fh, np.array([[0, 2, 7]], np.int32)])                             # the vertex on the bound: a sliver across the image, drawn
    edge = geometry.render_mesh(_mesh(Vb, Fe, Ch), cameras=cam)
    _same(edge, R.render_views(Vb, Fe, Ch, w2ch, R.EYE_K.astype(np.float32), HH, HW, dtype=np.float32))
    assert int((edge.face == 2).sum()) > 10
    # z_min between the sphere's near and far side: fragments nearer than it do not count, faces with a vertex nearer than it are dropped
    mid = geometry.render_mesh(mesh, scene, z_min=560.0)
    _same(mid, R.render_views(V, F, C, w2c, K, H, W, dtype=np.float32, z_min=560.0))
    d = mid.depth[mid.mask]
    assert d.numel() > 50 and float(d.min()) > 560.0


# ------------------------------------------------------------------ (d) edge shapes
def test_edge_shapes():
    # a 1 x 1 image
    K1 = np.array([[[FOCAL1, 0.0, 0.0], [0.0, FOCAL1, 0.0], [0.0, 0.0, 1.0]]])
    V = np.array([[-1.0, -1.0, 4.0], [3.0, -1.0, 4.0], [-1.0, 3.0, 8.0]], np.float32)
    F = np.array([[0, 1, 2]], np.int32)
    C = np.array([[10, 20, 30], [200, 100, 50], [0, 255, 128]], np.uint8)
    w2c = np.linalg.inv(R.EYE_C2W)[:, :3, :4].astype(np.float32)
    img = geometry.render_mesh(_mesh(V, F, C), cameras=(R.EYE_C2W, K1, (1, 1)))
    _same(img, R.render_views(V, F, C, w2c, K1.astype(np.float32), 1, 1, dtype=np.float32))
    assert img.face.tolist() == [[[0]]]
    # zero faces, and zero vertices: all background, face -1, depth 0
    for Vz, Cz in ((V, C), (V[:0], C[:0])):
        for col in (Cz, None):
            none = geometry.render_mesh(_mesh(Vz, F[:0], col), cameras=(R.EYE_C2W, R.EYE_K, (5, 7)), background=(9, 8, 7))
            assert tuple(none.depth.shape) == (1, 5, 7) and (none.face == -1).all() and (none.depth == 0).all() and not none.mask.any()
            assert (none.colors is None) if col is None else (none.colors.cpu().numpy() == np.array([9, 8, 7], np.uint8)).all()
    assert geometry.face_views(none.face, 0).numel() == 0
    # a capacity-extracted mesh: rows past the count hold 0x7fffffff (faces) and NaN (vertices) and are never read
    V, F, C, w2c, K, (H, W), scene, mesh = _rig("9x11x13")
    nv, nf = len(V) // 3, len(F) // 3
    Vp, Fp, Cp = V.copy(), F.copy(), C.copy()
    Vp[nv:], Fp[nf:] = np.nan, 0x7fffffff
    roomy = _mesh(Vp, Fp, Cp, count=(nv, nf))
    ref = R.render_views(V, F, C, w2c, K, H, W, dtype=np.float32, count=(nv, nf))
    img = geometry.render_mesh(roomy, scene)
    _same(img, ref)
    assert (ref["face"] != _ref("9x11x13")["face"]).any()                               # (the cut mesh is another mesh)
    over = geometry.render_mesh(_mesh(V, F, C, count=(len(V) + 50, len(F) + 50)), scene)  # a count above the rows: the rows bound it
    _same(over, _ref("9x11x13"))
    # two runs, the same bytes
    again = geometry.render_mesh(roomy, scene)
    assert torch.equal(again.face, img.face) and torch.equal(again.depth.view(torch.int32), img.depth.view(torch.int32)) and torch.equal(again.colors, img.colors)
    # the tools honour the count too
    keep = torch.ones((len(F),), dtype=torch.bool, device=DEV)
    sub = geometry.filter_mesh(roomy, keep)
    want = R.filter_mesh(Vp, Fp, np.ones(len(F), bool), count=(nv, nf))
    assert sub.count.tolist() == [len(want["vertices"]), len(want["faces"])] and len(want["faces"]) < nf and (sub.faces.cpu().numpy() == want["faces"]).all()
    assert (_bits(sub.vertices) == _bits(want["vertices"])).all()


FOCAL1 = 0.25


# ------------------------------------------------------------------ (e) visibility and filtering
def test_face_views_against_its_restatement():
    V, F, C, _, _, _, scene, mesh = _rig("9x11x13")
    img = geometry.render_mesh(mesh, scene)
    n = geometry.face_views(img.face, len(F))
    want, seen = R.face_views(img.face.cpu().numpy(), len(F))
    assert n.dtype == torch.int32 and tuple(n.shape) == (len(F),) and (n.cpu().numpy() == want).all()
    assert int(n.max()) == 5 and int((n == 0).sum()) > len(F) // 3                       # the far side of the sphere is seen by nobody
    assert (ops.mesh_face_views(img.face, len(F))[1].cpu().numpy() == seen).all()
    # a smaller n_faces ignores the face numbers past it
    assert (geometry.face_views(img.face, 100).cpu().numpy() == R.face_views(img.face.cpu().numpy(), 100)[0]).all()
    # 33 views of 8 x 8: two words per face
    c2w, K, _, _, _ = R.rig(8, 8, 33, True)
    many = geometry.render_mesh(mesh, cameras=(c2w, K, (8, 8)))
    n33, seen33 = ops.mesh_face_views(many.face, len(F))
    want, seen = R.face_views(many.face.cpu().numpy(), len(F))
    assert tuple(seen33.shape) == (len(F), 2) and (seen33.cpu().numpy() == seen).all() and (n33.cpu().numpy() == want).all()
    assert (seen[:, 1] != 0).any() and (seen[:, 0] != 0).any() and (geometry.face_views(many.face, len(F)).cpu().numpy() == want).all()


def _mesh_equal(sub, want, colors=True):
    assert (_bits(sub.vertices) == _bits(want["vertices"])).all() and (sub.faces.cpu().numpy() == want["faces"]).all()
    assert (_bits(sub.ndc) == _bits(want["ndc"])).all() and (sub.vertex_edge.cpu().numpy() == want["vertex_edge"]).all()
    assert sub.vertex_index.dtype == torch.int64 and (sub.vertex_index.cpu().numpy() == want["vertex_index"]).all()
    assert sub.face_index.dtype == torch.int64 and (sub.face_index.cpu().numpy() == want["face_index"]).all()
    assert sub.count.tolist() == [len(want["vertices"]), len(want["faces"])] and sub.faces.dtype == torch.int32
    if colors:
        assert (sub.colors.cpu().numpy() == want["colors"]).all()


def test_filter_mesh_against_its_restatement():
    V, F, C, _, _, _, scene, mesh = _rig("17x19x23")          # 5 464 faces and 2 734 vertices: more than one workgroup, no multiple of 256
    rows = dict(ndc=mesh.ndc.cpu().numpy(), vertex_edge=mesh.vertex_edge.cpu().numpy(), colors=C)
    every = geometry.filter_mesh(mesh, torch.ones((len(F),), dtype=torch.bool, device=DEV))
    _mesh_equal(every, R.filter_mesh(V, F, np.ones(len(F), bool), **rows))
    assert torch.equal(every.vertices, mesh.vertices) and torch.equal(every.faces, mesh.faces) and torch.equal(every.colors, mesh.colors)   # an equal mesh
    none = geometry.filter_mesh(mesh, torch.zeros((len(F),), dtype=torch.uint8, device=DEV))
    assert none.count.tolist() == [0, 0] and tuple(none.vertices.shape) == (0, 3) and tuple(none.faces.shape) == (0, 3) and none.face_index.numel() == 0
    keep = np.random.default_rng(11).random(len(F)) < 0.3
    keep8 = (keep * np.random.default_rng(12).integers(1, 256, len(F))).astype(np.uint8)            # any non-zero byte keeps
    want = R.filter_mesh(V, F, keep, **rows)
    assert 0 < len(want["vertices"]) < len(V)
    for k in (torch.from_numpy(keep).to(DEV), torch.from_numpy(keep8).to(DEV)):
        sub = geometry.filter_mesh(mesh, k)
        _mesh_equal(sub, want)
        assert (V[want["vertex_index"]] == sub.vertices.cpu().numpy()).all() and int(sub.faces.max()) == len(want["vertices"]) - 1
    # a mesh without colours, ndc or edges; a kept face with a vertex number outside the mesh is dropped
    F2 = F.copy()
    F2[7, 1], F2[9, 0] = len(V), -3
    bare = _mesh(V, F2)
    bare.ndc = bare.vertex_edge = None
    sub = geometry.filter_mesh(bare, torch.from_numpy(keep | (np.arange(len(F)) < 16)).to(DEV))
    want = R.filter_mesh(V, F2, keep | (np.arange(len(F)) < 16))
    assert sub.colors is None and sub.ndc is None and sub.vertex_edge is None and (sub.faces.cpu().numpy() == want["faces"]).all()
    assert (sub.face_index.cpu().numpy() == want["face_index"]).all() and 7 not in want["face_index"] and 9 not in want["face_index"]


def test_cull_unseen_renders_the_same_depths():
    V, F, C, w2c, K, (H, W), scene, mesh = _rig("9x11x13")
    img = geometry.render_mesh(mesh, scene)
    sub = geometry.cull_unseen(mesh, scene)
    n = R.face_views(img.face.cpu().numpy(), len(F))[0]
    want = R.filter_mesh(V, F, n >= 1, ndc=mesh.ndc.cpu().numpy(), vertex_edge=mesh.vertex_edge.cpu().numpy(), colors=C)
    _mesh_equal(sub, want)
    assert 0 < int(sub.count[1]) < len(F) // 2
    again = geometry.render_mesh(sub, scene)
    assert torch.equal(again.depth.view(torch.int32), img.depth.view(torch.int32)) and torch.equal(again.colors, img.colors)
    assert torch.equal(sub.face_index[again.face.long().clamp(min=0)][again.mask], img.face.long()[img.mask])
    two = geometry.cull_unseen(mesh, scene, min_views=2, cull=1)
    assert (two.face_index.cpu().numpy() == np.nonzero(n >= 2)[0]).all()


# ------------------------------------------------------------------ (f) the chain
def test_fuse_mesh_render_chain():
    c = T.Case((24, 32), (9, 11, 13))
    scene = SceneRays(c.rgba, c.g["c2w"], c.g["K"], (300.0, 1000.0), device=DEV)
    vol = geometry.fuse_tsdf(scene, torch.from_numpy(c.d32).to(DEV), c.box, c.dims, trunc=c.trunc, valid=torch.from_numpy(c.valid).to(DEV))
    mesh = geometry.tsdf_mesh(vol)
    V, F, C = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), mesh.colors.cpu().numpy()
    assert len(F) > 100
    img = geometry.render_mesh(mesh, scene)
    _same(img, R.render_views(V, F, C, c.w2c32, c.K32, 24, 32, dtype=np.float32))       # the restatement's render of that same downloaded mesh
    depth = img.depth.cpu().numpy().astype(np.float64)
    both = img.mask.cpu().numpy() & (c.g["label"] >= 0)
    med = float(np.median(np.abs(depth[both] - c.g["depth"][both])))
    print(f"\nchain on the GPU: V {len(V)} T {len(F)}, jointly valid {float(both.mean()):.3f}, median |mesh depth - analytic depth| {med:.4f}, "
          f"allowed 2 x {R.CHAIN_MEDIAN}")
    assert both.mean() > 0.2 and med <= 2 * R.CHAIN_MEDIAN
    # the held-out-view use: the mesh's depth map scored against the analytic one
    seen = geometry.cull_unseen(mesh, scene)
    assert 0 < int(seen.count[1]) <= len(F)


# ------------------------------------------------------------------ (g) frames
def test_mesh_frames():
    V, F, C, _, _, (H, W), scene, mesh = _rig("9x11x13")
    g = R.rig(H, W, 3, True)
    poses, focal = g[0], 1.1 * W
    frames = geometry.mesh_frames(mesh, poses, (H, W), focal)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (3, H, 2 * W, 3)
    Kc = np.array([[focal, 0.0, W / 2], [0.0, focal, H / 2], [0.0, 0.0, 1.0]])
    img = geometry.render_mesh(mesh, cameras=(poses, Kc, (H, W)))
    mm = ops.depth_range(img.depth)
    for k in range(3):
        assert torch.equal(frames[k], ops.frame_u8(geometry.mesh_rgb(img.colors[k]), img.depth[k], minmax=mm))
        assert torch.equal(frames[k][:, :W], img.colors[k])                               # the rgb panel shows the colour map's own bytes
    assert img.mask.any() and float(mm[0]) > 0
    cropped = geometry.mesh_frames(mesh, poses, (H, W), focal, crop=True, cull=1)
    assert tuple(cropped.shape) == (3, H - 2 * (H // 20), 2 * (W - 2 * (W // 20)), 3)
    assert torch.equal(cropped[1][:, :W - 2 * (W // 20)], img.colors[1][H // 20:H - H // 20, W // 20:W - W // 20])
    grey = geometry.mesh_frames(_mesh(V, F), poses[:1], (H, W), (focal, focal))
    hit = img.mask[0]
    assert (grey[0][:, :W][hit] == 128).all() and (grey[0][:, :W][~hit] == 255).all()
