"""GPU: the mesh-extraction kernels (csrc/mesh.hip) against the restatement of their definition (tests/mesh_refs.py).

Everything is compared exactly.  Classification is a comparison of fp32 numbers, so faces and vertex_edge have no tolerance; vertices and ndc are held
BIT for bit to the fp32 restatement, whose every operation is rounded on its own as the kernels' are (tests/test_mesh_refs.py holds that restatement to the
float64 form).  The references are computed once per case and shared."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mesh_refs as R
from mvsnerf_amd import _lib, geometry, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("grid", "box", "table")

SPHERES = [(30.2, 30.1, 19.7, 12.3), (88.8, 40.4, 18.1, 15.2), (60.5, 33.3, 22.2, 9.1), (110.3, 60.6, 30.9, 6.7), (14.1, 55.2, 13.3, 10.4)]   # disjoint, inside
SHAPES = {
    "row": ((2, 2, 300), lambda s: R.spheres_field(s, [(40.3, 0.4, 0.3, 7.7), (200.2, 1.2, 0.8, 30.1), (299.0, 0.5, 0.5, 2.2)]), 0.0),
    "odd": ((5, 37, 67), lambda s: R.spheres_field(s, [(20.3, 15.4, 2.3, 6.7), (50.2, 22.2, 1.8, 9.1), (66.0, 36.0, 4.0, 3.3)]), 0.0),
    "big": ((40, 70, 130), lambda s: R.spheres_field(s, SPHERES), 0.0),      # 364000 nodes: 1422 workgroup counts, more than the scan kernel's 1024 threads
}


@functools.lru_cache(maxsize=None)
def _field(name):
    if name in R.CASES:
        return R.CASES[name][0](), R.CASES[name][1]
    shape, build, level = SHAPES[name]
    return build(shape), level


def _kw(mode, shape, dev=None):
    D, H, W = shape
    if mode == "box":
        return {"box": R.BOX}
    if mode == "table":
        P = R.node_table(D, H, W)
        return {"positions": torch.from_numpy(P).to(dev) if dev else P}
    return {}


@functools.lru_cache(maxsize=None)
def _ref(name, mode):
    f, level = _field(name)
    return R.extract(torch.from_numpy(f), level, dtype=torch.float32, **_kw(mode, f.shape))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(mesh, ref):
    V, T = ref["count"].tolist()
    assert mesh.count.tolist() == [V, T]
    assert tuple(mesh.vertices.shape) == (V, 3) and tuple(mesh.ndc.shape) == (V, 3) and tuple(mesh.faces.shape) == (T, 3)
    assert mesh.faces.dtype == torch.int32 and mesh.vertex_edge.dtype == torch.int64 and mesh.colors is None
    assert torch.equal(mesh.vertex_edge.cpu(), ref["vertex_edge"])
    assert torch.equal(mesh.faces.cpu(), ref["faces"])
    assert _same_bits(mesh.ndc, ref["ndc"]) and _same_bits(mesh.vertices, ref["vertices"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(R.CASES) + list(SHAPES))
def test_mesh_is_the_restatement_exactly(name, mode):
    f, level = _field(name)
    ref = _ref(name, mode)
    if name in R.CASES:
        assert ref["count"].tolist() == list(R.CASES[name][2:4])                        # the pinned totals
    else:
        assert ref["count"][0] > 0 and ref["count"][1] > 0
    mesh = geometry.extract_mesh(torch.from_numpy(f).to(DEV), level, **_kw(mode, f.shape, DEV))
    _check(mesh, ref)


def test_the_big_grid_is_closed_and_oriented():
    ref = _ref("big", "grid")
    closed, euler, used = R.surface_invariants(int(ref["count"][0]), ref["faces"].numpy())
    assert closed and used and euler == 2 * len(SPHERES) and R.signed_volume(ref["grid"].numpy(), ref["faces"].numpy()) > 0


@pytest.mark.parametrize("value", [-1.0, 1.0, float("nan")])
def test_empty_results(value):
    f = torch.full((4, 9, 35), value, device=DEV)
    for kw in ({}, {"box": R.BOX}, {"positions": torch.zeros((4, 9, 35, 3), device=DEV)}):
        mesh = geometry.extract_mesh(f, 0.0, **kw)
        assert mesh.count.tolist() == [0, 0]
        assert tuple(mesh.vertices.shape) == (0, 3) and tuple(mesh.ndc.shape) == (0, 3) and tuple(mesh.faces.shape) == (0, 3)
        assert tuple(mesh.vertex_edge.shape) == (0,)
    mesh = geometry.extract_mesh(f, 0.0, capacity=(5, 7))                               # nothing is written and nothing is read back
    assert mesh.count.tolist() == [0, 0] and tuple(mesh.vertices.shape) == (5, 3) and tuple(mesh.faces.shape) == (7, 3)


@pytest.mark.parametrize("mode", ["box", "table"])
def test_capacity_equal_to_the_totals_and_repeatability(mode):
    f, level = _field("odd")
    ref = _ref("odd", mode)
    V, T = ref["count"].tolist()
    d = torch.from_numpy(f).to(DEV)
    kw = _kw(mode, f.shape, DEV)
    a = geometry.extract_mesh(d, level, **kw)
    b = geometry.extract_mesh(d, level, capacity=(V, T), **kw)
    c = geometry.extract_mesh(d, level, **kw)
    for m in (b, c):
        assert torch.equal(m.count, a.count) and torch.equal(m.faces, a.faces) and torch.equal(m.vertex_edge, a.vertex_edge)
        assert _same_bits(m.vertices, a.vertices.cpu()) and _same_bits(m.ndc, a.ndc.cpu())
    _check(b, ref)
    roomy = geometry.extract_mesh(d, level, capacity=(V + 9, T + 11), **kw)              # rows past the totals exist and are nobody's
    assert roomy.count.tolist() == [V, T] and torch.equal(roomy.faces[:T], a.faces) and _same_bits(roomy.vertices[:V], a.vertices.cpu())


@pytest.mark.parametrize("caps", [(100, 150), (0, 40), (257, 0), (1, 1)])
def test_a_capacity_below_the_totals_cuts_and_writes_no_other_row(caps):
    f, level = _field("big")
    ref = _ref("big", "table")
    V, T = ref["count"].tolist()
    cv, cf = caps
    assert cv < V and cf < T
    D, H, W = f.shape
    d = torch.from_numpy(f).to(DEV)
    P = torch.from_numpy(R.node_table(D, H, W)).to(DEV)
    lib = _lib.lib()
    pad = 128
    vertices = torch.full((cv + pad, 3), -7.5, device=DEV)
    ndc = torch.full((cv + pad, 3), -7.5, device=DEV)
    vedge = torch.full((cv + pad,), -99, device=DEV, dtype=torch.int64)
    faces = torch.full((cf + pad, 3), -99, device=DEV, dtype=torch.int32)
    count = torch.full((2,), -1, device=DEV, dtype=torch.int64)
    ws = torch.empty((lib.mvsnerf_mesh_workspace_bytes(D, H, W) // 4 + 1,), device=DEV, dtype=torch.int32)
    rc = lib.mvsnerf_mesh_extract_fwd(d.data_ptr(), D, H, W, level, P.data_ptr(), None, cv, cf, vertices.data_ptr() if cv else 0, ndc.data_ptr() if cv else 0,
                                      vedge.data_ptr() if cv else 0, faces.data_ptr() if cf else 0, count.data_ptr(), ws.data_ptr(), ops.stream_ptr())
    assert rc == 0
    assert count.tolist() == [V, T]                                                     # the true totals: the caller sees that it was cut
    assert _same_bits(vertices[:cv], ref["vertices"][:cv]) and _same_bits(ndc[:cv], ref["ndc"][:cv])
    assert torch.equal(vedge[:cv].cpu(), ref["vertex_edge"][:cv]) and torch.equal(faces[:cf].cpu(), ref["faces"][:cf])
    assert bool((vertices[cv:] == -7.5).all()) and bool((ndc[cv:] == -7.5).all()) and bool((vedge[cv:] == -99).all()) and bool((faces[cf:] == -99).all())
    mesh = geometry.extract_mesh(d, level, positions=P, capacity=caps)
    assert mesh.count.tolist() == [V, T] and torch.equal(mesh.faces.cpu(), ref["faces"][:cf]) and _same_bits(mesh.vertices, ref["vertices"][:cv])


def test_entry_checks_its_arguments():
    f = torch.zeros((4, 4, 4), device=DEV)
    P = torch.zeros((4, 4, 4, 3), device=DEV)
    out = dict(vertices=torch.zeros((8, 3), device=DEV), ndc=torch.zeros((8, 3), device=DEV), vertex_edge=torch.zeros((8,), device=DEV, dtype=torch.int64),
               faces=torch.zeros((8, 3), device=DEV, dtype=torch.int32), count=torch.zeros((2,), device=DEV, dtype=torch.int64),
               workspace=torch.zeros((1024,), device=DEV, dtype=torch.int32))
    lib = _lib.lib()
    box = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    base = dict(field=f.data_ptr(), D=4, H=4, W=4, level=0.0, positions=0, box=None, cap_v=8, cap_f=8, **{k: v.data_ptr() for k, v in out.items()})
    order = ("field", "D", "H", "W", "level", "positions", "box", "cap_v", "cap_f", "vertices", "ndc", "vertex_edge", "faces", "count", "workspace")
    call = lambda **kw: lib.mvsnerf_mesh_extract_fwd(*[{**base, **kw}[k] for k in order], ops.stream_ptr())
    assert call() == 0 and call(positions=P.data_ptr()) == 0 and call(box=box) == 0
    assert call(cap_v=0, cap_f=0, vertices=0, ndc=0, vertex_edge=0, faces=0) == 0       # the count alone needs no output
    for kw in ({"field": 0}, {"count": 0}, {"workspace": 0}, {"vertices": 0}, {"faces": 0}, {"cap_v": -1}):
        assert call(**kw) == -1, kw
    for kw in ({"D": 1}, {"W": 1}, {"D": 513, "H": 512, "W": 512}, {"level": float("nan")}, {"level": -float("inf")}, {"positions": P.data_ptr(), "box": box}):
        assert call(**kw) == -2, kw
    for kw in ({"field": base["field"] + 2}, {"vertex_edge": base["vertex_edge"] + 4}, {"count": base["count"] + 4}, {"faces": base["faces"] + 2},
               {"workspace": base["workspace"] + 1}):
        assert call(**kw) == -3, kw
    o = torch.zeros(3, device=DEV)
    assert lib.mvsnerf_mesh_dirs_fwd(out["vertices"].data_ptr(), 0, 8, out["ndc"].data_ptr(), ops.stream_ptr()) == -1
    assert lib.mvsnerf_mesh_dirs_fwd(out["vertices"].data_ptr(), o.data_ptr() + 2, 8, out["ndc"].data_ptr(), ops.stream_ptr()) == -3
    raw = torch.zeros((8, 4), device=DEV)
    assert lib.mvsnerf_mesh_rgb_u8_fwd(raw.data_ptr() + 4, 7, out["faces"].data_ptr(), ops.stream_ptr()) == -3
    assert lib.mvsnerf_mesh_rgb_u8_fwd(raw.data_ptr(), 1 << 31, out["faces"].data_ptr(), ops.stream_ptr()) == -2
    with pytest.raises(RuntimeError, match="float32"):
        ops.mesh_extract(f.double(), 0.0)
    torch.cuda.synchronize()


def test_the_two_colour_kernels():
    g = torch.Generator().manual_seed(2)
    v = (torch.randn((1001, 3), generator=g) * 300).to(DEV)
    o = torch.tensor([12.5, -340.25, 7.125], device=DEV)
    assert torch.equal(ops.mesh_dirs(v, o), v - o)
    raw = torch.randn((1001, 4), generator=g) * 0.8 + 0.4
    raw[::7, 1] = float("nan")
    raw[3::11, 0], raw[5::13, 2] = float("inf"), -float("inf")
    raw[1, :3], raw[2, :3] = torch.tensor([1.0, 0.0, 254.999 / 255]), torch.tensor([-0.0, 0.99999994, 1.0000001])
    want = (torch.nan_to_num(raw[:, :3], nan=0.0).clamp(0, 1) * 255).to(torch.int32).to(torch.uint8)      # one fp32 product, truncated
    assert torch.equal(ops.mesh_rgb_u8(raw.to(DEV)).cpu(), want)
    assert tuple(ops.mesh_dirs(v[:0], o).shape) == (0, 3) and tuple(ops.mesh_rgb_u8(raw[:0].to(DEV)).shape) == (0, 3)


# ------------------------------------------------------------------ the two systems
def _border_only_open(mesh):
    """Closed and consistently oriented wherever the surface does not touch the grid border: every directed edge once; an edge without its reverse has
    both ends on one border plane of the grid (ndc 0 or 1 on a common axis)."""
    V = int(mesh.count[0])
    f = mesh.faces.cpu().numpy().astype(np.int64)
    ndc = mesh.ndc.cpu().numpy()
    directed = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    code = directed[:, 0] * (V + 1) + directed[:, 1]
    assert len(np.unique(code)) == len(code)
    lone = directed[~np.isin(code, directed[:, 1] * (V + 1) + directed[:, 0])]
    a, b = ndc[lone[:, 0]], ndc[lone[:, 1]]
    on_plane = ((a == b) & ((a == 0) | (a == 1))).any(1)
    assert on_plane.all()
    assert len(np.unique(f)) == V
    return len(lone)


@functools.lru_cache(maxsize=None)
def _fusion():
    from tests.test_gpu_fusion import fusion_system, fusion_views
    views, bbox, img_wh, focal = fusion_views()
    with torch.no_grad():
        sysm, _ = fusion_system(views, bbox, img_wh, focal)
    vol_cl = ops.channels_last_volume(sysm.volume.feat_volume.detach())
    net, pose = sysm.network_fn, sysm.pose_source_ref
    src = dict(vol_cl=vol_cl, packed=net.packed(20), w2cs=pose["w2cs"][:3].contiguous())
    return sysm, src, pose, dict(box=sysm.bbox_3d)


@functools.lru_cache(maxsize=None)
def _finetune():
    from tests.test_gpu_finetune_render import _system
    ft, _, _ = _system(V=3)
    vol_cl = ops.channels_last_volume(ft.volume.feat_volume.detach())
    net, pose = ft.network_fn, ft.pose_source
    camera = dict(K_ref=pose["intrinsics"][0], c2w_ref=pose["c2ws"][0], near_far=ft.near_far_source, ref_hw=(64, 96), pad=ft.args.pad)
    src = dict(vol_cl=vol_cl, packed=net.packed(20), w2cs=pose["w2cs"][:3].contiguous(), imgs=ft.imgs[0].contiguous(),
               intrinsics=pose["intrinsics"][:3].contiguous(), camera=camera)
    D, H, W = vol_cl.shape[:3]
    with torch.no_grad():
        positions = ops.voxel_points(D, H, W, device=vol_cl.device, **camera)[1].view(D, H, W, 3)
    return ft, src, pose, dict(positions=positions)


def _explicit_colors(sysm, src, pose, mesh, origin):
    """Section 4 of the definition, in one chunk, from public calls."""
    n = mesh.vertices.shape[0]
    ndc = mesh.ndc.view(n, 1, 3)
    if "imgs" in src:
        feat, _ = ops.gather(src["vol_cl"], src["imgs"], src["w2cs"], src["intrinsics"], mesh.vertices.view(n, 1, 3), ndc)
    else:
        feat, _ = ops.gather_colorvol(src["vol_cl"], ndc)
    dirs = ops.dir_feature((mesh.vertices - origin).contiguous(), pose["w2cs"][0].contiguous(), normalize=True)
    raw = ops.mlp_forward(src["packed"], 20, ndc.data_ptr(), 3, feat.data_ptr(), 20, dirs.data_ptr(), 3, n, 1, 0, mesh.vertices.device,
                          **sysm.network_fn.packed_alt(20))
    return (raw[:, :3].clamp(0, 1) * 255).to(torch.int32).to(torch.uint8)


@pytest.mark.parametrize("which", ["fusion", "finetune"])
def test_scene_mesh_and_vertex_colors(which):
    sysm, src, pose, where = _fusion() if which == "fusion" else _finetune()
    before = sysm.density_volume
    with torch.no_grad():
        field = ops.node_density(**src, **sysm.network_fn.packed_alt(20))
        level = float(field.flatten().sort().values[int(0.8 * field.numel())])           # a level the field crosses: its 80th percentile
        want = geometry.extract_mesh(field, level, **where)
        V, T = want.count.tolist()
        assert V > 100 and T > 100
        open_edges = _border_only_open(want)
        # colours: the explicit sequence, whatever the chunk
        origin = pose["c2ws"][0][:3, 3].contiguous()
        colors = _explicit_colors(sysm, src, pose, want, origin)
        assert tuple(colors.shape) == (V, 3) and colors.dtype == torch.uint8 and int(colors.max()) > int(colors.min())
        for chunk in (262144, 100, V - 1, 1 + V // 2):
            assert torch.equal(geometry.vertex_colors(sysm, want, chunk=chunk), colors), chunk
        far = torch.tensor([0.5, -0.25, -3.0], device=origin.device)
        elsewhere = _explicit_colors(sysm, src, pose, want, far)
        assert torch.equal(geometry.vertex_colors(sysm, want, origin=far.tolist(), chunk=777), elsewhere)
        # the scene in one call
        mesh = geometry.scene_mesh(sysm, level)
        assert sysm.density_volume is before
        assert mesh.count.tolist() == [V, T] and torch.equal(mesh.faces, want.faces) and torch.equal(mesh.vertex_edge, want.vertex_edge)
        assert torch.equal(mesh.vertices, want.vertices) and torch.equal(mesh.ndc, want.ndc) and torch.equal(mesh.colors, colors)
        bare = geometry.scene_mesh(sysm, level, colors=False, capacity=(V + 5, T + 5))
        assert bare.colors is None and bare.count.tolist() == [V, T] and torch.equal(bare.faces[:T], want.faces)
        assert sysm.density_volume is before
        dil = geometry.scene_mesh(sysm, level, colors=False, dilate=1)
        assert torch.equal(dil.faces, geometry.extract_mesh(ops.max_dilate3d(field, 1), level, **where).faces)
    print(f"{which}: level {level:.4g}, {V} vertices, {T} faces, {open_edges} open edges on the grid border")


def test_scene_mesh_refuses_other_systems():
    with pytest.raises(TypeError, match="MVSSystemFinetune or MVSSystemFusion"):
        geometry.scene_mesh(object(), 0.0)
