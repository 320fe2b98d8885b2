"""CPU-only: the Python surface of the mesh rasteriser (mvsnerf_amd/geometry.py) - what render_mesh, face_views, filter_mesh, cull_unseen and
mesh_frames refuse before the library is touched, the five new entries in the ctypes table and the internal header, and their argument checks."""
import os
import re

import numpy as np
import pytest
import torch

import depth_fusion_refs as R
from mvsnerf_amd import _lib, geometry
from mvsnerf_amd.rays import SceneRays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, H, W = 5, 6, 8
NAMES = {"mvsnerf_mesh_raster_workspace_bytes": 4, "mvsnerf_mesh_raster_fwd": 21, "mvsnerf_mesh_face_views_fwd": 11,
         "mvsnerf_mesh_filter_workspace_bytes": 2, "mvsnerf_mesh_filter_fwd": 21}


def _no_library(monkeypatch):
    """Any touch of the library from here on fails the test: the refusals below must come first."""
    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)


@pytest.fixture()
def scene():
    c2w, K = R.rig_cameras(H, W, M)
    return SceneRays(np.zeros((M, H, W, 3), np.uint8), c2w, K, (400.0, 900.0), device="cpu")


def _mesh(V=4, T=2, **kw):
    m = geometry.TriangleMesh(torch.zeros((V, 3)), torch.zeros((V, 3)), torch.zeros((T, 3), dtype=torch.int32), torch.zeros((V,), dtype=torch.int64),
                              torch.tensor([V, T]), torch.zeros((V, 3), dtype=torch.uint8))
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_new_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    stable = open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read()
    lib = _lib.lib()                                                 # binding resolves every name of the table in the shared library: exported
    for n, n_args in NAMES.items():
        assert n in _lib.SIGNATURES and n not in stable
        decl = re.search(rf"\b{n}\s*\(([^)]*)\)", code)
        assert decl and len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[n][1])
        assert getattr(lib, n).argtypes == _lib.SIGNATURES[n][1]
    assert lib.mvsnerf_abi_version() == 12                           # the stable tier is what it was
    assert "raster" not in stable and "mesh_filter" not in stable and "face_views" not in stable
    for word in ("SUB = 256", "top-left", "2^23", "float_bits(z) << 32 | face", "(1 - b1) - b2"):
        assert word in header                                       # the header comment carries the definition


def test_render_mesh_refusals_come_before_the_library(monkeypatch, scene):
    _no_library(monkeypatch)
    render = lambda mesh=None, **kw: geometry.render_mesh(_mesh() if mesh is None else mesh, kw.pop("scene", scene), **kw)
    with pytest.raises(TypeError, match="render_mesh: a TriangleMesh"):
        render(torch.zeros((4, 3)))
    with pytest.raises(TypeError, match="vertices must be a float32"):
        render(_mesh(vertices=torch.zeros((4, 3), dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"vertices must be \(V,3\)"):
        render(_mesh(vertices=torch.zeros((4, 2))))
    with pytest.raises(TypeError, match="faces must be an int32"):
        render(_mesh(faces=torch.zeros((2, 3), dtype=torch.int64)))
    with pytest.raises(ValueError, match=r"faces must be \(T,3\)"):
        render(_mesh(faces=torch.zeros((2, 4), dtype=torch.int32)))
    with pytest.raises(ValueError, match="vertices' device"):
        render(_mesh(faces=torch.zeros((2, 3), dtype=torch.int32, device="meta")))
    with pytest.raises(TypeError, match="colors must be None or a uint8"):
        render(_mesh(colors=torch.zeros((4, 3))))
    with pytest.raises(ValueError, match=r"colors must be \(4,3\)"):
        render(_mesh(colors=torch.zeros((5, 3), dtype=torch.uint8)))
    with pytest.raises(ValueError, match="mesh.count"):
        render(_mesh(count=torch.zeros((3,), dtype=torch.int64)))
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        render(_mesh(faces=torch.empty((1 << 31, 3), dtype=torch.int32, device="meta"), vertices=torch.empty((4, 3), device="meta"), colors=None, count=None))
    with pytest.raises(TypeError, match="a SceneRays expected"):
        render(scene=None)
    with pytest.raises(TypeError, match="a SceneRays expected"):
        render(scene=torch.zeros(3))
    with pytest.raises(ValueError, match="bank's device"):
        render(_mesh(vertices=torch.empty((4, 3), device="meta"), faces=torch.empty((2, 3), dtype=torch.int32, device="meta"), colors=None, count=None))
    for cull in (2, -2, 0.5, None, "1", True):
        with pytest.raises(ValueError, match="cull must be"):
            render(cull=cull)
    for z_min in (-0.5, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="z_min"):
            render(z_min=z_min)
    for views in ([], [[0, 1]], [0.5, 1.0], [0, M], [-1, 2], 3):
        with pytest.raises(ValueError, match="views must"):
            render(views=views)
    for bg in ((255, 255), (0, 0, 256), (-1, 0, 0), 7, (0.5, 0, 0), "abc"):
        with pytest.raises(ValueError, match="background"):
            render(background=bg)
    c2w, K = R.rig_cameras(H, W, M)
    with pytest.raises(ValueError, match="exclude each other"):
        render(cameras=(c2w, K, (H, W)))
    cam = lambda *c: geometry.render_mesh(_mesh(), cameras=c if len(c) != 1 else c[0])
    with pytest.raises(ValueError, match="cameras must be"):
        cam(c2w)
    with pytest.raises(ValueError, match=r"\(M,4,4\) or \(M,3,4\)"):
        cam(c2w[0], K, (H, W))
    with pytest.raises(ValueError, match="intrinsics"):
        cam(c2w, K[:2], (H, W))
    for hw in ((0, 8), (8, (1 << 15) + 1)):
        with pytest.raises(ValueError, match="pixels"):
            cam(c2w, K, hw)


def test_face_views_and_filter_mesh_refusals_come_before_the_library(monkeypatch, scene):
    _no_library(monkeypatch)
    face = torch.zeros((M, H, W), dtype=torch.int32)
    with pytest.raises(TypeError, match="face must be an int32"):
        geometry.face_views(face.long(), 4)
    with pytest.raises(TypeError, match="int32"):
        geometry.face_views(face.numpy(), 4)
    for bad in (face[0], face[:0]):
        with pytest.raises(ValueError, match=r"non-empty \(M,H,W\)"):
            geometry.face_views(bad, 4)
    for n in (-1, 1 << 31, 2.5, True):
        with pytest.raises(ValueError, match="n_faces"):
            geometry.face_views(face, n)
    with pytest.raises(TypeError, match="keep must be a bool or uint8"):
        geometry.filter_mesh(_mesh(), torch.ones((2,)))
    with pytest.raises(TypeError, match="keep must be"):
        geometry.filter_mesh(_mesh(), np.ones((2,), bool))
    for bad in (torch.ones((3,), dtype=torch.bool), torch.ones((2, 1), dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"keep must be \(2,\)"):
            geometry.filter_mesh(_mesh(), bad)
    with pytest.raises(ValueError, match="mesh's device"):
        geometry.filter_mesh(_mesh(), torch.empty((2,), dtype=torch.bool, device="meta"))
    with pytest.raises(TypeError, match="filter_mesh: a TriangleMesh"):
        geometry.filter_mesh(torch.zeros((4, 3)), torch.ones((2,), dtype=torch.bool))
    with pytest.raises(ValueError, match="mesh.ndc"):
        geometry.filter_mesh(_mesh(ndc=torch.zeros((3, 3))), torch.ones((2,), dtype=torch.bool))
    with pytest.raises(ValueError, match="mesh.vertex_edge"):
        geometry.filter_mesh(_mesh(vertex_edge=torch.zeros((4,), dtype=torch.int32)), torch.ones((2,), dtype=torch.bool))
    for mv in (-1, 1.5, True):
        with pytest.raises(ValueError, match="min_views"):
            geometry.cull_unseen(_mesh(), scene, min_views=mv)
    with pytest.raises(ValueError, match="cull must be"):
        geometry.cull_unseen(_mesh(), scene, cull=3)
    poses = R.rig_cameras(H, W, 3)[0]
    with pytest.raises(ValueError, match="crop"):
        geometry.mesh_frames(_mesh(), poses, (H, W), 9.0, crop=(3, 0))
    with pytest.raises(ValueError, match="z_min"):
        geometry.mesh_frames(_mesh(), poses, (H, W), 9.0, z_min=-1.0)
    with pytest.raises(ValueError, match=r"\(M,4,4\) or \(M,3,4\)"):
        geometry.mesh_frames(_mesh(), poses[0], (H, W), 9.0)


def test_the_entries_refuse_bad_arguments_without_a_gpu():
    """The argument checks come before the first launch, so they can be asked on a machine without a GPU."""
    lib = _lib.lib()
    ok = 1 << 12                                                    # any aligned non-null address: a refused call dereferences nothing
    assert lib.mvsnerf_mesh_raster_workspace_bytes(1000, 5, 24, 32) == 5 * 24 * 32 * 8 + 4 * 5 * (32 + 8 + 1024) + 8
    for bad in ((-1, 5, 24, 32), (1 << 31, 5, 24, 32), (10, 0, 24, 32), (10, 65536, 24, 32), (10, 5, 0, 32), (10, 5, 24, (1 << 15) + 1),
                ((1 << 22) * 256, 2, 24, 32)):
        assert lib.mvsnerf_mesh_raster_workspace_bytes(*bad) == 0, bad
    order = (("vertices", ok), ("n_vertices", 8), ("faces", ok), ("n_faces", 4), ("colors", 0), ("mesh_count", 0), ("w2c", ok), ("K", ok), ("view_ids", 0),
             ("n_views", 0), ("M", 3), ("H", 6), ("W", 8), ("cull", 0), ("z_min", 0.0), ("background", 0), ("depth", ok), ("face", ok), ("out_colors", 0),
             ("workspace", ok), ("stream", 0))
    call = lambda **kw: lib.mvsnerf_mesh_raster_fwd(*[kw.get(k, d) for k, d in order])
    for kw in ({"vertices": 0}, {"faces": 0}, {"w2c": 0}, {"K": 0}, {"depth": 0}, {"face": 0}, {"workspace": 0}, {"n_vertices": -1}, {"n_faces": -1},
               {"colors": ok}, {"out_colors": ok}, {"cull": 2}, {"cull": -2}, {"M": 0}, {"H": 0}, {"W": 0}, {"view_ids": ok, "n_views": 0}):
        assert call(**kw) == -1, kw
    for kw in ({"n_faces": 1 << 31}, {"n_vertices": 1 << 31}, {"H": (1 << 15) + 1}, {"W": (1 << 15) + 1}, {"view_ids": ok, "n_views": 65536}, {"M": 65536},
               {"M": 1 << 22, "view_ids": ok, "n_views": 2}, {"z_min": -1.0}, {"z_min": float("nan")}, {"z_min": float("inf")},
               {"n_faces": (1 << 22) * 256, "M": 2}):
        assert call(**kw) == -2, kw
    for kw in ({"vertices": ok + 2}, {"faces": ok + 1}, {"mesh_count": ok + 4}, {"w2c": ok + 2}, {"K": ok + 1}, {"view_ids": ok + 2, "n_views": 2},
               {"depth": ok + 2}, {"face": ok + 1}, {"workspace": ok + 4}):
        assert call(**kw) == -3, kw
    order = (("face", ok), ("n_maps", 3), ("H", 6), ("W", 8), ("view_ids", 0), ("M", 3), ("n_faces", 4), ("mesh_count", 0), ("seen", ok), ("n", ok), ("stream", 0))
    call = lambda **kw: lib.mvsnerf_mesh_face_views_fwd(*[kw.get(k, d) for k, d in order])
    for kw in ({"face": 0}, {"seen": 0}, {"n": 0}, {"n_maps": 0}, {"H": 0}, {"W": 0}, {"M": 0}, {"n_faces": -1}, {"M": 4}):
        assert call(**kw) == -1, kw
    for kw in ({"n_faces": 1 << 31}, {"n_maps": 65536, "M": 65536}, {"H": (1 << 15) + 1}, {"M": 1 << 22, "view_ids": ok}):
        assert call(**kw) == -2, kw
    for kw in ({"face": ok + 2}, {"view_ids": ok + 1}, {"mesh_count": ok + 4}, {"seen": ok + 2}, {"n": ok + 1}):
        assert call(**kw) == -3, kw
    assert call(n_faces=0, seen=0, n=0) == 0                        # nothing to do, nothing launched
    assert lib.mvsnerf_mesh_filter_workspace_bytes(10, 10) == (10 + 2 + 2) * 4 + 20 + 8
    assert lib.mvsnerf_mesh_filter_workspace_bytes(-1, 10) == 0 and lib.mvsnerf_mesh_filter_workspace_bytes(10, 1 << 31) == 0
    order = (("vertices", ok), ("ndc", 0), ("vertex_edge", 0), ("colors", 0), ("n_vertices", 8), ("faces", ok), ("n_faces", 4), ("mesh_count", 0), ("keep", ok),
             ("cap_v", 8), ("cap_f", 4), ("out_vertices", ok), ("out_ndc", 0), ("out_vertex_edge", 0), ("out_colors", 0), ("vertex_index", ok), ("out_faces", ok),
             ("face_index", ok), ("count", ok), ("workspace", ok), ("stream", 0))
    call = lambda **kw: lib.mvsnerf_mesh_filter_fwd(*[kw.get(k, d) for k, d in order])
    for kw in ({"vertices": 0}, {"faces": 0}, {"keep": 0}, {"count": 0}, {"workspace": 0}, {"n_vertices": -1}, {"n_faces": -1}, {"cap_v": -1}, {"cap_f": -1},
               {"out_vertices": 0}, {"vertex_index": 0}, {"out_faces": 0}, {"face_index": 0}, {"ndc": ok}, {"vertex_edge": ok}, {"colors": ok}):
        assert call(**kw) == -1, kw
    for kw in ({"n_vertices": 1 << 31}, {"n_faces": 1 << 31}, {"cap_v": 1 << 31}, {"cap_f": 1 << 31}):
        assert call(**kw) == -2, kw
    for kw in ({"vertices": ok + 2}, {"ndc": ok + 2, "out_ndc": ok}, {"vertex_edge": ok + 4, "out_vertex_edge": ok}, {"faces": ok + 1}, {"mesh_count": ok + 4},
               {"out_vertices": ok + 2}, {"vertex_index": ok + 4}, {"out_faces": ok + 2}, {"face_index": ok + 4}, {"count": ok + 4}, {"workspace": ok + 2}):
        assert call(**kw) == -3, kw
