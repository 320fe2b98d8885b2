"""CPU-only: the Python surface of the mesh extraction (mvsnerf_amd/geometry.py) - what extract_mesh refuses before the library is touched,
the PLY writer for a TriangleMesh (and, unchanged, for a PointCloud), and the new entries in the ctypes table and the internal header."""
import os
import re

import numpy as np
import pytest
import torch

from mvsnerf_amd import _lib, geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_library(monkeypatch):
    """Any touch of the library from here on fails the test: the refusals below must come first."""
    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)


def test_refusals_come_before_the_library(monkeypatch):
    _no_library(monkeypatch)
    f = torch.zeros((3, 4, 5))
    with pytest.raises(TypeError, match="float32"):
        geometry.extract_mesh(f.double(), 0.0)
    with pytest.raises(TypeError, match="float32"):
        geometry.extract_mesh(f.numpy(), 0.0)
    for bad in (f[0], f[None], torch.zeros((1, 4, 5)), torch.zeros((3, 4, 1))):
        with pytest.raises(ValueError, match=r"\(D,H,W\)"):
            geometry.extract_mesh(bad, 0.0)
    with pytest.raises(ValueError, match="2\\^27"):
        geometry.extract_mesh(torch.empty((513, 512, 512), device="meta"), 0.0)
    for level in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            geometry.extract_mesh(f, level)
    P = torch.zeros((3, 4, 5, 3))
    with pytest.raises(ValueError, match="exclude each other"):
        geometry.extract_mesh(f, 0.0, positions=P, box=((0, 0, 0), (1, 1, 1)))
    with pytest.raises(TypeError, match="positions"):
        geometry.extract_mesh(f, 0.0, positions=P.double())
    with pytest.raises(ValueError, match=r"\(3,4,5,3\)"):
        geometry.extract_mesh(f, 0.0, positions=P[:, :, :-1])
    with pytest.raises(ValueError, match="field's device"):
        geometry.extract_mesh(f, 0.0, positions=torch.empty((3, 4, 5, 3), device="meta"))
    for box in ((0, 0, 0), ((0, 0, 0), (1, 1, float("nan"))), torch.zeros((2, 4))):
        with pytest.raises(ValueError, match="box"):
            geometry.extract_mesh(f, 0.0, box=box)
    for cap in (7, (1,), (1, 2, 3), (-1, 5), (5, -1), ("a", 1)):
        with pytest.raises(ValueError, match="capacity"):
            geometry.extract_mesh(f, 0.0, capacity=cap)


def _parse_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int(re.fullmatch(r"element vertex (\d+)", lines[2]).group(1))
    assert lines[3:9] == ["property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue"]
    nf = int(re.fullmatch(r"element face (\d+)", lines[9]).group(1))
    assert lines[10:] == ["property list uchar int vertex_indices", ""]
    assert len(body) == 15 * nv + 13 * nf
    verts = np.frombuffer(body[:15 * nv], dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    faces = np.frombuffer(body[15 * nv:], dtype=np.dtype([("n", "u1"), ("v", "<i4", 3)]))
    assert (faces["n"] == 3).all()
    return verts, faces


@pytest.mark.parametrize("nv,nf", [(0, 0), (4, 2), (301, 598)])
def test_save_ply_of_a_mesh_round_trip(tmp_path, nv, nf):
    g = np.random.default_rng(nv)
    xyz = (g.standard_normal((nv, 3)) * 100).astype(np.float32)
    rgb = g.integers(0, 256, (nv, 3)).astype(np.uint8)
    tri = g.integers(0, max(nv, 1), (nf, 3)).astype(np.int32)
    path = str(tmp_path / "mesh.ply")
    t = torch.from_numpy
    mesh = geometry.TriangleMesh(t(xyz), t(xyz) * 0, t(tri), torch.arange(nv), torch.tensor([nv, nf]), colors=t(rgb))
    assert geometry.save_ply(path, mesh) == (nv, nf)
    verts, faces = _parse_ply(path)
    assert verts["xyz"].tobytes() == xyz.tobytes() and verts["rgb"].tobytes() == rgb.tobytes() and faces["v"].tobytes() == tri.tobytes()
    mesh.colors = None                                              # no colours: grey
    assert geometry.save_ply(path, mesh) == (nv, nf)
    verts, faces = _parse_ply(path)
    assert verts["xyz"].tobytes() == xyz.tobytes() and (verts["rgb"] == 128).all() and faces["v"].tobytes() == tri.tobytes()
    # a caller-given capacity: the first min(count, rows) rows of each array, whichever is smaller
    pad = lambda a, k: t(np.concatenate((a, np.full((k,) + a.shape[1:], 77, a.dtype))))
    roomy = geometry.TriangleMesh(pad(xyz, 3), pad(xyz, 3), pad(tri, 5), torch.arange(nv + 3), torch.tensor([nv, nf]), colors=pad(rgb, 3))
    assert geometry.save_ply(path, roomy) == (nv, nf)
    verts, faces = _parse_ply(path)
    assert verts["xyz"].tobytes() == xyz.tobytes() and verts["rgb"].tobytes() == rgb.tobytes() and faces["v"].tobytes() == tri.tobytes()
    cut = geometry.TriangleMesh(t(xyz), t(xyz), t(tri), torch.arange(nv), torch.tensor([nv + 10, nf + 20]), colors=t(rgb))
    assert geometry.save_ply(path, cut) == (nv, nf)


def test_save_ply_of_a_point_cloud_is_unchanged(tmp_path):
    g = np.random.default_rng(5)
    n = 33
    xyz = (g.standard_normal((n, 3)) * 10).astype(np.float32)
    rgb = g.integers(0, 256, (n, 3)).astype(np.uint8)
    want = (b"ply\nformat binary_little_endian 1.0\nelement vertex 33\nproperty float x\nproperty float y\nproperty float z\n"
            b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    want += b"".join(xyz[k].tobytes() + rgb[k].tobytes() for k in range(n))
    path = str(tmp_path / "cloud.ply")
    assert geometry.save_ply(path, (torch.from_numpy(xyz), torch.from_numpy(rgb))) == n
    assert open(path, "rb").read() == want
    cloud = geometry.PointCloud(torch.from_numpy(np.concatenate((xyz, xyz[:4]))), torch.from_numpy(np.concatenate((rgb, rgb[:4]))), None, None,
                                torch.tensor([n]), None, None, None, None)
    assert geometry.save_ply(path, cloud) == n
    assert open(path, "rb").read() == want


def test_new_entries_are_bound_and_declared():
    names = {"mvsnerf_mesh_workspace_bytes": 3, "mvsnerf_mesh_extract_fwd": 16, "mvsnerf_mesh_dirs_fwd": 5, "mvsnerf_mesh_rgb_u8_fwd": 4}
    header = open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    stable = open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read()
    for n, n_args in names.items():
        assert n in _lib.SIGNATURES and n not in stable
        decl = re.search(rf"\b{n}\s*\(([^)]*)\)", code)
        assert decl and len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[n][1])


def test_workspace_query_runs_without_a_gpu():
    q = _lib.lib().mvsnerf_mesh_workspace_bytes
    assert q(1, 5, 5) == 0 and q(5, 5, 1) == 0 and q(0, 0, 0) == 0 and q(-2, 4, 4) == 0
    assert q(513, 512, 512) == 0 and q(1 << 20, 1 << 20, 1 << 20) == 0
    assert q(2, 2, 2) == 8 * 5 + 16 and q(4, 8, 8) == 256 * 5 + 16 and q(4, 8, 9) == 288 * 5 + 32
    assert q(512, 512, 512) == (1 << 27) * 5 + (1 << 19) * 16


def test_the_entries_refuse_bad_arguments_without_a_gpu():
    """The argument checks come before the first launch, so they can be asked on a machine without a GPU."""
    import ctypes
    lib = _lib.lib()
    ok = 1 << 12                                                    # any aligned non-null address: a refused call dereferences nothing
    box = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    call = lambda **kw: lib.mvsnerf_mesh_extract_fwd(*[kw.get(k, d) for k, d in (
        ("field", ok), ("D", 4), ("H", 4), ("W", 4), ("level", 0.0), ("positions", 0), ("box", None), ("cap_v", 8), ("cap_f", 8), ("vertices", ok), ("ndc", ok),
        ("vertex_edge", ok), ("faces", ok), ("count", ok), ("workspace", ok), ("stream", 0))])
    for kw in ({"field": 0}, {"count": 0}, {"workspace": 0}, {"vertices": 0}, {"ndc": 0}, {"vertex_edge": 0}, {"faces": 0}, {"cap_v": -1}, {"cap_f": -1}):
        assert call(**kw) == -1, kw
    for kw in ({"D": 1}, {"H": 1}, {"W": 0}, {"D": 513, "H": 512, "W": 512}, {"level": float("nan")}, {"level": float("inf")}, {"positions": ok, "box": box}):
        assert call(**kw) == -2, kw
    for kw in ({"field": ok + 2}, {"positions": ok + 1}, {"vertices": ok + 2}, {"ndc": ok + 2}, {"vertex_edge": ok + 4}, {"faces": ok + 1}, {"count": ok + 4},
               {"workspace": ok + 2}):
        assert call(**kw) == -3, kw
    assert lib.mvsnerf_mesh_dirs_fwd(ok, 0, 4, ok, 0) == -1 and lib.mvsnerf_mesh_dirs_fwd(0, ok, 4, ok, 0) == -1 and lib.mvsnerf_mesh_dirs_fwd(ok, ok, -1, ok, 0) == -1
    assert lib.mvsnerf_mesh_dirs_fwd(ok, ok, 1 << 31, ok, 0) == -2 and lib.mvsnerf_mesh_dirs_fwd(ok + 2, ok, 4, ok, 0) == -3
    assert lib.mvsnerf_mesh_rgb_u8_fwd(0, 4, ok, 0) == -1 and lib.mvsnerf_mesh_rgb_u8_fwd(ok, 4, 0, 0) == -1 and lib.mvsnerf_mesh_rgb_u8_fwd(ok, -1, ok, 0) == -1
    assert lib.mvsnerf_mesh_rgb_u8_fwd(ok, 1 << 31, ok, 0) == -2 and lib.mvsnerf_mesh_rgb_u8_fwd(ok + 4, 4, ok, 0) == -3
