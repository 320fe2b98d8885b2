"""CPU-only: the Python surface of the depth-fusion feature (mvsnerf_amd/geometry.py) - what fuse_depths refuses before the library is touched, the
default source-view selection, the PLY writer, and the new entries in the ctypes table and the internal header."""
import os
import re

import numpy as np
import pytest
import torch

import depth_fusion_refs as R
from mvsnerf_amd import _lib, geometry, utils
from mvsnerf_amd.rays import SceneRays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, H, W = 5, 6, 8


def _no_library(monkeypatch):
    """Any touch of the library from here on fails the test: the refusals below must come first."""
    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)


@pytest.fixture()
def scene():
    c2w, K = R.rig_cameras(H, W, M)
    return SceneRays(np.zeros((M, H, W, 3), np.uint8), c2w, K, (400.0, 900.0), device="cpu")


def test_refusals_come_before_the_library(monkeypatch, scene):
    _no_library(monkeypatch)
    d = torch.ones((M, H, W))
    with pytest.raises(TypeError, match="float32"):
        geometry.fuse_depths(scene, d.double())
    with pytest.raises(ValueError, match=rf"\({M},{H},{W}\)"):
        geometry.fuse_depths(scene, d[:, :-1])
    with pytest.raises(ValueError, match=rf"\({M},{H},{W}\)"):
        geometry.fuse_depths(scene, d[0])
    with pytest.raises(ValueError, match="bank's device"):
        geometry.fuse_depths(scene, torch.empty((M, H, W), device="meta"))
    with pytest.raises(ValueError, match="valid must be"):
        geometry.fuse_depths(scene, d, valid=torch.ones((M, H, W + 1), dtype=torch.bool))
    ids = R.default_src_ids(M, 2)
    for bad in (M, -2):
        b = ids.copy()
        b[1, 0] = bad
        with pytest.raises(ValueError, match=rf"\[0, {M}\) or -1"):
            geometry.fuse_depths(scene, d, src_ids=b)
    b = ids.copy()
    b[3, 1] = 3
    with pytest.raises(ValueError, match="view 3 as a source of itself"):
        geometry.fuse_depths(scene, d, src_ids=b)
    with pytest.raises(ValueError, match=rf"\({M}, n_src\)"):
        geometry.fuse_depths(scene, d, src_ids=ids[:-1])
    with pytest.raises(ValueError, match="1..32"):
        geometry.fuse_depths(scene, d, n_src=33)
    with pytest.raises(ValueError, match="1..32"):
        geometry.fuse_depths(scene, d, n_src=0)
    with pytest.raises(ValueError, match="1..32"):
        geometry.fuse_depths(scene, d, src_ids=np.full((M, 33), -1))
    for kw in ({"pix_thr": 0.0}, {"pix_thr": -1.0}, {"rel_thr": 0.0}, {"rel_thr": float("nan")}, {"pix_thr": float("inf")}):
        with pytest.raises(ValueError, match="finite and > 0"):
            geometry.fuse_depths(scene, d, **kw)
    with pytest.raises(ValueError, match="min_views"):
        geometry.fuse_depths(scene, d, min_views=-1)
    with pytest.raises(ValueError, match="capacity"):
        geometry.fuse_depths(scene, d, capacity=-1)


def test_default_sources_are_the_nearest_other_views(scene):
    c2w = scene._c2w64.numpy()
    for n_src in (1, 3, 4):
        ids = geometry.nearest_source_ids(scene, n_src)
        assert ids.shape == (M, n_src) and ids.dtype == np.int32
        for r in range(M):
            others = np.array([m for m in range(M) if m != r])
            want = others[utils.get_nearest_pose_ids(c2w[r:r + 1], c2w[others], n_src)[0]]
            assert (ids[r] == want).all() and r not in ids[r]
            dist = np.linalg.norm(c2w[ids[r], :3, 3] - c2w[r, :3, 3], axis=-1)
            assert (np.diff(dist) >= 0).all()                                           # nearest first
    ids = geometry.nearest_source_ids(scene, 6)                                         # more than the scene has: padded with -1
    assert (ids[:, 4:] == -1).all() and (ids[:, :4] >= 0).all()
    assert all(sorted(ids[r, :4]) == [m for m in range(M) if m != r] for r in range(M))


def _parse_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = int(re.fullmatch(r"element vertex (\d+)", lines[2]).group(1))
    assert lines[3:10] == ["property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue", ""]
    rec = np.frombuffer(body, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    assert len(rec) == n and len(body) == 15 * n
    return rec


@pytest.mark.parametrize("n", [0, 1, 257])
def test_save_ply_round_trip(tmp_path, n):
    g = np.random.default_rng(n)
    xyz = g.standard_normal((n, 3)).astype(np.float32) * 100
    rgb = g.integers(0, 256, (n, 3)).astype(np.uint8)
    path = str(tmp_path / "cloud.ply")
    assert geometry.save_ply(path, (torch.from_numpy(xyz), torch.from_numpy(rgb))) == n
    rec = _parse_ply(path)
    assert rec["xyz"].tobytes() == xyz.tobytes() and rec["rgb"].tobytes() == rgb.tobytes()
    # a PointCloud with a caller-given capacity: the first min(count, capacity) rows
    cap = n + 3
    cloud = geometry.PointCloud(torch.zeros((cap, 3)), torch.zeros((cap, 3), dtype=torch.uint8), None, None, torch.tensor([n]), None, None, None, None)
    cloud.points[:n], cloud.colors[:n] = torch.from_numpy(xyz), torch.from_numpy(rgb)
    assert geometry.save_ply(path, cloud) == n
    assert _parse_ply(path)["xyz"].tobytes() == xyz.tobytes()
    with pytest.raises(ValueError, match="save_ply"):
        geometry.save_ply(path, (xyz, rgb.astype(np.float32)))


def test_new_entries_are_bound_and_declared():
    names = ["mvsnerf_depth_consistency_fwd", "mvsnerf_point_cloud_workspace_bytes", "mvsnerf_point_cloud_fwd"]
    header = open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    stable = open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read()
    for n in names:
        assert n in _lib.SIGNATURES and re.search(rf"\b{n}\s*\(", code) and n not in stable
    assert len(_lib.SIGNATURES["mvsnerf_depth_consistency_fwd"][1]) == 18
    assert len(_lib.SIGNATURES["mvsnerf_point_cloud_fwd"][1]) == 17


def test_workspace_query_runs_without_a_gpu():
    q = _lib.lib().mvsnerf_point_cloud_workspace_bytes
    assert q(0) == 0 and q(-5) == 0 and q(1 << 31) == 0
    assert q(1) == 8 and q(1024) == 8 and q(1025) == 16 and q((1 << 31) - 1) == 8 * (1 << 21)
