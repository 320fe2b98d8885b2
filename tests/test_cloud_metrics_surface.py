"""CPU-only: the Python surface of the cloud scores (geometry.PointGrid, geometry.sample_mesh, evaluate.cloud_metrics) - the new entries in the
ctypes table and the internal header, what is refused before the library is touched, the host-side queries and refusals of the C entries, and the grid
layout the host chooses."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mvsnerf_amd import _lib, evaluate, geometry, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mvsnerf_grid_bounds_workspace_bytes": 1, "mvsnerf_grid_bounds_fwd": 5, "mvsnerf_grid_build_workspace_bytes": 4, "mvsnerf_grid_build_fwd": 11,
         "mvsnerf_grid_nearest_fwd": 13, "mvsnerf_cloud_metrics_workspace_bytes": 1, "mvsnerf_cloud_metrics_fwd": 7,
         "mvsnerf_mesh_sample_workspace_bytes": 1, "mvsnerf_mesh_sample_fwd": 12}


def _no_library(monkeypatch):
    """Any touch of the library from here on fails the test: the refusals below must come first."""
    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)


def test_new_entries_are_bound_and_declared():
    header = open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    stable = open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read()
    for n, n_args in NAMES.items():
        assert n in _lib.SIGNATURES and re.search(rf"\b{n}\s*\(", code) and n not in stable
        assert len(_lib.SIGNATURES[n][1]) == n_args
        decl = re.search(rf"\b{n}\s*\(([^)]*)\)", code).group(1)
        assert len(decl.split(",")) == n_args, n                                    # the binding has the header's number of arguments
    assert _lib.lib().mvsnerf_abi_version() == 12                                   # the internal tier grows without an ABI bump
    mk = open(os.path.join(ROOT, "mvsnerf_amd", "csrc", "Makefile")).read()
    assert "build/cloud_metrics.o: cloud_metrics.hip" in mk


def test_point_grid_refusals_come_before_the_library(monkeypatch):
    _no_library(monkeypatch)
    p = torch.zeros((5, 3))
    for bad in (p.double(), p.int(), torch.zeros((5, 4)), torch.zeros((5,)), torch.zeros((2, 5, 3)), p.numpy(), None):
        with pytest.raises(ValueError, match=r"float32 tensor of shape \(n,3\)"):
            geometry.PointGrid(bad, 1.0)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e30, 1e-30, "far"):          # 1e30, 1e-30: the fp32 square is not a finite, positive number
        with pytest.raises(ValueError, match="max_dist"):
            geometry.PointGrid(p, bad)
    for bad in (0.0, -2.0, float("nan"), float("inf"), 1e-44):
        with pytest.raises(ValueError, match="cell must be"):
            geometry.PointGrid(p, 1.0, cell=bad)
    for bad in ((0, 0, 0), ((0, 0, 0), (1, 1, float("nan"))), ((0, 0, 0), (1, -1, 1)), torch.zeros((2, 4))):
        with pytest.raises(ValueError, match="box must be"):
            geometry.PointGrid(p, 1.0, box=bad)


def test_nearest_refusals_come_before_the_library(monkeypatch):
    grid = object.__new__(geometry.PointGrid)                                       # (building one needs the GPU)
    grid.device, grid.max_dist = torch.device("cpu"), 1.0
    _no_library(monkeypatch)
    for bad in (torch.zeros((4, 3)).double(), torch.zeros((4, 2)), torch.zeros((3,))):
        with pytest.raises(ValueError, match=r"query must be a float32 tensor of shape \(n,3\)"):
            grid.nearest(bad)
    with pytest.raises(ValueError, match="grid's device"):
        grid.nearest(torch.zeros((4, 3), device="meta"))


def _mesh(vertices=None, faces=None):
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=torch.float32) if vertices is None else vertices
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32) if faces is None else faces
    return geometry.TriangleMesh(v, None, f, None, None)


def test_sample_mesh_refusals_come_before_the_library(monkeypatch):
    _no_library(monkeypatch)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60, "fine"):
        with pytest.raises(ValueError, match="spacing must be"):
            geometry.sample_mesh(_mesh(), bad)
    with pytest.raises(ValueError, match="TriangleMesh"):
        geometry.sample_mesh(torch.zeros((3, 3)), 0.1)
    with pytest.raises(ValueError, match="mesh.vertices"):
        geometry.sample_mesh(_mesh(vertices=torch.zeros((3, 3)).double()), 0.1)
    for bad in (torch.zeros((1, 3), dtype=torch.int64), torch.zeros((1, 4), dtype=torch.int32), torch.zeros((3,), dtype=torch.int32)):
        with pytest.raises(ValueError, match="mesh.faces"):
            geometry.sample_mesh(_mesh(faces=bad), 0.1)
    for bad in (-1, 1 << 31):
        with pytest.raises(ValueError, match="capacity"):
            geometry.sample_mesh(_mesh(), 0.1, capacity=bad)


def test_cloud_metrics_refusals_come_before_the_library(monkeypatch):
    _no_library(monkeypatch)
    p = torch.zeros((5, 3))
    for bad in (0.0, -3.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_dist"):
            evaluate.cloud_metrics(p, p, bad)
    for bad in ((), [], (1.0,) * 9, (1.0, float("nan")), 2.0, ("a",)):
        with pytest.raises(ValueError, match="taus"):
            evaluate.cloud_metrics(p, p, 1.0, taus=bad)
    for bad in (p.double(), torch.zeros((5, 2)), torch.zeros((3,)), None, geometry.PointCloud(p.half(), *[None] * 8)):
        with pytest.raises(ValueError, match=r"pred must be a float32 tensor of shape \(n,3\)"):
            evaluate.cloud_metrics(bad, p, 1.0)
        with pytest.raises(ValueError, match=r"gt must be a float32 tensor of shape \(n,3\)"):
            evaluate.cloud_metrics(p, bad, 1.0)
    with pytest.raises(ValueError, match="spacing="):
        evaluate.cloud_metrics(_mesh(), p, 1.0)
    with pytest.raises(ValueError, match="spacing="):
        evaluate.cloud_metrics(p, _mesh(), 1.0)
    with pytest.raises(ValueError, match="spacing must be"):
        evaluate.cloud_metrics(p, _mesh(), 1.0, spacing=0.0)
    with pytest.raises(ValueError, match="grids must be a pair"):
        evaluate.cloud_metrics(p, p, 1.0, grids=(None, None))
    grid = object.__new__(geometry.PointGrid)
    grid.max_dist, grid.n, grid.device = 2.0, 5, p.device
    with pytest.raises(ValueError, match="grids were built for max_dist"):
        evaluate.cloud_metrics(p, p, 1.0, grids=(grid, grid))
    grid.max_dist = 1.0
    with pytest.raises(ValueError, match="grids hold"):
        evaluate.cloud_metrics(p[:4], p, 1.0, grids=(grid, grid))


def test_grid_layout_grows_the_edge_to_the_cap():
    lo, cell, dims = geometry._grid_layout((0, 0, 0), (10, 10, 10), 1.0, geometry.GRID_CELL_CAP)
    assert lo == [0.0, 0.0, 0.0] and cell == 1.0 and dims == (11, 11, 11)
    lo, cell, dims = geometry._grid_layout((0, 0, 0), (0, 0, 0), 0.5, geometry.GRID_CELL_CAP)
    assert dims == (1, 1, 1)                                                        # a cloud of one position
    lo, cell, dims = geometry._grid_layout((-1, 2, 3), (1e6, 2, 1e6), 1e-3, geometry.GRID_CELL_CAP)
    assert dims[1] == 1 and dims[0] * dims[2] <= geometry.GRID_CELL_CAP < 1.6 * dims[0] * dims[2] and cell > 1e-3
    assert geometry.GRID_CELL_CAP <= ops.GRID_MAX_CELLS
    assert float(np.float32(cell)) == cell and all(float(np.float32(v)) == v for v in lo)


def test_workspace_queries_run_without_a_gpu():
    lib = _lib.lib()
    q = lib.mvsnerf_grid_bounds_workspace_bytes
    assert q(-1) == 0 and q(1 << 31) == 0 and q(0) == 24 and q(2048) == 24 and q(2049) == 48
    q = lib.mvsnerf_grid_build_workspace_bytes
    assert q(10, 0, 1, 1) == 0 and q(10, 1, 1, -1) == 0 and q(1 << 31, 1, 1, 1) == 0 and q(-1, 1, 1, 1) == 0
    assert q(10, 256, 256, 257) == 0 and q(10, 1 << 20, 1 << 20, 1) == 0          # more than 2^24 cells
    assert q(0, 1, 1, 1) == 4 * (1 + 1) and q(10, 256, 256, 256) == 4 * ((1 << 24) + (1 << 13) + 1) and q(10, 2047, 1, 1) == 4 * (2047 + 1)
    q = lib.mvsnerf_cloud_metrics_workspace_bytes
    assert q(-1) == 0 and q(1 << 31) == 0 and q(0) == 80 and q(8192) == 80 and q(8193) == 160
    q = lib.mvsnerf_mesh_sample_workspace_bytes
    assert q(-1) == 0 and q(1 << 31) == 0 and q(0) == 8 and q(256) == 8 * (256 + 2) + 4 + 8 and q(257) == 8 * (257 + 4) + 8 + 8


def test_c_entries_refuse_on_the_host():
    """Every refusal of the new entries comes before the first launch, so it can be exercised without a GPU: made-up, suitably aligned addresses stand for
    device memory, and a refused call never dereferences them."""
    lib = _lib.lib()
    A = 0x10000                                                                     # 64 KiB aligned; A + 4, A + 8, A + 2: misaligned for 8, 16, 4
    EINVAL, EUNSUP, EALIGN = -1, -2, -3
    big = 1 << 31
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    nan3 = (ctypes.c_float * 3)(0, float("nan"), 0)
    t2 = (ctypes.c_float * 2)(1, 2)
    b = lib.mvsnerf_grid_bounds_fwd
    assert b(0, 5, A, A, 0) == EINVAL and b(A, 5, 0, A, 0) == EINVAL and b(A, 5, A, 0, 0) == EINVAL and b(A, -1, A, A, 0) == EINVAL
    assert b(A, big, A, A, 0) == EUNSUP and b(A + 2, 5, A, A, 0) == EALIGN and b(A, 5, A + 2, A, 0) == EALIGN and b(A, 5, A, A + 1, 0) == EALIGN
    g = lib.mvsnerf_grid_build_fwd
    ok = [A, 5, f3, 1.0, 2, 2, 2, A, A, A, 0]

    def alt(args, **kw):
        out = list(args)
        for k, v in kw.items():
            out[int(k[1:])] = v
        return out
    for k in (0, 2, 7, 8, 9):
        assert g(*alt(ok, **{f"a{k}": None if k == 2 else 0})) == EINVAL, k
    assert g(*alt(ok, a1=-1)) == EINVAL
    for kw in ({"a1": big}, {"a4": 0}, {"a5": -1}, {"a4": 4096, "a5": 4096, "a6": 2}, {"a3": 0.0}, {"a3": -1.0}, {"a3": float("nan")}, {"a3": float("inf")},
               {"a3": 1e-44}, {"a2": nan3}):
        assert g(*alt(ok, **kw)) == EUNSUP, kw
    for k, off in ((0, 2), (7, 2), (8, 8), (9, 2)):
        assert g(*alt(ok, **{f"a{k}": A + off})) == EALIGN, k
    n = lib.mvsnerf_grid_nearest_fwd
    ok = [f3, 1.0, 2, 2, 2, A, A, A, 7, 0.5, A, A, 0]
    for k in (0, 5, 7, 10, 11):
        assert n(*alt(ok, **{f"a{k}": None if k == 0 else 0})) == EINVAL, k
    assert n(*alt(ok, a8=-1)) == EINVAL
    for kw in ({"a8": big}, {"a2": 0}, {"a2": 1 << 12, "a3": 1 << 12, "a4": 2}, {"a1": 0.0}, {"a1": float("nan")}, {"a0": nan3}, {"a9": 0.0}, {"a9": -1.0},
               {"a9": float("inf")}, {"a9": float("nan")}, {"a9": 1e30}):
        assert n(*alt(ok, **kw)) == EUNSUP, kw
    for k, off in ((5, 2), (6, 8), (7, 2), (10, 2), (11, 2)):
        assert n(*alt(ok, **{f"a{k}": A + off})) == EALIGN, k
    assert n(*alt(ok, a6=0, a7=0, a8=0, a10=0, a11=0)) == 0                         # no query: nothing is launched (an empty grid has no records either)
    m = lib.mvsnerf_cloud_metrics_fwd
    ok = [A, 9, t2, 2, A, A, 0]
    for k in (0, 2, 4, 5):
        assert m(*alt(ok, **{f"a{k}": None if k == 2 else 0})) == EINVAL, k
    assert m(*alt(ok, a1=-1)) == EINVAL and m(*alt(ok, a3=-1)) == EINVAL
    assert m(*alt(ok, a1=big)) == EUNSUP and m(*alt(ok, a3=9)) == EUNSUP
    for k, off in ((0, 2), (4, 4), (5, 4)):
        assert m(*alt(ok, **{f"a{k}": A + off})) == EALIGN, k
    s = lib.mvsnerf_mesh_sample_fwd
    ok = [A, 3, A, 1, A, 0.5, 4, A, A, A, A, 0]
    for k in (0, 2, 7, 8, 9, 10):
        assert s(*alt(ok, **{f"a{k}": 0})) == EINVAL, k
    for k in (1, 3, 6):
        assert s(*alt(ok, **{f"a{k}": -1})) == EINVAL, k
        assert s(*alt(ok, **{f"a{k}": big})) == EUNSUP, k
    for sp in (0.0, -1.0, float("nan"), float("inf")):
        assert s(*alt(ok, a5=sp)) == EUNSUP
    for k, off in ((0, 2), (2, 2), (4, 4), (7, 2), (8, 2), (9, 4), (10, 4)):
        assert s(*alt(ok, **{f"a{k}": A + off})) == EALIGN, k
