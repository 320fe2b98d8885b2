"""CPU-only: the Python surface of the TSDF feature (mvsnerf_amd/geometry.py) - what fuse_tsdf, tsdf_mesh and extract_mesh(valid=) refuse
before the library is touched, and the new entries in the ctypes table and the internal header."""
import ctypes
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
BOX = ((-1.0, -1.0, -1.0), (1.0, 2.0, 3.0))


def _no_library(monkeypatch):
    """Any touch of the library from here on fails the test: the refusals below must come first."""
    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)


@pytest.fixture()
def scene():
    c2w, K = R.rig_cameras(H, W, M)
    return SceneRays(np.zeros((M, H, W, 3), np.uint8), c2w, K, (400.0, 900.0), device="cpu")


def test_fuse_tsdf_refusals_come_before_the_library(monkeypatch, scene):
    _no_library(monkeypatch)
    d = torch.ones((M, H, W))
    fuse = lambda depths=d, box=BOX, dims=(4, 4, 4), **kw: geometry.fuse_tsdf(scene, depths, box, dims, **kw)
    with pytest.raises(TypeError, match="fuse_tsdf: depths must be a float32"):
        fuse(d.double())
    with pytest.raises(TypeError, match="float32"):
        fuse(d.numpy())
    for bad in (d[:, :-1], d[0]):
        with pytest.raises(ValueError, match=rf"\({M},{H},{W}\)"):
            fuse(bad)
    with pytest.raises(ValueError, match="bank's device"):
        fuse(torch.empty((M, H, W), device="meta"))
    with pytest.raises(ValueError, match="valid must be"):
        fuse(valid=torch.ones((M, H, W + 1), dtype=torch.bool))
    with pytest.raises(TypeError, match="valid must be a bool or uint8"):
        fuse(valid=torch.ones((M, H, W)))
    with pytest.raises(ValueError, match="bank's device"):
        fuse(valid=torch.empty((M, H, W), dtype=torch.uint8, device="meta"))
    for box in ((0, 0, 0), ((0, 0, 0), (1, 1, float("nan"))), ((0, 0, 0), (1, float("inf"), 1)), torch.zeros((2, 4))):
        with pytest.raises(ValueError, match="box must be"):
            fuse(box=box)
    for box in (((0, 0, 0), (1, 1, 0)), ((0, 0, 0), (1, -1, 1)), ((1, 1, 1), (0, 0, 0))):
        with pytest.raises(ValueError, match="hi > lo"):
            fuse(box=box)
    for dims in ((4, 4), (4, 4, 1), (1, 4, 4), (4, 4, 4, 4), 7, (4, 4.5, 4), ("a", 4, 4)):
        with pytest.raises(ValueError, match="dims must be"):
            fuse(dims=dims)
    with pytest.raises(ValueError, match="2\\^27"):
        fuse(dims=(513, 512, 512))
    for trunc in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="trunc"):
            fuse(trunc=trunc)
    for z_min in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="z_min"):
            fuse(z_min=z_min)
    for views in ([], [[0, 1]], [0.5, 1.0], [0, M], [-1, 2], [1, 1], 3):
        with pytest.raises(ValueError, match="views must"):
            fuse(views=views)


def test_tsdf_mesh_refusals_come_before_the_library(monkeypatch):
    _no_library(monkeypatch)
    vol = geometry.TSDFVolume(torch.ones((3, 4, 5)), torch.zeros((3, 4, 5), dtype=torch.int32), torch.zeros((3, 4, 5, 4), dtype=torch.uint8),
                              torch.tensor(BOX), 0.5)
    with pytest.raises(TypeError, match="TSDFVolume"):
        geometry.tsdf_mesh(vol.tsdf)
    for mw in (0, -1, 1.5):
        with pytest.raises(ValueError, match="min_weight"):
            geometry.tsdf_mesh(vol, min_weight=mw)
    for cap in (7, (1,), (-1, 5), ("a", 1)):
        with pytest.raises(ValueError, match="capacity"):
            geometry.tsdf_mesh(vol, capacity=cap)
    with pytest.raises(TypeError, match="float32"):
        geometry.tsdf_mesh(geometry.TSDFVolume(vol.tsdf.double(), vol.weight, vol.colors, vol.box, 0.5))


def test_extract_mesh_refuses_a_bad_mask_before_the_library(monkeypatch):
    _no_library(monkeypatch)
    f = torch.zeros((3, 4, 5))
    for bad in (torch.ones((3, 4, 5)), torch.ones((3, 4, 5), dtype=torch.int32), np.ones((3, 4, 5), np.uint8)):
        with pytest.raises(TypeError, match="valid must be a bool or uint8"):
            geometry.extract_mesh(f, 0.0, valid=bad)
    for bad in (torch.ones((3, 4, 4), dtype=torch.bool), torch.ones((60,), dtype=torch.uint8), torch.ones((1, 3, 4, 5), dtype=torch.bool)):
        with pytest.raises(ValueError, match=r"valid must be \(3,4,5\)"):
            geometry.extract_mesh(f, 0.0, valid=bad)
    with pytest.raises(ValueError, match="field's device"):
        geometry.extract_mesh(f, 0.0, valid=torch.empty((3, 4, 5), dtype=torch.bool, device="meta"))


def test_new_entries_are_bound_and_declared():
    names = {"mvsnerf_mesh_extract_masked_fwd": 17, "mvsnerf_tsdf_integrate_fwd": 21, "mvsnerf_tsdf_vertex_colors_fwd": 10}
    header = open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    stable = open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read()
    for n, n_args in names.items():
        assert n in _lib.SIGNATURES and n not in stable
        decl = re.search(rf"\b{n}\s*\(([^)]*)\)", code)
        assert decl and len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[n][1])


def test_the_entries_refuse_bad_arguments_without_a_gpu():
    """The argument checks come before the first launch, so they can be asked on a machine without a GPU."""
    lib = _lib.lib()
    ok = 1 << 12                                                    # any aligned non-null address: a refused call dereferences nothing
    box = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    order = (("depth", ok), ("valid", 0), ("images", ok), ("alpha", 1), ("w2c", ok), ("K", ok), ("view_ids", 0), ("n_views", 0), ("M", 3), ("H_img", 6),
             ("W_img", 8), ("box", box), ("D", 4), ("H", 4), ("W", 4), ("trunc", 0.5), ("z_min", 0.0), ("tsdf", ok), ("weight", ok), ("colors", ok), ("stream", 0))
    call = lambda **kw: lib.mvsnerf_tsdf_integrate_fwd(*[kw.get(k, d) for k, d in order])
    for kw in ({"depth": 0}, {"images": 0}, {"w2c": 0}, {"K": 0}, {"box": None}, {"tsdf": 0}, {"weight": 0}, {"colors": 0}):
        assert call(**kw) == -1, kw
    nan_box = (ctypes.c_float * 6)(0, 0, 0, 1, float("nan"), 1)
    for kw in ({"D": 1}, {"H": 1}, {"W": 0}, {"D": 513, "H": 512, "W": 512}, {"trunc": 0.0}, {"trunc": -1.0}, {"trunc": float("nan")}, {"trunc": float("inf")},
               {"z_min": -1.0}, {"z_min": float("nan")}, {"M": 0}, {"H_img": 0}, {"W_img": 0}, {"view_ids": ok, "n_views": 0}, {"box": nan_box}):
        assert call(**kw) == -2, kw
    for kw in ({"depth": ok + 2}, {"images": ok + 1}, {"w2c": ok + 2}, {"K": ok + 1}, {"view_ids": ok + 2, "n_views": 2}, {"tsdf": ok + 2}, {"weight": ok + 1},
               {"colors": ok + 2}):
        assert call(**kw) == -3, kw
    order = (("tsdf", ok), ("node_colors", ok), ("D", 4), ("H", 4), ("W", 4), ("vertex_edge", ok), ("count", ok), ("rows", 8), ("colors", ok), ("stream", 0))
    call = lambda **kw: lib.mvsnerf_tsdf_vertex_colors_fwd(*[kw.get(k, d) for k, d in order])
    for kw in ({"tsdf": 0}, {"node_colors": 0}, {"count": 0}, {"vertex_edge": 0}, {"colors": 0}, {"rows": -1}):
        assert call(**kw) == -1, kw
    for kw in ({"D": 1}, {"W": 1}, {"D": 513, "H": 512, "W": 512}, {"rows": 1 << 31}):
        assert call(**kw) == -2, kw
    for kw in ({"tsdf": ok + 2}, {"node_colors": ok + 1}, {"vertex_edge": ok + 4}, {"count": ok + 4}):
        assert call(**kw) == -3, kw
    # the masked mesher: the unmasked entry's checks, and a mask needs no alignment
    order = (("field", ok), ("valid", ok + 1), ("D", 4), ("H", 4), ("W", 4), ("level", 0.0), ("positions", 0), ("box", None), ("cap_v", 8), ("cap_f", 8),
             ("vertices", ok), ("ndc", ok), ("vertex_edge", ok), ("faces", ok), ("count", ok), ("workspace", ok), ("stream", 0))
    call = lambda **kw: lib.mvsnerf_mesh_extract_masked_fwd(*[kw.get(k, d) for k, d in order])
    assert call(field=0) == -1 and call(count=0) == -1 and call(D=1) == -2 and call(level=float("nan")) == -2 and call(field=ok + 2) == -3
