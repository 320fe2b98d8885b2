"""CPU-only: the surface of the renderer-consistent density volume - symbols, argument codes of the two C entries, and the Python refusals that come
before the library."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvsnerf_voxel_points_fwd", "mvsnerf_max_dilate3d_fwd")
OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
PTR = 0x10000        # non-NULL, 16-byte aligned, never dereferenced (device pointers: every refusal comes before a launch)


def test_symbols_are_declared_exported_and_bound():
    from mvsnerf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read(), flags=re.S)
    stable = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert not re.search(rf"\b{name}\s*\(", stable), name            # internal tier only: the stable header and its ABI number do not change
        assert name in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(SYMBOLS) <= {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert _lib.lib().mvsnerf_abi_version() == 12
    from mvsnerf_amd import ops
    assert callable(ops.voxel_points) and callable(ops.max_dilate3d) and callable(ops.node_density)


def test_entries_refuse_bad_arguments_before_any_launch():
    from mvsnerf_amd import _lib
    L = _lib.lib()
    # the camera arrays are HOST memory and are read by the entry: real arrays here
    K = (ctypes.c_float * 9)(100.0, 0.0, 48.0, 0.0, 100.0, 32.0, 0.0, 0.0, 1.0)
    singular = (ctypes.c_float * 9)(1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 0.0, 0.0, 1.0)
    nan_k = (ctypes.c_float * 9)(float("nan"), 0.0, 48.0, 0.0, 100.0, 32.0, 0.0, 0.0, 1.0)
    c2w = (ctypes.c_float * 16)(1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    nf, nf_zero, nf_inf = (ctypes.c_float * 2)(2.0, 6.0), (ctypes.c_float * 2)(0.0, 6.0), (ctypes.c_float * 2)(2.0, float("inf"))
    addr = lambda a: 0 if a is None else ctypes.addressof(a)

    def points(D=4, H=6, W=8, d0=0, d1=4, K=K, c2w=c2w, nf=nf, W_img=96, H_img=64, pad=2, lindisp=0, ndc=PTR, pts=PTR):
        return L.mvsnerf_voxel_points_fwd(D, H, W, d0, d1, addr(K), addr(c2w), addr(nf), W_img, H_img, pad, lindisp, ndc, pts, None)
    for kw in (dict(ndc=0), dict(D=0), dict(H=0), dict(W=-1), dict(d0=-1), dict(d1=5), dict(d0=3, d1=2), dict(K=None), dict(c2w=None), dict(nf=None),
               dict(W_img=1), dict(H_img=0), dict(pad=-1), dict(K=singular), dict(K=nan_k), dict(nf=nf_inf), dict(nf=nf_zero, lindisp=1)):
        assert points(**kw) == EINVAL, kw
    assert points(D=2 ** 11, H=2 ** 10, W=2 ** 10, d1=1) == EUNSUPPORTED          # 2^31 nodes, whatever the plane range
    assert points(ndc=PTR + 2) == EALIGN and points(pts=PTR + 1) == EALIGN
    assert points(d0=2, d1=2) == OK                                              # an empty range: nothing launched
    assert points(d0=2, d1=2, pts=0, K=None, c2w=None, nf=None) == OK            # the ndc-only form needs no camera
    assert points(nf=nf_zero, d0=1, d1=1) == OK                                  # a zero near plane is refused under lindisp only

    def dilate(src=PTR, D=4, H=6, W=8, r=1, out=PTR + 0x1000, ws=PTR + 0x2000):
        return L.mvsnerf_max_dilate3d_fwd(src, D, H, W, r, out, ws, None)
    for kw in (dict(src=0), dict(out=0), dict(ws=0), dict(D=0), dict(H=-2), dict(W=0), dict(r=-1), dict(r=3), dict(out=PTR), dict(ws=PTR),
               dict(ws=PTR + 0x1000), dict(out=PTR, r=0, ws=0)):
        assert dilate(**kw) == EINVAL, kw
    assert dilate(D=2 ** 11, H=2 ** 10, W=2 ** 10) == EUNSUPPORTED
    assert dilate(src=PTR + 2) == EALIGN and dilate(out=PTR + 0x1001) == EALIGN and dilate(ws=PTR + 0x2002) == EALIGN


def _bare(cls):
    """A system built without its constructor (that builds networks): the refusals need nothing of it."""
    from mvsnerf_amd import train
    s = getattr(train, cls).__new__(getattr(train, cls))
    torch.nn.Module.__init__(s)
    return s


def test_python_faces_refuse_before_the_library(monkeypatch):
    from mvsnerf_amd import _lib, ops

    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.max_dilate3d(torch.zeros((2, 3, 4), requires_grad=True), 1)
    with pytest.raises(ValueError, match="r must be"):
        ops.max_dilate3d(torch.zeros((2, 3, 4)), 3)
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.node_density(torch.zeros((2, 3, 4, 20), requires_grad=True), None, torch.zeros((3, 4, 4)))
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.node_density(torch.zeros((2, 3, 4, 8)), None, torch.zeros((3, 4, 4)), imgs=torch.zeros((3, 3, 8, 8), requires_grad=True),
                         intrinsics=torch.zeros((3, 3, 3)), camera={})
    with pytest.raises(ValueError, match="dilate"):
        ops.node_density(torch.zeros((2, 3, 4, 20)), None, torch.zeros((3, 4, 4)), dilate=3)
    with pytest.raises(RuntimeError, match="planes"):
        ops.voxel_points(4, 5, 6, planes=(3, 2))

    mv = _bare("MVSSystem")
    batch = {}
    with pytest.raises(ValueError, match="NaN"):
        mv.render_view(batch, skip_empty=float("nan"))
    with pytest.raises(ValueError, match="whole_frame_off"):
        mv.render_view(batch, skip_empty=0.0, whole_frame_off=True)
    with pytest.raises(ValueError, match="skip_empty"):
        mv.render_view(batch, density=torch.zeros((4, 4, 4)))
    with pytest.raises(RuntimeError, match="density"):
        mv.render_view(batch, skip_empty=0.0, density=torch.zeros((4, 4, 5)), volume=torch.zeros((1, 8, 4, 4, 4)))
    with pytest.raises(RuntimeError, match="density"):
        mv.render_view(batch, skip_empty=0.0, density=torch.zeros((1, 4, 4, 4)))
    with pytest.raises(ValueError, match="NaN"):
        mv.render_path_skip_empty(batch, torch.eye(4)[None], float("nan"))
    with pytest.raises(TypeError, match="chunk"):
        mv.render_path_skip_empty(batch, torch.eye(4)[None], 0.0, chunk=5)
    fu = _bare("MVSSystemFusion")
    with pytest.raises(ValueError, match="NaN"):
        fu.render_rays(torch.zeros((5, 8)), skip_empty=float("nan"))
