"""CPU-only: the surface of the device resampler and the source-view kernel - symbols, argument codes, signatures and the refusals that
come before the library."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvsnerf_resample_u8_workspace_bytes", "mvsnerf_resample_u8_fwd", "mvsnerf_source_images_fwd")
OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
PTR = 0x10000        # non-NULL, 16-byte aligned, never dereferenced


def test_symbols_are_declared_exported_and_bound_and_the_stable_tier_is_unchanged():
    from mvsnerf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read(), flags=re.S)
    stable = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert not re.search(rf"\b{name}\s*\(", stable), name            # internal tier only
        assert name in _lib.SIGNATURES
    assert "resample_u8" not in stable and "source_images" not in stable
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(SYMBOLS) <= {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert _lib.lib().mvsnerf_abi_version() == 12


def test_resample_entry_refuses_bad_arguments_before_any_launch():
    from mvsnerf_amd import _lib
    L = _lib.lib()

    def fwd(src=PTR, M=3, Hin=37, Win=53, dst=PTR, Hout=12, Wout=16, xwin=PTR, xkk=PTR, xks=21, ywin=PTR, ykk=PTR, yks=21, mode=0, work=PTR):
        return L.mvsnerf_resample_u8_fwd(src, M, Hin, Win, dst, Hout, Wout, xwin, xkk, xks, ywin, ykk, yks, mode, work, None)
    # NULL pointers, sizes < 1, an unknown alpha_mode
    for kw in (dict(src=0), dict(dst=0), dict(M=0), dict(Hin=0), dict(Win=0), dict(Hout=0), dict(Wout=0), dict(M=-1), dict(Wout=-4), dict(mode=2), dict(mode=-1),
               dict(xwin=0), dict(xkk=0), dict(xks=0), dict(ywin=0), dict(ykk=0), dict(yks=0), dict(yks=-2), dict(work=0)):
        assert fwd(**kw) == EINVAL, kw
    # the tables of an axis that keeps its size are not needed, the workspace only when both passes run
    for kw in (dict(Wout=53, xwin=0, xks=0, yks=0), dict(Hout=37, ywin=0, xks=0, yks=0), dict(Wout=53, work=0, ywin=0), dict(Hout=37, work=0, xkk=0)):
        assert fwd(**kw) == EINVAL, kw
    # src, dst, the workspace and the tables are read and written as 32-bit words
    for kw in (dict(src=PTR + 2), dict(dst=PTR + 1), dict(work=PTR + 2), dict(xwin=PTR + 2), dict(xkk=PTR + 1), dict(ywin=PTR + 3), dict(ykk=PTR + 2)):
        assert fwd(**kw) == EALIGN, kw
    # per-image pixel counts beyond 2^31 - 1 (source, horizontal pass's output, result), a pass beyond 2^38 pixels, ksize beyond 65535
    for kw in (dict(Hin=2 ** 16, Win=2 ** 15), dict(Hin=2 ** 16, Wout=2 ** 15), dict(Hout=2 ** 16, Wout=2 ** 15), dict(Hin=2 ** 31 - 1, Win=2 ** 31 - 1),
               dict(M=2 ** 20, Hin=2 ** 10, Win=2 ** 9), dict(M=2 ** 20, Hout=2 ** 10, Wout=2 ** 9), dict(xks=65536), dict(yks=2 ** 31 - 1)):
        assert fwd(**kw) == EUNSUPPORTED, kw

    def ws(M=3, Hin=37, Win=53, Hout=12, Wout=16):
        return L.mvsnerf_resample_u8_workspace_bytes(M, Hin, Win, Hout, Wout)
    assert ws() == 3 * 37 * 16 * 4                                       # the horizontal pass's output
    assert ws(Hout=37) == 0 and ws(Wout=53) == 0 and ws(Hout=37, Wout=53) == 0      # one pass, or the copy
    assert ws(M=0) == 0 and ws(Wout=-1) == 0 and ws(Hin=2 ** 16, Win=2 ** 15) == 0  # nothing for what the entry refuses
    assert ws(M=2 ** 8, Hin=2 ** 15, Win=2 ** 15, Hout=2 ** 14, Wout=2 ** 15 - 1) == 2 ** 8 * 2 ** 15 * (2 ** 15 - 1) * 4    # beyond 32 bits


def test_source_images_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    from mvsnerf_amd import _lib
    L = _lib.lib()
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def fwd(images=PTR, ids=PTR, V=3, M=4, H=20, W=28, mean=f3, std=f3, out=PTR):
        return L.mvsnerf_source_images_fwd(images, ids, V, M, H, W, mean, std, out, None)
    for kw in (dict(images=0), dict(ids=0), dict(out=0), dict(mean=None), dict(std=None), dict(V=0), dict(M=0), dict(H=0), dict(W=-1)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(images=PTR + 2), dict(ids=PTR + 4), dict(out=PTR + 1)):
        assert fwd(**kw) == EALIGN, kw
    for kw in (dict(H=2 ** 16, W=2 ** 15), dict(V=2 ** 20, H=2 ** 10, W=2 ** 9)):
        assert fwd(**kw) == EUNSUPPORTED, kw


def test_signatures():
    from mvsnerf_amd import ops, rays
    p = inspect.signature(ops.resample_u8).parameters
    assert list(p) == ["src", "size_hw", "resample", "premultiply", "out"]
    assert p["resample"].default == "lanczos" and p["premultiply"].default is False and p["out"].default is None
    p = inspect.signature(rays.SceneRays.from_images).parameters
    assert list(p) == ["images", "c2ws", "intrinsics", "near_far", "img_wh", "resample", "depths", "device"]
    assert p["resample"].default == "lanczos" and p["depths"].default is None and p["device"].default == "cuda"
    p = inspect.signature(rays.SceneRays.source_views).parameters
    assert list(p) == ["self", "ids", "on_device"] and p["on_device"].default is False


def test_python_refuses_before_the_library(monkeypatch):
    from mvsnerf_amd import _lib, ops
    from mvsnerf_amd.rays import SceneRays

    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)
    M, H, W = 2, 8, 10
    c2ws, K, nf = torch.eye(4).expand(M, 4, 4), torch.eye(3), torch.tensor([2.0, 6.0])
    u8 = np.zeros((M, H, W, 3), dtype=np.uint8)
    kw = dict(img_wh=(5, 4), device="cpu")
    for bad in (u8.astype(np.float32), u8.astype(np.float64) / 255, u8.astype(np.float16), u8.astype(np.int32), torch.zeros((M, H, W, 4))):
        with pytest.raises(TypeError, match="uint8"):                    # a float image would be quantised silently
            SceneRays.from_images(bad, c2ws, K, nf, **kw)
    with pytest.raises(TypeError, match="uint8"):                        # a sequence with one member that is not 8-bit
        SceneRays.from_images([u8[0], np.zeros((6, 7, 3), dtype=np.float32)], c2ws, K, nf, **kw)
    for resample in ("bicubic", "LANCZOS", None, 1):
        with pytest.raises(ValueError, match="resample"):
            SceneRays.from_images(u8, c2ws, K, nf, resample=resample, **kw)
    for wh in ((0, 4), (5, 0), (-1, 4)):
        with pytest.raises(ValueError, match="img_wh"):
            SceneRays.from_images(u8, c2ws, K, nf, img_wh=wh, device="cpu")
    for shape in ((M, H, W, 1), (M, H, W, 5), (M, H, W)):
        with pytest.raises(ValueError, match="image"):
            SceneRays.from_images(np.zeros(shape, dtype=np.uint8), c2ws, K, nf, **kw)
    with pytest.raises(ValueError, match="channel"):                     # RGB and RGBA members mixed
        SceneRays.from_images([u8[0], np.zeros((6, 7, 4), dtype=np.uint8)], c2ws, K, nf, **kw)
    with pytest.raises(ValueError, match="no images"):
        SceneRays.from_images([], c2ws, K, nf, **kw)
    with pytest.raises(ValueError, match="tall"):                        # Pillow 12 resizes these vertically first (tests/resample_refs.py)
        SceneRays.from_images(np.zeros((1, 1100, 5, 3), dtype=np.uint8), c2ws[:1], K, nf, img_wh=(3, 300), device="cpu")
    with pytest.raises(ValueError, match="c2ws"):                        # the cameras are those of the constructor: checked before any upload
        SceneRays.from_images(u8, torch.eye(4).expand(M + 1, 4, 4), K, nf, **kw)
    with pytest.raises(ValueError, match="depths"):                      # depths are those of the resized images
        SceneRays.from_images(u8, c2ws, K, nf, depths=torch.zeros((M, H, W)), **kw)
    with pytest.raises(ValueError, match="resample"):
        ops.resample_u8(torch.zeros((1, 4, 4, 4), dtype=torch.uint8), (2, 2), resample="nearest")
    with pytest.raises(RuntimeError, match="uint8"):                     # a host tensor, a float tensor
        ops.resample_u8(torch.zeros((1, 4, 4, 4), dtype=torch.uint8), (2, 2))
    with pytest.raises(IndexError):
        SceneRays(torch.from_numpy(u8), c2ws, K, nf, device="cpu").source_views([0, M], on_device=True)
