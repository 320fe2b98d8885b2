"""CPU-only: the surface of the frame writer - symbols, the default colour table, and the refusals that come before any launch."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SYMBOLS = ("mvsnerf_depth_range_workspace_floats", "mvsnerf_depth_range_fwd", "mvsnerf_frame_u8_fwd")


def test_symbols_are_declared_exported_and_bound():
    from mvsnerf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    stable = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read(), flags=re.S)
    for name in FRAME_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert not re.search(rf"\b{name}\s*\(", stable), name            # internal tier only: the stable header and ABI 12 do not change
        assert name in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(FRAME_SYMBOLS) <= {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert _lib.lib().mvsnerf_abi_version() == 12


def test_workspace_query():
    from mvsnerf_amd import _lib
    q = _lib.lib().mvsnerf_depth_range_workspace_floats
    assert q(0) == 0 and q(-5) == 0
    assert q(1) == 2 and q(1024) == 2 and q(1025) == 4            # one {min, max} pair per workgroup of 1024 elements ...
    assert q(512 * 640) == 2 * 320 and q(1 << 40) == 2 * 1024      # ... up to 1024 workgroups


def test_entries_refuse_bad_arguments_before_any_launch():
    """NULL pointers, sizes and crops are refused by the argument checks: no device is touched (there is none here)."""
    from mvsnerf_amd import _lib
    L = _lib.lib()
    EINVAL, EALIGN, EUNSUPPORTED = -1, -3, -2
    assert L.mvsnerf_depth_range_fwd(0, 4, 16, 32, None) == EINVAL
    assert L.mvsnerf_depth_range_fwd(16, 0, 16, 32, None) == EINVAL
    assert L.mvsnerf_depth_range_fwd(18, 4, 16, 32, None) == EALIGN
    f = L.mvsnerf_frame_u8_fwd
    assert f(16, 32, 4, 4, 48, 64, 0, 0, 1, 0, None) == EINVAL            # no out
    assert f(0, 0, 4, 4, 0, 0, 0, 0, 0, 80, None) == EINVAL               # no panel at all
    assert f(16, 0, 4, 4, 48, 64, 0, 0, 1, 80, None) == EINVAL            # depth panel without depth
    assert f(16, 32, 4, 4, 0, 64, 0, 0, 1, 80, None) == EINVAL            # ... without minmax
    assert f(16, 32, 4, 4, 48, 0, 0, 0, 1, 80, None) == EINVAL            # ... without a table
    assert f(16, 32, 0, 4, 48, 64, 0, 0, 1, 80, None) == EINVAL
    assert f(16, 32, 4, 4, 48, 64, 2, 0, 1, 80, None) == EINVAL           # the crop leaves no row
    assert f(16, 32, 4, 4, 48, 64, 0, -1, 1, 80, None) == EINVAL
    assert f(16, 32, 4, 4, 48, 64, 0, 0, 2, 80, None) == EINVAL
    assert f(18, 32, 4, 4, 48, 64, 0, 0, 1, 81, None) == EALIGN           # rgb; an odd `out` is fine
    assert f(16, 32, 1 << 14, 1 << 14, 48, 64, 0, 0, 1, 81, None) == EUNSUPPORTED


def test_jet_lut_closed_form():
    from mvsnerf_amd import ops
    lut = ops.jet_lut("cpu")
    assert lut.shape == (256, 3) and lut.dtype == torch.uint8 and lut.device.type == "cpu"
    # r = clamp(1.5 - |4x - 3|), g = clamp(1.5 - |4x - 2|), b = clamp(1.5 - |4x - 1|) at x = i / 255, times 255, halves rounded up
    table = {0: (0, 0, 128), 32: (0, 1, 255), 96: (2, 255, 254), 128: (130, 255, 126), 160: (255, 253, 0), 224: (252, 0, 0), 255: (128, 0, 0)}
    for i, rgb in table.items():
        assert tuple(lut[i].tolist()) == rgb, (i, lut[i].tolist())
    assert ops.jet_lut("cpu") is lut                                       # built once per device
    # the ramp in exact rationals: 255 c = 382.5 - |4 i - 765 + 255 k| clamped to [0, 255]
    from fractions import Fraction
    import math
    for i in range(256):
        for k in range(3):
            v = min(max(Fraction(765, 2) - abs(4 * i - 765 + 255 * k), 0), 255)
            assert int(lut[i, k]) == math.floor(v + Fraction(1, 2)), (i, k)


def test_python_faces_refuse_before_the_library(monkeypatch):
    from mvsnerf_amd import _lib, ops, utils

    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)
    with pytest.raises(RuntimeError, match="rgb, depth or both"):
        ops.frame_u8(None)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_u8(torch.zeros((4, 4, 3)))
    with pytest.raises(RuntimeError, match="non-empty"):
        ops.depth_range(torch.zeros((0,)))
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        utils.visualize_depth_numpy(torch.zeros((4,)))
    with pytest.raises(ValueError, match="uint8"):
        utils.save_frames(torch.zeros((2, 4, 4, 3)), "unused")
