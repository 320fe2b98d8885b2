"""CPU-only: the surface of empty-space skipping - symbols, the workspace query, argument codes, and the refusals that come before the library."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARSE_SYMBOLS = ("mvsnerf_live_samples_workspace_bytes", "mvsnerf_live_samples_fwd", "mvsnerf_expand_rows_fwd")
OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
PTR = 0x10000        # non-NULL, 16-byte aligned, never dereferenced


def test_symbols_are_declared_exported_and_bound():
    from mvsnerf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read(), flags=re.S)
    stable = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read(), flags=re.S)
    for name in SPARSE_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert not re.search(rf"\b{name}\s*\(", stable), name            # internal tier only: the stable header and its ABI number do not change
        assert name in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(SPARSE_SYMBOLS) <= {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert _lib.lib().mvsnerf_abi_version() == 12
    from mvsnerf_amd import ops
    assert callable(ops.live_samples) and callable(ops.expand_rows) and callable(ops.raymarch_sparse)


def test_workspace_query():
    from mvsnerf_amd import _lib
    q = _lib.lib().mvsnerf_live_samples_workspace_bytes
    per_group = 16 * 8 + 2 * 4                                   # 16 ballot words, one count, one offset per workgroup of 1024 samples
    assert q(0) == 0 and q(-3) == 0 and q(2 ** 31) == 0
    assert q(1) == per_group and q(1024) == per_group and q(1025) == 2 * per_group
    assert q(2 ** 31 - 1) == (2 ** 31 // 1024) * per_group


def test_entries_refuse_bad_arguments_before_any_launch():
    from mvsnerf_amd import _lib
    L = _lib.lib()

    def live(density=PTR, D=4, H=4, W=4, thr=0.0, ndc=PTR, pts=PTR, rays_dir=PTR, N=8, S=4, count=PTR, idx=PTR, ndc_c=PTR, pts_c=PTR, dir_c=PTR, ws=PTR):
        return L.mvsnerf_live_samples_fwd(density, D, H, W, thr, ndc, pts, rays_dir, N, S, count, idx, ndc_c, pts_c, dir_c, ws, None)
    for kw in (dict(density=0), dict(count=0), dict(ndc=0), dict(idx=0), dict(ndc_c=0), dict(ws=0), dict(pts_c=0), dict(dir_c=0), dict(D=0), dict(H=0),
               dict(W=0), dict(N=-1), dict(S=0), dict(thr=float("nan"))):
        assert live(**kw) == EINVAL, kw
    assert live(N=2 ** 24, S=128) == EUNSUPPORTED                # 2^31 samples: idx is int32
    assert live(N=2 ** 31 - 1, S=2 ** 31 - 1) == EUNSUPPORTED
    assert live(ws=PTR + 4) == EALIGN and live(ndc=PTR + 2) == EALIGN and live(idx=PTR + 1) == EALIGN

    def expand(src=PTR, idx=PTR, count=PTR, n=8, P=32, C=4, dst=PTR):
        return L.mvsnerf_expand_rows_fwd(src, idx, count, n, P, C, dst, None)
    for kw in (dict(count=0), dict(dst=0), dict(src=0), dict(idx=0), dict(n=-1), dict(n=33), dict(P=-1), dict(C=0)):
        assert expand(**kw) == EINVAL, kw
    assert expand(C=65) == EUNSUPPORTED and expand(n=0, P=2 ** 31) == EUNSUPPORTED
    assert expand(dst=PTR + 2) == EALIGN and expand(count=PTR + 1) == EALIGN
    assert expand(n=0, P=0, src=0, idx=0) == OK                  # nothing to write, nothing launched


def test_python_faces_refuse_before_the_library(monkeypatch):
    from mvsnerf_amd import _lib, ops, train

    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)
    density, ndc = torch.zeros((4, 4, 4)), torch.zeros((2, 3, 3))
    with pytest.raises(ValueError, match="NaN"):
        ops.live_samples(density, ndc, float("nan"))
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.live_samples(density, ndc.clone().requires_grad_(True), 0.0)
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.live_samples(density.clone().requires_grad_(True), ndc, 0.0)
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.expand_rows(torch.zeros((2, 4), requires_grad=True), torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 4)
    z = torch.zeros((2, 3))
    with pytest.raises(ValueError, match="NaN"):
        ops.raymarch_sparse(torch.zeros((4, 4, 4, 8)), None, None, None, None, ndc, ndc, z, torch.zeros((2, 3)), density, float("nan"))
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.raymarch_sparse(torch.zeros((4, 4, 4, 8), requires_grad=True), None, None, None, None, ndc, ndc, z, torch.zeros((2, 3)), density, 0.0)

    # the system: built without its constructor (that encodes a scene); the refusals need nothing of it but the missing density volume
    ft = train.MVSSystemFinetune.__new__(train.MVSSystemFinetune)
    torch.nn.Module.__init__(ft)
    ft.density_volume = None
    rays = torch.zeros((5, 8))
    with pytest.raises(RuntimeError, match=r"update_density_volume\(\)"):
        ft.render_rays(rays, skip_empty=0.0)
    with pytest.raises(ValueError, match="whole_frame_off"):
        ft.render_rays(rays, skip_empty=0.0, whole_frame_off=True)
    with pytest.raises(ValueError, match="NaN"):
        ft.render_rays(rays, skip_empty=float("nan"))
