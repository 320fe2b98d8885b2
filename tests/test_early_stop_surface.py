"""CPU-only: the surface of early ray termination - symbols, the workspace query, argument codes, and the refusals that come before
the library."""
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvsnerf_ray_transmittance_fwd", "mvsnerf_live_samples_range_workspace_bytes", "mvsnerf_live_samples_range_fwd", "mvsnerf_scatter_rows_fwd")
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
PTR = 0x10000        # non-NULL, 16-byte aligned, never dereferenced


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
    assert all(callable(getattr(ops, n)) for n in ("ray_transmittance", "live_samples_range", "scatter_rows", "raymarch_early_stop"))


def test_keywords_come_last_with_their_defaults():
    from mvsnerf_amd import ops, train
    for fn in (train.MVSSystem.render_view, train.MVSSystemFinetune.render_rays, train.MVSSystemFusion.render_rays):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ["early_stop", "stop_every"] and p["early_stop"].default is None and p["stop_every"].default == 32
    p = inspect.signature(ops.raymarch_early_stop).parameters
    assert list(p) == ["vol_cl", "imgs", "w2cs", "intrinsics", "packed", "rays_pts", "rays_ndc", "z_vals", "rays_dir", "eps", "stop_every", "density", "thr",
                       "white_bkgd", "want", "packed_alt"]
    assert p["stop_every"].default == 32 and p["density"].default is None and p["thr"].default is None


def test_workspace_query():
    from mvsnerf_amd import _lib
    q, q0 = _lib.lib().mvsnerf_live_samples_range_workspace_bytes, _lib.lib().mvsnerf_live_samples_workspace_bytes
    assert q(0, 8) == 0 and q(8, 0) == 0 and q(-1, 8) == 0 and q(2 ** 24, 128) == 0
    for N, G in ((1, 1), (37, 8), (1030, 16), (16384, 32)):
        assert q(N, G) == q0(N * G) > 0


def test_entries_refuse_bad_arguments_before_any_launch():
    from mvsnerf_amd import _lib
    L = _lib.lib()

    def trans(raw=PTR, N=8, S=24, s0=8, s1=16, ray_T=PTR):
        return L.mvsnerf_ray_transmittance_fwd(raw, N, S, s0, s1, ray_T, None)
    for kw in (dict(raw=0), dict(ray_T=0), dict(N=-1), dict(S=0), dict(s0=-1), dict(s1=25), dict(s0=16), dict(s0=17), dict(raw=PTR + 4), dict(raw=PTR + 8),
               dict(ray_T=PTR + 2)):
        assert trans(**kw) == EINVAL, kw
    assert trans(N=2 ** 24, S=128, s1=16) == EUNSUPPORTED
    assert trans(N=0) == OK                                       # nothing to do, nothing launched

    def live(density=PTR, D=4, H=4, W=4, thr=0.0, ndc=PTR, pts=PTR, rays_dir=PTR, N=8, S=24, s0=8, s1=16, ray_T=PTR, eps=0.01, count=PTR, idx=PTR,
             ndc_c=PTR, pts_c=PTR, dir_c=PTR, ws=PTR):
        return L.mvsnerf_live_samples_range_fwd(density, D, H, W, thr, ndc, pts, rays_dir, N, S, s0, s1, ray_T, eps, count, idx, ndc_c, pts_c, dir_c, ws, None)
    for kw in (dict(count=0), dict(ndc=0), dict(idx=0), dict(ndc_c=0), dict(ws=0), dict(pts_c=0), dict(dir_c=0), dict(D=0), dict(H=0), dict(W=0), dict(N=-1),
               dict(S=0), dict(thr=float("nan")), dict(eps=float("nan")), dict(s0=-1), dict(s1=25), dict(s0=16), dict(s0=20),
               dict(ws=PTR + 4), dict(ndc=PTR + 2), dict(idx=PTR + 1), dict(ray_T=PTR + 2), dict(density=PTR + 1)):
        assert live(**kw) == EINVAL, kw
    assert live(N=2 ** 24, S=128) == EUNSUPPORTED                 # 2^31 samples: idx is int32
    assert live(density=0, D=0, H=0, W=0, thr=float("nan"), N=-1) == EINVAL             # without a density its size and threshold are not read; N still is

    def scatter(src=PTR, idx=PTR, count=PTR, n=8, P=32, C=4, dst=PTR):
        return L.mvsnerf_scatter_rows_fwd(src, idx, count, n, P, C, dst, None)
    for kw in (dict(count=0), dict(dst=0), dict(src=0), dict(idx=0), dict(n=-1), dict(n=33), dict(P=-1), dict(C=0), dict(dst=PTR + 2), dict(count=PTR + 1),
               dict(src=PTR + 3), dict(idx=PTR + 2)):
        assert scatter(**kw) == EINVAL, kw
    assert scatter(C=65) == EUNSUPPORTED and scatter(n=0, P=2 ** 31) == EUNSUPPORTED
    assert scatter(n=0, P=0, src=0, idx=0) == OK                  # nothing to write, nothing launched


def test_python_faces_refuse_before_the_library(monkeypatch):
    from mvsnerf_amd import _lib, ops, train

    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)
    density, ndc, z, dirs = torch.zeros((4, 4, 4)), torch.zeros((2, 3, 3)), torch.zeros((2, 3)), torch.zeros((2, 3))
    vol = torch.zeros((4, 4, 4, 8))

    def march(eps=0.01, **kw):
        return ops.raymarch_early_stop(vol, None, None, None, None, ndc, ndc, z, dirs, eps, **kw)
    for eps in (float("nan"), -0.1, 1.0, 1.5, float("inf")):
        with pytest.raises(ValueError, match="early_stop"):
            march(eps)
    for g in (0, -3, 2.5):
        with pytest.raises(ValueError, match="stop_every"):
            march(stop_every=g)
    with pytest.raises(ValueError, match="together"):
        march(density=density)
    with pytest.raises(ValueError, match="together"):
        march(thr=0.0)
    with pytest.raises(ValueError, match="NaN"):
        march(density=density, thr=float("nan"))
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.raymarch_early_stop(vol.clone().requires_grad_(True), None, None, None, None, ndc, ndc, z, dirs, 0.01)
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.ray_transmittance(torch.zeros((2, 3, 4), requires_grad=True), 0, 3, torch.ones(2))
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.live_samples_range(None, ndc.clone().requires_grad_(True), 0.0, 0, 3)
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.scatter_rows(torch.zeros((2, 4), requires_grad=True), torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros((4, 4)))
    with pytest.raises(RuntimeError, match="window"):
        ops.ray_transmittance(torch.zeros((2, 3, 4)), 2, 2, torch.ones(2))
    with pytest.raises(RuntimeError, match="window"):
        ops.live_samples_range(None, ndc, 0.0, 0, 4)

    # the systems: built without their constructors (those encode a scene); the refusals need nothing of them
    rays = torch.zeros((5, 8))
    for cls in (train.MVSSystemFinetune, train.MVSSystemFusion):
        sysm = cls.__new__(cls)
        torch.nn.Module.__init__(sysm)
        for bad in (float("nan"), -1e-3, 1.0):
            with pytest.raises(ValueError, match="early_stop"):
                sysm.render_rays(rays, early_stop=bad)
        with pytest.raises(ValueError, match="stop_every"):
            sysm.render_rays(rays, early_stop=0.01, stop_every=0)
    ft = train.MVSSystemFinetune.__new__(train.MVSSystemFinetune)
    torch.nn.Module.__init__(ft)
    with pytest.raises(ValueError, match="whole_frame_off"):
        ft.render_rays(rays, early_stop=0.01, whole_frame_off=True)
    s = train.MVSSystem.__new__(train.MVSSystem)
    torch.nn.Module.__init__(s)
    for bad in (float("nan"), -1e-3, 1.0):
        with pytest.raises(ValueError, match="early_stop"):
            s.render_view({}, early_stop=bad)
    with pytest.raises(ValueError, match="stop_every"):
        s.render_view({}, early_stop=0.01, stop_every=0)
    with pytest.raises(ValueError, match="whole_frame_off"):
        s.render_view({}, early_stop=0.01, whole_frame_off=True)
