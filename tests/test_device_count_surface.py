"""CPU-only: the surface of the counted launches and of device_count= - symbols, argument codes, keywords and the refusals that
come before the library."""
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvsnerf_mlp_fwd_counted", "mvsnerf_mlp_fwd_guarded_counted", "mvsnerf_mlp_fwd_split_counted", "mvsnerf_mlp_fwd_wide_counted",
           "mvsnerf_gather_fwd_counted", "mvsnerf_gather_colorvol_fwd_counted")
OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
PTR = 0x10000        # non-NULL, 16-byte aligned, never dereferenced
SPLIT_FP16 = 18


def test_symbols_are_declared_exported_and_bound_and_the_stable_tier_is_unchanged():
    from mvsnerf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read(), flags=re.S)
    stable = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert not re.search(rf"\b{name}\s*\(", stable), name            # internal tier only
        assert name in _lib.SIGNATURES
    assert "counted" not in stable
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(SYMBOLS) <= {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert _lib.lib().mvsnerf_abi_version() == 12


def test_keywords_and_their_defaults():
    from mvsnerf_amd import ops, train
    faces = (ops.raymarch_sparse, train._render_sparse_batches, train.MVSSystem.render_view, train.MVSSystem.render_path_skip_empty,
             train.MVSSystemFinetune.render_rays, train.MVSSystemFinetune.render_path, train.MVSSystemFusion.render_rays,
             train.MVSSystemFusion.render_path)
    for fn in faces:
        p = inspect.signature(fn).parameters
        assert "device_count" in p and p["device_count"].default is False, fn.__qualname__
    # raymarch_early_stop's named parameters are pinned (tests/test_early_stop_surface.py): the switch is a keyword among **packed_alt, default
    # False - the refusal below shows that it is read, and a host-count call does not hand it on to the kernel choice
    assert list(inspect.signature(ops.raymarch_early_stop).parameters)[-1] == "packed_alt"
    for fn, kw in ((ops.mlp_forward, ("count", "out")), (ops.gather, ("count", "out")), (ops.gather_colorvol, ("count", "out"))):
        p = inspect.signature(fn).parameters
        assert all(k in p and p[k].default is None for k in kw), fn.__qualname__


def test_entries_refuse_bad_arguments_before_any_launch():
    from mvsnerf_amd import _lib
    L = _lib.lib()

    def mlp(packed=PTR, F=20, ndc=PTR, feat=PTR, dirs=PTR, cap=700, count=PTR, ao=0, raw=PTR):
        return L.mvsnerf_mlp_fwd_counted(packed, F, ndc, feat, dirs, cap, count, ao, raw, None)

    def guarded(ph=PTR, packed=PTR, F=20, ndc=PTR, feat=PTR, dirs=PTR, cap=700, count=PTR, ao=0, raw=PTR, guard=PTR):
        return L.mvsnerf_mlp_fwd_guarded_counted(ph, packed, F, ndc, feat, dirs, cap, count, ao, raw, guard, None)

    def split(ph=PTR, packed=PTR, F=20, n_split=SPLIT_FP16, ndc=PTR, feat=PTR, dirs=PTR, cap=700, count=PTR, ao=0, raw=PTR):
        return L.mvsnerf_mlp_fwd_split_counted(ph, packed, F, n_split, ndc, feat, dirs, cap, count, ao, raw, None)

    def wide(packed=PTR, F=20, width=256, ndc=PTR, feat=PTR, dirs=PTR, cap=700, count=PTR, ao=0, raw=PTR):
        return L.mvsnerf_mlp_fwd_wide_counted(packed, F, width, ndc, feat, dirs, cap, count, ao, raw, None)
    for fn in (mlp, guarded, split, wide):
        for kw in (dict(count=0), dict(packed=0), dict(ndc=0), dict(feat=0), dict(raw=0), dict(dirs=0), dict(cap=-1)):
            assert fn(**kw) == EINVAL, (fn.__name__, kw)
        # (the split entry, like its namesake, asks 16 bytes of the planes and of raw, not of the fp32 buffer)
        for kw in (dict(count=PTR + 2), dict(count=PTR + 1), dict(raw=PTR + 4)) + (() if fn is split else (dict(packed=PTR + 8),)):
            assert fn(**kw) == EALIGN, (fn.__name__, kw)
        for kw in (dict(cap=2 ** 31), dict(F=21), dict(F=0), dict(F=42)):
            assert fn(**kw) == EUNSUPPORTED, (fn.__name__, kw)
        assert fn(cap=0) == OK                                   # nothing to do, nothing enqueued
        assert fn(dirs=0, ao=1, cap=0) == OK                     # a sigma-only query reads no direction
    assert guarded(guard=0) == EINVAL and guarded(ph=0) == EINVAL and split(ph=0) == EINVAL
    assert guarded(ph=PTR + 4) == EALIGN and split(ph=PTR + 4) == EALIGN
    for n_split in (1, 2, 3, 0):
        assert split(n_split=n_split) == EUNSUPPORTED            # the bf16 splits have no counted form
    assert wide(width=128) == EUNSUPPORTED

    def gather(vol=PTR, D=4, H=4, W=4, imgs=PTR, V=3, IH=8, IW=8, w2c=PTR, K=PTR, pts=PTR, ndc=PTR, cap=700, count=PTR, rays_dir=PTR, feat=PTR, fs=20,
               dirs=PTR, layout=0):
        return L.mvsnerf_gather_fwd_counted(vol, D, H, W, imgs, V, IH, IW, w2c, K, pts, ndc, cap, count, rays_dir, feat, fs, dirs, layout, None)
    for kw in (dict(count=0), dict(vol=0), dict(imgs=0), dict(w2c=0), dict(K=0), dict(pts=0), dict(ndc=0), dict(feat=0), dict(rays_dir=0), dict(cap=-1),
               dict(D=0), dict(V=0), dict(IH=1), dict(fs=16), dict(layout=7)):
        assert gather(**kw) == EINVAL, kw
    for kw in (dict(count=PTR + 2), dict(feat=PTR + 4), dict(vol=PTR + 8), dict(imgs=PTR + 4), dict(fs=22)):
        assert gather(**kw) == EALIGN, kw
    assert gather(cap=2 ** 31) == EUNSUPPORTED and gather(cap=0) == OK

    def colorvol(vol=PTR, D=4, H=4, W=4, C=20, ndc=PTR, cap=700, count=PTR, rays_dir=PTR, w2c=PTR, feat=PTR, fs=20, dirs=PTR, layout=0, f64=0):
        return L.mvsnerf_gather_colorvol_fwd_counted(vol, D, H, W, C, ndc, cap, count, rays_dir, w2c, feat, fs, dirs, layout, f64, None)
    for kw in (dict(count=0), dict(vol=0), dict(ndc=0), dict(feat=0), dict(rays_dir=0), dict(cap=-1), dict(W=0), dict(fs=16), dict(layout=7)):
        assert colorvol(**kw) == EINVAL, kw
    for kw in (dict(count=PTR + 2), dict(feat=PTR + 4), dict(vol=PTR + 8), dict(fs=22)):
        assert colorvol(**kw) == EALIGN, kw
    for kw in (dict(cap=2 ** 31), dict(C=8, fs=8), dict(C=44, fs=44), dict(C=18)):
        assert colorvol(**kw) == EUNSUPPORTED, kw
    assert colorvol(cap=0) == OK


def _bare(cls):
    s = cls.__new__(cls)                 # without the constructor (that encodes a scene); the refusals need nothing of it
    torch.nn.Module.__init__(s)
    return s


def test_python_faces_refuse_before_the_library(monkeypatch):
    from mvsnerf_amd import _lib, ops, train

    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)
    density, ndc, z, dirs = torch.zeros((4, 4, 4)), torch.zeros((2, 3, 3)), torch.zeros((2, 3)), torch.zeros((2, 3))
    vol = torch.zeros((4, 4, 4, 8))
    bf16, planes = torch.zeros(8, dtype=torch.bfloat16), torch.zeros(8, dtype=torch.bfloat16)

    # the bf16 family, by name, at both marches (ops.mlp_forward(count=) refuses it too, behind its check of the count: tests/test_gpu_device_count.py)
    for alt, name in ((dict(packed_bf16=bf16), "'bf16'"), (dict(packed_split=(planes, 2)), "'bf16x3'"), (dict(packed_split=(planes, 3)), "'bf16x6'")):
        with pytest.raises(NotImplementedError, match=name):
            ops.raymarch_sparse(vol, None, None, None, None, ndc, ndc, z, dirs, density, 0.0, device_count=True, **alt)
        with pytest.raises(NotImplementedError, match=name):
            ops.raymarch_early_stop(vol, None, None, None, None, ndc, ndc, z, dirs, 0.01, device_count=True, **alt)

    # a count that is not the int32 one-element device tensor (this machine has no device: a host tensor is one such count)
    for bad in (torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), 3):
        with pytest.raises(RuntimeError, match="count"):
            ops.mlp_forward(None, 20, 0, 3, 0, 20, 0, 3, 8, 1, 0, "cpu", count=bad)
        with pytest.raises(RuntimeError, match="count"):
            ops.gather(vol, torch.zeros((3, 3, 8, 8)), None, None, torch.zeros((8, 1, 3)), torch.zeros((8, 1, 3)), count=bad)
        with pytest.raises(RuntimeError, match="count"):
            ops.gather_colorvol(torch.zeros((4, 4, 4, 20)), torch.zeros((8, 1, 3)), count=bad)

    # the systems: device_count belongs to the sparse paths ...
    rays = torch.zeros((5, 8))
    for cls in (train.MVSSystemFinetune, train.MVSSystemFusion):
        s = _bare(cls)
        with pytest.raises(ValueError, match="device_count"):
            s.render_rays(rays, device_count=True)
        with pytest.raises(ValueError, match="device_count"):
            s.render_path(torch.eye(4)[None], (4, 4), 1.0, device_count=True)
    s = _bare(train.MVSSystem)
    with pytest.raises(ValueError, match="device_count"):
        s.render_view({}, device_count=True)
    # ... and is refused under the bf16 family by the mode's name, before anything is packed
    for mode in ("bf16", "bf16x3", "bf16x6"):
        with ops.mlp_precision(mode):
            for cls in (train.MVSSystemFinetune, train.MVSSystemFusion):
                with pytest.raises(NotImplementedError, match=f"'{mode}'"):
                    _bare(cls).render_rays(rays, skip_empty=0.0, device_count=True)
                with pytest.raises(NotImplementedError, match=f"'{mode}'"):
                    _bare(cls).render_rays(rays, early_stop=0.01, device_count=True)
                with pytest.raises(NotImplementedError, match=f"'{mode}'"):
                    _bare(cls).render_path(torch.eye(4)[None], (4, 4), 1.0, skip_empty=0.0, device_count=True)
            with pytest.raises(NotImplementedError, match=f"'{mode}'"):
                _bare(train.MVSSystem).render_view({}, skip_empty=0.0, device_count=True)
            with pytest.raises(NotImplementedError, match=f"'{mode}'"):
                _bare(train.MVSSystem).render_path_skip_empty({}, torch.eye(4)[None], 0.0, device_count=True)
    # device_count=False is today's call: the earlier refusals are the first thing it meets
    ft = _bare(train.MVSSystemFinetune)
    ft.density_volume = None
    with pytest.raises(RuntimeError, match=r"update_density_volume\(\)"):
        ft.render_rays(rays, skip_empty=0.0, device_count=False)
