"""CPU-only: the surface of the scene ray bank - symbols, argument codes, signatures and the refusals that come before the library."""
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvsnerf_scene_rays_gather_fwd", "mvsnerf_scene_rays_march_fwd")
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
PTR = 0x10000        # non-NULL, 16-byte aligned, never dereferenced


def test_symbols_are_declared_exported_and_bound_and_the_stable_tier_is_unchanged():
    from mvsnerf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read(), flags=re.S)
    stable = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert not re.search(rf"\b{name}\s*\(", stable), name            # internal tier only
        assert name in _lib.SIGNATURES
    assert "scene_rays" not in stable
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(SYMBOLS) <= {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert _lib.lib().mvsnerf_abi_version() == 12


def test_entries_refuse_bad_arguments_before_any_launch():
    from mvsnerf_amd import _lib
    L = _lib.lib()

    def gather(images=PTR, c2w=PTR, K=PTR, nf=PTR, depth_bank=PTR, M=3, H=20, W=28, idx=PTR, B=700, rays=PTR, rgb=PTR, depth=PTR, mask=PTR):
        return L.mvsnerf_scene_rays_gather_fwd(images, c2w, K, nf, depth_bank, M, H, W, idx, B, rays, rgb, depth, mask, None)

    def march(images=PTR, c2w=PTR, K=PTR, nf=PTR, M=3, H=20, W=28, idx=PTR, B=700, t=PTR, S=16, jitter=PTR, perturb=1.0, lindisp=0, w2c=PTR, Kr=PTR, nfr=PTR,
              Wr=28, Hr=20, pad=4, rays=PTR, rgb=PTR, z=PTR, pts=PTR, ndc=PTR):
        return L.mvsnerf_scene_rays_march_fwd(images, c2w, K, nf, M, H, W, idx, B, t, S, jitter, perturb, lindisp, w2c, Kr, nfr, Wr, Hr, pad, rays, rgb, z,
                                              pts, ndc, None)
    for fn in (gather, march):
        # NULL required pointers, sizes < 1, B < 0
        for kw in (dict(images=0), dict(c2w=0), dict(K=0), dict(nf=0), dict(idx=0), dict(rays=0), dict(rgb=0), dict(M=0), dict(H=0), dict(W=0),
                   dict(M=-1), dict(B=-1)):
            assert fn(**kw) == EINVAL, (fn.__name__, kw)
        # pointers misaligned for their element type: images and floats 4 bytes, idx 8
        for kw in (dict(images=PTR + 2), dict(c2w=PTR + 2), dict(K=PTR + 1), dict(nf=PTR + 2), dict(idx=PTR + 4), dict(rays=PTR + 2), dict(rgb=PTR + 1)):
            assert fn(**kw) == EINVAL, (fn.__name__, kw)
        # M*H*W above INT64_MAX / 8 (also when the product leaves 64 bits)
        for kw in (dict(M=2 ** 31 - 1, H=2 ** 31 - 1, W=2), dict(M=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1), dict(M=2 ** 30, H=2 ** 30, W=1)):
            assert fn(**kw) == EUNSUPPORTED, (fn.__name__, kw)            # (2^60 is the first count above INT64_MAX / 8 = 2^60 - 1)
        assert fn(M=2 ** 30, H=2 ** 30 - 1, W=1, B=0) == OK               # the largest bank of this shape that is inside; B == 0 launches nothing
        assert fn(B=0) == OK and fn(B=0, idx=0) == OK
    # gather: optional outputs may be NULL, a depth output needs the depth bank; march: the depths' inputs, the optional reference camera
    assert gather(B=0, depth=0, mask=0, depth_bank=0) == OK
    assert gather(depth_bank=0) == EINVAL and gather(depth=PTR + 2) == EINVAL and gather(depth_bank=PTR + 2) == EINVAL
    for kw in (dict(t=0), dict(S=0), dict(S=-3), dict(z=0), dict(pts=0), dict(jitter=0), dict(perturb=-1.0), dict(perturb=float("nan")),
               dict(w2c=0), dict(Kr=0), dict(nfr=0), dict(Wr=1), dict(Hr=1), dict(pad=-1),
               dict(t=PTR + 2), dict(jitter=PTR + 2), dict(z=PTR + 1), dict(pts=PTR + 2), dict(ndc=PTR + 2), dict(w2c=PTR + 2), dict(Kr=PTR + 2), dict(nfr=PTR + 2)):
        assert march(**kw) == EINVAL, kw
    assert march(B=0, jitter=0, perturb=0.0) == OK                       # no jitter without perturb
    assert march(B=0, ndc=0, w2c=0, Kr=0, nfr=0, Wr=0, Hr=0, pad=0) == OK    # no reference camera without ndc


def test_fit_scene_signatures():
    from mvsnerf_amd import ops, rays, train
    for cls in (train.MVSSystemFinetune, train.MVSSystemFusion):
        p = inspect.signature(cls.fit_scene).parameters
        assert list(p) == ["self", "scene", "n_steps", "batch_size", "seed", "optimizer"], cls.__name__
        assert p["batch_size"].default is None and p["seed"].default == 0 and p["optimizer"].default is None
    p = inspect.signature(rays.SceneRays.__init__).parameters
    assert list(p) == ["self", "images", "c2ws", "intrinsics", "near_far", "depths", "device"] and p["depths"].default is None and p["device"].default == "cuda"
    p = inspect.signature(rays.SceneRays.march).parameters
    assert list(p) == ["self", "idx", "N_samples", "perturb", "jitter", "lindisp", "ref"] and p["perturb"].default == 0.0 and p["ref"].default is None
    assert list(inspect.signature(rays.SceneRays.epoch).parameters)[:3] == ["self", "batch_size", "generator"]
    p = inspect.signature(ops.scene_rays_gather).parameters
    assert list(p)[-3:] == ["idx", "want_depth", "want_mask"] and p["want_depth"].default is False and p["want_mask"].default is False
    p = inspect.signature(ops.scene_rays_march).parameters
    assert list(p)[-7:] == ["idx", "N_samples", "t", "jitter", "perturb", "lindisp", "ref"]
    assert list(inspect.signature(train.MVSSystemFinetune._step_body).parameters) == ["self", "rays", "target", "rays_o", "rays_d", "z_vals", "pts", "ndc"]


def test_scene_rays_refuses_before_the_library(monkeypatch):
    from mvsnerf_amd import _lib
    from mvsnerf_amd.rays import SceneRays

    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)
    M, H, W = 2, 4, 5
    c2ws, K, nf = torch.eye(4).expand(M, 4, 4), torch.eye(3), torch.tensor([2.0, 6.0])
    u8 = torch.zeros((M, H, W, 3), dtype=torch.uint8)
    for bad in (u8.float(), u8.double() / 255, u8.to(torch.float16), u8.int()):
        with pytest.raises(TypeError, match="uint8"):                    # a float image would be quantised silently
            SceneRays(bad, c2ws, K, nf, device="cpu")
    for shape in ((M, H, W, 1), (M, H, W, 5), (M, H, W), (M, 3, H, W)):
        with pytest.raises(ValueError, match="images"):
            SceneRays(torch.zeros(shape, dtype=torch.uint8), c2ws, K, nf, device="cpu")
    with pytest.raises(ValueError, match="c2ws"):                        # mismatched M
        SceneRays(u8, torch.eye(4).expand(M + 1, 4, 4), K, nf, device="cpu")
    with pytest.raises(ValueError, match="intrinsics"):
        SceneRays(u8, c2ws, torch.eye(3).expand(M + 1, 3, 3), nf, device="cpu")
    with pytest.raises(ValueError, match="near_far"):
        SceneRays(u8, c2ws, K, torch.zeros((M + 1, 2)), device="cpu")
    with pytest.raises(ValueError, match="depths"):
        SceneRays(u8, c2ws, K, nf, depths=torch.zeros((M, H, W + 1)), device="cpu")
    s = SceneRays(u8, c2ws[:, :3], K, nf, depths=torch.zeros((M, H, W)), device="cpu")      # (M,3,4) poses, shared K and near / far
    assert (s.n_rays, s.hw, s.n_views) == (M * H * W, (H, W), M)
    assert s.images.shape == (M, H, W, 4) and bool((s.images[..., 3] == 255).all())          # three-channel input gets alpha 255
    assert s.c2ws.shape == (M, 3, 4) and s.intrinsics.shape == (M, 3, 3) and s.near_far.shape == (M, 2)
    with pytest.raises(IndexError):
        s.view(M)
    with pytest.raises(IndexError):
        s.source_views([0, M])
