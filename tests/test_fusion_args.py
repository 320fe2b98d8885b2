"""CPU-only: the surface and argument handling of the fusion entries (mvsnerf_volume_fuse_*, mvsnerf_ray_march_bbox_fwd) and of their Python faces.
Every call here is rejected, or is a no-op, before the first launch: there is no GPU, and the pointers are made-up addresses nothing may dereference."""
import os
import subprocess

import pytest
import torch

from mvsnerf_amd import _lib

OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
PTR = 0x10000        # non-NULL, 16-byte aligned, never dereferenced
NEW = ("mvsnerf_volume_fuse_workspace_words", "mvsnerf_volume_fuse_splat", "mvsnerf_volume_fuse_finish", "mvsnerf_ray_march_bbox_fwd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_new_exports_are_bound_and_exported(lib):
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    for n in NEW:
        assert n in names and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.mvsnerf_abi_version() == 12                      # internal tier: no ABI bump
    from mvsnerf_amd import fusion
    assert (fusion.HEADER_WORDS, fusion.SCALE_LOG2, fusion.LIMIT) == (8, 32, 2.0 ** 20)


def test_workspace_is_a_header_and_one_row_per_voxel(lib):
    f = lib.mvsnerf_volume_fuse_workspace_words
    assert f(10, 12, 14, 20) == 8 + 10 * 12 * 14 * 24
    assert f(128, 128, 128, 20) == 8 + 128 ** 3 * 24 and f(2, 2, 2, 4) == 8 + 8 * 8
    assert f(2048, 2048, 2048, 40) == 8 + 2048 ** 3 * 44          # beyond 2^32 words: 64-bit sizes
    for bad in ((1, 12, 14, 20), (10, 1, 14, 20), (10, 12, 0, 20), (10, 12, 14, 0), (10, 12, 14, 18), (10, 12, 14, 44), (-1, 12, 14, 20)):
        assert f(*bad) == 0, bad


def _splat(lib, D=10, H=12, W=14, C=20, ndc=PTR, P=100, feat=PTR, stride=20, alpha=PTR, ws=PTR):
    return lib.mvsnerf_volume_fuse_splat(D, H, W, C, ndc, P, feat, stride, alpha, ws, None)


def test_splat_argument_codes(lib):
    for f in ("ndc", "feat", "alpha", "ws"):
        assert _splat(lib, **{f: 0}) == EINVAL, f
    assert _splat(lib, P=-1) == EINVAL and _splat(lib, stride=19) == EINVAL and _splat(lib, P=(1 << 32) + 1) == EINVAL
    assert _splat(lib, D=1) == EINVAL and _splat(lib, H=0) == EINVAL and _splat(lib, W=-2) == EINVAL
    for C in (0, 2, 18, 44):
        assert _splat(lib, C=C, stride=64) == EUNSUPPORTED, C
    assert _splat(lib, ws=PTR + 4) == EALIGN
    assert _splat(lib, P=0) == OK and _splat(lib, P=0, ndc=0, feat=0, alpha=0) == OK      # an empty batch is a no-op


def test_finish_and_march_argument_codes(lib):
    fin = lambda D=10, H=12, W=14, C=20, ws=PTR, vol=PTR, dens=PTR: lib.mvsnerf_volume_fuse_finish(D, H, W, C, ws, vol, dens, None)
    assert fin(ws=0) == EINVAL and fin(vol=0) == EINVAL and fin(dens=0) == EINVAL and fin(D=1) == EINVAL
    assert fin(C=22) == EUNSUPPORTED and fin(ws=PTR + 8) == EALIGN
    march = lambda rays=PTR, bbox=PTR, t=PTR, jit=0, perturb=0.0, N=4, S=8, z=PTR, pts=PTR, ndc=PTR: lib.mvsnerf_ray_march_bbox_fwd(
        rays, bbox, t, jit, perturb, 0, N, S, z, pts, ndc, None)
    for f in ("rays", "bbox", "t", "z", "pts", "ndc"):
        assert march(**{f: 0}) == EINVAL, f
    assert march(perturb=1.0) == EINVAL                           # perturb > 0 reads the caller's draw
    assert march(perturb=-1.0) == EINVAL and march(perturb=float("nan")) == EINVAL
    assert march(S=0) == EINVAL and march(N=-1) == EINVAL and march(N=0) == OK


def test_python_faces_refuse_bad_input():
    from mvsnerf_amd import fusion, ops, train
    with pytest.raises(RuntimeError, match="VolumeFuser"):
        fusion.VolumeFuser([14, 12, 10], 18, "cpu")
    with pytest.raises(RuntimeError, match="VolumeFuser"):
        fusion.VolumeFuser([14, 1, 10], 20, "cpu")
    rays, bbox = torch.zeros((4, 8)), torch.zeros((2, 3))
    with pytest.raises(RuntimeError, match="ray_march_bbox"):
        ops.ray_march_bbox(rays[:, :6], bbox, 8)
    with pytest.raises(RuntimeError, match="ray_march_bbox"):
        ops.ray_march_bbox(rays, bbox, 8, perturb=1.0)
    with pytest.raises(RuntimeError, match="float32 tensor on the GPU"):
        ops.ray_march_bbox(rays, bbox, 8)
    # train.dda is host-side torch (data/ray_utils.py:143-150): a ray along +z from the origin enters the box z in [2, 3] at 2 and leaves at 3
    near, far = train.dda(torch.zeros((1, 3)), torch.tensor([[0.0, 0.0, 1.0]]), torch.tensor([[-1.0, -1.0, 2.0], [1.0, 1.0, 3.0]]))
    assert abs(float(near) - 2.0) < 1e-5 and abs(float(far) - 3.0) < 1e-5
    d = train.get_ray_directions(4, 6, [3.0, 2.0])
    assert d.shape == (4, 6, 3) and torch.equal(d[0, 0], torch.tensor([-1.0, -1.0, 1.0])) and torch.equal(d[2, 3], torch.tensor([0.0, 0.0, 1.0]))
    ro, rd = train.get_rays(d, torch.eye(4)[:3])
    assert torch.equal(rd, d.reshape(-1, 3)) and not ro.any()
