"""CPU-only: argument handling of the fine-tuned-scene render entries (mvsnerf_gather_colorvol_fwd, mvsnerf_render_rays_fwd,
mvsnerf_render_rays_workspace_floats, mvsnerf_raymarch_colorvol_fwd_batched).  Every call here must be rejected (or found empty) before
the first launch: there is no GPU, and the pointers are made-up addresses that nothing may dereference."""
import ctypes
import subprocess

import pytest

from mvsnerf_amd import _lib

OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
PTR = 0x10000        # non-NULL, 16-byte aligned, never dereferenced
NEW = ("mvsnerf_gather_colorvol_fwd", "mvsnerf_raymarch_colorvol_fwd_batched", "mvsnerf_render_rays_workspace_floats", "mvsnerf_render_rays_fwd")


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_new_exports_are_bound_and_exported(lib):
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    for n in NEW:
        assert n in names and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.mvsnerf_abi_version() == 12                      # internal tier: no ABI bump


def _r4(n):
    return (n + 3) & ~3


def _ws(B, S, NI, F):
    """pts, ndc (3P each), merged depths (P), coarse depths (B*S, only with importance sampling), feature rows (F*P), raw (4P), compact ray
    directions and direction features (3B each); every block rounded up to 16 bytes; P = B * (S + NI)."""
    P = B * (S + NI)
    return _r4(3 * P) * 2 + _r4(P) + (_r4(B * S) if NI > 0 else 0) + _r4(F * P) + _r4(4 * P) + _r4(3 * B) * 2


@pytest.mark.parametrize("B,S,NI,F", [(16384, 128, 0, 20), (1000, 128, 0, 28), (4096, 128, 64, 20), (1, 3, 1, 12), (333, 37, 5, 40), (7, 1, 0, 20)])
def test_workspace_formula(lib, B, S, NI, F):
    assert lib.mvsnerf_render_rays_workspace_floats(B, S, NI, F) == _ws(B, S, NI, F)


def test_workspace_rejects_bad_sizes(lib):
    for bad in ((0, 128, 0, 20), (16, 0, 0, 20), (16, 8, -1, 20), (16, 8, 0, 8), (16, 8, 0, 22)):
        assert lib.mvsnerf_render_rays_workspace_floats(*bad) == 0, bad


def _args(**over):
    """A complete, valid 8-channel argument block (made-up pointers); `over` overrides fields."""
    d = dict(vol=PTR, D=16, H=24, W=32, C=8, vol_layout=0, imgs_nhwc4=PTR, V=3, IH=64, IW=96, w2c=PTR, K=PTR, K_ref=PTR, w2c_ref=PTR, near_far_ref=PTR,
             W_ref=96, H_ref=64, pad=4, lindisp=0, packed_mlp=PTR, rays=PTR, first_ray=0, n_rays=100, t=PTR, S=32, white_bkgd=0, batch_rays=64,
             workspace=PTR, workspace_floats=_ws(64, 32, 0, 20), rgb=PTR, depth=PTR)
    d.update(over)
    return _lib.RenderRaysArgs(**d)


def _call(lib, **over):
    a = _args(**over)
    return lib.mvsnerf_render_rays_fwd(ctypes.byref(a), None)


def test_render_rays_argument_codes(lib):
    assert lib.mvsnerf_render_rays_fwd(None, None) == EINVAL
    assert _call(lib, n_rays=0) == OK                           # an empty range is not an error, and nothing is launched
    for f in ("vol", "packed_mlp", "K_ref", "w2c_ref", "near_far_ref", "rays", "t", "workspace", "rgb"):
        assert _call(lib, **{f: 0}) == EINVAL, f
    for f in ("imgs_nhwc4", "w2c", "K"):                        # the image gather of an 8-channel volume needs them ...
        assert _call(lib, **{f: 0}) == EINVAL, f
    for f, v in (("n_rays", -1), ("first_ray", -1), ("S", 0), ("V", 0), ("batch_rays", 0), ("W_ref", 1), ("H_ref", 1), ("pad", -1), ("D", 0),
                 ("n_importance", -1), ("vol_layout", 2), ("IH", 1)):
        assert _call(lib, **{f: v}) == EINVAL, f
    assert _call(lib, workspace_floats=_ws(64, 32, 0, 20) - 1) == EINVAL
    # a guard needs the fp16 split planes
    assert _call(lib, guard=PTR) == EINVAL
    assert _call(lib, guard=PTR, packed_mlp_split=PTR, n_split=2) == EINVAL
    # channel counts: 8 or 8 + 4V, nothing else
    for C in (4, 12, 16, 21, 28):
        assert _call(lib, C=C) == EUNSUPPORTED, C
    assert _call(lib, V=9, C=44, workspace_floats=_ws(64, 32, 0, 44)) == EUNSUPPORTED       # F = 44 is beyond the MLP kernels
    # importance sampling: u and the density volume's size are required, S >= 3, at most 512 samples
    ws_f = _ws(64, 32, 16, 20)
    assert _call(lib, density=PTR, DD=16, DH=24, DW=32, n_importance=16, workspace_floats=ws_f) == EINVAL                       # no u
    assert _call(lib, density=PTR, DD=0, DH=24, DW=32, u=PTR, n_importance=16, workspace_floats=ws_f) == EINVAL
    assert _call(lib, density=PTR, DD=16, DH=24, DW=32, u=PTR, n_importance=16, S=2, workspace_floats=ws_f) == EINVAL
    assert _call(lib, density=PTR, DD=16, DH=24, DW=32, u=PTR, n_importance=600, workspace_floats=_ws(64, 32, 600, 20)) == EUNSUPPORTED
    assert _call(lib, density=PTR, DD=16, DH=24, DW=32, u=PTR, n_importance=16, workspace_floats=_ws(64, 32, 0, 20)) == EINVAL   # workspace of the coarse-only size
    # alignment
    assert _call(lib, workspace=PTR + 4) == EALIGN
    assert _call(lib, vol=PTR + 8) == EALIGN


def test_render_rays_colour_volume_needs_no_images(lib):
    """C == 8 + 4V: imgs / w2c / K may be NULL; a wrong guard or channel count is still rejected first.  (A valid block would launch, so the
    accepted case is only checked through the empty range.)"""
    cv = dict(C=20, imgs_nhwc4=0, w2c=0, K=0, IH=0, IW=0)
    assert _call(lib, **cv, n_rays=0) == OK
    assert _call(lib, **cv, guard=PTR) == EINVAL
    assert _call(lib, **cv, V=5) == EUNSUPPORTED                # 20 channels are not 8 + 4 * 5
    assert _call(lib, **cv, workspace_floats=10) == EINVAL


def test_gather_colorvol_argument_codes(lib):
    f = lib.mvsnerf_gather_colorvol_fwd

    def call(vol=PTR, D=8, H=8, W=8, C=20, ndc=PTR, N=4, S=4, rays_dir=PTR, w2c=PTR, feat=PTR, stride=20, dirs=PTR, layout=0, force=0):
        return f(vol, D, H, W, C, ndc, N, S, rays_dir, w2c, feat, stride, dirs, layout, force, None)
    assert call(N=0) == OK
    for kw in (dict(vol=0), dict(ndc=0), dict(feat=0), dict(D=0), dict(N=-1), dict(S=0), dict(stride=16), dict(layout=3), dict(rays_dir=0)):
        assert call(**kw) == EINVAL, kw
    for C in (4, 8, 10, 44):
        assert call(C=C, stride=48) == EUNSUPPORTED, C
    assert call(stride=22) == EALIGN
    assert call(feat=PTR + 4) == EALIGN
    assert call(vol=PTR + 4) == EALIGN


def test_raymarch_colorvol_batched_argument_codes(lib):
    f = lib.mvsnerf_raymarch_colorvol_fwd_batched
    assert f(None, 1, 20, None) == EINVAL
    blk = (_lib.RaymarchArgs * 1)()
    assert f(blk, 0, 20, None) == OK
    full = dict(vol=PTR, D=8, H=8, W=8, V=3, w2c=PTR, packed_mlp=PTR, rays_ndc=PTR, z_vals=PTR, rays_dir=PTR, N=4, S=4, dirs_tmp=PTR, input_feat=PTR, raw=PTR)
    for miss in ("vol", "w2c", "packed_mlp", "rays_ndc", "z_vals", "rays_dir", "dirs_tmp", "input_feat", "raw"):
        blk[0] = _lib.RaymarchArgs(**{**full, miss: 0})
        assert f(blk, 1, 20, None) == EINVAL, miss
    blk[0] = _lib.RaymarchArgs(**full)
    assert f(blk, 1, 28, None) == EUNSUPPORTED                  # 28 channels are not 8 + 4 * 3
    blk[0] = _lib.RaymarchArgs(**full, guard=PTR)
    assert f(blk, 1, 20, None) == EINVAL                        # guard without the fp16 split planes


def test_misspelt_field_raises():
    with pytest.raises((AttributeError, TypeError)):
        _lib.RenderRaysArgs(n_ray=3)
    a = _lib.RenderRaysArgs()
    with pytest.raises(AttributeError):
        a.batch_ray = 4
    assert [n for n, _ in _lib.RenderRaysArgs._fields_][:6] == ["vol", "D", "H", "W", "C", "vol_layout"]
