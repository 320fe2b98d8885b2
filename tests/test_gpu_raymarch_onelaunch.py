"""The one-launch fp32 ray march (raymarch_fused_kernel, csrc/mlp.hip) against the launch sequence it replaces.

ops.raymarch in fp32 mode on a depth-fastest volume runs lookups, MLP and - when a tile of 128 samples holds whole rays - compositing in
one launch.  Every output must be BIT-identical to the same inputs pushed through the stable entries one by one: mvsnerf_gather_fwd ->
mvsnerf_mlp_fwd -> mvsnerf_composite_fwd.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BASELINES = (0.0, 0.25, -0.25, 0.1, 0.15, -0.1, 0.2, -0.15)


def _inputs(N, S, V=3, D=16, h=24, w=32, H=96, W=128, seed=0):
    from mvsnerf_amd.synth import make_rig, pose_ref_of
    from oracle import mvsnerf_oracle as O
    rig = make_rig(H, W, n_views=V + 1, baselines=BASELINES[:V + 1], seed=1234, rot_deg=2.0, smooth=True)
    pose = pose_ref_of(rig)
    g = torch.Generator().manual_seed(seed)
    vol = torch.randn((1, 8, D, h, w), generator=g)
    pts, dirs, _, ndc, z, _, _ = O.build_rays(rig["images_raw"], pose, rig["near_fars"], N, S, pad=4 if h < 100 else 24,
                                              t_rand=torch.rand((N, S), generator=g), generator=g)
    t = lambda x: x.contiguous().to(DEV)
    return dict(imgs=t(rig["images_raw"][0, :V]), w2cs=t(pose["w2cs"][:V]), Ks=t(pose["intrinsics"][:V]), vol=vol,
                pts=t(pts), dirs=t(dirs), ndc=t(ndc), z=t(z))


def _hwdc(vol):
    """(1,C,D,H,W) -> (D,H,W,C)-shaped view of depth-fastest vol[y][x][d][c] memory (MVSNERF_VOL_HWDC, the encoder's layout)."""
    return vol[0].permute(2, 3, 1, 0).contiguous().to(DEV).permute(2, 0, 1, 3)


def _packed(V):
    from mvsnerf_amd import models
    from tests.util import load_weights
    F = 8 + 4 * V
    m = models.MVSNeRF(D=6, W=128, input_ch_pts=63, input_ch_views=3, input_ch_feat=F, skips=[4], net_type="v0")
    if F == 20:
        m.load_state_dict(load_weights()[0])
    else:
        torch.manual_seed(F)
        for p in m.parameters():
            torch.nn.init.uniform_(p, -0.15, 0.15)
    return m.to(DEV).packed(F)


def _stepwise(vol_cl, x, packed, white_bkgd):
    """The launch sequence: the three stable entries one after the other."""
    from mvsnerf_amd import ops
    N, S = x["z"].shape
    F = 8 + 4 * x["imgs"].shape[0]
    feat, dirs = ops.gather(vol_cl, x["imgs"], x["w2cs"], x["Ks"], x["pts"], x["ndc"], x["dirs"])
    raw = ops.mlp_forward(packed, F, x["ndc"].data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, N, S, 0, x["ndc"].device).view(N, S, 4)
    rgb, disp, acc, weights, depth, alpha = ops.composite(raw, x["z"], white_bkgd)
    return {"input_feat": feat, "raw": raw, "_dirs_tmp": dirs, "rgb_map": rgb, "disp": disp, "acc": acc, "weights": weights, "depth": depth,
            "alpha": alpha}


def _check(vol_cl, x, packed, white_bkgd=False):
    from mvsnerf_amd import ops
    with torch.no_grad():
        one = ops.raymarch(vol_cl, x["imgs"], x["w2cs"], x["Ks"], packed, x["pts"], x["ndc"], x["z"], x["dirs"], white_bkgd=white_bkgd,
                           want=("disp", "acc"))
        ref = _stepwise(vol_cl, x, packed, white_bkgd)
    torch.cuda.synchronize()
    assert set(one) == set(ref)
    for k in ref:
        assert one[k].shape == ref[k].shape, k
        assert torch.equal(one[k], ref[k]), (k, float((one[k] - ref[k]).abs().max()))


@pytest.mark.parametrize("N,S", [(300, 1), (37, 16), (50, 64), (20, 128), (7, 128)])
@pytest.mark.parametrize("white_bkgd", [False, True])
def test_onelaunch_composited_in_tile(N, S, white_bkgd):
    x = _inputs(N, S, seed=S)
    _check(_hwdc(x["vol"]), x, _packed(3), white_bkgd)


@pytest.mark.parametrize("N,S", [(100, 7), (9, 200), (5, 300)])
@pytest.mark.parametrize("white_bkgd", [False, True])
def test_onelaunch_composite_falls_back(N, S, white_bkgd):
    x = _inputs(N, S, seed=S)
    _check(_hwdc(x["vol"]), x, _packed(3), white_bkgd)


@pytest.mark.parametrize("V", [1, 3, 5, 7])
def test_onelaunch_views(V):
    """V = 7 (F = 36): the lookups' rows do not fit behind the first weight slab and take the other buffer."""
    x = _inputs(45, 64, V=V, seed=V)
    _check(_hwdc(x["vol"]), x, _packed(V))


def test_onelaunch_config2_shape():
    x = _inputs(1024, 128, D=128, h=176, w=208, H=512, W=640, seed=3)
    _check(_hwdc(x["vol"]), x, _packed(3))


def test_dhwc_volume_takes_the_launch_sequence():
    from mvsnerf_amd import ops
    x = _inputs(60, 64, seed=5)
    vol_cl = ops.channels_last_volume(x["vol"].to(DEV))
    assert vol_cl.is_contiguous()                        # vol[d][y][x][c]: MVSNERF_VOL_DHWC
    _check(vol_cl, x, _packed(3))


def test_render_pixels_fp32_frame_matches_the_sequence():
    """render_pixels on the depth-fastest volume (ray generation + one-launch ray march per sub-batch) against the same frame on the
    vol[d][y][x][c] copy of the volume, which takes the four-launch sequence (the lookups of the two layouts are bit-identical,
    tests/test_gpu_layout.py)."""
    from mvsnerf_amd import ops
    from mvsnerf_amd.synth import make_rig, pose_ref_of
    H, W, S, pad = 48, 64, 24, 4
    rig = make_rig(H, W, seed=11, rot_deg=2.0, smooth=True)
    pd = {k: v.to(DEV) for k, v in pose_ref_of(rig).items()}
    vol = torch.randn((1, 8, 16, H // 4 + 2 * pad, W // 4 + 2 * pad), generator=torch.Generator().manual_seed(2))
    imgs = rig["images_raw"][0, :3].to(DEV)
    packed = _packed(3)
    outs = []
    for vol_cl in (_hwdc(vol), vol[0].permute(1, 2, 3, 0).contiguous().to(DEV)):
        args = (vol_cl, imgs, pd["w2cs"][:3].contiguous(), pd["intrinsics"][:3].contiguous(), packed, H, W, pd["intrinsics"][-1], pd["c2ws"][-1],
                pd["intrinsics"][-1], pd["w2cs"][0], pd["near_fars"][-1], pd["near_fars"][0], S)
        with torch.no_grad():
            outs.append(ops.render_pixels(*args, first_pixel=100, n_pixels=2500, pad=pad, batch_rays=1024, want=("depth", "acc", "disp")))
    for k in ("rgb", "depth", "acc", "disp"):
        assert torch.equal(outs[0][k], outs[1][k]), k
