"""The renderer-consistent density volume on the GPU (csrc/occupancy.hip, ops.voxel_points / max_dilate3d / node_density) and the empty-space path of
the pretrained and fused systems (MVSSystem.scene_density / render_view(skip_empty=) / render_path, MVSSystemFusion.update_density_volume /
render_rays(skip_empty=), MVSSystemFinetune.update_density_volume(render_space=)).

Yardsticks: the node coordinates, the dilation, the density values and every rendered frame are torch.equal to their restatement (tests/occupancy_refs.py,
tests/sparse_refs.py, the dense launch sequence with the dead rows zeroed); the nodes' world positions are held to 4 x the fp32 CPU restatement's own largest
error against float64 on the same inputs; the guarded fp16x3 mode ("auto") through its error next to the dense "auto" sequence's."""
import functools

import pytest
import torch

from tests import occupancy_refs as R
from tests import sparse_refs as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------ A. voxel_points
POINT_CASES = [((5, 6, 7), (24, 32), 0), ((4, 10, 12), (24, 32), 2), ((9, 20, 37), (64, 96), 0)]       # 6660 nodes: 27 workgroups, the last with 4 rows


@functools.lru_cache(maxsize=None)
def _world_refs(grid, ref_hw, pad, lindisp):
    """(float64 world positions, fp32 CPU restatement) of every node, computed once and shared."""
    K, c2w, _, nf = R.camera(seed=grid[0], ref_hw=ref_hw)
    w64 = R.ndc_to_world(R.node_grid(*grid, dtype=torch.float64), K, c2w, nf, ref_hw, pad=pad, lindisp=lindisp, dtype=torch.float64)
    w32 = R.ndc_to_world(R.node_grid(*grid), K, c2w, nf, ref_hw, pad=pad, lindisp=lindisp, dtype=torch.float32)
    return w64, w32


@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("planes", ["all", (1, 3), (2, 2)])
@pytest.mark.parametrize("grid,ref_hw,pad", POINT_CASES)
def test_voxel_points(grid, ref_hw, pad, planes, lindisp):
    from mvsnerf_amd import ops
    D, H, W = grid
    d0, d1 = (0, D) if planes == "all" else planes
    K, c2w, _, nf = R.camera(seed=D, ref_hw=ref_hw)
    ndc, pts = ops.voxel_points(D, H, W, K.to(DEV), c2w.to(DEV), nf.to(DEV), ref_hw, pad=pad, lindisp=lindisp, planes=None if planes == "all" else planes)
    n = (d1 - d0) * H * W
    assert ndc.shape == (n, 3) and pts.shape == (n, 3) and ndc.is_cuda and pts.is_cuda
    assert torch.equal(ndc.cpu(), R.node_grid(D, H, W, planes=(d0, d1)))
    if n == 0:
        return
    rows = slice(d0 * H * W, d1 * H * W)
    w64, w32 = _world_refs(grid, ref_hw, pad, lindisp)
    e_gpu = float((pts.cpu().double() - w64[rows]).abs().max())
    e_cpu = float((w32[rows].double() - w64[rows]).abs().max())
    print(f"voxel_points {grid} pad {pad} planes [{d0},{d1}) lindisp {lindisp}: kernel {e_gpu:.3g}, fp32 restatement {e_cpu:.3g}, ratio {e_gpu / e_cpu:.2f}")
    assert e_gpu <= 4 * e_cpu


def test_voxel_points_unit_axes_ndc_only_and_untouched_rows():
    from mvsnerf_amd import ops
    K, c2w, _, nf = R.camera(seed=1, ref_hw=(24, 32))
    # axes of size 1 give coordinate 0 (and a finite world position)
    ndc, pts = ops.voxel_points(1, 6, 1, K, c2w, nf, (24, 32))
    assert torch.equal(ndc.cpu(), R.node_grid(1, 6, 1)) and bool(torch.isfinite(pts).all())
    want = R.ndc_to_world(R.node_grid(1, 6, 1, dtype=torch.float64), K, c2w, nf, (24, 32))
    assert float((pts.cpu().double() - want).abs().max()) < 1e-5
    # the ndc-only form: no camera, a NULL world pointer
    ndc, none = ops.voxel_points(9, 20, 37, planes=(2, 7))
    assert none is None and torch.equal(ndc.cpu(), R.node_grid(9, 20, 37, planes=(2, 7)))
    # a caller's buffers: the rows of the plane range are written, no other; an unaligned first row takes the dword stores
    D, H, W = 5, 3, 7
    for with_pts in (True, False):
        a, b = torch.full((D * H * W, 3), -7.0, device=DEV), torch.full((D * H * W, 3), -7.0, device=DEV)
        cam = dict(K_ref=K, c2w_ref=c2w, near_far=nf, ref_hw=(24, 32)) if with_pts else {}
        ndc, pts = ops.voxel_points(D, H, W, planes=(1, 4), out=(a, b if with_pts else None), **cam)
        lo, hi = 1 * H * W, 4 * H * W
        assert ndc.data_ptr() == a[lo:].data_ptr() and torch.equal(a[lo:hi].cpu(), R.node_grid(D, H, W, planes=(1, 4)))
        assert bool((a[:lo] == -7.0).all()) and bool((a[hi:] == -7.0).all())
        if with_pts:
            _, fresh = ops.voxel_points(D, H, W, planes=(1, 4), **cam)
            assert torch.equal(b[lo:hi], fresh) and bool((b[:lo] == -7.0).all()) and bool((b[hi:] == -7.0).all())
        else:
            assert pts is None and bool((b == -7.0).all())


# ------------------------------------------------------------------ B. max_dilate3d
@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (7, 9, 70), (1, 1, 4), (3, 5, 8), (6, 7, 72), "unaligned"])
def test_max_dilate3d(shape, r):
    """A row of 70 crosses a wave; rows of 4, 8 and 72 take the four-voxels-per-thread form (one, two and 18 quads per row: the window reaches into
    no, one and both neighbouring quads); "unaligned" is (6,7,72) one float into its buffer, which takes the one-voxel form again."""
    from mvsnerf_amd import ops
    unaligned = shape == "unaligned"
    shape = (6, 7, 72) if unaligned else shape
    x = R.planted(shape, seed=r + shape[2])
    want = R.max_dilate3d(x, r)
    if unaligned:
        src = torch.zeros(x.numel() + 1, device=DEV)[1:].view(shape).copy_(x)
        assert src.data_ptr() % 16 == 4 and src.is_contiguous()
    else:
        src = x.to(DEV)
    with torch.no_grad():
        got = ops.max_dilate3d(src, r)
    assert got.shape == shape and got.data_ptr() != src.data_ptr()
    assert torch.equal(src.cpu().view(torch.int32), x.view(torch.int32))                        # the input is never written
    got = got.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(got[~torch.isnan(want)], want[~torch.isnan(want)])
    if shape[2] > 5:
        assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any())


# ------------------------------------------------------------------ C. node_density on an encoded scene (64 x 96 views, 16 planes, pad 4)
@pytest.fixture(scope="module")
def scene():
    from mvsnerf_amd import train
    from tests.util import load_weights
    mlp_sd, mvs_sd = load_weights()
    args = train.default_args(pad=4, batch_size=64, N_samples=32, chunk=1024)
    s = train.MVSSystem(args, n_depth_planes=16)
    s.render_kwargs_train["network_fn"].load_state_dict(mlp_sd)
    s.MVSNet.load_state_dict(mvs_sd)
    s = s.to(DEV)
    batch = train.synthetic_batch(64, 96, seed=8, smooth=True)
    vol = s.encode_scene(batch)
    assert tuple(vol.shape) == (1, 8, 16, 24, 32)
    return s, batch, vol


def _views(s, batch):
    """What render_view takes from the batch: un-normalised source images, the source cameras, the reference view's camera."""
    data, pose = s.decode_batch(dict(batch))
    imgs = s.unpreprocess(data["images"])
    V = imgs.shape[1] - 1
    H, W = imgs.shape[-2:]
    cam = dict(K_ref=pose["intrinsics"][0], c2w_ref=pose["c2ws"][0], near_far=pose["near_fars"][0], ref_hw=(int(H), int(W)), pad=s.args.pad)
    return imgs[0, :V].contiguous(), pose["w2cs"][:V].contiguous(), pose["intrinsics"][:V].contiguous(), cam, pose


def _node_rays(D, H, W, cam=None):
    """The nodes as one "ray" per (k,j) row with W samples: (pts | None, ndc, z, dirs)."""
    from mvsnerf_amd import ops
    ndc, pts = ops.voxel_points(D, H, W, device=torch.device(DEV, torch.cuda.current_device()), **(cam or {}))
    g = torch.Generator().manual_seed(3)
    z = (torch.linspace(2.0, 5.0, W)[None] + torch.rand((D * H, 1), generator=g)).contiguous().to(DEV)
    dirs = torch.nn.functional.normalize(torch.randn((D * H, 3), generator=g), dim=1).to(DEV)
    return None if pts is None else pts.view(D * H, W, 3), ndc.view(D * H, W, 3), z, dirs


def test_node_density_is_the_ray_march_sigma_at_the_nodes(scene):
    from mvsnerf_amd import ops
    s, batch, vol = scene
    imgs, w2cs, Ks, cam, _ = _views(s, batch)
    net = s.render_kwargs_train["network_fn"]
    vol_cl = ops.channels_last_volume(vol)
    D, H, W = vol_cl.shape[:3]
    with torch.no_grad(), ops.mlp_precision("fp32"):
        dens = {p: ops.node_density(vol_cl, net.packed(20), w2cs, imgs=imgs, intrinsics=Ks, camera=cam, planes_per_call=p) for p in (1, 5, 16)}
        default = ops.node_density(vol_cl, net.packed(20), w2cs, imgs=imgs, intrinsics=Ks, camera=cam)
        pts, ndc, z, dirs = _node_rays(D, H, W, cam)
        raw = ops.raymarch(vol_cl, imgs, w2cs, Ks, net.packed(20), pts, ndc, z, dirs)["raw"]
        dil = ops.node_density(vol_cl, net.packed(20), w2cs, imgs=imgs, intrinsics=Ks, camera=cam, dilate=1)
        via_system = s.scene_density(batch, volume=vol)
        encoded_here = s.scene_density(batch)
    want = raw[..., 3].reshape(D, H, W)
    assert dens[16].shape == (D, H, W) and bool(torch.isfinite(want).all()) and float(want.max()) > 0
    print(f"node density: max {float(want.max()):.4g}, share above 0: {float((want > 0).float().mean()):.3f}")
    assert torch.equal(dens[16], want)
    assert torch.equal(dens[1], dens[16]) and torch.equal(dens[5], dens[16]) and torch.equal(default, dens[16])
    assert torch.equal(dil, ops.max_dilate3d(dens[16], 1)) and torch.equal(dil.cpu(), R.max_dilate3d(dens[16].cpu(), 1))
    assert torch.equal(via_system, dens[16]) and torch.equal(encoded_here, dens[16])


def test_node_density_v2_has_no_relu(scene):
    from mvsnerf_amd import models, ops
    s, batch, vol = scene
    imgs, w2cs, Ks, cam, _ = _views(s, batch)
    m = models.MVSNeRF(D=6, W=128, input_ch_pts=63, input_ch_views=3, input_ch_feat=20, skips=[4], net_type="v2")
    torch.manual_seed(20)
    for p in m.parameters():
        torch.nn.init.uniform_(p, -0.15, 0.15)
    m = m.to(DEV)
    vol_cl = ops.channels_last_volume(vol)
    D, H, W = vol_cl.shape[:3]
    with torch.no_grad(), ops.mlp_precision("fp32"):
        dens = ops.node_density(vol_cl, m.packed(20), w2cs, imgs=imgs, intrinsics=Ks, camera=cam, planes_per_call=5, **m.packed_alt(20))
        pts, ndc, _, _ = _node_rays(D, H, W, cam)
        feat, _ = ops.gather(vol_cl, imgs, w2cs, Ks, pts, ndc)
        want = s.render_kwargs_train["network_query_fn"](ndc, None, feat, m)                     # forward_alpha semantics: viewdirs None
    assert want.shape == (D * H, W, 1)
    assert torch.equal(dens, want.reshape(D, H, W))
    assert bool((dens < 0).any()) and bool((dens > 0).any())                                     # no ReLU on a v2 sigma


def test_node_density_colour_volume(scene):
    from mvsnerf_amd import ops
    s, batch, vol = scene
    _, w2cs, _, _, _ = _views(s, batch)
    net = s.render_kwargs_train["network_fn"]
    g = torch.Generator().manual_seed(11)
    cvol = torch.cat((ops.channels_last_volume(vol).contiguous(), torch.rand((16, 24, 32, 12), generator=g).to(DEV)), -1).contiguous()
    with torch.no_grad(), ops.mlp_precision("fp32"):
        dens = ops.node_density(cvol, net.packed(20), w2cs, planes_per_call=5)
        _, ndc, z, dirs = _node_rays(16, 24, 32)
        raw = ops.raymarch_colorvol_batched(cvol, w2cs, net.packed(20), [(ndc, z, dirs)])[0]["raw"]
        feat, _ = ops.gather_colorvol(cvol, ndc)
        sigma = net.query(ndc, feat, None, 16 * 24, 32)
    assert torch.equal(dens, raw[..., 3].reshape(16, 24, 32)) and torch.equal(dens, sigma.reshape(16, 24, 32))


# ------------------------------------------------------------------ D. MVSSystem.render_view(skip_empty=)
def _band(lo=4, hi=8, shape=(16, 24, 32)):
    d = torch.zeros(shape)
    d[lo:hi] = 1.0
    return d


def _loop(s, batch, vol, density, thr, B, target=None, zero=True):
    """render_view(skip_empty=thr, density=) spelled out: per sub-batch of B pixels ops.raygen -> the dense launch sequence -> the dead rows of raw (the CPU
    oracle's) zeroed -> ops.composite.  Returns rgb (H,W,3), depth (H,W) and the oracle's live fraction."""
    from mvsnerf_amd import ops
    a = s.args
    imgs, w2cs, Ks, _, pose = _views(s, batch)
    H, W = imgs.shape[-2:]
    K_tgt, c2w_tgt, K_ndc, nf_t, ref_hw = pose["intrinsics"][-1], pose["c2ws"][-1], pose["intrinsics"][-1], pose["near_fars"][-1], None
    if target is not None:
        ref_hw, (H, W) = (H, W), target["hw"]
        K_tgt, c2w_tgt, K_ndc = target["intrinsic"].to(DEV), target["c2w"].to(DEV), pose["intrinsics"][0]
        nf_t = target.get("near_far", nf_t).to(DEV)
    net = s.render_kwargs_train["network_fn"]
    vol_cl = ops.channels_last_volume(vol)
    F = a.feat_dim
    packed, alt = net.packed(F), net.packed_alt(F)
    rgbs, depths, live_n, total = [], [], 0, 0
    for first in range(0, H * W, B):
        n = min(B, H * W - first)
        pts, dirs, ndc, z, _ = ops.raygen(H, W, K_tgt, c2w_tgt, K_ndc, pose["w2cs"][0], nf_t.reshape(-1)[:2].contiguous(),
                                          pose["near_fars"][0].reshape(-1)[:2].contiguous(), a.N_samples, pad=a.pad, first_pixel=first, n_rays=n, ref_hw=ref_hw)
        if net.wide:
            feat, dd = ops.gather(vol_cl, imgs, w2cs, Ks, pts, ndc, dirs)
            full = ops.mlp_forward(packed, F, ndc.data_ptr(), 3, feat.data_ptr(), F, dd.data_ptr(), 3, n, a.N_samples, 0, ndc.device).view(n, a.N_samples, 4)
        else:
            full = ops.raymarch(vol_cl, imgs, w2cs, Ks, packed, pts, ndc, z, dirs, **alt)["raw"]
        live = SR.live_mask(density.cpu(), ndc.cpu(), thr).to(DEV).view(n, a.N_samples)
        raw = torch.where(live[..., None], full, torch.zeros_like(full)) if zero else full
        rgb, _, _, _, depth, _ = ops.composite(raw.contiguous(), z, False)
        rgbs.append(rgb)
        depths.append(depth)
        live_n += int(live.sum())
        total += live.numel()
    return torch.cat(rgbs).reshape(H, W, 3), torch.cat(depths).reshape(H, W), live_n / total


def test_render_view_skip_empty_equals_the_loop(scene):
    from mvsnerf_amd import ops
    s, batch, vol = scene
    band = _band().to(DEV)
    with torch.no_grad(), ops.mlp_precision("fp32"):
        rgb, depth = s.render_view(batch, volume=vol, skip_empty=0.0, density=band, batch_rays=1000)          # 6144 pixels: six sub-batches of 1000, one of 144
        frac = s.last_live_fraction
        want_rgb, want_depth, want_frac = _loop(s, batch, vol, band, 0.0, 1000)
        other, _ = s.render_view(batch, volume=vol, skip_empty=0.0, density=band, batch_rays=4096)
        dense_rgb, dense_depth = s.render_view(batch, volume=vol)
        zeros = s.render_view(batch, volume=vol, skip_empty=0.0, density=torch.zeros_like(band), batch_rays=1000)
        f_zero = s.last_live_fraction
        ones = s.render_view(batch, volume=vol, skip_empty=0.0, density=torch.ones_like(band), batch_rays=1000)
        f_one = s.last_live_fraction
    assert rgb.shape == (64, 96, 3) and depth.shape == (64, 96)
    print(f"band planes 4..7: live fraction {frac:.4f}")
    assert 0.0 < frac < 1.0 and frac == want_frac
    assert torch.equal(rgb, want_rgb) and torch.equal(depth, want_depth)
    assert torch.equal(other, rgb)                                                                         # the sub-batch size is a free parameter
    assert f_zero == 0.0 and not bool(zeros[0].any()) and not bool(zeros[1].any())                        # nothing live: the background frame
    assert not torch.equal(rgb, dense_rgb)
    print(f"all-one density: live fraction {f_one:.6f}")                                                   # 1 when every sample's cell touches the grid
    assert torch.equal(ones[0], dense_rgb) and torch.equal(ones[1], dense_depth)                          # an all-one density: the dense frame


def test_render_view_all_live_equals_the_dense_frame_at_a_target_grid(scene):
    """The reference view's own camera at 20 x 28 pixels: its rays stay inside its frustum volume, so an all-one density keeps every sample and the
    frame is the dense one, through the whole-frame entry's target= arithmetic."""
    from mvsnerf_amd import ops
    s, batch, vol = scene
    ones = torch.ones((16, 24, 32), device=DEV)
    pose = _views(s, batch)[4]
    with torch.no_grad(), ops.mlp_precision("fp32"):
        target = dict(hw=(20, 28), intrinsic=pose["intrinsics"][0] * torch.tensor([[28 / 96], [20 / 64], [1.0]], device=DEV), c2w=pose["c2ws"][0])
        rgb, depth = s.render_view(batch, volume=vol, target=target, skip_empty=0.0, density=ones, batch_rays=300)
        frac = s.last_live_fraction
        dense_rgb, dense_depth = s.render_view(batch, volume=vol, target=target)
    print(f"reference-view camera at 20 x 28, all-one density: live fraction {frac:.4f}")
    assert frac == 1.0                                                       # the reference view's own rays stay inside its frustum volume
    assert torch.equal(rgb, dense_rgb) and torch.equal(depth, dense_depth)


def test_render_view_skip_empty_with_a_target_grid(scene):
    from mvsnerf_amd import ops
    s, batch, vol = scene
    pose = _views(s, batch)[4]
    scale = torch.tensor([[28 / 96], [20 / 64], [1.0]], device=DEV)
    target = dict(hw=(20, 28), intrinsic=pose["intrinsics"][1] * scale, c2w=pose["c2ws"][2], near_far=torch.tensor([2.2, 4.4]))
    band = _band().to(DEV)
    with torch.no_grad(), ops.mlp_precision("fp32"):
        rgb, depth = s.render_view(batch, volume=vol, target=target, skip_empty=0.0, density=band, batch_rays=150)
        frac = s.last_live_fraction
        want = _loop(s, batch, vol, band, 0.0, 150, target=target)
    assert rgb.shape == (20, 28, 3) and 0.0 < frac < 1.0 and frac == want[2]
    assert torch.equal(rgb, want[0]) and torch.equal(depth, want[1])


def test_render_view_skip_empty_auto_mode_error_is_the_dense_error(scene):
    """As tests/test_gpu_sparse_render.py::test_raymarch_sparse_auto_mode_error_is_the_dense_error: regrouping the live samples into other MLP tiles
    changes no product's rounding in the guarded fp16x3 sequence; 1.25 is the margin of one re-associated chain."""
    from mvsnerf_amd import ops
    s, batch, vol = scene
    band = _band().to(DEV)
    with torch.no_grad():
        with ops.mlp_precision("fp32"):
            ref_rgb, ref_depth, _ = _loop(s, batch, vol, band, 0.0, 1000)
        with ops.mlp_precision("auto"):
            n0 = ops.guard_fallbacks()
            assert "guard" in s.render_kwargs_train["network_fn"].packed_alt(20)
            rgb, depth = s.render_view(batch, volume=vol, skip_empty=0.0, density=band, batch_rays=1000)
            dense_rgb, dense_depth, _ = _loop(s, batch, vol, band, 0.0, 1000)
            assert ops.guard_fallbacks() == n0
    e_sparse, e_dense = float((rgb - ref_rgb).abs().max()), float((dense_rgb - ref_rgb).abs().max())
    d_sparse, d_dense = float((depth - ref_depth).abs().max()), float((dense_depth - ref_depth).abs().max())
    print(f"auto vs fp32: rgb e_sparse {e_sparse:.3g} e_dense {e_dense:.3g}; depth e_sparse {d_sparse:.3g} e_dense {d_dense:.3g}")
    assert e_sparse <= 1.25 * e_dense and d_sparse <= 1.25 * d_dense


def test_render_view_default_density_and_render_path(scene):
    from mvsnerf_amd import ops
    from tests.test_gpu_frames import _path_of
    s, batch, vol = scene
    pose = _views(s, batch)[4]
    poses = _path_of(pose["c2ws"][:3])
    H, W = 20, 28
    K = pose["intrinsics"][0] * torch.tensor([[W / 96], [H / 64], [1.0]], device=DEV)
    with torch.no_grad(), ops.mlp_precision("fp32"):
        dens = s.scene_density(batch, volume=vol)
        dil = s.scene_density(batch, volume=vol, dilate=1)
        thr = float(dens[dens > 0].median()) if bool((dens > 0).any()) else 0.0
        a = s.render_view(batch, volume=vol, skip_empty=thr, batch_rays=2048)
        fa = s.last_live_fraction
        b = s.render_view(batch, volume=vol, skip_empty=thr, density=dens, batch_rays=2048)
        assert fa == s.last_live_fraction and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        c = s.render_view(batch, volume=vol, skip_empty=thr, dilate=1, batch_rays=2048)
        fc = s.last_live_fraction
        d = s.render_view(batch, volume=vol, skip_empty=thr, density=dil, batch_rays=2048)
        assert torch.equal(c[0], d[0]) and fc >= fa
        print(f"scene density at its median {thr:.4g}: live fraction {fa:.4f}, dilated by one voxel {fc:.4f}")
        frames = s.render_path_skip_empty(batch, poses, thr, dilate=1, hw=(H, W), intrinsic=K, volume=vol)
        dense = s.render_path(batch, poses, hw=(H, W), intrinsic=K, volume=vol)
        nf = pose["near_fars"][-1]
        for k in range(poses.shape[0]):
            tgt = dict(hw=(H, W), intrinsic=K, c2w=torch.as_tensor(poses[k]).float().to(DEV), near_far=nf)
            rgb, depth = s.render_view(batch, volume=vol, target=tgt, skip_empty=thr, density=dil)
            assert torch.equal(frames[k], ops.frame_u8(rgb, depth, minmax=pose["near_fars"][0])), k
    assert frames.shape == dense.shape and frames.dtype == torch.uint8


def test_render_view_skip_empty_netwidth_256_v2():
    from mvsnerf_amd import train
    args = train.default_args(pad=4, batch_size=64, N_samples=16, chunk=256, netwidth=256, net_type="v2")
    torch.manual_seed(256)
    s = train.MVSSystem(args, n_depth_planes=16).to(DEV)                   # seeded weights; the volume is handed in, so nothing is encoded
    batch = train.synthetic_batch(64, 96, seed=8, smooth=True)
    pose = _views(s, batch)[4]
    vol = torch.randn((1, 8, 16, 24, 32), generator=torch.Generator().manual_seed(7)).to(DEV)
    target = dict(hw=(10, 12), intrinsic=pose["intrinsics"][0] * torch.tensor([[12 / 96], [10 / 64], [1.0]], device=DEV), c2w=pose["c2ws"][1])
    band = _band().to(DEV)
    with torch.no_grad():
        rgb, depth = s.render_view(batch, volume=vol, target=target, skip_empty=0.0, density=band, batch_rays=37)      # 120 pixels: 37, 37, 37, 9
        frac = s.last_live_fraction
        want = _loop(s, batch, vol, band, 0.0, 37, target=target)
        dens = s.scene_density(batch, volume=vol)
    assert 0.0 < frac < 1.0 and frac == want[2]
    assert torch.equal(rgb, want[0]) and torch.equal(depth, want[1])
    assert tuple(dens.shape) == (16, 24, 32) and bool((dens < 0).any())


# ------------------------------------------------------------------ E. the fused scene (tests/test_gpu_fusion.py's smallest fixture)
def _fusion_loop(sysm, rays, density, thr, B):
    from mvsnerf_amd import ops
    a = sysm.args
    vol_cl = ops.channels_last_volume(sysm.volume.feat_volume)
    net = sysm.network_fn
    w2cs = sysm.pose_source_ref["w2cs"][:3].contiguous()
    rays = rays.to(DEV)
    rgbs, depths, live_n, total = [], [], 0, 0
    for i in range(0, rays.shape[0], B):
        r = rays[i:i + B]
        pts, ndc, z = ops.ray_march_bbox(r, sysm.bbox_3d, a.N_samples)
        full = ops.raymarch_colorvol_batched(vol_cl, w2cs, net.packed(20), [(ndc, z, r[:, 3:6].contiguous())], **net.packed_alt(20))[0]["raw"]
        live = SR.live_mask(density.cpu(), ndc.cpu(), thr).to(DEV).view(z.shape)
        raw = torch.where(live[..., None], full, torch.zeros_like(full))
        rgb, _, _, _, depth, _ = ops.composite(raw.contiguous(), z, False)
        rgbs.append(rgb)
        depths.append(depth)
        live_n += int(live.sum())
        total += live.numel()
    return torch.cat(rgbs), torch.cat(depths), live_n / total


def test_fusion_skip_empty_and_update_density_volume():
    from mvsnerf_amd import ops, train
    from tests.test_gpu_fusion import DIMS, fusion_system, fusion_views
    views, bbox, img_wh, focal = fusion_views()
    with ops.mlp_precision("fp32"), torch.no_grad():
        sysm, _ = fusion_system(views, bbox, img_wh, focal)
        assert tuple(sysm.density_volume.shape) == (1, 1, *DIMS)
        ro, rd = train.get_rays(train.get_ray_directions(64, 96, focal), views[1][4])
        pick = torch.randperm(ro.shape[0], generator=torch.Generator().manual_seed(3))[:300]
        rays = torch.cat([ro[pick], rd[pick], torch.full((300, 1), 2.125), torch.full((300, 1), 4.525)], 1)
        dense_rgb, _ = sysm.render_rays(rays)
        fused = sysm.density_volume.reshape(DIMS).clone()
        band = torch.zeros(DIMS, device=DEV)
        band[3:6] = 1.0
        for name, density in (("fused", fused), ("band", band)):
            sysm.density_volume = density.view(1, 1, *DIMS)
            rgb, depth = sysm.render_rays(rays, skip_empty=0.0, batch_rays=128)
            frac = sysm.last_live_fraction
            want = _fusion_loop(sysm, rays, density, 0.0, 128)
            print(f"fusion, {name} density: live fraction {frac:.4f}, max |rgb - dense| {float((rgb - dense_rgb).abs().max()):.3g}")
            assert rgb.shape == (300, 3) and depth.shape == (300,) and frac == want[2]
            assert torch.equal(rgb, want[0]) and torch.equal(depth, want[1])
            if name == "band":
                assert 0.0 < frac < 1.0
        out = sysm.update_density_volume()
        assert out is sysm.density_volume and tuple(out.shape) == (1, 1, *DIMS)
        D, H, W = DIMS
        _, ndc, z, dirs = _node_rays(D, H, W)
        raw = ops.raymarch_colorvol_batched(ops.channels_last_volume(sysm.volume.feat_volume), sysm.pose_source_ref["w2cs"][:3].contiguous(),
                                            sysm.network_fn.packed(20), [(ndc, z, dirs)])[0]["raw"]
        assert torch.equal(out.reshape(DIMS), raw[..., 3].reshape(DIMS))
        rgb, _ = sysm.render_rays(rays, skip_empty=0.0, batch_rays=128)
        want = _fusion_loop(sysm, rays, out.reshape(DIMS), 0.0, 128)
        assert torch.equal(rgb, want[0]) and sysm.last_live_fraction == want[2]
        dil = sysm.update_density_volume(dilate=1)
        assert torch.equal(dil.reshape(DIMS), ops.max_dilate3d(out.reshape(DIMS), 1))


# ------------------------------------------------------------------ F. the fine-tuned scene
@pytest.mark.parametrize("color", [False, True])
def test_finetune_update_density_volume_both_spaces(color):
    from mvsnerf_amd import ops, utils
    from mvsnerf_amd.renderer import render_density
    from tests.test_gpu_finetune_render import _system
    ft, _, _ = _system(V=3, **({"use_color_volume": True} if color else {}))
    Dv, Hv, Wv = ft.volume.feat_volume.shape[-3:]
    with ops.mlp_precision("fp32"):
        # no arguments: the reference-faithful volume, restated from public calls as the method ran them before render_space existed
        ft.update_density_volume()
        world_space = ft.density_volume
        with torch.no_grad():
            K = ft.pose_source["intrinsics"][0].clone()
            K[:2] /= 4
            vox = utils.get_ptsvolume(Hv - 2 * ft.args.pad, Wv - 2 * ft.args.pad, Dv, ft.args.pad, ft.near_far_source, K, ft.pose_source["c2ws"][0]).contiguous()
            vol_cl = ops.channels_last_volume(ft.volume.feat_volume.detach())
            cf = utils.build_color_volume(vox, ft.pose_source, ft.imgs, with_mask=True)
            feats = vol_cl.reshape(Dv * Hv, Wv, 20) if color else torch.cat((vol_cl.reshape(Dv * Hv, Wv, 8), cf), -1)
            want = render_density(ft.network_fn, vox, feats, ft.render_kwargs_train["network_query_fn"]).reshape(Dv, Hv, Wv)
        assert torch.equal(world_space, want)
        ft.update_density_volume(render_space=False)
        assert torch.equal(ft.density_volume, want)
        # render_space=True: ops.node_density on the learnt volume
        ft.update_density_volume(render_space=True)
        ndc_space = ft.density_volume
        with torch.no_grad():
            src = {} if color else dict(imgs=ft.imgs[0].contiguous(), intrinsics=ft.pose_source["intrinsics"][:3].contiguous(),
                                        camera=dict(K_ref=ft.pose_source["intrinsics"][0], c2w_ref=ft.pose_source["c2ws"][0], near_far=ft.near_far_source,
                                                    ref_hw=(64, 96), pad=ft.args.pad))
            direct = ops.node_density(vol_cl, ft.network_fn.packed(20), ft.pose_source["w2cs"][:3].contiguous(), **src)
        assert tuple(ndc_space.shape) == (Dv, Hv, Wv) and torch.equal(ndc_space, direct)
        assert not torch.equal(ndc_space, world_space)                                       # two different functions of the same weights
        ft.update_density_volume(render_space=True, dilate=2)
        assert torch.equal(ft.density_volume, ops.max_dilate3d(direct, 2))
        print(f"fine-tuned scene (colour volume {color}): share of voxels above 0 - world-space query {float((world_space > 0).float().mean()):.3f}, "
              f"renderer-consistent {float((ndc_space > 0).float().mean()):.3f}")
