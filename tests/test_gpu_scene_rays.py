"""The scene ray bank on the GPU (csrc/scene_rays.hip, mvsnerf_amd/rays.py, fit_scene of the two per-scene systems).

Reference: tests/scene_rays_refs.py, the elementwise torch-CPU restatement that tests/test_scene_rays_refs.py pins to the reference's own outputs.
Shapes: a bank of M = 3 views of 20 x 28 pixels with distinct intrinsics, poses and near / far; 700 indices holding the first and last pixel of every
view, duplicates, -1 and n_rays and a seeded draw - the smallest that cross a 256-thread block, a wave and a view boundary; S in {1, 3, 16}.

A  gather and march equal the restatement bit for bit (rays, colours, mask, depth, depths of the samples); points and NDC coordinates equal
   ops.ray_points on the kernel's own rays and depths; march's rows equal gather's; rows of an index outside the bank are zero.
B  nothing is written outside the outputs (sentinel-padded buffers, which also puts rays off 16 bytes: the scalar-store form of gather); B = 0.
C  view(m) is the split='val' item: train._path_rays of get_ray_directions / get_rays, the stored image and depth.
D  fit_scene computes what fit_steps computes on the gathered batches, for MVSSystemFinetune (plain, colour volume, importance sampling) and
   MVSSystemFusion: losses and the final volume, bit for bit, with the volume gradient's deterministic scatter.
"""
import math

import pytest
import torch

from tests import scene_rays_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
M, H, W, B = 3, 20, 28, 700


def _rot(ax, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    return torch.tensor({"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[ax],
                        dtype=torch.float64)


@pytest.fixture(scope="module")
def bank():
    """CPU tensors of the bank (RGB and RGBA images), the index batch and the reference camera; computed once, never modified."""
    g = torch.Generator().manual_seed(17)
    rgba = torch.randint(0, 256, (M, H, W, 4), generator=g, dtype=torch.uint8)
    rgba[0, :, :9, 3] = 0                          # alphas 0, 255 and in between
    rgba[1, :, 5:, 3] = 255
    c2ws = torch.eye(4, dtype=torch.float64).repeat(M, 1, 1)
    c2ws[1, :3, :3], c2ws[2, :3, :3] = _rot("y", 14.0) @ _rot("x", -6.0), _rot("z", 9.0) @ _rot("y", -11.0)
    c2ws[:, :3, 3] = torch.tensor([[0.1, -0.2, 0.05], [-0.3, 0.15, 0.4], [0.25, 0.1, -0.2]], dtype=torch.float64)
    K = torch.tensor([[[25.3, 0, 14.0], [0, 24.9, 10.0], [0, 0, 1]], [[23.7, 0, 13.25], [0, 26.1, 9.5], [0, 0, 1]], [[27.9, 0, 14.5], [0, 25.5, 10.75], [0, 0, 1]]])
    nf = torch.tensor([[2.125, 4.525], [1.9, 5.3], [2.4, 6.0]])
    depths = torch.rand((M, H, W), generator=g) * 3 + 2
    n = M * H * W
    edges = [v * H * W for v in range(M)] + [(v + 1) * H * W - 1 for v in range(M)]
    idx = torch.randint(0, n, (B,), generator=g)
    idx[:6] = torch.tensor(edges)
    idx[6:12] = torch.tensor(edges[::-1])          # duplicates
    idx[100], idx[101], idx[255], idx[256], idx[699] = -1, n, n + 5, idx[5], -7
    idx[300:310] = idx[400]
    # reference camera: view 0 of a 4x larger image (H_ref, W_ref), pad 4
    ref = (torch.linalg.inv(c2ws[0]).float().contiguous(), torch.tensor([[60.0, 0, 40.0], [0, 60.0, 32.0], [0, 0, 1]]), torch.tensor([2.0, 5.0]), (64, 80), 4)
    return dict(rgba=rgba, rgb=rgba[..., :3].contiguous(), c2ws=c2ws.float(), K=K, nf=nf, depths=depths, idx=idx, ref=ref, n=n,
                valid=(idx >= 0) & (idx < n))


@pytest.fixture(scope="module")
def scenes(bank):
    from mvsnerf_amd.rays import SceneRays
    return {k: SceneRays(bank[k], bank["c2ws"], bank["K"], bank["nf"], depths=bank["depths"], device=DEV) for k in ("rgb", "rgba")}


def _ref_dev(ref):
    return tuple(t.to(DEV) if torch.is_tensor(t) else t for t in ref)


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("kind", ["rgb", "rgba"])
def test_gather_equals_the_restatement(bank, scenes, kind):
    from mvsnerf_amd import ops
    s = scenes[kind]
    idx = bank["idx"].to(DEV)
    rays, rgbs, depth, mask = ops.scene_rays_gather(s.images, s.c2ws, s.intrinsics, s.near_far, s.depths, idx, want_depth=True, want_mask=True)
    e_rays, e_rgb, e_depth, e_mask = R.gather_ref(bank[kind], bank["c2ws"], bank["K"], bank["nf"], bank["depths"], bank["idx"])
    assert torch.equal(rays.cpu(), e_rays) and torch.equal(rgbs.cpu(), e_rgb) and torch.equal(depth.cpu(), e_depth)
    assert mask.dtype == torch.bool and torch.equal(mask.cpu(), e_mask)
    bad = ~bank["valid"]
    assert int(bad.sum()) == 4 and not rays.cpu()[bad].any() and not rgbs.cpu()[bad].any() and not depth.cpu()[bad].any() and not mask.cpu()[bad].any()
    assert bool(rays.cpu()[bank["valid"]][:, 5].ne(0).all())                     # ... and only those
    if kind == "rgba":
        assert bool((~e_mask[bank["valid"]]).any()) and bool(e_mask.any())       # the batch holds transparent and opaque pixels
    r2, c2 = s.gather(bank["idx"])                                               # the method, from a host index tensor
    assert torch.equal(r2, rays) and torch.equal(c2, rgbs)
    r3, c3, d3, m3 = ops.scene_rays_gather(s.images, s.c2ws, s.intrinsics, s.near_far, None, idx)       # a bank without depths
    assert torch.equal(r3, rays) and torch.equal(c3, rgbs) and d3 is None and m3 is None


@pytest.mark.parametrize("with_ref", [False, True])
@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("perturb", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("S", [1, 3, 16])
def test_march_equals_the_restatement(bank, scenes, S, perturb, lindisp, with_ref):
    from mvsnerf_amd import ops
    kind = "rgba" if lindisp else "rgb"
    s = scenes[kind]
    draw = torch.rand((B, S), generator=torch.Generator().manual_seed(S))
    ref = _ref_dev(bank["ref"]) if with_ref else None
    out = s.march(bank["idx"], S, perturb=perturb, jitter=draw.to(DEV) if perturb > 0 else None, lindisp=lindisp, ref=ref)
    e_rays, e_rgb, e_z = R.march_ref(bank[kind], bank["c2ws"], bank["K"], bank["nf"], bank["idx"], S, draw, perturb, lindisp)
    assert torch.equal(out["rays"].cpu(), e_rays) and torch.equal(out["rgbs"].cpu(), e_rgb) and torch.equal(out["z_vals"].cpu(), e_z)
    g_rays, g_rgb = s.gather(bank["idx"])
    assert torch.equal(out["rays"], g_rays) and torch.equal(out["rgbs"], g_rgb)
    ok, bad = bank["valid"].to(DEV), (~bank["valid"]).to(DEV)
    rays = out["rays"][ok]
    kw = dict(w2c_ref=ref[0], K_ref=ref[1], near_far_ref=ref[2], ref_hw=ref[3], pad=ref[4], lindisp=lindisp) if with_ref else {}
    pts, ndc = ops.ray_points(rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous(), out["z_vals"][ok].contiguous(), **kw)
    assert out["pts"].shape == (B, S, 3) and torch.equal(out["pts"][ok], pts)
    assert not out["pts"][bad].any() and not out["z_vals"][bad].any()
    if with_ref:
        assert out["ndc"].shape == (B, S, 3) and torch.equal(out["ndc"][ok], ndc) and not out["ndc"][bad].any()
        assert bool(torch.isfinite(ndc).all()) and float(ndc[..., 2].max()) > 0      # the rays do cross the reference frustum
    else:
        assert out["ndc"] is None
    if perturb > 0 and S > 1:
        plain = s.march(bank["idx"], S, lindisp=lindisp)["z_vals"]
        assert not torch.equal(plain, out["z_vals"])                             # the draw is used


def test_march_refuses_a_missing_draw(bank, scenes):
    with pytest.raises(RuntimeError, match="jitter"):
        scenes["rgb"].march(bank["idx"], 4, perturb=1.0)
    with pytest.raises(RuntimeError, match="jitter"):
        scenes["rgb"].march(bank["idx"], 4, perturb=1.0, jitter=torch.zeros((B, 5), device=DEV))


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("off", [0, 1])
def test_no_stray_writes(bank, scenes, off):
    """Outputs placed `off` floats (bytes for the mask) into sentinel-filled buffers with 64 sentinel elements behind them.  off = 1 also takes rays off
    16 bytes, which runs the scalar-store form of the gather kernel: the same bits."""
    from mvsnerf_amd import _lib, ops
    s, S = scenes["rgba"], 3
    idx = bank["idx"].to(DEV)
    sent = -12345.0
    ref = _ref_dev(bank["ref"])
    draw = torch.rand((B, S), generator=torch.Generator().manual_seed(2)).to(DEV)
    t = torch.linspace(0, 1, S, device=DEV)
    want = s.march(idx, S, perturb=1.0, jitter=draw, ref=ref)
    _, _, depth, mask = ops.scene_rays_gather(s.images, s.c2ws, s.intrinsics, s.near_far, s.depths, idx, want_depth=True, want_mask=True)

    def padded(n):
        return torch.full((off + n + 64,), sent, device=DEV)

    def check(buf, n, expect):
        assert bool((buf[:off] == sent).all()) and bool((buf[off + n:] == sent).all())
        assert torch.equal(buf[off:off + n], expect.reshape(-1))
    rays, rgb, dep, z, pts, ndc = padded(B * 8), padded(B * 3), padded(B), padded(B * S), padded(B * S * 3), padded(B * S * 3)
    msk = torch.full((off + B + 64,), 77, device=DEV, dtype=torch.uint8)
    p = lambda x, size=4: x.data_ptr() + off * size
    L = _lib.lib()
    ops.check(L.mvsnerf_scene_rays_gather_fwd(s.images.data_ptr(), s.c2ws.data_ptr(), s.intrinsics.data_ptr(), s.near_far.data_ptr(), s.depths.data_ptr(),
                                              M, H, W, idx.data_ptr(), B, p(rays), p(rgb), p(dep), p(msk, 1), ops.stream_ptr()), "scene_rays_gather_fwd")
    torch.cuda.synchronize()
    check(rays, B * 8, want["rays"]), check(rgb, B * 3, want["rgbs"]), check(dep, B, depth)
    assert bool((msk[:off] == 77).all()) and bool((msk[off + B:] == 77).all()) and torch.equal(msk[off:off + B].bool(), mask)
    rays.fill_(sent), rgb.fill_(sent)
    ops.check(L.mvsnerf_scene_rays_march_fwd(s.images.data_ptr(), s.c2ws.data_ptr(), s.intrinsics.data_ptr(), s.near_far.data_ptr(), M, H, W, idx.data_ptr(), B,
                                             t.data_ptr(), S, draw.data_ptr(), 1.0, 0, ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), ref[3][1],
                                             ref[3][0], ref[4], p(rays), p(rgb), p(z), p(pts), p(ndc), ops.stream_ptr()), "scene_rays_march_fwd")
    torch.cuda.synchronize()
    check(rays, B * 8, want["rays"]), check(rgb, B * 3, want["rgbs"]), check(z, B * S, want["z_vals"])
    check(pts, B * S * 3, want["pts"]), check(ndc, B * S * 3, want["ndc"])


def test_empty_batch(scenes):
    s = scenes["rgb"]
    none = torch.empty((0,), dtype=torch.int64)
    rays, rgbs = s.gather(none)
    assert rays.shape == (0, 8) and rgbs.shape == (0, 3) and rays.is_cuda
    out = s.march(none, 5)
    assert out["rays"].shape == (0, 8) and out["rgbs"].shape == (0, 3) and out["z_vals"].shape == (0, 5) and out["pts"].shape == (0, 5, 3) and out["ndc"] is None


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("m", [0, 1, 2])
def test_view_is_the_validation_item(bank, scenes, m):
    from mvsnerf_amd import train
    K, c2w, nf = bank["K"][m], bank["c2ws"][m], bank["nf"][m]
    want = train._path_rays(train.get_ray_directions(H, W, (K[0, 0], K[1, 1]), (K[0, 2], K[1, 2])), c2w, nf)
    rays, img, depth = scenes["rgb"].view(m)
    assert rays.shape == (H * W, 8) and img.shape == (H, W, 3) and depth.shape == (H, W)
    rays = rays.cpu()
    assert torch.equal(rays[:, 0:3], want[:, 0:3]) and torch.equal(rays[:, 6:8], want[:, 6:8])
    assert bool(((rays[:, 3:6].double() - want[:, 3:6].double()).abs() <= R.rays_d_bound(c2w, K, H, W)).all())
    assert torch.equal(img.cpu(), bank["rgb"][m].float().div(255)) and torch.equal(depth.cpu(), bank["depths"][m])
    assert torch.equal(scenes["rgba"].view(m)[0].cpu(), rays)


# ------------------------------------------------------------------ D
def _training_scene():
    """The rig of tests/test_gpu_backward.py as a scene: its four views as 8-bit images, its cameras."""
    from mvsnerf_amd.rays import SceneRays
    from mvsnerf_amd.synth import make_rig
    rig = make_rig(64, 96, seed=21, rot_deg=2.0, smooth=True)
    u8 = (rig["images_raw"][0].permute(0, 2, 3, 1) * 255).round().to(torch.uint8)
    return SceneRays(u8, rig["c2ws"][0], rig["intrinsics"][0], rig["near_fars"][0], device=DEV)


def _finetune_system(scene, **over):
    from mvsnerf_amd import train
    from tests.util import load_weights
    mlp_sd, mvs_sd = load_weights()
    torch.manual_seed(1)                                                         # identical initialisation of whatever the checkpoint does not hold
    ft = train.MVSSystemFinetune(train.default_args(pad=4, batch_size=64, N_samples=16, **over), scene.source_views([0, 1, 2]), n_depth_planes=16).to(DEV)
    ft.network_fn.load_state_dict(mlp_sd)
    return ft


@pytest.fixture
def deterministic_fp32():
    from mvsnerf_amd import ops
    saved = ops.VOLUME_BWD_DETERMINISTIC, ops.MLP_PRECISION
    ops.VOLUME_BWD_DETERMINISTIC, ops.MLP_PRECISION = True, "fp32"
    yield
    ops.VOLUME_BWD_DETERMINISTIC, ops.MLP_PRECISION = saved


@pytest.mark.parametrize("over", [dict(), dict(use_color_volume=True), dict(N_importance=8, use_density_volume=True)], ids=["plain", "color_volume", "importance"])
def test_fit_scene_equals_fit_steps_on_gathered_batches(deterministic_fp32, over):
    """4 steps of B = 64, S = 16.  Two runs of fit_steps on identical batches are bit-equal under ops.VOLUME_BWD_DETERMINISTIC with the fp32 MLP
    (established on the parent commit), so all four losses and the final volume must agree, not the first step only."""
    from mvsnerf_amd import train
    scene = _training_scene()
    a, b = _finetune_system(scene, **over), _finetune_system(scene, **over)
    with torch.no_grad():
        b.volume.feat_volume.copy_(a.volume.feat_volume)                         # identically initialised, whatever the encoder's run-to-run bits are
    v0 = a.volume.feat_volume.detach().clone()
    torch.manual_seed(7)
    la = a.fit_scene(scene, 4, 64, seed=3)
    batches = list(train._scene_index_batches(scene, 4, 64, 3))
    assert len(batches) == 4 and all(i.shape == (64,) and i.is_cuda for i in batches)
    torch.manual_seed(7)
    lb = b.fit_steps([{"rays": scene.gather(i)[0][None], "rgbs": scene.gather(i)[1][None]} for i in batches])
    print("losses", la, lb)
    assert la[0] == lb[0] and math.isfinite(la[0]) and la[0] > 0
    assert la == lb
    assert torch.equal(a.volume.feat_volume, b.volume.feat_volume)
    assert all(torch.equal(p, q) for p, q in zip(a.network_fn.parameters(), b.network_fn.parameters()))
    assert a.global_step == b.global_step == 4
    assert not torch.equal(a.volume.feat_volume, v0)                             # and the steps did train the volume


def test_fit_scene_starts_a_new_epoch_and_defaults_the_batch_size(deterministic_fp32):
    from mvsnerf_amd.rays import SceneRays
    from mvsnerf_amd.synth import make_rig
    rig = make_rig(64, 96, seed=21, rot_deg=2.0, smooth=True)
    u8 = (rig["images_raw"][0].permute(0, 2, 3, 1) * 255).round().to(torch.uint8)
    full = SceneRays(u8, rig["c2ws"][0], rig["intrinsics"][0], rig["near_fars"][0], device=DEV)
    ft = _finetune_system(full)
    # a scene of 100 rays (one view cropped to 10 x 10; its principal point moves with the crop): batches of 64, 36, 64 - a short one, then a new epoch
    K = rig["intrinsics"][0, 3].clone()
    K[0, 2] -= 40
    K[1, 2] -= 30
    small = SceneRays(u8[3:, 30:40, 40:50].contiguous(), rig["c2ws"][0, 3:], K, rig["near_fars"][0, 3:], device=DEV)
    torch.manual_seed(2)
    losses = ft.fit_scene(small, 3)
    assert len(losses) == 3 and all(math.isfinite(l) for l in losses) and ft.global_step == 3
    # ... and the rest of the README's flow: frames along a path, the validation item of a view
    K = rig["intrinsics"][0, 3]
    frames = ft.render_path(rig["c2ws"][0, 3:4], full.hw, (float(K[0, 0]), float(K[1, 1])))
    assert frames.shape == (1, 64, 96 * 2, 3) and frames.dtype == torch.uint8 and frames.is_cuda and int(frames.max()) > 0
    rays, img, depth = full.view(3)
    assert depth is None and math.isfinite(float(ft.validation_step({"rays": rays, "rgbs": img}, 0)["val_psnr_all"]))


def test_fusion_fit_scene_equals_training_step_on_gathered_batches(deterministic_fp32):
    from mvsnerf_amd import train
    from mvsnerf_amd.rays import SceneRays
    from mvsnerf_amd.synth import make_rig
    from tests.test_gpu_fusion import fusion_system, fusion_views
    views, bbox, img_wh, focal = fusion_views()
    rig = make_rig(64, 96, n_views=3, seed=8, rot_deg=2.0, smooth=True)           # the rig fusion_views builds its cameras from
    u8 = (rig["images_raw"][0].permute(0, 2, 3, 1) * 255).round().to(torch.uint8)
    scene = SceneRays(u8, rig["c2ws"][0], rig["intrinsics"][0], rig["near_fars"][0], device=DEV)
    a, b = fusion_system(views, bbox, img_wh, focal)[0], fusion_system(views, bbox, img_wh, focal)[0]
    assert torch.equal(a.volume.feat_volume, b.volume.feat_volume)               # (the splat is bit-reproducible: tests/test_gpu_fusion.py)
    v0 = a.volume.feat_volume.detach().clone()
    torch.manual_seed(7)
    la = a.fit_scene(scene, 4, 64, seed=3)
    batches = list(train._scene_index_batches(scene, 4, 64, 3))
    torch.manual_seed(7)
    opt = b.configure_optimizers()[0][0]
    lb = []
    for i, idx in enumerate(batches):
        rays, rgbs = scene.gather(idx)
        opt.zero_grad(set_to_none=True)
        out = b.training_step({"rays": rays[None], "rgbs": rgbs[None]}, i)
        out["loss"].backward()
        opt.step()
        lb.append(float(out["loss"].detach()))
    print("losses", la, lb)
    assert la[0] == lb[0] and math.isfinite(la[0]) and la[0] > 0
    assert la == lb and torch.equal(a.volume.feat_volume, b.volume.feat_volume) and a.global_step == 4
    assert not torch.equal(a.volume.feat_volume, v0)
