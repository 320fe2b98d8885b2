"""CPU-only: the restatement of the scene ray bank's arithmetic (tests/scene_rays_refs.py) against the reference's own outputs
(tests/golden/caseF_scene_rays.npz, written by tests/gen_golden_scene_rays.py), and the host-side parts of rays.SceneRays - source_views and the
epoch sampler."""
import numpy as np
import pytest
import torch

from tests import scene_rays_refs as R

H, W = 6, 7


@pytest.fixture(scope="module")
def g():
    return {k: torch.from_numpy(v) for k, v in R.golden().items()}


def test_rays_against_the_reference(g):
    idx = torch.arange(2 * H * W)
    rays, _, _, _ = R.gather_ref(torch.zeros((2, H, W, 3), dtype=torch.uint8), g["c2ws"], g["intrinsics"], g["near_far"], None, idx)
    ref = g["all_rays"]
    assert torch.equal(rays[:, 0:3], ref[:, 0:3]) and torch.equal(rays[:, 6:8], ref[:, 6:8])       # rays_o, near, far: copies
    # rays_d: two fp32 evaluations of one 3-term dot product, the reference's through a matmul
    bound = torch.cat([R.rays_d_bound(g["c2ws"][m], g["intrinsics"][m], H, W) for m in range(2)], 0)
    err = (rays[:, 3:6].double() - ref[:, 3:6].double()).abs()
    print("rays_d: max error / bound", float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())
    # a shuffled, repeated index batch picks the same rows
    pick = torch.tensor([83, 0, 41, 42, 41, 7])
    assert torch.equal(R.gather_ref(torch.zeros((2, H, W, 3), dtype=torch.uint8), g["c2ws"], g["intrinsics"], g["near_far"], None, pick)[0], rays[pick])


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("lindisp", [0, 1])
@pytest.mark.parametrize("perturb", [0, 1])
def test_depths_against_the_reference(g, S, lindisp, perturb):
    idx = torch.arange(2 * H * W)
    _, _, z = R.march_ref(torch.zeros((2, H, W, 3), dtype=torch.uint8), g["c2ws"], g["intrinsics"], g["near_far"], idx, S, g[f"draw_S{S}"], float(perturb),
                          bool(lindisp))
    assert torch.equal(z, g[f"z_S{S}_l{lindisp}_p{perturb}"])


def test_out_of_range_rows_are_zero(g):
    idx = torch.tensor([-1, 5, 2 * H * W, 2 * H * W + 9, -2 ** 40])
    imgs = torch.full((2, H, W, 4), 200, dtype=torch.uint8)
    rays, rgb, depth, mask = R.gather_ref(imgs, g["c2ws"], g["intrinsics"], g["near_far"], torch.ones((2, H, W)), idx)
    _, _, z = R.march_ref(imgs, g["c2ws"], g["intrinsics"], g["near_far"], idx, 5, torch.rand((5, 5)), 1.0, True)
    for row in (0, 2, 3, 4):
        assert not rays[row].any() and not rgb[row].any() and not depth[row] and not mask[row] and not z[row].any()
    assert rays[1].any() and rgb[1].any() and depth[1] == 1 and mask[1] and z[1].all()


def test_colours_are_totensor_and_the_blend_onto_white():
    gen = torch.Generator().manual_seed(5)
    M, h, w = 2, 5, 9
    u8 = torch.randint(0, 256, (M, h, w, 4), generator=gen, dtype=torch.uint8)
    u8[0, 0, :3, 3] = torch.tensor([0, 255, 1], dtype=torch.uint8)
    u8[1, 1] = torch.arange(w * 4, dtype=torch.uint8).reshape(w, 4) * 7
    c2ws, K, nf = torch.eye(4).expand(M, 4, 4), torch.tensor([[5.0, 0, 4.5], [0, 5.0, 2.5], [0, 0, 1]]), torch.tensor([2.0, 6.0])
    idx = torch.arange(M * h * w)
    # RGB: ToTensor alone, what Image -> self.transform -> view(3, -1).permute(1, 0) leaves (data/dtu_ft.py:162-166)
    _, rgb, _, mask = R.gather_ref(u8[..., :3].contiguous(), c2ws, K, nf, None, idx)
    assert torch.equal(rgb, torch.from_numpy(u8[..., :3].numpy()).float().div(255).reshape(-1, 3)) and bool(mask.all())
    # RGBA: data/blender.py:67-70 on the (4, h, w) tensor of each image
    _, rgb, _, mask = R.gather_ref(u8, c2ws, K, nf, None, idx)
    for m in range(M):
        img = torch.from_numpy(u8[m].numpy()).float().div(255).permute(2, 0, 1)        # ToTensor: (4, h, w)
        img = img.reshape(4, -1).permute(1, 0)
        assert torch.equal(mask[m * h * w:(m + 1) * h * w], (img[:, -1:] > 0)[:, 0])
        assert torch.equal(rgb[m * h * w:(m + 1) * h * w], img[:, :3] * img[:, -1:] + (1 - img[:, -1:]))
    # every byte value: the 256-entry table of ToTensor
    table = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()
    _, rgb, _, _ = R.gather_ref(table, c2ws[:1], K, nf, None, torch.arange(256))
    assert torch.equal(rgb[:, 0], torch.arange(256) / 255)


def test_source_views_match_make_rig():
    """A bank built from the cameras of synth.make_rig (fp32, as the rig hands them out): proj_mats within one fp32 unit in the last place of the rig's
    own, entry by entry - both are float64 products rounded once, from inputs that differ by the fp32 rounding of the cameras."""
    from mvsnerf_amd.rays import SceneRays
    from mvsnerf_amd.synth import IMAGENET_MEAN, IMAGENET_STD, make_rig
    rig = make_rig(32, 40, n_views=4, seed=3)
    u8 = (rig["images_raw"][0].permute(0, 2, 3, 1) * 255).round().to(torch.uint8)
    nf = rig["near_fars"][0].clone()
    nf[2] = torch.tensor([1.5, 7.0])
    scene = SceneRays(u8, rig["c2ws"][0], rig["intrinsics"][0], nf, device="cpu")
    imgs, proj, near_far, pose = scene.source_views([0, 1, 2])
    assert imgs.shape == (1, 3, 3, 32, 40) and proj.shape == (1, 3, 3, 4) and near_far.shape == (2,)
    ref = rig["proj_mats"][:, :3]
    ulp = torch.from_numpy(np.spacing(ref.abs().numpy()))
    print("proj_mats: max |difference| in ulps", float(((proj - ref).abs() / ulp).max()))
    assert bool(((proj - ref).abs() <= ulp).all())
    assert torch.equal(proj[0, 0], torch.eye(4)[:3])                     # the reference view's is the identity
    assert torch.equal(near_far, nf[2])                                  # that of ids[-1] (data/dtu_ft.py:88)
    assert torch.equal(pose["intrinsics"], rig["intrinsics"][0, :3])     # full resolution
    assert torch.equal(pose["c2ws"], rig["c2ws"][0, :3]) and pose["w2cs"].shape == (3, 4, 4)
    assert float((pose["w2cs"] - rig["w2cs"][0, :3]).abs().max()) < 1e-6
    mean, std = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
    assert torch.equal(imgs[0], (u8[:3].float().div(255).permute(0, 3, 1, 2) - mean) / std)
    # another reference view: its projection is the identity and the others are relative to it
    _, proj2, near_far2, _ = scene.source_views([2, 0])
    assert torch.equal(proj2[0, 0], torch.eye(4)[:3]) and torch.equal(near_far2, nf[0]) and not torch.equal(proj2[0, 1], proj[0, 2])
    # RGBA sources are blended onto white (data/blender.py:135)
    rgba = torch.cat((u8, torch.full_like(u8[..., :1], 64)), -1)
    rgba[0, 0, 0, 3] = 0
    imgs_a = SceneRays(rgba, rig["c2ws"][0], rig["intrinsics"][0], nf, device="cpu").source_views([0, 1, 2])[0]
    c = rgba[:3].float().div(255).permute(0, 3, 1, 2)
    assert torch.equal(imgs_a[0], ((c[:, :3] * c[:, 3:] + (1 - c[:, 3:])) - mean) / std)
    assert torch.equal(imgs_a[0, 0, :, 0, 0], (torch.ones(3) - mean.view(3)) / std.view(3))      # alpha 0: white


def test_epoch_is_one_shuffled_pass():
    from mvsnerf_amd.rays import SceneRays
    M, h, w, B = 3, 5, 7, 16
    scene = SceneRays(torch.zeros((M, h, w, 3), dtype=torch.uint8), torch.eye(4).expand(M, 4, 4), torch.eye(3), torch.tensor([2.0, 6.0]), device="cpu")
    n = scene.n_rays
    batches = list(scene.epoch(B, torch.Generator().manual_seed(4)))
    assert len(batches) == -(-n // B) and all(b.shape == (B,) for b in batches[:-1]) and batches[-1].shape == (n % B,)     # drop_last=False
    assert all(b.dtype == torch.int64 for b in batches)
    assert torch.equal(torch.sort(torch.cat(batches))[0], torch.arange(n))           # every ray exactly once
    assert not torch.equal(torch.cat(batches), torch.arange(n))
    again = list(scene.epoch(B, torch.Generator().manual_seed(4)))
    assert all(torch.equal(a, b) for a, b in zip(batches, again))                    # one seed, one order
    other = list(scene.epoch(B, torch.Generator().manual_seed(5)))
    assert not torch.equal(torch.cat(other), torch.cat(batches))
    gen = torch.Generator().manual_seed(4)                                           # one generator, consecutive epochs differ
    first, second = torch.cat(list(scene.epoch(B, gen))), torch.cat(list(scene.epoch(B, gen)))
    assert torch.equal(first, torch.cat(batches)) and not torch.equal(second, first)
    assert [b.shape[0] for b in scene.epoch(n, torch.Generator().manual_seed(1))] == [n]     # a batch of the whole scene
    with pytest.raises(ValueError):
        next(scene.epoch(0))
    # the batches of fit_scene: epochs follow one another from one seeded generator
    from mvsnerf_amd.train import _scene_index_batches
    steps = list(_scene_index_batches(scene, 9, 16, 4))
    assert len(steps) == 9 and torch.equal(torch.cat(steps[:7]), first) and torch.equal(torch.cat(steps[7:]), second[:32])
