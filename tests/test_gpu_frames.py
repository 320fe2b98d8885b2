"""The 8-bit frame writer (csrc/frames.hip: ops.depth_range, ops.frame_u8, utils.visualize_depth*) against the reference's numpy lines, and the
systems' render_path against the per-frame sequence it stands for.  The kernel's arithmetic is numpy's on float32 (each operation rounded on its
own), so the yardstick is np.array_equal / torch.equal on inputs for which numpy's float -> uint8 cast is defined."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
MI, MA = 2.125, 4.525
SHAPES = [((1, 1), (0, 0)), ((3, 5), (0, 0)), ((17, 23), (0, 1)), ((40, 64), (2, 3)), ((64, 200), (0, 0))]      # (H, W), crop
GUARD = 64


# ------------------------------------------------------------------ the reference's lines
def np_depth_panel(depth, minmax, lut):
    """utils.py:35-43 as written there, a table lookup in place of cv2.applyColorMap."""
    x = np.nan_to_num(depth)
    if minmax is None:
        mi = np.min(x[x > 0])
        ma = np.max(x)
    else:
        mi, ma = minmax
    x = (x - mi) / (ma - mi + 1e-8)
    x = (255 * x).astype(np.uint8)
    return lut[x], [mi, ma]


def np_colour_panel(rgb):
    """renderer_video.ipynb: torch.clamp(rgb, 0, 1).numpy() * 255, then .astype('uint8')."""
    return (torch.clamp(torch.from_numpy(rgb), 0, 1.0).numpy() * 255).astype("uint8")


def np_frame(rgb, depth, minmax, lut, crop):
    H, W = rgb.shape[:2]
    ch, cw = crop
    panels = [np_colour_panel(rgb)] + ([] if depth is None else [np_depth_panel(depth, minmax, lut)[0]])
    return np.concatenate([p[ch:H - ch, cw:W - cw] for p in panels], axis=1)


def _inputs(H, W, seed):
    g = np.random.default_rng(seed)
    rgb = g.uniform(-0.2, 1.2, (H, W, 3)).astype(np.float32)
    depth = np.clip((MI + (MA - MI) * g.uniform(0.0, 1.0, (H, W))).astype(np.float32), np.float32(MI), np.float32(MA))
    return rgb, depth


def _random_lut(seed=3):
    return np.random.default_rng(seed).integers(0, 256, (256, 3)).astype(np.uint8)


def _guarded(shape, k=3):
    """A (k, *shape) uint8 view GUARD bytes inside a buffer filled with a pattern: (buffer, frames, the pattern's copy)."""
    n = int(np.prod(shape))
    buf = (torch.arange(2 * GUARD + k * n, dtype=torch.int64) * 37 % 251).to(torch.uint8).to(DEV)
    return buf, buf[GUARD:GUARD + k * n].view(k, *shape), buf.clone()


def _write_and_check(rgb, depth, minmax, lut, crop):
    """ops.frame_u8 into frame 1 of 3 (an odd base address for odd sizes) == the numpy lines; nothing else in the buffer changes."""
    from mvsnerf_amd import ops
    want = np_frame(rgb, depth, minmax, ops.jet_lut("cpu").numpy() if lut is None else lut, crop)
    buf, frames, before = _guarded(want.shape)
    out = ops.frame_u8(torch.from_numpy(rgb).to(DEV), None if depth is None else torch.from_numpy(depth).to(DEV), minmax=minmax,
                       lut=None if lut is None else torch.from_numpy(lut), crop=crop, out=frames[1])
    assert out.data_ptr() == frames[1].data_ptr() and out.dtype == torch.uint8 and tuple(out.shape) == want.shape
    got = frames[1].cpu().numpy()
    assert np.array_equal(got, want), (int((got != want).sum()), want.shape)
    n = want.size
    after = buf.cpu()
    assert torch.equal(after[:GUARD + n], before.cpu()[:GUARD + n]) and torch.equal(after[GUARD + 2 * n:], before.cpu()[GUARD + 2 * n:])      # guards, frames 0 and 2
    fresh = ops.frame_u8(torch.from_numpy(rgb).to(DEV), None if depth is None else torch.from_numpy(depth).to(DEV), minmax=minmax,
                         lut=None if lut is None else torch.from_numpy(lut).to(DEV), crop=crop)
    assert np.array_equal(fresh.cpu().numpy(), want)                # out=None allocates the same frame


# ------------------------------------------------------------------ the writer against the numpy lines
@pytest.mark.parametrize("table", ["random", "default"])
@pytest.mark.parametrize("depth_panel", [True, False])
@pytest.mark.parametrize("hw,crop", SHAPES)
def test_writer_equals_the_numpy_lines(hw, crop, depth_panel, table):
    rgb, depth = _inputs(*hw, seed=hw[0] * 1000 + hw[1])
    lut = _random_lut() if table == "random" else None
    _write_and_check(rgb, depth if depth_panel else None, (MI, MA), lut, crop)


@pytest.mark.parametrize("hw,crop", SHAPES)
def test_writer_with_the_range_from_the_device(hw, crop):
    """minmax=None: min of the positive depths and max, on the device (every depth strictly positive: numpy's cast is defined)."""
    from mvsnerf_amd import ops
    rgb, depth = _inputs(*hw, seed=7 + hw[1])
    depth = (depth * np.float32(0.37)).astype(np.float32)
    assert float(depth.min()) > 0
    _write_and_check(rgb, depth, None, _random_lut(5), crop)
    rng = ops.depth_range(torch.from_numpy(depth).to(DEV)).cpu().numpy()
    assert rng.tobytes() == np.array([depth.min(), depth.max()], dtype=np.float32).tobytes()


def test_every_table_boundary_and_its_neighbours():
    """Depths mi + (ma - mi) k / 255 and their float32 neighbours on both sides: only a correctly rounded subtract, divide and multiply gives numpy's
    index at every one of them."""
    k = np.arange(256, dtype=np.float64)
    mid = (MI + (MA - MI) * k / 255).astype(np.float32)
    row = np.concatenate([np.nextafter(mid, np.float32(-np.inf)), mid, np.nextafter(mid, np.float32(np.inf))]).astype(np.float32)
    depth = np.stack([row, row[::-1]])                                # (2, 768)
    idx = np_depth_panel(depth, (MI, MA), np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1))[0][..., 0]
    assert idx.min() == 0 and idx.max() == 255 and len(np.unique(idx)) == 256
    rgb = np.zeros(depth.shape + (3,), dtype=np.float32)
    _write_and_check(rgb, depth, (MI, MA), _random_lut(9), (0, 0))
    # the colour boundaries j / 255 and their neighbours, too
    c = (np.arange(256, dtype=np.float64) / 255).astype(np.float32)
    crow = np.concatenate([np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]).astype(np.float32)
    rgb = np.stack([crow, crow[::-1], np.roll(crow, 5)], -1)[None]    # (1, 768, 3)
    _write_and_check(rgb, None, None, None, (0, 0))


# ------------------------------------------------------------------ what is defined here
def test_out_of_range_and_non_finite_values():
    from mvsnerf_amd import ops
    nan, inf = float("nan"), float("inf")
    lut = _random_lut(11)
    depth = torch.tensor([[1.0, 5.0, nan, inf, -inf, MI, 3.325]])
    rgb = torch.tensor([[[nan, 0.5, 2.0], [inf, -inf, -0.0], [1.0, 0.999999, 1.0 / 255], [0.0] * 3, [0.0] * 3, [0.0] * 3, [0.25, 0.75, nan]]])
    out = ops.frame_u8(rgb.to(DEV), depth.to(DEV), minmax=(MI, MA), lut=torch.from_numpy(lut)).cpu().numpy()
    assert out.shape == (1, 14, 3)
    want_rgb = [[0, 127, 255], [255, 0, 0], [255, 254, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0], [63, 191, 0]]
    # below mi -> 0, above ma -> 255, NaN -> the byte of x0 = 0 (below mi: 0), +inf -> FLT_MAX -> 255, -inf -> 0, mi -> 0, the middle -> trunc(127.5)
    want_idx = [0, 255, 0, 255, 0, 0, 127]
    assert out[0, :7].tolist() == want_rgb
    assert out[0, 7:].tolist() == [lut[i].tolist() for i in want_idx]
    # a range given as a device tensor is the same range
    out2 = ops.frame_u8(rgb.to(DEV), depth.to(DEV), minmax=torch.tensor([MI, MA]).to(DEV), lut=torch.from_numpy(lut).to(DEV))
    assert np.array_equal(out2.cpu().numpy(), out)


def test_zeros_and_negatives_do_not_set_the_minimum():
    from mvsnerf_amd import ops, utils
    nan, inf = float("nan"), float("inf")
    depth = torch.tensor([[0.0, -1.0, 2.0, 4.0], [3.0, nan, 2.5, -inf]])
    assert ops.depth_range(depth.to(DEV)).cpu().tolist() == [2.0, 4.0]
    want_idx = np.array([[0, 0, 0, 255], [127, 0, 63, 0]])
    lut = _random_lut(13)
    img, mm = utils.visualize_depth_numpy(depth.numpy(), cmap=lut)
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (2, 4, 3) and np.array_equal(img, lut[want_idx])
    assert [type(v) for v in mm] == [np.float32, np.float32] and mm == [2.0, 4.0]
    jet = ops.jet_lut("cpu").numpy()
    for d in (depth, depth.to(DEV), depth.numpy()):                       # a tensor anywhere, or an array
        t, mm = utils.visualize_depth(d)
        assert torch.is_tensor(t) and t.dtype == torch.float32 and t.device.type == "cpu" and t.shape == (3, 2, 4) and mm == [2.0, 4.0]
        assert torch.equal(t, torch.from_numpy(jet[want_idx]).permute(2, 0, 1).float() / 255)
    img, mm = utils.visualize_depth_numpy(depth, (MI, MA))
    assert mm == [MI, MA] and np.array_equal(img, jet[np.array([[0, 0, 0, 199], [92, 0, 39, 0]])])      # trunc(255 (x - 2.125) / 2.4)


@pytest.mark.parametrize("fn", ["visualize_depth", "visualize_depth_numpy"])
def test_no_positive_depth_raises(fn):
    from mvsnerf_amd import ops, utils
    depth = np.array([[0.0, -2.0], [np.nan, -np.inf]], dtype=np.float32)
    rng = ops.depth_range(torch.from_numpy(depth).to(DEV)).cpu()
    assert float(rng[0]) == float("inf") and float(rng[1]) == 0.0
    with pytest.raises(ValueError, match="positive"):
        getattr(utils, fn)(depth)
    img, _ = getattr(utils, fn)(depth, (MI, MA))                         # with a range given there is nothing to take a minimum of
    assert tuple(img.shape) in ((2, 2, 3), (3, 2, 2))


@pytest.mark.parametrize("n", [1, 63, 40 * 64, 512 * 640 + 1])
def test_depth_range_is_numpys(n):
    from mvsnerf_amd import ops
    g = np.random.default_rng(n)
    x = g.normal(1.0, 2.0, (n,)).astype(np.float32)
    if n == 1:
        x = np.abs(x) + np.float32(0.1)
    else:
        x[g.integers(0, n, 5)] = [np.nan, np.inf, -np.inf, 0.0, -0.0][:5]
        x[0] = np.float32(0.5)                                           # at least one positive element
    x0 = np.nan_to_num(x)
    want = np.array([np.min(x0[x0 > 0]), np.max(x0)], dtype=np.float32)
    d = torch.from_numpy(x).to(DEV)
    a, b = ops.depth_range(d), ops.depth_range(d)
    assert a.shape == (2,) and a.dtype == torch.float32 and a.is_cuda
    assert a.cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))         # two runs: the same bits
    if n > 63:
        assert torch.equal(ops.depth_range(d.view(-1, 64) if n % 64 == 0 else d.view(1, -1)).view(torch.int32), a.view(torch.int32))


# ------------------------------------------------------------------ render_path is the per-frame sequence
def _path_of(c2ws, n_views=3):
    from mvsnerf_amd import utils
    return utils.gen_render_path(c2ws.cpu().numpy().astype(np.float64), N_views=n_views)


@pytest.fixture(scope="module")
def mvs_scene():
    from mvsnerf_amd import train
    from tests.util import load_weights
    H, W = 24, 32
    args = train.default_args(pad=4, batch_size=64, N_samples=8, chunk=256)
    sys_ = train.MVSSystem(args, n_depth_planes=16)
    sys_.render_kwargs_train["network_fn"].load_state_dict(load_weights()[0])
    sys_ = sys_.to(DEV)
    batch = train.synthetic_batch(H, W, seed=5, smooth=True)
    # a frame this small has no encode: the volume is handed in, as tests/test_gpu_mlp_wide.py::test_render_view_is_the_per_chunk_loop does
    vol = torch.randn((1, 8, 16, 24, 32), generator=torch.Generator().manual_seed(7)).to(DEV)
    poses = _path_of(batch["c2ws"][0, :3])
    assert poses.shape == (3, 4, 4)
    return sys_, batch, vol, poses


@pytest.mark.parametrize("crop", [False, True])
@pytest.mark.parametrize("depth_panel", [True, False])
def test_render_path_is_render_view_then_the_writer(mvs_scene, depth_panel, crop):
    from mvsnerf_amd import ops
    sys_, batch, vol, poses = mvs_scene
    H, W = 24, 32
    frames = sys_.render_path(batch, poses, depth_panel=depth_panel, crop=crop, volume=vol)
    ch, cw = (H // 20, W // 20) if crop else (0, 0)
    assert frames.dtype == torch.uint8 and frames.is_cuda and frames.shape == (3, H - 2 * ch, (W - 2 * cw) * (2 if depth_panel else 1), 3)
    _, pose_ref = sys_.decode_batch(dict(batch))
    nf_src = pose_ref["near_fars"][0]
    for k in range(3):
        rgb, depth = sys_.render_view(batch, volume=vol, target=dict(hw=(H, W), intrinsic=pose_ref["intrinsics"][-1],
                                                                     c2w=torch.from_numpy(poses[k]).float(), near_far=pose_ref["near_fars"][-1]))
        want = ops.frame_u8(rgb, depth if depth_panel else None, minmax=nf_src, crop=(ch, cw))
        assert torch.equal(frames[k], want), k
    assert len({bytes(f.cpu().numpy().tobytes()) for f in frames}) == 3          # three poses, three different frames
    if depth_panel and not crop:
        again = sys_.render_path(batch, poses, volume=vol, minmax=(float(nf_src[0]), float(nf_src[1])), cmap=ops.jet_lut("cpu").numpy(),
                                 hw=(H, W), intrinsic=pose_ref["intrinsics"][-1], near_far=pose_ref["near_fars"][-1])
        assert torch.equal(again, frames)                                        # the defaults, spelled out


def _rays_of(train, H, W, focal, c2w, near_far):
    ro, rd = train.get_rays(train.get_ray_directions(H, W, focal).to(DEV), torch.as_tensor(c2w).float().to(DEV))
    nf = near_far.to(DEV).float()
    return torch.cat([ro, rd, nf[0] * torch.ones_like(ro[:, :1]), nf[1] * torch.ones_like(ro[:, :1])], 1)


def test_finetune_render_path_is_render_rays_then_the_writer(tmp_path):
    from mvsnerf_amd import ops, train, utils
    from tests.test_gpu_finetune_render import _system
    ft, rig, pose = _system(V=3)
    H, W = 20, 28
    focal = [float(pose["intrinsics"][0, 0, 0]) * W / 96, float(pose["intrinsics"][0, 1, 1]) * H / 64]
    poses = _path_of(pose["c2ws"][:3])
    for depth_panel, crop in ((True, False), (False, True), (True, (2, 3))):
        frames = ft.render_path(poses, (H, W), focal, depth_panel=depth_panel, crop=crop)
        cr = (H // 20, W // 20) if crop is True else (crop or (0, 0))
        assert frames.shape == (3, H - 2 * cr[0], (W - 2 * cr[1]) * (2 if depth_panel else 1), 3) and frames.dtype == torch.uint8
        for k in range(3):
            rgb, depth = ft.render_rays(_rays_of(train, H, W, focal, poses[k], ft.near_far_source))
            want = ops.frame_u8(rgb.reshape(H, W, 3), depth.reshape(H, W) if depth_panel else None, minmax=ft.near_far_source, crop=cr)
            assert torch.equal(frames[k], want), (depth_panel, crop, k)
    # save_frames: PIL reads the bytes back
    from PIL import Image
    paths = utils.save_frames(frames, str(tmp_path / "video"), prefix="ft_")
    assert [os.path.basename(p) for p in paths] == ["ft_0000.png", "ft_0001.png", "ft_0002.png"]
    for p, f in zip(paths, frames.cpu().numpy()):
        assert np.array_equal(np.asarray(Image.open(p)), f)
    assert [os.path.basename(p) for p in utils.save_frames(frames.cpu().numpy()[:1], str(tmp_path / "video"))] == ["0000.png"]


def test_fusion_render_path_is_render_rays_then_the_writer():
    from mvsnerf_amd import ops, train
    from tests.test_gpu_fusion import fusion_system, fusion_views
    views, bbox, img_wh, focal = fusion_views()
    sysm, _ = fusion_system(views, bbox, img_wh, focal)
    H, W = 16, 24
    f4 = [f / 4.0 for f in focal]
    poses = np.stack([np.asarray(views[i][4], dtype=np.float64) for i in (0, 2)])
    nf = views[0][2]
    for depth_panel, crop in ((True, False), (False, (1, 2))):
        frames = sysm.render_path(poses, (H, W), f4, depth_panel=depth_panel, crop=crop)
        cr = crop or (0, 0)
        assert frames.shape == (2, H - 2 * cr[0], (W - 2 * cr[1]) * (2 if depth_panel else 1), 3)
        for k in range(2):
            rgb, depth = sysm.render_rays(_rays_of(train, H, W, f4, poses[k], nf))
            want = ops.frame_u8(rgb.reshape(H, W, 3), depth.reshape(H, W) if depth_panel else None, minmax=nf.to(DEV), crop=cr)
            assert torch.equal(frames[k], want), (depth_panel, crop, k)
