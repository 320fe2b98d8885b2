"""Empty-space skipping on the GPU (csrc/sparse.hip, ops.live_samples / expand_rows / raymarch_sparse, MVSSystemFinetune.render_rays(skip_empty=)).

The yardstick is torch.equal throughout: the predicate and the compaction are integer work on fp32 index arithmetic that torch restates exactly
(tests/sparse_refs.py), and a live sample's MLP column has the bits of the dense sequence.  Only the guarded fp16x3 mode ("auto") is compared through
its error against the fp32 kernel, next to the dense "auto" run's own error."""
import functools

import pytest
import torch

from tests import sparse_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------ A. live_samples against the oracle
@functools.lru_cache(maxsize=None)
def _live_case(grid, N, S):
    """Inputs on the CPU, computed once per (grid, shape) and shared; nobody writes to them."""
    g = torch.Generator().manual_seed(N * 1000 + S + grid[0])
    density = R.sparse_density(grid, g, nan_voxel=True)
    return density, R.coords(N, S, grid, g), torch.randn((N, S, 3), generator=g), torch.randn((N, 3), generator=g)


def _run_live(density, ndc, thr, pts, dirs):
    from mvsnerf_amd import ops
    d = lambda t: None if t is None else t.to(DEV)
    with torch.no_grad():
        out = ops.live_samples(d(density), d(ndc), thr, d(pts), d(dirs))
    torch.cuda.synchronize()
    return out


def _check_live(density, ndc, thr, pts, dirs):
    n, idx, ndc_c, pts_c, dir_c = R.live_samples(density, ndc, thr, pts, dirs)
    runs = [_run_live(density, ndc, thr, pts, dirs) for _ in range(2)]
    for count, gidx, *rows in runs:
        assert count.dtype == torch.int32 and gidx.dtype == torch.int32 and int(count.item()) == n, (int(count.item()), n)
        assert torch.equal(gidx[:n].cpu(), idx)
        for got, want in zip(rows, (ndc_c, pts_c, dir_c)):
            if want is None:
                assert got is None
            else:                                                  # bytes, so that NaN coordinates compare too
                assert torch.equal(got[:n].cpu().view(torch.int32), want.contiguous().view(torch.int32))
    a, b = runs
    assert torch.equal(a[1][:n], b[1][:n])
    assert all(torch.equal(x[:n].view(torch.int32), y[:n].view(torch.int32)) for x, y in zip(a[2:], b[2:]) if x is not None)
    return n


@pytest.mark.parametrize("thr", [-1.0, 0.0, 0.5, "max"])
@pytest.mark.parametrize("N,S", [(1, 1), (37, 24), (300, 128)])
@pytest.mark.parametrize("grid", R.GRIDS)
def test_live_samples_equals_the_oracle(grid, N, S, thr):
    density, ndc, pts, dirs = _live_case(grid, N, S)
    t = float(torch.nan_to_num(density, nan=0.0).max()) if thr == "max" else thr
    n = _check_live(density, ndc, t, pts, dirs)
    print(f"grid {grid} (N,S)=({N},{S}) thr {t:.3g}: {n} of {N * S} live")
    if N * S > 100 and thr in (0.0, 0.5):
        assert 0 < n < N * S                                       # a mixed case


def test_live_samples_all_none_and_optional_rows():
    grid = R.GRIDS[0]
    density, ndc, pts, dirs = _live_case(grid, 37, 24)
    clean, inside = torch.nan_to_num(density, nan=0.25), torch.nan_to_num(ndc, nan=0.5, posinf=0.5, neginf=0.5).clamp(0, 1)
    assert _check_live(clean, inside, -1.0, pts, dirs) == 37 * 24                   # every sample live
    assert _check_live(clean, inside, float(clean.max()), pts, dirs) == 0            # none
    assert _check_live(density, ndc, 0.5, None, dirs) > 0                            # a colour volume takes no world points
    assert _check_live(density, ndc, 0.5, None, None) > 0


def test_live_samples_scan_runs_longer_than_one():
    """2100 x 128 samples are 263 workgroup counts: the 256 threads of the scan own runs of two."""
    density, ndc, pts, dirs = _live_case(R.GRIDS[0], 2100, 128)
    n = _check_live(density, ndc, 0.5, pts, dirs)
    assert 0 < n < 2100 * 128


# ------------------------------------------------------------------ B. expand_rows
@pytest.mark.parametrize("C", [1, 4])
def test_expand_rows_writes_every_row(C):
    from mvsnerf_amd import ops
    P = 2500                                                       # three tiles of 1024 rows, the last one partial
    g = torch.Generator().manual_seed(C)
    mixed = torch.sort(torch.randperm(P, generator=g)[:777])[0]
    cases = [(torch.empty(0, dtype=torch.int64), 0), (torch.tensor([1500]), 1), (torch.arange(P), P), (mixed, 777),
             (mixed, 300)]                                          # count below the rows handed in: the device count decides
    for idx64, count in cases:
        n = idx64.numel()
        src = torch.randn((n, C), generator=g)
        want = R.expand_rows(src, idx64.to(torch.int32), count, P)
        dst = torch.full((P, C), float("nan"), device=DEV)
        with torch.no_grad():
            got = ops.expand_rows(src.to(DEV), idx64.to(torch.int32).to(DEV), torch.tensor([count], dtype=torch.int32).to(DEV), P, out=dst)
        assert got is dst and torch.equal(dst.cpu(), want), (C, n, count)
        with torch.no_grad():
            fresh = ops.expand_rows(src.to(DEV), idx64.to(torch.int32).to(DEV), torch.tensor([count], dtype=torch.int32).to(DEV), P)
        assert torch.equal(fresh.cpu(), want)


# ------------------------------------------------------------------ C / D. raymarch_sparse against the dense sequence
GRID = (16, 24, 32)


@functools.lru_cache(maxsize=None)
def _rays(N, S):
    from tests.test_gpu_raymarch_onelaunch import _inputs, _hwdc
    x = _inputs(N, S, seed=S)
    x["vol_cl"] = _hwdc(x["vol"])
    x["cvol_cl"] = torch.randn((*GRID, 20), generator=torch.Generator().manual_seed(S)).to(DEV)
    return x


def _band(lo=4, hi=9):
    d = torch.zeros(GRID)
    d[lo:hi] = 1.0
    return d


@functools.lru_cache(maxsize=None)
def _net(kind):
    """(packed, model | None): the shipped v0 checkpoint, a seeded v2 network, the netwidth-256 weights of tests/wide_refs.py (all F = 20)."""
    from mvsnerf_amd import models, ops
    from tests.util import load_weights
    if kind == "wide":
        from tests import wide_refs
        ws, bs = wide_refs.weights(20)
        return ops.mlp_pack_wide([w.to(DEV) for w in ws], [b.to(DEV) for b in bs], 20, wide_refs.WIDE, 0), None
    m = models.MVSNeRF(D=6, W=128, input_ch_pts=63, input_ch_views=3, input_ch_feat=20, skips=[4], net_type=kind)
    if kind == "v0":
        m.load_state_dict(load_weights()[0])
    else:
        torch.manual_seed(20)
        for p in m.parameters():
            torch.nn.init.uniform_(p, -0.15, 0.15)
    m = m.to(DEV)
    with ops.mlp_precision("fp32"):
        return m.packed(20), m


def _dense(x, packed, density, thr, white, colour, **alt):
    """gather -> mlp_forward over all N*S samples -> the dead rows zeroed -> composite.  Returns the outputs, the untouched raw and the live mask."""
    from mvsnerf_amd import ops
    N, S = x["z"].shape
    if colour:
        feat, dirs = ops.gather_colorvol(x["cvol_cl"], x["ndc"], x["dirs"], x["w2cs"][0].contiguous())
    else:
        feat, dirs = ops.gather(x["vol_cl"], x["imgs"], x["w2cs"], x["Ks"], x["pts"], x["ndc"], x["dirs"])
    full = ops.mlp_forward(packed, 20, x["ndc"].data_ptr(), 3, feat.data_ptr(), 20, dirs.data_ptr(), 3, N, S, 0, x["ndc"].device, **alt).view(N, S, 4)
    live = R.live_mask(density, x["ndc"].cpu(), thr).to(DEV).view(N, S)
    raw = torch.where(live[..., None], full, torch.zeros_like(full))
    rgb, disp, acc, weights, depth, alpha = ops.composite(raw, x["z"], white)
    return {"raw": raw, "rgb_map": rgb, "disp": disp, "acc": acc, "weights": weights, "depth": depth, "alpha": alpha}, full, live


def _sparse(x, packed, density, thr, white, colour, **alt):
    from mvsnerf_amd import ops
    vol = x["cvol_cl"] if colour else x["vol_cl"]
    return ops.raymarch_sparse(vol, None if colour else x["imgs"], x["w2cs"], None if colour else x["Ks"], packed, x["pts"], x["ndc"], x["z"], x["dirs"],
                               density.to(DEV), thr, white_bkgd=white, want=("disp", "acc"), **alt)


def _check_fp32(x, kind, density, thr, white=False, colour=False):
    from mvsnerf_amd import ops
    packed, _ = _net(kind)
    with torch.no_grad(), ops.mlp_precision("fp32"):
        got = _sparse(x, packed, density, thr, white, colour)
        ref, _, live = _dense(x, packed, density, thr, white, colour)
    torch.cuda.synchronize()
    assert got["n_live"] == int(live.sum())
    for k in ("raw", "rgb_map", "weights", "depth", "alpha", "disp", "acc"):
        assert got[k].shape == ref[k].shape, k
        assert torch.equal(got[k], ref[k]), (k, float((got[k] - ref[k]).abs().max()))
    return got["n_live"]


SHAPES = [(37, 24), (20, 128)]


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("N,S", SHAPES)
def test_raymarch_sparse_v0_equals_the_dense_sequence(N, S, white):
    n = _check_fp32(_rays(N, S), "v0", _band(), 0.0, white=white)
    assert 0 < n < N * S


@pytest.mark.parametrize("N,S", SHAPES)
@pytest.mark.parametrize("kind", ["v2", "wide"])
def test_raymarch_sparse_other_networks(kind, N, S):
    n = _check_fp32(_rays(N, S), kind, _band(), 0.0)
    assert 0 < n < N * S


@pytest.mark.parametrize("N,S", SHAPES)
def test_raymarch_sparse_colour_volume(N, S):
    n = _check_fp32(_rays(N, S), "v0", _band(), 0.0, colour=True)
    assert 0 < n < N * S


def test_raymarch_sparse_live_counts_none_all_and_ragged():
    N, S = 37, 24
    x = _rays(N, S)
    assert _check_fp32(x, "v0", torch.zeros(GRID), 0.0) == 0                        # nothing live: no gather, no MLP launch
    inside = dict(x, ndc=x["ndc"].clamp(0, 1).contiguous())
    assert _check_fp32(inside, "v0", torch.ones(GRID), 0.0) == N * S                # everything live
    n = _check_fp32(x, "v0", _band(3, 8), 0.0, white=True)
    assert n % 128 != 0 and 0 < n < N * S                                           # the last MLP tile is partial


@pytest.mark.parametrize("N,S", SHAPES)
def test_raymarch_sparse_auto_mode_error_is_the_dense_error(N, S):
    """The guarded fp16x3 sequence scales a tile's operands by exact powers of two, so regrouping the samples into other tiles changes no
    product's rounding: the expected ratio of the two errors is 1; 1.25 is the margin tests/test_gpu_mlp_fold.py gives one re-associated chain."""
    from mvsnerf_amd import ops
    x, density = _rays(N, S), _band()
    packed, m = _net("v0")
    with torch.no_grad():
        with ops.mlp_precision("fp32"):
            _, full32, live = _dense(x, packed, density, 0.0, False, False)
        with ops.mlp_precision("auto"):
            n0 = ops.guard_fallbacks()
            alt = m.packed_alt(20)
            assert "guard" in alt
            sparse = _sparse(x, m.packed(20), density, 0.0, False, False, **alt)
            _, full_auto, _ = _dense(x, m.packed(20), density, 0.0, False, False, **alt)
            assert ops.guard_fallbacks() == n0
    assert bool(live.any()) and not bool(sparse["raw"][~live].any())
    e_sparse = float((sparse["raw"][live] - full32[live]).abs().max())
    e_dense = float((full_auto[live] - full32[live]).abs().max())
    print(f"(N,S)=({N},{S}) auto vs fp32 over {int(live.sum())} live rows: e_sparse {e_sparse:.3g}, e_dense {e_dense:.3g}")
    assert e_sparse <= 1.25 * e_dense


# ------------------------------------------------------------------ E. the system (64 x 96 source views, 16 planes, 32 samples, pad 4)
def _loop(ft, rays, thr, B, u=None):
    """render_rays(skip_empty=thr) spelled out: per sub-batch of B rays ray_marcher -> ray_points -> [ray_marcher_fine] -> the dense sequence with the
    oracle's dead rows zeroed.  Returns rgb, depth and the oracle's live fraction."""
    from mvsnerf_amd import ops, train
    a = ft.args
    H, W = ft.imgs.shape[-2:]
    V = ft.imgs.shape[1]
    w2c, K = ft.pose_source["w2cs"][0], ft.pose_source["intrinsics"][0]
    vol_cl = ops.channels_last_volume(ft.volume.feat_volume)
    net = ft.network_fn
    white = bool(getattr(a, "white_bkgd", False))
    rays = rays.to(DEV)
    rgbs, depths, live_n, total = [], [], 0, 0
    for i in range(0, rays.shape[0], B):
        r = rays[i:i + B]
        _, ro, rd, z = train.ray_marcher(r, N_samples=a.N_samples)
        pts, ndc = ops.ray_points(ro, rd, z, w2c, K, ft.near_far_source, ref_hw=(H, W), pad=a.pad)
        if u is not None:
            z = ops.ray_marcher_fine_z(ft.density_volume, ndc, z.contiguous(), u[i:i + B].to(DEV).contiguous())
            pts, ndc = ops.ray_points(ro, rd, z, w2c, K, ft.near_far_source, ref_hw=(H, W), pad=a.pad)
        N, S = z.shape
        if vol_cl.shape[-1] == 8:
            feat, dirs = ops.gather(vol_cl, ft.imgs[0].contiguous(), ft.pose_source["w2cs"][:V].contiguous(), ft.pose_source["intrinsics"][:V].contiguous(),
                                    pts, ndc, rd.contiguous())
        else:
            feat, dirs = ops.gather_colorvol(vol_cl, ndc, rd.contiguous(), w2c.contiguous())
        F = a.feat_dim
        full = ops.mlp_forward(net.packed(F), F, ndc.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, N, S, 0, ndc.device, **net.packed_alt(F)).view(N, S, 4)
        live = R.live_mask(ft.density_volume.cpu(), ndc.cpu(), thr).to(DEV).view(N, S)
        raw = torch.where(live[..., None], full, torch.zeros_like(full))
        rgb, _, _, _, depth, _ = ops.composite(raw, z.contiguous(), white)
        rgbs.append(rgb)
        depths.append(depth)
        live_n += int(live.sum())
        total += N * S
    return torch.cat(rgbs), torch.cat(depths), live_n / total


def _check_system(ft, rays, thr, u=None):
    from mvsnerf_amd import ops
    with torch.no_grad(), ops.mlp_precision("fp32"):
        rgb, depth = ft.render_rays(rays, skip_empty=thr, batch_rays=1000, u=u)
        frac = ft.last_live_fraction
        want_rgb, want_depth, want_frac = _loop(ft, rays, thr, 1000, u=u)
        dense_rgb, _ = ft.render_rays(rays, u=u)
    assert rgb.shape == (rays.shape[0], 3) and depth.shape == (rays.shape[0],)
    assert torch.equal(rgb, want_rgb) and torch.equal(depth, want_depth)
    assert frac == want_frac
    print(f"live fraction {frac:.4f} at thr {thr:.4g}; max |rgb - dense rgb| {float((rgb - dense_rgb).abs().max()):.3g}")
    return frac


@pytest.fixture(scope="module")
def plain_system():
    from tests.test_gpu_finetune_render import _system
    ft, _, pose = _system(V=3)                                                       # built WITHOUT use_density_volume
    assert ft.density_volume is None and getattr(ft, "vox_pts", None) is None
    ft.update_density_volume()
    assert tuple(ft.density_volume.shape) == tuple(ft.volume.feat_volume.shape[-3:]) and bool(torch.isfinite(ft.density_volume).all())
    return ft, pose


def test_render_rays_skip_empty_equals_the_loop(plain_system):
    from tests.test_gpu_finetune_render import _rays as scene_rays
    ft, _ = plain_system
    learnt = ft.density_volume
    rays = scene_rays(2500)
    try:
        thr = float(learnt[learnt > 0].median()) if bool((learnt > 0).any()) else 0.0
        f = _check_system(ft, rays, thr)                                             # the volume of update_density_volume()
        assert 0.0 <= f <= 1.0
        band = torch.zeros_like(learnt)
        band[4:9] = 1.0
        ft.density_volume = band
        f = _check_system(ft, rays, 0.0)                                             # planes [4, 9) occupied
        assert 0.0 < f < 1.0
    finally:
        ft.density_volume = learnt


def test_render_rays_skip_empty_with_importance_sampling():
    from tests.test_gpu_finetune_render import _system, _rays as scene_rays
    ft, _, _ = _system(V=3, N_importance=16)
    ft.update_density_volume()
    band = torch.zeros_like(ft.density_volume)
    band[4:9] = 1.0
    ft.density_volume = band
    u = torch.rand((1500, 16), generator=torch.Generator().manual_seed(5))
    f = _check_system(ft, scene_rays(1500, seed=3), 0.0, u=u)
    assert 0.0 < f < 1.0


def test_render_path_forwards_skip_empty(plain_system):
    from mvsnerf_amd import ops, train
    from tests.test_gpu_frames import _path_of, _rays_of
    ft, pose = plain_system
    learnt = ft.density_volume
    band = torch.zeros_like(learnt)
    band[4:9] = 1.0
    H, W = 20, 28
    focal = [float(pose["intrinsics"][0, 0, 0]) * W / 96, float(pose["intrinsics"][0, 1, 1]) * H / 64]
    poses = _path_of(pose["c2ws"][:3])
    try:
        ft.density_volume = band
        with ops.mlp_precision("fp32"):
            frames = ft.render_path(poses, (H, W), focal, skip_empty=0.0)
            dense = ft.render_path(poses, (H, W), focal)
            for k in range(3):
                rgb, depth = ft.render_rays(_rays_of(train, H, W, focal, poses[k], ft.near_far_source), skip_empty=0.0)
                want = ops.frame_u8(rgb.reshape(H, W, 3), depth.reshape(H, W), minmax=ft.near_far_source)
                assert torch.equal(frames[k], want), k
        assert frames.shape == dense.shape and 0.0 < ft.last_live_fraction < 1.0    # the switch arrived: the last frame skipped samples
    finally:
        ft.density_volume = learnt


def test_update_density_volume_on_a_colour_volume():
    """A colour volume's feature rows are its own 8 + 4V channels: the same rows as [8 volume channels | the projected colours]."""
    from mvsnerf_amd import ops
    from mvsnerf_amd.renderer import render_density
    from tests.test_gpu_finetune_render import _system, _rays as scene_rays
    ft, _, _ = _system(V=3, use_color_volume=True)
    assert ft.density_volume is None and ft.volume.feat_volume.shape[1] == 20
    ft.update_density_volume()
    Dv, Hv, Wv = ft.volume.feat_volume.shape[-3:]
    assert tuple(ft.density_volume.shape) == (Dv, Hv, Wv)
    with torch.no_grad():
        vol_cl = ops.channels_last_volume(ft.volume.feat_volume.detach())
        feats = torch.cat((vol_cl[..., :8].reshape(Dv * Hv, Wv, 8), ft.color_feature), -1)
        want = render_density(ft.network_fn, ft.vox_pts, feats, ft.render_kwargs_train["network_query_fn"]).reshape(Dv, Hv, Wv)
    assert torch.equal(ft.density_volume, want)
    band = torch.zeros_like(ft.density_volume)
    band[4:9] = 1.0
    ft.density_volume = band
    f = _check_system(ft, scene_rays(1200, seed=4), 0.0)
    assert 0.0 < f < 1.0
