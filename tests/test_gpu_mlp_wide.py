"""The netwidth-256 fp32 MLP kernel (mvsnerf_mlp_fwd_wide, csrc/mlp_wide.hip, csrc/mlp_wide_layout.h) and its wiring, v0 and v2.

References and weights: tests/wide_refs.py (the fp32 restatement is pinned to the real reference by tests/test_wide_refs.py on the CPU).
Shapes (N, S): (1, 1) one point, (5, 7) a partial wave, (4, 32) exactly one 128-point tile, (37, 24) seven tiles with a partial last one.
F = 12 / 20 / 36 / 40: 8 / 12 / 20 / 20 feature k-steps.

A  neutral bias: v2 with pts_bias = (0, 0) and v0 with pts_bias = (0, 1) on otherwise equal weights are the same function; the kernel returns
   the same bits for both (full forward, relu(sigma-only)), and the network is not dead.
B  sigma-only: relu(sigma-only) is the full forward's sigma bit for bit; v2's sigma-only output is negative wherever float64 is negative by more
   than the kernel's own measured sigma error; v0's is clamped.
C  accuracy on (37, 24), rgb and sigma separately: r = mean|kernel - f64| / mean|torch fp32 CPU - f64|; r_256 of the wide kernel on the wide
   network against r_128 of the 128-wide fp32 kernel ("fp32" mode) on a 128-wide network of the same recipe (a = 0.15), same run:
   r_256 <= 2 x 1.25 x r_128 (1.25: the margin tests/test_gpu_mlp_fold.py gives one re-associated chain; 2: the worst-case growth of a
   sequential fp32 chain's rounding error when its length doubles).  A wrong index or a missing k-step is off by orders of magnitude.
D  MVSNeRF.forward(x) / forward_alpha(x) on the concatenated rows equal query() with per-ray directions bit for bit.
E  no stray writes: 128 sentinel rows behind raw are untouched.
F  wiring: renderer.rendering() = dir_feature -> gen_pts_feats -> mlp_forward -> composite bit for bit; rendering_batched = rendering() per batch;
   run_network_mvs and render_density return the kernel's values; MVSSystem.render_view = the per-chunk loop.
G  refusals before any launch, and "auto" runs the wide kernel without touching the guard.
"""
import ctypes
import functools

import pytest
import torch

from tests import wide_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NETS = list(R.VARIANTS)
CASES = [(N, S, F) for (N, S) in R.SHAPES for F in R.FS]


# ------------------------------------------------------------------ the kernels
def _pack(ws, bs, F, variant, W=R.WIDE):
    from mvsnerf_amd import ops
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    packed = ops.mlp_pack_wide(wd, bd, F, W, variant) if W == R.WIDE else ops.mlp_pack(wd, bd, F, variant=variant)
    torch.cuda.synchronize()
    return packed


def _fwd(packed, F, x, alpha_only=0):
    from mvsnerf_amd import ops
    ndc, feat, dirs = x
    N, S = ndc.shape[:2]
    raw = ops.mlp_forward(packed, F, ndc.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, N, S, alpha_only, ndc.device)
    torch.cuda.synchronize()
    return raw


@functools.lru_cache(maxsize=None)
def _case(N, S, F, net_type):
    """the wide kernel's two outputs on one case, computed once and shared (with the CPU references of wide_refs.reference)"""
    ref = R.reference(N, S, F, net_type)
    x = tuple(t.to(DEV) for t in ref["x"])
    packed = _pack(*ref["w"], F, R.VARIANTS[net_type])
    return dict(ref=ref, x=x, packed=packed, raw=_fwd(packed, F, x), alpha=_fwd(packed, F, x, alpha_only=1))


def _state_dict(ws, bs):
    from mvsnerf_amd import ops
    sd = {}
    for name, w, b in zip(ops.MLP_ORDER, ws, bs):
        sd[f"nerf.{name}.weight"], sd[f"nerf.{name}.bias"] = w.clone(), b.clone()
    return sd


def _args(net_type, F=20, **kw):
    import types
    d = dict(feat_dim=F, img_downscale=1.0, use_color_volume=False, net_type=net_type, multires=10, i_embed=0, pts_dim=3,
             multires_views=4, dir_dim=3, netdepth=6, netwidth=R.WIDE, N_importance=0, netchunk=1024, ckpt=None, perturb=1.0,
             N_samples=32, use_viewdirs=True, white_bkgd=False, raw_noise_std=0.0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _network(net_type, F=20):
    """(args, network_fn on the GPU with wide_refs.weights(F), network_query_fn) as create_nerf_mvs builds them at netwidth 256"""
    from mvsnerf_amd import models
    args = _args(net_type, F)
    kw, _, _, _ = models.create_nerf_mvs(args, use_mvs=False, dir_embedder=False, pts_embedder=True)
    kw["network_fn"].load_state_dict(_state_dict(*R.weights(F)))
    return args, kw["network_fn"].to(DEV), kw["network_query_fn"]


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("N,S,F", CASES)
def test_neutral_bias_v2_is_v0(N, S, F):
    ws, bs = R.weights(F)
    x = tuple(t.to(DEV) for t in R._inputs(N, S, F))
    zero = torch.zeros_like(ws[6])
    w0 = ws[:6] + [zero] + ws[7:]
    p_v2 = _pack(w0, bs[:6] + [torch.zeros_like(bs[6])] + bs[7:], F, 1)
    p_v0 = _pack(w0, bs[:6] + [torch.ones_like(bs[6])] + bs[7:], F, 0)
    raw2, raw0 = _fwd(p_v2, F, x), _fwd(p_v0, F, x)
    assert torch.equal(raw2, raw0)
    assert torch.equal(torch.relu(_fwd(p_v2, F, x, 1)), _fwd(p_v0, F, x, 1))
    if N * S >= 35:
        assert float(raw2[:, 3].max()) > 0 and float(raw2[:, :3].std()) > 0          # not a dead network


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("net_type", NETS)
@pytest.mark.parametrize("N,S,F", CASES)
def test_sigma_only(N, S, F, net_type):
    c = _case(N, S, F, net_type)
    raw, alpha = c["raw"], c["alpha"]
    assert raw.shape == (N * S, 4) and alpha.shape == (N * S, 1)
    assert bool(torch.isfinite(raw).all()) and bool(torch.isfinite(alpha).all())
    assert torch.equal(torch.relu(alpha[:, 0]), raw[:, 3])
    a64 = c["ref"]["f64"][2].reshape(-1)                          # alpha_linear's output before any ReLU
    if net_type == "v2":
        err = float((alpha[:, 0].cpu().double() - a64).abs().max())
        neg = a64 < -err
        print(f"v2 ({N},{S}) F={F}: sigma-only max err {err:.2e}, float64 negative beyond it on {int(neg.sum())} of {N * S} points")
        assert bool((alpha[:, 0].cpu()[neg] < 0).all())
        if N * S >= 35:
            assert int(neg.sum()) > 0
    else:
        assert float(alpha.min()) >= 0.0
        assert torch.equal(alpha[:, 0], raw[:, 3])


# ------------------------------------------------------------------ C
def _ratios(got, f32, f64):
    """(r_rgb, r_sigma) of the docstring"""
    got, f32, f64 = got.cpu().double().reshape(-1, 4), f32.double().reshape(-1, 4), f64.reshape(-1, 4)
    e_k, e_t = (got - f64).abs(), (f32 - f64).abs()
    return float(e_k[:, :3].mean() / e_t[:, :3].mean()), float(e_k[:, 3].mean() / e_t[:, 3].mean())


@pytest.mark.parametrize("net_type", NETS)
@pytest.mark.parametrize("F", R.FS)
def test_accuracy_against_float64_calibrated_on_the_128_wide_kernel(F, net_type):
    from mvsnerf_amd import ops
    N, S = 37, 24
    c = _case(N, S, F, net_type)
    r256 = _ratios(c["raw"], c["ref"]["f32"][0], c["ref"]["f64"][0])
    ref128 = R.reference(N, S, F, net_type, W=128)
    with ops.mlp_precision("fp32"):
        raw128 = _fwd(_pack(*ref128["w"], F, R.VARIANTS[net_type], W=128), F, c["x"])
    r128 = _ratios(raw128, ref128["f32"][0], ref128["f64"][0])
    print(f"{net_type} F={F}: r_256 rgb {r256[0]:.3f} sigma {r256[1]:.3f}; r_128 rgb {r128[0]:.3f} sigma {r128[1]:.3f}")
    assert r256[0] <= 2 * 1.25 * r128[0], (r256, r128)
    assert r256[1] <= 2 * 1.25 * r128[1], (r256, r128)


# ------------------------------------------------------------------ D
@pytest.mark.parametrize("net_type", NETS)
@pytest.mark.parametrize("N,S", R.SHAPES)
def test_row_path_is_the_per_ray_path(N, S, net_type):
    F = 20
    _, net, _ = _network(net_type, F)
    c = _case(N, S, F, net_type)
    ndc, feat, dirs = c["x"]
    x = R.rows(*c["ref"]["x"]).to(DEV)
    with torch.no_grad():
        raw_q = net.query(ndc, feat, dirs, N, S)
        sig_q = net.query(ndc, feat, None, N, S)
        raw_r = net(x)
        sig_r = net.forward_alpha(x[..., :63 + F])
    assert torch.equal(raw_q, c["raw"]) and torch.equal(sig_q, c["alpha"])
    assert raw_r.shape == (N, S, 4) and sig_r.shape == (N, S, 1)
    assert torch.equal(raw_r.reshape(-1, 4), raw_q) and torch.equal(sig_r.reshape(-1, 1), sig_q)


# ------------------------------------------------------------------ E
@pytest.mark.parametrize("alpha_only", [0, 1])
@pytest.mark.parametrize("N,S", R.SHAPES)
def test_no_stray_writes(N, S, alpha_only):
    from mvsnerf_amd import _lib, ops
    F, net_type = 20, "v2"
    c = _case(N, S, F, net_type)
    ndc, feat, dirs = c["x"]
    P, C = N * S, 1 if alpha_only else 4
    sentinel = -12345.0
    buf = torch.full((P + 128, C), sentinel, device=DEV)
    ops.check(_lib.lib().mvsnerf_mlp_fwd_wide(c["packed"].buffer.data_ptr(), F, R.WIDE, ndc.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3,
                                              N, S, alpha_only, buf.data_ptr(), ops.stream_ptr()), "mlp_fwd_wide")
    torch.cuda.synchronize()
    assert bool((buf[P:] == sentinel).all())
    assert torch.equal(buf[:P], c["alpha"] if alpha_only else c["raw"])


def test_entry_checks_its_arguments():
    from mvsnerf_amd import _lib, ops
    c = _case(5, 7, 20, "v0")
    ndc, feat, dirs = c["x"]
    raw = torch.zeros((35, 4), device=DEV)
    f = _lib.lib().mvsnerf_mlp_fwd_wide
    io = (ndc.data_ptr(), 3, feat.data_ptr(), 20, dirs.data_ptr(), 3, 5, 7, 0)
    assert f(c["packed"].buffer.data_ptr(), 20, 128, *io, raw.data_ptr(), ops.stream_ptr()) == -2
    assert f(c["packed"].buffer.data_ptr(), 21, 256, ndc.data_ptr(), 3, feat.data_ptr(), 21, dirs.data_ptr(), 3, 5, 7, 0, raw.data_ptr(), ops.stream_ptr()) == -2
    assert f(0, 20, 256, *io, raw.data_ptr(), ops.stream_ptr()) == -1
    assert f(c["packed"].buffer.data_ptr(), 20, 256, *io, raw.data_ptr() + 4, ops.stream_ptr()) == -3
    assert f(c["packed"].buffer.data_ptr(), 20, 256, ndc.data_ptr(), 3, feat.data_ptr(), 20, 0, 3, 5, 7, 0, raw.data_ptr(), ops.stream_ptr()) == -1
    with pytest.raises(RuntimeError, match="feat_dim"):
        ops.mlp_forward(c["packed"], 12, *io[:8], False, DEV)


# ------------------------------------------------------------------ F
@functools.lru_cache(maxsize=None)
def _scene(n_rays, n_samples):
    from tests.test_gpu_backward import _setup
    rig, pose, vol, pts, dirs, ndc, z, ro, _, _ = _setup(n_rays, n_samples, 5 + n_rays)
    return dict(rig=rig, pose=pose, vol=vol, pts=pts, dirs=dirs, ndc=ndc, z=z, ro=ro)


def _render_args(s):
    t = lambda x: x.to(DEV)
    return ({k: t(v) for k, v in s["pose"].items()}, t(s["pts"]), t(s["ndc"]), t(s["z"]), t(s["ro"]), t(s["dirs"]))


@pytest.mark.parametrize("net_type", NETS)
def test_rendering_is_the_explicit_sequence(net_type):
    from mvsnerf_amd import renderer, ops
    args, net, qfn = _network(net_type)
    scenes = [_scene(37, 16), _scene(5, 7)]
    imgs = scenes[0]["rig"]["images_raw"][:, :3].to(DEV)
    vol = scenes[0]["vol"].to(DEV)
    singles = []
    with torch.no_grad():
        for s in scenes:
            pose_d, pts, ndc, z, ro, rdir = _render_args(s)
            out = renderer.rendering(args, pose_d, pts, ndc, z, ro, rdir, vol, imgs, network_fn=net, network_query_fn=qfn)
            raw = renderer.rendering.last_raw
            N, S = z.shape
            # the explicit sequence
            ang = ops.dir_feature(rdir.contiguous(), pose_d["w2cs"][0].contiguous(), normalize=True)
            feat = renderer.gen_pts_feats(imgs, vol, pts, pose_d, ndc, 20)
            raw_x = ops.mlp_forward(net.packed(20), 20, ndc.data_ptr(), 3, feat.data_ptr(), 20, ang.data_ptr(), 3, N, S, False, ndc.device)
            rgb, _, _, weights, depth, alpha = ops.composite(raw_x.view(N, S, 4), z.contiguous(), False)
            assert torch.equal(raw.reshape(-1, 4), raw_x) and torch.equal(out[1], feat)
            for a, b in ((out[0], rgb), (out[2], weights), (out[3], depth), (out[4], alpha)):
                assert torch.equal(a, b)
            assert bool(torch.isfinite(out[0]).all()) and float(out[2].abs().max()) > 0
            singles.append(out)
        pose_d = _render_args(scenes[0])[0]
        outs = renderer.rendering_batched(args, pose_d, [_render_args(s)[1:] for s in scenes], vol, imgs, network_fn=net, network_query_fn=qfn)
    assert len(outs) == 2
    for o, single in zip(outs, singles):
        for i in range(5):
            assert torch.equal(o[i], single[i]), i


@pytest.mark.parametrize("net_type", NETS)
def test_run_network_mvs_and_render_density(net_type):
    from mvsnerf_amd import renderer
    _, net, qfn = _network(net_type)
    c = _case(37, 24, 20, net_type)
    ndc, feat, dirs = c["x"]
    with torch.no_grad():
        raw = qfn(ndc, dirs, feat, net)
        sig = qfn(ndc, None, feat, net)
        dens = renderer.render_density(net, ndc, feat, qfn, chunk=10)
    assert raw.shape == (37, 24, 4) and sig.shape == (37, 24, 1)
    assert torch.equal(raw.reshape(-1, 4), c["raw"]) and torch.equal(sig.reshape(-1, 1), c["alpha"])
    assert torch.equal(dens, sig)
    assert (float(dens.min()) < 0) == (net_type == "v2")


def test_render_view_is_the_per_chunk_loop():
    from mvsnerf_amd import train, renderer
    from mvsnerf_amd.utils import build_rays_test
    H, W, S, chunk = 24, 32, 8, 256
    args = train.default_args(pad=4, batch_size=64, N_samples=S, chunk=chunk, netwidth=R.WIDE, net_type="v2")
    sys_ = train.MVSSystem(args, n_depth_planes=16)
    sys_.render_kwargs_train["network_fn"].load_state_dict(_state_dict(*R.weights(20)))
    sys_ = sys_.to(DEV)
    batch = train.synthetic_batch(H, W, seed=5, smooth=True)
    # the scene's volume is handed in (render_view(volume=...)): a frame this small has no encode (CostRegNet wants h/4 + 2 pad, w/4 + 2 pad divisible
    # by 8), and the MLP's wiring is what is under test
    vol = torch.randn((1, 8, 16, 24, 32), generator=torch.Generator().manual_seed(7)).to(DEV)
    rgb, depth = sys_.render_view(batch, volume=vol)
    assert rgb.shape == (H, W, 3) and depth.shape == (H, W)
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(depth).all())
    # the loop, spelled out
    with torch.no_grad():
        data, pose_ref = sys_.decode_batch(dict(batch))
        imgs = sys_.unpreprocess(data["images"])
        nf = pose_ref["near_fars"]
        parts = []
        for idx in range((H * W + chunk - 1) // chunk):
            pts, rdir, ndc, z, ro, _ = build_rays_test(H, W, pose_ref["c2ws"][-1], pose_ref["w2cs"][0], pose_ref["intrinsics"][-1], nf, nf[-1], S,
                                                       pad=args.pad, chunk=chunk, idx=idx)
            out = renderer.rendering(args, pose_ref, pts, ndc, z, ro, rdir, vol, imgs[:, :-1], img_feat=None, **sys_.render_kwargs_train)
            parts.append((out[0], out[3]))
    assert torch.equal(rgb.reshape(-1, 3), torch.cat([p[0] for p in parts]))
    assert torch.equal(depth.reshape(-1), torch.cat([p[1] for p in parts]))
    rgb2, depth2 = sys_.render_view(batch, volume=vol, whole_frame_off=True)
    assert torch.equal(rgb2, rgb) and torch.equal(depth2, depth)


# ------------------------------------------------------------------ G
def test_refusals_come_before_any_launch():
    from mvsnerf_amd import models, renderer, ops
    args, net, qfn = _network("v2")
    s = _scene(37, 16)
    pose_d, *rays = _render_args(s)
    vol, imgs = s["vol"].to(DEV), s["rig"]["images_raw"][:, :3].to(DEV)
    with torch.no_grad():
        wp = net.packed(20)
    assert isinstance(wp, ops.WidePacked) and not torch.is_tensor(wp) and (wp.width, wp.F, wp.variant) == (256, 20, 1)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="netwidth"):
        ops.raymarch(ops.channels_last_volume(vol), imgs[0].contiguous(), pose_d["w2cs"][:3].contiguous(), pose_d["intrinsics"][:3].contiguous(), wp,
                     rays[0], rays[1], rays[2], rays[4])
    with pytest.raises(NotImplementedError, match="training at netwidth 256"):
        renderer.rendering(args, pose_d, *rays, models.RefVolume(vol), imgs, network_fn=net, network_query_fn=qfn)
    for p in net.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="training at netwidth 256"):
        renderer.rendering(args, pose_d, *rays, vol.clone().requires_grad_(True), imgs, network_fn=net, network_query_fn=qfn)
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "bf16x6", "fp16x3"])
def test_16_bit_modes_refuse_netwidth_256(mode):
    from mvsnerf_amd import renderer, ops
    args, net, qfn = _network("v0")
    s = _scene(37, 16)
    pose_d, *rays = _render_args(s)
    vol, imgs = s["vol"].to(DEV), s["rig"]["images_raw"][:, :3].to(DEV)
    with ops.mlp_precision(mode), torch.no_grad():
        with pytest.raises(NotImplementedError, match="netwidth"):
            renderer.rendering(args, pose_d, *rays, vol, imgs, network_fn=net, network_query_fn=qfn)
        with pytest.raises(NotImplementedError, match="netwidth"):
            qfn(rays[1], None, torch.zeros((37, 16, 20), device=DEV), net)


@pytest.mark.parametrize("net_type", NETS)
def test_auto_runs_the_wide_kernel(net_type):
    from mvsnerf_amd import renderer, ops
    args, net, qfn = _network(net_type)
    s = _scene(37, 16)
    pose_d, *rays = _render_args(s)
    vol, imgs = s["vol"].to(DEV), s["rig"]["images_raw"][:, :3].to(DEV)
    with ops.mlp_precision("fp32"), torch.no_grad():
        want = renderer.rendering(args, pose_d, *rays, vol, imgs, network_fn=net, network_query_fn=qfn)
    before = ops.guard_fallbacks()
    with ops.mlp_precision("auto"), torch.no_grad():
        assert net.packed_alt(20) == {}
        got = renderer.rendering(args, pose_d, *rays, vol, imgs, network_fn=net, network_query_fn=qfn)
    assert ops.guard_fallbacks() == before
    for i in range(5):
        assert torch.equal(got[i], want[i]), i
