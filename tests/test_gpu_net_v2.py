"""net_type 'v2' (Renderer_linear, reference models.py:464-538) on the fp32 ray-march kernels (csrc/mlp.hip, csrc/mlp_bwd.hip; V_ADD of mlp_layout.h).

v2 has v0's layers and state_dict; it differs in h_i = relu(pts_linears.i(h) + bias) (v0: * bias), bias = pts_bias(feat), and in forward_alpha, which
returns alpha_linear(h) without the ReLU.  The packed buffer carries the variant (ops.mlp_pack(variant=1) -> mvsnerf_mlp_pack_fold_variant) and every
fp32 kernel handed it follows.  The oracle has no v2 network, so the network is stated here with torch.nn.functional.linear (_trunk_v2; the tail is
v0's, tests/test_gpu_mlp_fold.py:_tail) and evaluated in float64 on the CPU; lookups and compositing come from the oracle.

A  neutral bias: v2 with pts_bias = (0, 0) and v0 with pts_bias = (0, 1) on otherwise equal weights are the same function and acc + 0 / acc * 1 are
   both exact -> equal values from the full forward, the training forward, ops.raymarch (NR = 2 and NR = 1), ops.render_pixels and relu(sigma-only).
B  the v2 sigma-only launch is un-clamped: negative where float64 is negative by more than the kernel's own sigma error; its relu is the full
   forward's sigma bit for bit.
C  accuracy against float64, calibrated on the unchanged v0 kernel: r = mean|kernel - f64| / mean|fp32 torch CPU - f64|, r_v2 <= 1.25 r_v0, for
   rgb and sigma separately (1.25: the margin test_gpu_mlp_fold.py (ii) gives one re-associated chain).
D  ops.raymarch (one launch) = gather -> mlp_forward -> composite on a v2 buffer, bit for bit.
E  renderer.rendering() / rendering_batched() / run_network_mvs / render_density with a v2 network against the float64 composition, within the
   bounds tests/test_gpu_raymarch.py applies in fp32 mode (3e-6 + 2e-6 |ref|).
F  gradients of rendering() (learnable RefVolume + the 22 tensors) against autograd through the float64 composition: loss within 1e-3, every
   gradient within 2e-3 of max |ref| (test_raymarch_backward_vs_autograd's yardstick).
G  "auto" runs v2 on the fp32 kernel; the 16-bit modes - use_amp's included - raise NotImplementedError.

Weights: torch.manual_seed(SEED[F]), every parameter uniform(-0.15, 0.15) - not the shipped checkpoint, which was trained as v0 and saturates
under v2.  Per F, float64 alpha_linear output must be negative on >= 5 % and positive on >= 5 % of the (37, 24) points, or B sees nothing.
"""
import functools
import types

import pytest
import torch

from tests.test_gpu_mlp_fold import _inputs, _embed, _tail, _trunk, _fwd, _fwd_train, _bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(5, 7), (37, 24)]
FS = [12, 20, 36]
CASES = [(N, S, F) for (N, S) in SHAPES for F in FS]
SEED = {12: 12, 20: 20, 36: 36}          # torch.manual_seed(F), as tests/test_gpu_mlp_fold.py; a seed that misses the sign condition is replaced, the share is not lowered


# ------------------------------------------------------------------ the network in torch
def _weights(F):
    """11 (weight, bias) fp32 CPU pairs in ops.MLP_ORDER, uniform(-0.15, 0.15)"""
    from mvsnerf_amd import models
    m = models.MVSNeRF(D=6, W=128, input_ch_pts=63, input_ch_views=3, input_ch_feat=F, skips=[4], net_type="v2")
    torch.manual_seed(SEED[F])
    for p in m.parameters():
        torch.nn.init.uniform_(p, -0.15, 0.15)
    lins = m.nerf._linears()
    return [l.weight.detach().clone().contiguous() for l in lins], [l.bias.detach().clone().contiguous() for l in lins]


def _trunk_v2(ws, bs, ndc, feat):
    """-> (h5, alpha_linear(h5) WITHOUT the ReLU) of Renderer_linear (models.py:499-507, 515-521) in the dtype of the arguments"""
    lin = torch.nn.functional.linear
    pts = _embed(ndc)
    bias = lin(feat, ws[6], bs[6])
    h = pts
    for i in range(6):
        h = torch.relu(lin(h, ws[i], bs[i]) + bias)
        if i == 4:
            h = torch.cat([pts, h], -1)
    return h, lin(h, ws[8], bs[8])


def _net_v2(ws, bs, ndc, feat, dirs):
    """Renderer_linear.forward (models.py:510-538) -> (..., 4)"""
    h5, a = _trunk_v2(ws, bs, ndc, feat)
    return torch.cat([_tail(ws, bs, h5, dirs), torch.relu(a)], -1)


def _net_v0(ws, bs, ndc, feat, dirs):
    h5, s = _trunk(ws, bs, ndc, feat)
    return torch.cat([_tail(ws, bs, h5, dirs), s], -1)


def _dbl(ts):
    return [t.double() for t in ts]


def _pack(ws, bs, F, variant):
    from mvsnerf_amd import ops
    p = ops.mlp_pack([w.to(DEV) for w in ws], [b.to(DEV) for b in bs], F, variant=variant)
    torch.cuda.synchronize()
    return p


def _neutral(ws, bs, b):
    """the same weights with pts_bias = (0, b)"""
    ws2, bs2 = list(ws), list(bs)
    ws2[6], bs2[6] = torch.zeros_like(ws[6]), torch.full_like(bs[6], b)
    return ws2, bs2


@functools.lru_cache(maxsize=None)
def _net(F):
    ws, bs = _weights(F)
    return dict(ws=ws, bs=bs, v2=_pack(ws, bs, F, 1), v0=_pack(ws, bs, F, 0),
                n2=_pack(*_neutral(ws, bs, 0.0), F, 1), n0=_pack(*_neutral(ws, bs, 1.0), F, 0))


@functools.lru_cache(maxsize=None)
def _case(N, S, F):
    """inputs, the kernels' outputs and the float64 / fp32 CPU evaluations of one case, computed once and shared"""
    net = _net(F)
    xc = _inputs(N, S, F)
    x = tuple(t.to(DEV) for t in xc)
    ws, bs = net["ws"], net["bs"]
    h5, a64 = _trunk_v2(_dbl(ws), _dbl(bs), xc[0].double(), xc[1].double())
    ref = torch.cat([_tail(_dbl(ws), _dbl(bs), h5, xc[2].double()), torch.relu(a64)], -1).reshape(N * S, 4)
    return dict(net=net, x=x, xc=xc, raw=_fwd(net["v2"], F, x), alpha=_fwd(net["v2"], F, x, alpha_only=1), ref=ref, a64=a64.reshape(N * S))


def _state_dict(ws, bs):
    from mvsnerf_amd import ops
    sd = {}
    for name, w, b in zip(ops.MLP_ORDER, ws, bs):
        sd[f"nerf.{name}.weight"], sd[f"nerf.{name}.bias"] = w.clone(), b.clone()
    return sd


def _args(net_type="v2", **kw):
    d = dict(feat_dim=20, img_downscale=1.0, use_color_volume=False, net_type=net_type, multires=10, i_embed=0, pts_dim=3,
             multires_views=4, dir_dim=3, netdepth=6, netwidth=128, N_importance=0, netchunk=1024, ckpt=None, perturb=1.0,
             N_samples=32, use_viewdirs=True, white_bkgd=False, raw_noise_std=0.0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _network(net_type="v2", F=20):
    """(args, network_fn on the GPU with _weights(F), network_query_fn) as create_nerf_mvs builds them"""
    from mvsnerf_amd import models
    args = _args(net_type, feat_dim=F)
    kw, _, _, _ = models.create_nerf_mvs(args, use_mvs=False, dir_embedder=False, pts_embedder=True)
    ws, bs = _weights(F)
    kw["network_fn"].load_state_dict(_state_dict(ws, bs))
    return args, kw["network_fn"].to(DEV), kw["network_query_fn"]


# ------------------------------------------------------------------ the condition on the weights
@pytest.mark.parametrize("F", FS)
def test_weights_put_alpha_on_both_sides_of_zero(F):
    a = _case(37, 24, F)["a64"]
    neg, pos = float((a < 0).double().mean()), float((a > 0).double().mean())
    print(f"v2 weights F={F} seed {SEED[F]}: float64 alpha_linear negative on {neg:.3f}, positive on {pos:.3f} of the points")
    assert neg >= 0.05 and pos >= 0.05, (neg, pos)


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("N,S,F", CASES)
def test_neutral_bias_is_v0(N, S, F):
    c = _case(N, S, F)
    net, x = c["net"], c["x"]
    r2, r0 = _fwd(net["n2"], F, x), _fwd(net["n0"], F, x)
    assert r2.shape == (N * S, 4) and torch.equal(r2, r0), [float((r2[:, k] - r0[:, k]).abs().max()) for k in range(4)]
    assert float(r0[:, 3].max()) > 0 and float(r0[:, :3].std()) > 0                       # not a dead network
    a2, a0 = _fwd(net["n2"], F, x, alpha_only=1), _fwd(net["n0"], F, x, alpha_only=1)
    assert torch.equal(torch.relu(a2), a0)
    if F <= 32:                                        # the training forward takes F <= 32 (include/mvsnerf_hip.h)
        (t2, _), (t0, _) = _fwd_train(net["n2"], F, x), _fwd_train(net["n0"], F, x)
        assert torch.equal(t2, t0), [float((t2[:, k] - t0[:, k]).abs().max()) for k in range(4)]
        # the training forward ignores the fold (its backward consumes feature_linear's output), so only sigma is the no-grad kernel's bits
        assert torch.equal(t2[:, 3], r0[:, 3])


@pytest.mark.parametrize("N,S", [(37, 16), (20, 128)])
def test_neutral_bias_raymarch_is_v0(N, S):
    """ops.raymarch, NR = 2 (S = 16) and NR = 1 (S = 128): every output equal"""
    from tests.test_gpu_raymarch_onelaunch import _hwdc, _inputs as rm_inputs
    from mvsnerf_amd import ops
    net = _net(20)
    x = rm_inputs(N, S, seed=S)
    vol_cl = _hwdc(x["vol"])
    with torch.no_grad():
        o2, o0 = (ops.raymarch(vol_cl, x["imgs"], x["w2cs"], x["Ks"], net[k], x["pts"], x["ndc"], x["z"], x["dirs"], want=("disp", "acc"))
                  for k in ("n2", "n0"))
    torch.cuda.synchronize()
    assert set(o2) == set(o0)
    for k in o0:
        assert torch.equal(o2[k], o0[k]), (k, float((o2[k] - o0[k]).abs().max()))
    assert float(o0["acc"].max()) > 0


def test_neutral_bias_render_pixels_is_v0():
    """ops.render_pixels (ray generation + one-launch ray march per sub-batch): the frame of the v2 buffer is v0's"""
    from tests.test_gpu_raymarch_onelaunch import _hwdc
    from mvsnerf_amd import ops
    from mvsnerf_amd.synth import make_rig, pose_ref_of
    H, W, S, pad = 48, 64, 24, 4
    rig = make_rig(H, W, seed=11, rot_deg=2.0, smooth=True)
    pd = {k: v.to(DEV) for k, v in pose_ref_of(rig).items()}
    vol = torch.randn((1, 8, 16, H // 4 + 2 * pad, W // 4 + 2 * pad), generator=torch.Generator().manual_seed(2))
    imgs = rig["images_raw"][0, :3].to(DEV)
    net = _net(20)
    outs = []
    for k in ("n2", "n0"):
        args = (_hwdc(vol), imgs, pd["w2cs"][:3].contiguous(), pd["intrinsics"][:3].contiguous(), net[k], H, W, pd["intrinsics"][-1], pd["c2ws"][-1],
                pd["intrinsics"][-1], pd["w2cs"][0], pd["near_fars"][-1], pd["near_fars"][0], S)
        with torch.no_grad():
            outs.append(ops.render_pixels(*args, first_pixel=100, n_pixels=1500, pad=pad, batch_rays=1024, want=("depth", "acc", "disp")))
    for k in ("rgb", "depth", "acc", "disp"):
        assert torch.equal(outs[0][k], outs[1][k]), k


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("N,S,F", CASES)
def test_sigma_only_is_unclamped(N, S, F):
    c = _case(N, S, F)
    a, full = c["alpha"], c["raw"][:, 3]
    assert a.shape == (N * S, 1)
    assert _bits(torch.relu(a[:, 0]), full)
    err = float((full.cpu().double() - c["ref"][:, 3]).abs().max())                     # the kernel's own sigma error (C)
    must = c["a64"] < -err
    got = a[:, 0].cpu()
    print(f"v2 sigma-only (N,S,F)=({N},{S},{F}): {int(must.sum())} of {N * S} points negative in float64 by more than {err:.2e}; min {float(got.min()):.4f}")
    assert bool((got[must] < 0).all())
    if (N, S) == (37, 24):
        assert bool(must.any())


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("F", FS)
def test_accuracy_against_float64_calibrated_on_v0(F):
    N, S = 37, 24
    c = _case(N, S, F)
    ws, bs, (ndc, feat, dirs) = c["net"]["ws"], c["net"]["bs"], c["xc"]
    ref0 = _net_v0(_dbl(ws), _dbl(bs), ndc.double(), feat.double(), dirs.double()).reshape(N * S, 4)
    t2 = _net_v2(ws, bs, ndc, feat, dirs).reshape(N * S, 4).double()
    t0 = _net_v0(ws, bs, ndc, feat, dirs).reshape(N * S, 4).double()
    k2, k0 = c["raw"].cpu().double(), _fwd(c["net"]["v0"], F, c["x"]).cpu().double()
    for name, sl in (("rgb", slice(0, 3)), ("sigma", slice(3, 4))):
        e = lambda a, b: float((a[:, sl] - b[:, sl]).abs().mean())
        r2, r0 = e(k2, c["ref"]) / e(t2, c["ref"]), e(k0, ref0) / e(t0, ref0)
        print(f"v2 accuracy F={F} {name}: e_k/e_t v2 {r2:.3f} ({e(k2, c['ref']):.3e} / {e(t2, c['ref']):.3e})  v0 {r0:.3f} ({e(k0, ref0):.3e} / {e(t0, ref0):.3e})")
        assert r2 <= 1.25 * r0, (name, r2, r0)


# ------------------------------------------------------------------ D
@pytest.mark.parametrize("N,S", [(37, 16), (20, 128)])
def test_onelaunch_on_a_v2_buffer(N, S):
    from tests.test_gpu_raymarch_onelaunch import _check, _hwdc, _inputs as rm_inputs
    x = rm_inputs(N, S, seed=S)
    _check(_hwdc(x["vol"]), x, _net(20)["v2"])
    _check(_hwdc(x["vol"]), x, _net(20)["v2"], white_bkgd=True)


# ------------------------------------------------------------------ E, F: the float64 composition
def _close(a, b, what):
    """tests/test_gpu_raymarch.py close(): 3e-6 + 2e-6 |ref| (its bound on rgb, weights, depth, alpha and raw in fp32 mode)"""
    a, b = a.detach().cpu().double().reshape(b.shape), b.detach().double()
    err = (a - b).abs()
    print(f"  {what}: max err {float(err.max()):.2e} (max |ref| {float(b.abs().max()):.3g})")
    assert bool((err <= 3e-6 + 2e-6 * b.abs()).all()), (what, float(err.max()))


def _compose64(rig, pose, vol, pts, dirs, ndc, z, ws, bs, white=False):
    """rendering() (renderer.py:138-165) with Renderer_linear in float64.  The lookups are the oracle's in fp32 (the kernels reproduce them bit for
    bit); the volume part is looked up again in float64 when `vol` is a float64 tensor (gradients).  -> (rgb, feat32, weights, depth, alpha, raw)"""
    from oracle import mvsnerf_oracle as O
    ang = O.gen_dir_feature(pose["w2cs"][0], dirs / torch.norm(dirs, dim=-1).unsqueeze(-1))
    feat32 = O.gen_pts_feats(rig["images_raw"][:, :3], vol.detach().float(), pts, pose, ndc)
    feat = feat32.double()
    if vol.dtype == torch.float64:
        feat = torch.cat([O.index_point_feature(vol, ndc.double()), feat[..., 8:]], -1)
    raw = _net_v2(ws, bs, ndc.double(), feat, ang.double())
    rgb, _, _, weights, depth, alpha = O.raw2outputs(raw, z.double(), white)
    return rgb, feat32, weights, depth, alpha, raw


@functools.lru_cache(maxsize=None)
def _scene(n_rays, n_samples, white=False):
    from tests.test_gpu_backward import _setup
    rig, pose, vol, pts, dirs, ndc, z, ro, _, G = _setup(n_rays, n_samples, 5 + n_rays, white)
    return dict(rig=rig, pose=pose, vol=vol, pts=pts, dirs=dirs, ndc=ndc, z=z, ro=ro, G=G)


def _render_args(s):
    t = lambda x: x.to(DEV)
    return ({k: t(v) for k, v in s["pose"].items()}, t(s["pts"]), t(s["ndc"]), t(s["z"]), t(s["ro"]), t(s["dirs"]))


def test_rendering_and_batched_against_float64():
    from mvsnerf_amd import renderer, ops
    args, net, qfn = _network()
    ws, bs = _weights(20)
    shapes = [(37, 24), (5, 7), (20, 128)]
    scenes = [_scene(*sh) for sh in shapes]
    imgs = scenes[0]["rig"]["images_raw"][:, :3].to(DEV)
    vol = scenes[0]["vol"].to(DEV)                                          # one scene (same rig, same volume), three ray batches
    singles = []
    with ops.mlp_precision("fp32"), torch.no_grad():
        for sh, s in zip(shapes, scenes):
            pose_d, *rays = _render_args(s)
            out = renderer.rendering(args, pose_d, *rays, vol, imgs, network_fn=net, network_query_fn=qfn)
            raw = renderer.rendering.last_raw
            ref = _compose64(s["rig"], s["pose"], scenes[0]["vol"], s["pts"], s["dirs"], s["ndc"], s["z"], _dbl(ws), _dbl(bs))
            print(f"rendering() v2 {sh}:")
            assert torch.equal(out[1].cpu(), ref[1])                        # the lookups are exact
            for a, b, k in ((out[0], ref[0], "rgb"), (out[2], ref[2], "weights"), (out[3], ref[3], "depth"), (out[4], ref[4], "alpha"), (raw, ref[5], "raw")):
                _close(a, b, k)
            singles.append((out, raw))
        pose_d = _render_args(scenes[0])[0]
        outs = renderer.rendering_batched(args, pose_d, [_render_args(s)[1:] for s in scenes], vol, imgs, network_fn=net, network_query_fn=qfn)
    assert len(outs) == len(singles)
    for o, (single, _) in zip(outs, singles):
        for i in range(5):
            assert torch.equal(o[i], single[i]), i


def test_run_network_mvs_and_render_density():
    """the piecewise entries: run_network_mvs with and without view directions, render_density (sigma-only: un-clamped, negative values pass through)"""
    from mvsnerf_amd import renderer, ops
    args, net, qfn = _network()
    c = _case(37, 24, 20)
    ndc, feat, dirs = c["x"]
    with ops.mlp_precision("fp32"), torch.no_grad():
        raw = qfn(ndc, dirs, feat, net)
        sig = qfn(ndc, None, feat, net)
        dens = renderer.render_density(net, ndc, feat, qfn, chunk=10)
    assert raw.shape == (37, 24, 4) and sig.shape == (37, 24, 1)
    assert torch.equal(raw.reshape(-1, 4), c["raw"]) and torch.equal(sig.reshape(-1, 1), c["alpha"])
    assert torch.equal(dens, sig) and float(dens.min()) < 0
    _close(raw, c["ref"].reshape(37, 24, 4), "run_network_mvs raw")
    # the reference's concatenated rows through MVSNeRF.forward / forward_alpha
    x = torch.cat([_embed(ndc.cpu()).to(DEV), feat, dirs[:, None].expand(-1, 24, -1)], -1)
    with ops.mlp_precision("fp32"), torch.no_grad():
        assert torch.equal(net(x).reshape(-1, 4), c["raw"])
        assert torch.equal(net.forward_alpha(x[..., :83]).reshape(-1, 1), c["alpha"])


# ------------------------------------------------------------------ F
@pytest.mark.parametrize("n_rays,n_samples,white", [(37, 16, True), (8, 128, False), (130, 3, False)])
def test_gradients_against_float64_autograd(n_rays, n_samples, white):
    from mvsnerf_amd import models, renderer, ops
    s = _scene(n_rays, n_samples, white)
    R, Q, Wt, A = s["G"]
    ws, bs = _weights(20)
    w64, b64 = [w.double().requires_grad_(True) for w in ws], [b.double().requires_grad_(True) for b in bs]
    vol64 = s["vol"].double().requires_grad_(True)
    out = _compose64(s["rig"], s["pose"], vol64, s["pts"], s["dirs"], s["ndc"], s["z"], w64, b64, white)
    loss_ref = (out[0] * R).sum() + (out[3] * Q).sum() + (out[2] * Wt).sum() + (out[4] * A).sum()
    loss_ref.backward()
    gref = {}
    for name, w, b in zip(ops.MLP_ORDER, w64, b64):
        gref[f"nerf.{name}.weight"], gref[f"nerf.{name}.bias"] = w.grad, b.grad

    args, net, qfn = _network()
    args.white_bkgd = white
    vol_g = models.RefVolume(s["vol"].to(DEV))
    pose_d, *rays = _render_args(s)
    with ops.mlp_precision("auto"):                                        # a step that needs gradients runs fp32 under "auto"
        rgb, feat, w, depth, alpha, _ = renderer.rendering(args, pose_d, *rays, vol_g, s["rig"]["images_raw"][:, :3].to(DEV), network_fn=net,
                                                           network_query_fn=qfn, white_bkgd=white)
        loss = (rgb * R.to(DEV)).sum() + (depth * Q.to(DEV)).sum() + (w * Wt.to(DEV)).sum() + (alpha * A.to(DEV)).sum()
        assert abs(float(loss.detach()) - float(loss_ref.detach())) < 1e-3 * max(1.0, abs(float(loss_ref.detach())))
        loss.backward()

    def rel(a, b):
        return float((a.cpu().double() - b).abs().max() / (b.abs().max() + 1e-12))
    errs = {"volume": rel(vol_g.feat_volume.grad, vol64.grad)}
    named = dict(net.named_parameters())
    assert set(named) == set(gref) and len(named) == 22
    for name, p in named.items():
        errs[name] = rel(p.grad, gref[name])
    print(f"v2 gradients ({n_rays},{n_samples},{white}): worst {max(errs.values()):.2e}", {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < 2e-3}
    assert not bad, f"gradient mismatches (rel. to max |ref|): {bad}\nall: {errs}"
    assert float(named["nerf.pts_bias.weight"].grad.abs().max()) > 0 and float(gref["nerf.pts_bias.weight"].abs().max()) > 0      # not a dead bias path


# ------------------------------------------------------------------ G
def test_auto_runs_v2_on_the_fp32_kernel():
    from mvsnerf_amd import renderer, ops
    args, net, qfn = _network()
    s = _scene(37, 24)
    pose_d, *rays = _render_args(s)
    vol, imgs = s["vol"].to(DEV), s["rig"]["images_raw"][:, :3].to(DEV)
    with ops.mlp_precision("fp32"), torch.no_grad():
        want = renderer.rendering(args, pose_d, *rays, vol, imgs, network_fn=net, network_query_fn=qfn)
    before = ops.guard_fallbacks()
    with ops.mlp_precision("auto"), torch.no_grad():
        assert net.packed_alt(20) == {}
        got = renderer.rendering(args, pose_d, *rays, vol, imgs, network_fn=net, network_query_fn=qfn)
        sig = qfn(rays[1], None, got[1], net)
    assert ops.guard_fallbacks() == before
    for i in range(5):
        assert torch.equal(got[i], want[i]), i
    assert torch.equal(torch.relu(sig[..., 0]), renderer.rendering.last_raw[..., 3])


@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "bf16x6", "fp16x3"])
def test_16_bit_modes_refuse_v2(mode):
    from mvsnerf_amd import renderer, ops
    args, net, qfn = _network()
    s = _scene(37, 24)
    pose_d, *rays = _render_args(s)
    vol, imgs = s["vol"].to(DEV), s["rig"]["images_raw"][:, :3].to(DEV)
    c = _case(5, 7, 20)
    with ops.mlp_precision(mode):
        with torch.no_grad():
            with pytest.raises(NotImplementedError, match=r"net_type v2.*fp32"):
                qfn(c["x"][0], c["x"][2], c["x"][1], net)
            with pytest.raises(NotImplementedError, match=r"net_type v2.*fp32"):
                qfn(c["x"][0], None, c["x"][1], net)
            with pytest.raises(NotImplementedError, match=r"net_type v2.*fp32"):
                renderer.rendering(args, pose_d, *rays, vol, imgs, network_fn=net, network_query_fn=qfn)
        if mode == "bf16":                                                  # what use_amp sets around a training step (train.py)
            with pytest.raises(NotImplementedError, match=r"net_type v2.*fp32"):
                renderer.rendering(args, pose_d, *rays, vol, imgs, network_fn=net, network_query_fn=qfn)
