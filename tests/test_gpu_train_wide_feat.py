"""Training the ray-march MLP with 7 and 8 source views: feat_dim F = 8 + 4V = 36 and 40, every even F up to 40 in the kernels.

The saved-activation format had 16 feature slots and the transposed pts_bias segment one block of 32 columns (csrc/mlp_layout.h), so everything
that needs gradients stopped at F = 32.  Feature operands 16..19 now live in slots 2..5 of the direction block (S_FV_HI), pts_bias^T has a second
block, its weight gradient contracts over [S_FV | the S_DR block] through a 64-entry column table.  Every case below was MVSNERF_EUNSUPPORTED.

A  training forward, F = 34 / 36 / 40 (one slot past 16; V = 7; all 20 slots), (N, S) = (5, 7) / (37, 24), v0 and v2 buffers: sigma is the no-grad
   fp32 forward's, bit for bit (the identity tests/test_gpu_mlp_fold.py B and tests/test_gpu_net_v2.py A hold for F <= 32); rgb against float64 with
   r = mean|kernel - f64| / mean|torch fp32 CPU - f64| and r(F) <= 1.25 r(32), r(32) from the same run, shape and variant (F = 32: the unchanged
   path; 1.25: the margin tests/test_gpu_mlp_fold.py (ii) gives one re-associated chain).
B  gradients of rendering() for V = 7 and V = 8 (learnable RefVolume + the 22 tensors): v0 against autograd through the oracle, v2 against the
   float64 composition; loss within 1e-3, every gradient within 2e-3 of max |ref| (tests/test_gpu_backward.py's yardstick), and
   pts_bias.weight.grad[:, 32:] on its own against max |ref| of those columns, which must be > 0.
C  use_color_volume, V = 7 (and 8): the 36- (40-) channel learnable volume against autograd, channels 32: bounded on their own; with the float-atomic
   and with the order-independent scatter (ops.VOLUME_BWD_DETERMINISTIC).
D  use_amp at F = 36 / 40: the comparison and the bounds of tests/test_gpu_backward.py::test_bf16_training_vs_torch_emulation.
E  MVSSystemFinetune with n_views = 7 on a 64 x 96 rig, fp32 and use_amp, then render_rays on the learnt volume: what
   tests/test_gpu_train.py::test_finetune_five_source_views_bf16 asserts.

Weights.  v0 (B, C, D): the shipped checkpoint widened to V views - pts_bias.weight column 8 + 4v + c takes the checkpoint's column 8 + 4(v % 3) + c
times 3 / V, so pts_bias(feat) keeps the scale the network was trained with (the bounds B and D reuse were set on this network).  v2 and A:
uniform(-0.15, 0.15) from torch.manual_seed(SEED[...]) as tests/test_gpu_net_v2.py (the checkpoint saturates under v2).  A seed whose float64
reference does not reach columns 32: is replaced, the condition is not relaxed.
"""
import functools
import types

import pytest
import torch

from tests.test_gpu_mlp_fold import _inputs, _tail, _trunk, _fwd, _fwd_train
from tests.test_gpu_net_v2 import _trunk_v2, _net_v2, _dbl, _state_dict
from tests.test_gpu_backward import _renderer_bf16_emulation
from tests.util import load_weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(5, 7), (37, 24)]
WIDE = [34, 36, 40]
SEED = {("v0", 32): 32, ("v0", 34): 34, ("v0", 36): 36, ("v0", 40): 40, ("v2", 32): 32, ("v2", 34): 34, ("v2", 36): 36, ("v2", 40): 40}
AMP_SEED = {7: 132, 8: 123}        # D: scenes on which the bf16 emulation itself lies within 0.10 of the fp32 oracle in every gradient (CPU, asserted below)
BASELINES = (0.0, 0.25, -0.25, 0.12, -0.12, 0.18, -0.18, 0.06, 0.1)


# ------------------------------------------------------------------ weights
def _random_weights(F, net_type):
    """11 (weight, bias) fp32 CPU pairs in ops.MLP_ORDER, uniform(-0.15, 0.15)"""
    from mvsnerf_amd import models
    m = models.MVSNeRF(D=6, W=128, input_ch_pts=63, input_ch_views=3, input_ch_feat=F, skips=[4], net_type=net_type)
    torch.manual_seed(SEED[(net_type, F)])
    for p in m.parameters():
        torch.nn.init.uniform_(p, -0.15, 0.15)
    lins = m.nerf._linears()
    return [l.weight.detach().clone().contiguous() for l in lins], [l.bias.detach().clone().contiguous() for l in lins]


def _widened_checkpoint(V):
    """state_dict of the shipped v0 network with pts_bias widened from 3 to V source views (module docstring)"""
    sd = {k: v.clone() for k, v in load_weights()[0].items()}
    w = sd["nerf.pts_bias.weight"]
    assert w.shape == (128, 20)
    cols = [w[:, :8]] + [w[:, 8 + 4 * (v % 3):12 + 4 * (v % 3)] * (3.0 / V) for v in range(V)]
    sd["nerf.pts_bias.weight"] = torch.cat(cols, 1).contiguous()
    return sd


def _sd_of(V, net_type):
    if net_type == "v0":
        return _widened_checkpoint(V)
    return _state_dict(*_random_weights(8 + 4 * V, "v2"))


def _lists(sd):
    from mvsnerf_amd import ops
    return [sd[f"nerf.{n}.weight"] for n in ops.MLP_ORDER], [sd[f"nerf.{n}.bias"] for n in ops.MLP_ORDER]


# ------------------------------------------------------------------ A
@functools.lru_cache(maxsize=None)
def _fwd_case(N, S, F, net_type):
    """one training forward and one no-grad forward on the same buffer, float64 and fp32 torch on the CPU: computed once"""
    from mvsnerf_amd import ops
    ws, bs = _random_weights(F, net_type)
    packed = ops.mlp_pack([w.to(DEV) for w in ws], [b.to(DEV) for b in bs], F, variant=1 if net_type == "v2" else 0)
    xc = _inputs(N, S, F)
    x = tuple(t.to(DEV) for t in xc)
    raw_t, saved = _fwd_train(packed, F, x)
    raw_n = _fwd(packed, F, x)

    def rgb(ws_, bs_, ndc, feat, dirs):
        h5, _ = (_trunk_v2 if net_type == "v2" else _trunk)(ws_, bs_, ndc, feat)
        return _tail(ws_, bs_, h5, dirs).reshape(N * S, 3)
    ref = rgb(_dbl(ws), _dbl(bs), *(_dbl(xc)))
    t32 = rgb(ws, bs, *xc).double()
    e_k, e_t = float((raw_t[:, :3].cpu().double() - ref).abs().mean()), float((t32 - ref).abs().mean())
    return dict(raw_t=raw_t, raw_n=raw_n, saved=saved, x=x, e_k=e_k, e_t=e_t, r=e_k / e_t)


@pytest.mark.parametrize("net_type", ["v0", "v2"])
@pytest.mark.parametrize("N,S", SHAPES)
@pytest.mark.parametrize("F", WIDE)
def test_training_forward(F, N, S, net_type):
    c, c32 = _fwd_case(N, S, F, net_type), _fwd_case(N, S, 32, net_type)
    assert c["raw_t"].shape == (N * S, 4)
    assert torch.equal(c["raw_t"][:, 3], c["raw_n"][:, 3]), float((c["raw_t"][:, 3] - c["raw_n"][:, 3]).abs().max())
    assert torch.equal(c32["raw_t"][:, 3], c32["raw_n"][:, 3])
    assert float(c["raw_n"][:, 3].max()) > 0 and float(c["raw_t"][:, :3].std()) > 0                   # not a dead network
    print(f"training forward {net_type} (N,S,F)=({N},{S},{F}): rgb e_k/e_t {c['r']:.3f} ({c['e_k']:.3e} / {c['e_t']:.3e})   F=32: {c32['r']:.3f} "
          f"({c32['e_k']:.3e} / {c32['e_t']:.3e})   ratio of the two {c['r'] / c32['r']:.3f}")
    assert c["r"] <= 1.25 * c32["r"], (c["r"], c32["r"])


@pytest.mark.parametrize("N,S", SHAPES)
@pytest.mark.parametrize("F", WIDE)
def test_training_forward_saves_every_feature_operand(F, N, S):
    """the slots the backward contracts over: operand t of lane half h is feature column h F/2 + t, t < 16 at S_FV, 16 <= t < 20 at S_DR + 2 (zero
    from F/2 on), the directions stay in S_DR + 0 / 1"""
    c = _fwd_case(N, S, F, "v0")
    feat = c["x"][1].reshape(N * S, F)
    n_tiles = ((N * S + 127) // 128) * 4
    sv = c["saved"].view(n_tiles, 608, 2, 32)
    P = N * S
    for t in range(20):
        slot = 32 + t if t < 16 else 592 + 2 + (t - 16)
        for h in range(2):
            got = sv[:, slot, h].reshape(-1)[:P]
            want = feat[:, h * (F // 2) + t] if t < F // 2 else torch.zeros(P, device=DEV)
            assert torch.equal(got, want), (t, h)
    d = c["x"][2][torch.arange(P, device=DEV) // S]                                        # the direction of each point's ray
    assert torch.equal(sv[:, 592, 0].reshape(-1)[:P], d[:, 0]) and torch.equal(sv[:, 592, 1].reshape(-1)[:P], d[:, 1])
    assert torch.equal(sv[:, 593, 0].reshape(-1)[:P], d[:, 2]) and float(sv[:, 593, 1].abs().max()) == 0.0
    c32 = _fwd_case(N, S, 32, "v0")
    sv32 = c32["saved"].view(n_tiles, 608, 2, 32)
    assert float(sv32[:, 594:608].abs().max()) == 0.0            # F <= 32 leaves those slots alone (the buffer was zero-filled)
    assert float(sv[:, 598:608].abs().max()) == 0.0


# ------------------------------------------------------------------ B - D: scenes and references
def _args(F, net_type, n_samples, white=False, color_vol=False):
    return types.SimpleNamespace(feat_dim=F, img_downscale=1.0, use_color_volume=color_vol, net_type=net_type, multires=10, i_embed=0,
                                 pts_dim=3, multires_views=4, dir_dim=3, netdepth=6, netwidth=128, N_importance=0, netchunk=1024,
                                 ckpt=None, perturb=1.0, N_samples=n_samples, use_viewdirs=True, white_bkgd=white, raw_noise_std=0.0)


@functools.lru_cache(maxsize=None)
def _scene(V, n_rays, n_samples, seed):
    """tests/test_gpu_backward.py:_setup with V source views (the last of the V + 1 is the target)"""
    from mvsnerf_amd.synth import make_rig, pose_ref_of
    from oracle import mvsnerf_oracle as O
    rig = make_rig(64, 96, n_views=V + 1, seed=21, baselines=BASELINES, rot_deg=2.0, smooth=True)
    pose = pose_ref_of(rig)
    g = torch.Generator().manual_seed(seed)
    vol = torch.randn((1, 8, 16, 24, 32), generator=g)
    pts, dirs, _, ndc, z, ro, _ = O.build_rays(rig["images_raw"], pose, rig["near_fars"], n_rays, n_samples, pad=4,
                                               t_rand=torch.rand((n_rays, n_samples), generator=g), generator=g)
    ndc = ndc * 1.2 - 0.1
    G = (torch.randn((n_rays, 3), generator=g), torch.randn((n_rays,), generator=g),
         torch.randn((n_rays, n_samples), generator=g) * 0.1, torch.randn((n_rays, n_samples), generator=g) * 0.1)
    return dict(rig=rig, pose=pose, imgs=rig["images_raw"][:, :V].contiguous(), vol=vol, pts=pts, dirs=dirs, ndc=ndc, z=z, ro=ro, G=G)


def _loss(rgb, depth, w, alpha, G, dev=None):
    R, Q, Wt, A = G if dev is None else [t.to(dev) for t in G]
    return (rgb * R).sum() + (depth * Q).sum() + (w * Wt).sum() + (alpha * A).sum()


def reference_gradients(V, net_type, n_rays, n_samples, white):
    """(loss, {name: grad}, volume grad) on the CPU: v0 = autograd through the oracle in fp32 (test_raymarch_backward_vs_autograd), v2 = autograd
    through the float64 composition (tests/test_gpu_net_v2.py F)"""
    from oracle import mvsnerf_oracle as O
    s = _scene(V, n_rays, n_samples, 5 + n_rays)
    sd0 = _sd_of(V, net_type)
    if net_type == "v0":
        sd = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
        vol = s["vol"].clone().requires_grad_(True)
        out = O.rendering(s["pose"], s["pts"], s["ndc"], s["z"], s["dirs"], vol, s["imgs"], sd, white_bkgd=white)
        loss = _loss(out[0], out[3], out[2], out[4], s["G"])
    else:
        sd = {k: v.double().requires_grad_(True) for k, v in sd0.items()}
        vol = s["vol"].double().requires_grad_(True)
        ws, bs = _lists(sd)
        ang = O.gen_dir_feature(s["pose"]["w2cs"][0], s["dirs"] / torch.norm(s["dirs"], dim=-1).unsqueeze(-1))
        feat32 = O.gen_pts_feats(s["imgs"], s["vol"], s["pts"], s["pose"], s["ndc"])
        feat = torch.cat([O.index_point_feature(vol, s["ndc"].double()), feat32[..., 8:].double()], -1)
        raw = _net_v2(ws, bs, s["ndc"].double(), feat, ang.double())
        rgb, _, _, w, depth, alpha = O.raw2outputs(raw, s["z"].double(), white)
        loss = _loss(rgb, depth, w, alpha, [t.double() for t in s["G"]])
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in sd.items()}, vol.grad


_reference_gradients = functools.lru_cache(maxsize=None)(reference_gradients)


def _rel(a, b):
    return float((a.detach().cpu().double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def _network(V, net_type, n_samples, white=False, color_vol=False):
    from mvsnerf_amd import models
    args = _args(8 + 4 * V, net_type, n_samples, white, color_vol)
    kw, _, _, _ = models.create_nerf_mvs(args, use_mvs=False, dir_embedder=False, pts_embedder=True)
    kw["network_fn"].load_state_dict(_sd_of(V, net_type))
    return args, kw["network_fn"].to(DEV), kw["network_query_fn"]


def _render(args, net, qfn, s, vol_g, white=False):
    from mvsnerf_amd import renderer
    t = lambda x: x.to(DEV)
    return renderer.rendering(args, {k: t(v) for k, v in s["pose"].items()}, t(s["pts"]), t(s["ndc"]), t(s["z"]), t(s["ro"]), t(s["dirs"]),
                              vol_g, t(s["imgs"]), network_fn=net, network_query_fn=qfn, white_bkgd=white)


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("n_rays,n_samples,white", [(37, 16, True), (8, 128, False), (130, 3, False)])
@pytest.mark.parametrize("net_type", ["v0", "v2"])
@pytest.mark.parametrize("V", [7, 8])
def test_gradients_of_rendering(V, net_type, n_rays, n_samples, white):
    from mvsnerf_amd import models, ops
    loss_ref, gref, gvol_ref = _reference_gradients(V, net_type, n_rays, n_samples, white)
    hi_ref = gref["nerf.pts_bias.weight"][:, 32:]
    assert hi_ref.shape == (128, 4 * V - 24) and float(hi_ref.abs().max()) > 0                        # the reference reaches the new block
    s = _scene(V, n_rays, n_samples, 5 + n_rays)
    args, net, qfn = _network(V, net_type, n_samples, white)
    vol_g = models.RefVolume(s["vol"].to(DEV))
    with ops.mlp_precision("auto"):                                        # a step that needs gradients runs fp32 under "auto"
        rgb, feat, w, depth, alpha, _ = _render(args, net, qfn, s, vol_g, white)
        loss = _loss(rgb, depth, w, alpha, s["G"], DEV)
        assert feat.shape == (n_rays, n_samples, 8 + 4 * V)
        assert abs(float(loss.detach()) - loss_ref) < 1e-3 * max(1.0, abs(loss_ref)), (float(loss.detach()), loss_ref)
        loss.backward()
    errs = {"volume": _rel(vol_g.feat_volume.grad, gvol_ref)}
    named = dict(net.named_parameters())
    assert set(named) == set(gref) and len(named) == 22
    for name, p in named.items():
        errs[name] = _rel(p.grad, gref[name])
    errs["pts_bias.weight[:, 32:]"] = _rel(named["nerf.pts_bias.weight"].grad[:, 32:], hi_ref)
    errs["pts_bias.weight[:, :32]"] = _rel(named["nerf.pts_bias.weight"].grad[:, :32], gref["nerf.pts_bias.weight"][:, :32])
    print(f"gradients V={V} {net_type} ({n_rays},{n_samples},{white}): worst {max(errs.values()):.2e}; max |ref| of pts_bias columns 32: "
          f"{float(hi_ref.abs().max()):.3e}, of all {float(gref['nerf.pts_bias.weight'].abs().max()):.3e}", {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < 2e-3}
    assert not bad, f"gradient mismatches (rel. to max |ref|): {bad}\nall: {errs}"


# ------------------------------------------------------------------ C
@functools.lru_cache(maxsize=None)
def _color_reference(V):
    from oracle import mvsnerf_oracle as O
    F = 8 + 4 * V
    s = _scene(V, 48, 24, 77)
    vol = torch.cat([s["vol"], torch.rand((1, F - 8, *s["vol"].shape[2:]), generator=torch.Generator().manual_seed(9))], 1)
    sd = {k: v.clone().requires_grad_(True) for k, v in _sd_of(V, "v0").items()}
    vol_ref = vol.clone().requires_grad_(True)
    feat = O.index_point_feature(vol_ref, s["ndc"])                                         # (N,S,F): one lookup, no colour projection
    angle = O.gen_dir_feature(s["pose"]["w2cs"][0], s["dirs"] / torch.norm(s["dirs"], dim=-1).unsqueeze(-1))
    raw = O.run_network_mvs(s["ndc"], angle, feat, sd)
    rgb, _, _, w, depth, alpha = O.raw2outputs(raw, s["z"], False)
    loss = _loss(rgb, depth, w, alpha, s["G"])
    loss.backward()
    return vol, feat.detach(), float(loss.detach()), {k: v.grad for k, v in sd.items()}, vol_ref.grad


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("V", [7, 8])
def test_color_volume_gradients(V, deterministic, monkeypatch):
    from mvsnerf_amd import models, ops
    F = 8 + 4 * V
    vol, feat_ref, loss_ref, gref, gr = _color_reference(V)
    assert gr.shape[1] == F and float(gr[:, 32:].abs().max()) > 0 and float(gref["nerf.pts_bias.weight"][:, 32:].abs().max()) > 0
    monkeypatch.setattr(ops, "VOLUME_BWD_DETERMINISTIC", deterministic)
    s = _scene(V, 48, 24, 77)
    args, net, qfn = _network(V, "v0", 24, color_vol=True)
    vol_g = models.RefVolume(vol.to(DEV))
    rgb, feat, w, depth, alpha, _ = _render(args, net, qfn, s, vol_g)
    assert float((feat.detach().cpu() - feat_ref).abs().max()) < 1e-5
    loss = _loss(rgb, depth, w, alpha, s["G"], DEV)
    assert abs(float(loss.detach()) - loss_ref) < 1e-3 * max(1.0, abs(loss_ref))
    loss.backward()
    gv = vol_g.feat_volume.grad
    assert gv.shape == (1, F, 16, 24, 32)
    errs = {"volume[0:8]": _rel(gv[:, :8], gr[:, :8]), "volume[8:32]": _rel(gv[:, 8:32], gr[:, 8:32]), f"volume[32:{F}]": _rel(gv[:, 32:], gr[:, 32:]),
            "volume": _rel(gv, gr)}
    named = dict(net.named_parameters())
    for name, p in named.items():
        errs[name] = _rel(p.grad, gref[name])
    errs["pts_bias.weight[:, 32:]"] = _rel(named["nerf.pts_bias.weight"].grad[:, 32:], gref["nerf.pts_bias.weight"][:, 32:])
    print(f"colour volume V={V} deterministic={deterministic}: worst {max(errs.values()):.2e}; max |ref| volume channels 32: {float(gr[:, 32:].abs().max()):.3e}, "
          f"all {float(gr.abs().max()):.3e}", {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < 2e-3}
    assert not bad, f"gradient mismatches: {bad}\nall: {errs}"


# ------------------------------------------------------------------ D
@functools.lru_cache(maxsize=None)
def _amp_reference(V, emulate):
    from oracle import mvsnerf_oracle as O
    s = _scene(V, 96, 32, AMP_SEED[V])
    sd = {k: v.clone().requires_grad_(True) for k, v in _sd_of(V, "v0").items()}
    vol_ref = s["vol"].clone().requires_grad_(True)
    feat = O.gen_pts_feats(s["imgs"], vol_ref, s["pts"], s["pose"], s["ndc"])
    angle = O.gen_dir_feature(s["pose"]["w2cs"][0], s["dirs"] / torch.norm(s["dirs"], dim=-1, keepdim=True))
    raw = _renderer_bf16_emulation(s["ndc"], angle, feat, sd) if emulate else O.run_network_mvs(s["ndc"], angle, feat, sd)
    rgb, _, _, w, depth, alpha = O.raw2outputs(raw, s["z"], False)
    loss = _loss(rgb, depth, w, alpha, s["G"])
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in sd.items()}, vol_ref.grad


@pytest.mark.parametrize("V", [7, 8])
def test_bf16_training_vs_torch_emulation_wide(V):
    from mvsnerf_amd import models, ops
    loss_e, g_e, vol_e = _amp_reference(V, True)
    loss_f, g_f, vol_f = _amp_reference(V, False)
    assert float(g_e["nerf.pts_bias.weight"][:, 32:].abs().max()) > 0
    # the loose bound below (0.15 against the fp32 oracle) measures what bf16 operands cost on a scene, which varies with the draw (0.08 .. 0.8 over
    # twenty seeds at V = 7 for the emulation itself); the scene is chosen, on the CPU references alone, so that the emulation keeps a third of it free
    gap = max([_rel(g_e[k], g_f[k]) for k in g_e] + [_rel(vol_e, vol_f)])
    print(f"bf16 training V={V}: the emulation against the fp32 oracle, worst gradient {gap:.3f}")
    assert gap < 0.10, gap
    s = _scene(V, 96, 32, AMP_SEED[V])
    args, net, qfn = _network(V, "v0", 32)
    vol_g = models.RefVolume(s["vol"].to(DEV))
    ops.set_mlp_precision("bf16")
    try:
        rgb, feat, w, depth, alpha, _ = _render(args, net, qfn, s, vol_g)
        loss = _loss(rgb, depth, w, alpha, s["G"], DEV)
        loss.backward()
    finally:
        ops.set_mlp_precision("fp32")
    for p in net.parameters():
        assert p.grad.dtype == torch.float32 and p.dtype == torch.float32          # fp32 master weights and gradients
    assert abs(float(loss.detach()) - loss_e) < 2e-3 * max(1.0, abs(loss_e)), (float(loss.detach()), loss_e)
    errs_e, errs_f = {"volume": _rel(vol_g.feat_volume.grad, vol_e)}, {"volume": _rel(vol_g.feat_volume.grad, vol_f)}
    named = dict(net.named_parameters())
    for name, p in named.items():
        errs_e[name], errs_f[name] = _rel(p.grad, g_e[name]), _rel(p.grad, g_f[name])
    hi = named["nerf.pts_bias.weight"].grad[:, 32:]
    errs_e["pts_bias.weight[:, 32:]"], errs_f["pts_bias.weight[:, 32:]"] = _rel(hi, g_e["nerf.pts_bias.weight"][:, 32:]), _rel(hi, g_f["nerf.pts_bias.weight"][:, 32:])
    print(f"bf16 training V={V}: max rel. gradient error vs bf16 emulation {max(errs_e.values()):.2e}, vs fp32 oracle {max(errs_f.values()):.2e}; "
          f"columns 32: {errs_e['pts_bias.weight[:, 32:]']:.2e} / {errs_f['pts_bias.weight[:, 32:]']:.2e}")
    bad = {k: v for k, v in errs_e.items() if not v < 5e-3}
    assert not bad, f"vs bf16 emulation: {bad}\nall: {errs_e}"
    bad = {k: v for k, v in errs_f.items() if not v < 0.15}
    assert not bad, f"vs fp32 oracle: {bad}\nall: {errs_f}"


# ------------------------------------------------------------------ E
@pytest.mark.parametrize("use_amp", [False, True])
def test_finetune_seven_source_views(use_amp):
    from mvsnerf_amd import train
    from mvsnerf_amd.synth import make_rig, pose_ref_of
    V = 7
    rig = make_rig(64, 96, n_views=V + 1, seed=9, baselines=BASELINES, smooth=True)
    pose = pose_ref_of(rig)
    src = (rig["images"][:, :V], rig["proj_mats"][:, :V], rig["near_fars"][0, 0], {k: v[:V] for k, v in pose.items()})
    args = train.default_args(pad=4, batch_size=256, N_samples=32, n_views=V, use_amp=use_amp)
    ft = train.MVSSystemFinetune(args, src, n_depth_planes=16).to(DEV)
    assert args.feat_dim == 36 and ft.volume.feat_volume.shape == (1, 8, 16, 24, 32)
    g = torch.Generator().manual_seed(1)
    rays = torch.cat([torch.zeros(256, 3), torch.nn.functional.normalize(torch.randn(256, 3, generator=g) * 0.05 + torch.tensor([0., 0., 1.]), dim=1),
                      torch.full((256, 1), 2.125), torch.full((256, 1), 4.525)], 1)
    batch = {"rays": rays[None], "rgbs": torch.rand(1, 256, 3, generator=g)}
    v0 = ft.volume.feat_volume.detach().clone()
    w0 = ft.network_fn.nerf.pts_bias.weight.detach().clone()
    torch.manual_seed(0)
    losses = ft.fit_steps([batch] * 8)
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
    assert float((ft.volume.feat_volume.detach() - v0).abs().max()) > 0
    assert float((ft.network_fn.nerf.pts_bias.weight.detach() - w0)[:, 32:].abs().max()) > 0         # the columns of the seventh view are trained
    rgb, depth = ft.render_rays(rays)
    assert rgb.shape == (256, 3) and depth.shape == (256,)
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(depth).all()) and float(rgb.std()) > 0
