"""Fine-tuning steps that skip empty space, on the GPU (csrc/sparse.hip compact_rows; ops.compact_rows / raymarch_sparse_train; the
args.skip_empty_train switch of MVSSystemFinetune and MVSSystemFusion).

1  compact_rows against the torch oracle: torch.equal, every row written, the range check seen inside memory the test owns.
2  The forward in fp32 and bf16: torch.equal with the dense training forward whose dead rows (the oracle's) are zeroed, and with ops.composite of that.
3  Gradients in fp32 against autograd through the reference with the dead rows of raw zeroed (tests/sparse_train_refs.py); the bounds are
   tests/test_gpu_train_wide_feat.py::test_gradients_of_rendering's: 1e-3 max(1, |loss|) on the loss, 2e-3 of max |ref| per tensor.
4  Gradients in bf16 (v0) against the masked bf16 emulation; the bounds are test_bf16_training_vs_torch_emulation_wide's tight leg: 2e-3 on the
   loss, 5e-3 per tensor.  Its loose leg against the fp32 oracle is not carried over: on the masked function the emulation's own distance to the
   fp32 oracle ranges from 0.09 to 4.2 over seeds 1..24 - it measures the draw, not the kernels.
5  Extremes: an all-one density against the dense rendering() step (bounds of 3), and thr = +inf (no live sample: background, exact zeros).
6  The systems: the switch on MVSSystemFinetune (fp32, use_amp) and MVSSystemFusion; without it the dense step, which never asks for live samples."""
import functools

import pytest
import torch

from tests import sparse_train_refs as T
from tests.sparse_train_refs import _scene, _loss, _rel
from tests.test_gpu_train_wide_feat import _args, BASELINES

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------ 1
def _compact_case(P, C, src, idx, count, n_rows):
    from mvsnerf_amd import ops
    want = T.compact_rows(src, idx, count, n_rows)
    d_src, d_idx, d_cnt = src.to(DEV), idx.to(DEV), torch.tensor([count], dtype=torch.int32, device=DEV)
    dst = torch.full((n_rows, C), float("nan"), device=DEV)
    with torch.no_grad():
        got = ops.compact_rows(d_src, d_idx, d_cnt, n_rows, out=dst)
        fresh = ops.compact_rows(d_src, d_idx, d_cnt, n_rows)
    assert got is dst and dst.shape == (n_rows, C)
    assert torch.equal(dst.cpu(), want), (P, C, count, n_rows)
    assert torch.equal(fresh.cpu(), want), (P, C, count, n_rows)


@pytest.mark.parametrize("P,C", [(1, 4), (1000, 4), (1025, 4), (2500, 1), (2048, 20)])
def test_compact_rows_equals_the_oracle(P, C):
    g = torch.Generator().manual_seed(P + C)
    src = torch.randn((P, C), generator=g)
    k = max(1, (3 * P) // 10)
    some = torch.sort(torch.randperm(P, generator=g)[:k])[0].to(torch.int32)
    every = torch.arange(P, dtype=torch.int32)
    _compact_case(P, C, src, some, 0, 0)                           # no destination row: nothing launched
    _compact_case(P, C, src, some, 0, k)                           # a zero count: every row zero
    _compact_case(P, C, src, some, k, k)                           # partial
    _compact_case(P, C, src, every, P, P)                          # full
    _compact_case(P, C, src, some, k // 2, k)                      # the device count below dst_rows: the tail rows are zero
    _compact_case(P, C, src, every, P, k)                          # ... and above: clamped to dst_rows


@pytest.mark.parametrize("P,C", [(1, 4), (1000, 4), (1025, 4), (2500, 1), (2048, 20)])
def test_compact_rows_checks_the_range_before_the_load(P, C):
    """src is rows [8, 8 + P) of a larger tensor filled with a sentinel: an unchecked idx of -1 or P would bring the sentinel back"""
    from mvsnerf_amd import ops
    g = torch.Generator().manual_seed(P * 3 + C)
    big = torch.full((P + 16, C), 777.0)
    big[8:8 + P] = torch.randn((P, C), generator=g)
    k = min(P, 40) + 4
    idx = torch.cat([torch.tensor([-1, P]), torch.randint(0, P, (k - 4,), generator=g), torch.tensor([P, -1])]).to(torch.int32)
    if k > P:                                                      # dst_rows <= P: one source row allows one destination row
        idx, k = torch.tensor([-1], dtype=torch.int32), 1
        also = torch.tensor([P], dtype=torch.int32)
    else:
        also = None
    d_big = big.to(DEV)
    src = d_big[8:8 + P]
    assert src.is_contiguous()
    for ix in [idx] + ([also] if also is not None else []):
        want = T.compact_rows(big[8:8 + P], ix, k, k)
        with torch.no_grad():
            got = ops.compact_rows(src, ix.to(DEV), torch.tensor([k], dtype=torch.int32, device=DEV), k).cpu()
        assert not bool((got == 777.0).any())
        bad = (ix < 0) | (ix >= P)
        assert bool(bad.any()) and not bool(got[bad].any())        # zero rows, not the neighbours
        assert torch.equal(got, want)
    assert torch.equal(d_big.cpu(), big)                           # nothing written to the source


# ------------------------------------------------------------------ scenes and networks
def _net(V, net_type, n_samples, white=False, color_vol=False):
    """(args, network, query function): tests/test_gpu_train_wide_feat.py:_network with the state dicts of tests/sparse_train_refs.py"""
    from mvsnerf_amd import models
    args = _args(8 + 4 * V, net_type, n_samples, white, color_vol)
    kw, _, _, _ = models.create_nerf_mvs(args, use_mvs=False, dir_embedder=False, pts_embedder=True)
    kw["network_fn"].load_state_dict(T.sd_of(V, net_type))
    return args, kw["network_fn"].to(DEV), kw["network_query_fn"]


@functools.lru_cache(maxsize=None)
def _dev_scene(V, n, s, seed):
    """the CPU scene's tensors on the device, in the order ops.raymarch_train / raymarch_sparse_train take them; shared, nobody writes to them"""
    sc = _scene(V, n, s, seed)
    t = lambda x: x.to(DEV).contiguous()
    return dict(imgs=t(sc["imgs"][0]), w2cs=t(sc["pose"]["w2cs"][:V]), Ks=t(sc["pose"]["intrinsics"][:V]), pts=t(sc["pts"]), ndc=t(sc["ndc"]), z=t(sc["z"]),
                dirs=t(sc["dirs"]), ro=t(sc["ro"]), pose={k: v.to(DEV) for k, v in sc["pose"].items()}, imgs5=sc["imgs"].to(DEV))


def _sparse(d, net, vol, density, thr, white, **over):
    from mvsnerf_amd import ops
    d = dict(d, **over)
    return ops.raymarch_sparse_train(vol, d["imgs"], d["w2cs"], d["Ks"], net, d["pts"], d["ndc"], d["z"], d["dirs"], density.to(DEV), thr, white_bkgd=white)


def _check_grads(net, vol_g, loss, loss_ref, gref, gvol_ref, loss_tol, tol, tag):
    assert abs(float(loss.detach()) - loss_ref) < loss_tol * max(1.0, abs(loss_ref)), (float(loss.detach()), loss_ref)
    loss.backward()
    errs = {"volume": _rel(vol_g.feat_volume.grad, gvol_ref)}
    named = dict(net.named_parameters())
    assert set(named) == set(gref) and len(named) == 22
    for name, p in named.items():
        assert p.grad.dtype == torch.float32 and p.dtype == torch.float32 and p.grad.shape == p.shape
        errs[name] = _rel(p.grad, gref[name])
    print(f"{tag}: loss {float(loss.detach()):.6f} (ref {loss_ref:.6f}); worst gradient {max(errs.values()):.2e}", {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < tol}
    assert not bad, f"gradient mismatches (rel. to max |ref|): {bad}\nall: {errs}"
    return errs


# ------------------------------------------------------------------ 2
def _forward_case(kind, n, s, white, mode):
    from mvsnerf_amd import ops
    V = 3
    colour = kind == "colour"
    net_type = "v0" if colour else kind
    sc = _scene(V, n, s, 5 + n)
    d = _dev_scene(V, n, s, 5 + n)
    live = T.live_of(sc)
    vol = (torch.cat([sc["vol"], torch.rand((1, 4 * V, *T.GRID), generator=torch.Generator().manual_seed(9))], 1) if colour else sc["vol"]).to(DEV)
    _, net, _ = _net(V, net_type, s, white, colour)
    with torch.no_grad(), ops.mlp_precision(mode):
        got = _sparse(d, net, vol, T.band(), 0.0, white)
        dense = ops.raymarch_train(vol, d["imgs"], d["w2cs"], d["Ks"], net, d["pts"], d["ndc"], d["z"], d["dirs"], white)["raw"]
        raw = torch.where(live.to(DEV)[..., None], dense, torch.zeros_like(dense))
        rgb, _, _, weights, depth, alpha = ops.composite(raw, d["z"], white)
    torch.cuda.synchronize()
    assert got["n_live"] == int(live.sum()) and 0 < got["n_live"] < n * s
    assert "input_feat" not in got and not got["raw"].requires_grad
    for k, want in (("raw", raw), ("rgb_map", rgb), ("weights", weights), ("depth", depth), ("alpha", alpha)):
        assert got[k].shape == want.shape, k
        assert torch.equal(got[k], want), (k, float((got[k] - want).abs().max()))
    assert float(got["raw"].abs().max()) > 0


@pytest.mark.parametrize("n,s,white", T.SHAPES[:2])
@pytest.mark.parametrize("kind", ["v0", "v2", "colour"])
def test_forward_equals_the_dense_training_forward_fp32(kind, n, s, white):
    _forward_case(kind, n, s, white, "fp32")


@pytest.mark.parametrize("n,s,white", T.SHAPES[:2])
def test_forward_equals_the_dense_training_forward_bf16(n, s, white):
    _forward_case("v0", n, s, white, "bf16")


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("V,n,s,white", [(3, *sh) for sh in T.SHAPES] + [(7, *T.SHAPES[0])])
@pytest.mark.parametrize("net_type", ["v0", "v2"])
def test_gradients_fp32(V, net_type, n, s, white):
    from mvsnerf_amd import models, ops
    loss_ref, gref, gvol_ref, live = T.masked_reference(V, net_type, n, s, white)
    sc, d = _scene(V, n, s, 5 + n), _dev_scene(V, n, s, 5 + n)
    _, net, _ = _net(V, net_type, s, white)
    vol_g = models.RefVolume(sc["vol"].to(DEV))
    with ops.mlp_precision("fp32"):
        o = _sparse(d, net, vol_g.feat_volume, T.band(), 0.0, white)
        assert o["n_live"] == int(live.sum())
        loss = _loss(o["rgb_map"], o["depth"], o["weights"], o["alpha"], sc["G"], DEV)
        errs = _check_grads(net, vol_g, loss, loss_ref, gref, gvol_ref, 1e-3, 2e-3, f"fp32 V={V} {net_type} ({n},{s},{white}) live {o['n_live']}/{n * s}")
    if V == 7:
        hi = _rel(dict(net.named_parameters())["nerf.pts_bias.weight"].grad[:, 32:], gref["nerf.pts_bias.weight"][:, 32:])
        assert hi < 2e-3, hi
    assert vol_g.feat_volume.grad.shape == (1, 8, *T.GRID) and errs


@pytest.mark.parametrize("deterministic", [False, True])
def test_gradients_colour_volume(deterministic, monkeypatch):
    from mvsnerf_amd import models, ops
    V = 3
    n, s, seed = T.COLOR_SCENE
    loss_ref, gref, gvol_ref, live = T.masked_color_reference(V)
    monkeypatch.setattr(ops, "VOLUME_BWD_DETERMINISTIC", deterministic)
    sc, d = _scene(V, n, s, seed), _dev_scene(V, n, s, seed)
    _, net, _ = _net(V, "v0", s, color_vol=True)
    vol_g = models.RefVolume(T.color_volume(V).to(DEV))
    with ops.mlp_precision("fp32"):
        o = _sparse(d, net, vol_g.feat_volume, T.band(), 0.0, False)
        assert o["n_live"] == int(live.sum())
        loss = _loss(o["rgb_map"], o["depth"], o["weights"], o["alpha"], sc["G"], DEV)
        _check_grads(net, vol_g, loss, loss_ref, gref, gvol_ref, 1e-3, 2e-3, f"colour volume deterministic={deterministic}")
    gv = vol_g.feat_volume.grad
    assert gv.shape == (1, 20, *T.GRID)
    assert _rel(gv[:, :8], gvol_ref[:, :8]) < 2e-3 and _rel(gv[:, 8:], gvol_ref[:, 8:]) < 2e-3


# ------------------------------------------------------------------ 4
def test_gradients_bf16():
    from mvsnerf_amd import models, ops
    n, s, seed = T.AMP_SCENE
    loss_ref, gref, gvol_ref, live = T.masked_amp_reference()
    sc, d = _scene(3, n, s, seed), _dev_scene(3, n, s, seed)
    _, net, _ = _net(3, "v0", s)
    vol_g = models.RefVolume(sc["vol"].to(DEV))
    with ops.mlp_precision("bf16"):
        o = _sparse(d, net, vol_g.feat_volume, T.band(), 0.0, False)
        assert o["n_live"] == int(live.sum())
        loss = _loss(o["rgb_map"], o["depth"], o["weights"], o["alpha"], sc["G"], DEV)
        _check_grads(net, vol_g, loss, loss_ref, gref, gvol_ref, 2e-3, 5e-3, f"bf16 live {o['n_live']}/{n * s}")
    assert vol_g.feat_volume.grad.dtype == torch.float32


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("net_type", ["v0", "v2"])
def test_all_one_density_is_the_dense_step(net_type):
    from mvsnerf_amd import models, ops, renderer
    V, (n, s, white) = 3, T.SHAPES[0]
    sc, d = _scene(V, n, s, 5 + n), _dev_scene(V, n, s, 5 + n)
    inside = d["ndc"].clamp(0, 1).contiguous()                     # a sample outside the grid has no in-grid corner: dead whatever the density
    args, net_d, qfn = _net(V, net_type, s, white)
    vol_d = models.RefVolume(sc["vol"].to(DEV))
    _, net_s, _ = _net(V, net_type, s, white)
    vol_s = models.RefVolume(sc["vol"].to(DEV))
    with ops.mlp_precision("fp32"):
        rgb, _, w, depth, alpha, _ = renderer.rendering(args, d["pose"], d["pts"], inside, d["z"], d["ro"], d["dirs"], vol_d, d["imgs5"], network_fn=net_d,
                                                        network_query_fn=qfn, white_bkgd=white)
        loss_d = _loss(rgb, depth, w, alpha, sc["G"], DEV)
        loss_d.backward()
        o = _sparse(d, net_s, vol_s.feat_volume, torch.ones(T.GRID), 0.0, white, ndc=inside)
        assert o["n_live"] == n * s
        loss_s = _loss(o["rgb_map"], o["depth"], o["weights"], o["alpha"], sc["G"], DEV)
        gref = {k: p.grad.cpu() for k, p in net_d.named_parameters()}
        _check_grads(net_s, vol_s, loss_s, float(loss_d.detach()), gref, vol_d.feat_volume.grad.cpu(), 1e-3, 2e-3, f"all-one density {net_type}")
    same = all(torch.equal(p.grad, q.grad) for p, q in zip(net_s.parameters(), net_d.parameters()))
    print(f"all-one density {net_type}: forward bit-equal {torch.equal(o['rgb_map'], rgb)}, MLP gradients bit-equal {same}, "
          f"volume gradient bit-equal {torch.equal(vol_s.feat_volume.grad, vol_d.feat_volume.grad)}")


@pytest.mark.parametrize("white", [False, True])
def test_no_live_sample(white):
    from mvsnerf_amd import models, ops
    V, (n, s, _) = 3, T.SHAPES[0]
    sc, d = _scene(V, n, s, 5 + n), _dev_scene(V, n, s, 5 + n)
    assert bool(torch.isfinite(sc["ndc"]).all())
    _, net, _ = _net(V, "v0", s, white)
    vol_g = models.RefVolume(sc["vol"].to(DEV))
    with ops.mlp_precision("fp32"):
        o = _sparse(d, net, vol_g.feat_volume, T.band(), float("inf"), white)
        assert o["n_live"] == 0 and not bool(o["raw"].any()) and o["raw"].shape == (n, s, 4)
        assert torch.equal(o["rgb_map"], torch.full((n, 3), 1.0 if white else 0.0, device=DEV))           # the background
        assert not bool(o["weights"].any()) and not bool(o["alpha"].any()) and not bool(o["depth"].any())
        loss = _loss(o["rgb_map"], o["depth"], o["weights"], o["alpha"], sc["G"], DEV)
        loss.backward()                                            # raises nothing
    gv = vol_g.feat_volume.grad
    assert gv.shape == (1, 8, *T.GRID) and not bool(gv.any())
    params = list(net.parameters())
    assert len(params) == 22
    for p in params:
        assert p.grad is not None and p.grad.shape == p.shape and not bool(p.grad.any())


# ------------------------------------------------------------------ 6
def _finetune(use_amp, **switch):
    """tests/test_gpu_train_wide_feat.py::test_finetune_seven_source_views' 64 x 96 rig and batch at V = 3"""
    from mvsnerf_amd import train
    from mvsnerf_amd.synth import make_rig, pose_ref_of
    V = 3
    rig = make_rig(64, 96, n_views=V + 1, seed=9, baselines=BASELINES, smooth=True)
    pose = pose_ref_of(rig)
    src = (rig["images"][:, :V], rig["proj_mats"][:, :V], rig["near_fars"][0, 0], {k: v[:V] for k, v in pose.items()})
    args = train.default_args(pad=4, batch_size=256, N_samples=32, n_views=V, use_amp=use_amp, **switch)
    ft = train.MVSSystemFinetune(args, src, n_depth_planes=16).to(DEV)
    g = torch.Generator().manual_seed(1)
    rays = torch.cat([torch.zeros(256, 3), torch.nn.functional.normalize(torch.randn(256, 3, generator=g) * 0.05 + torch.tensor([0., 0., 1.]), dim=1),
                      torch.full((256, 1), 2.125), torch.full((256, 1), 4.525)], 1)
    return ft, {"rays": rays[None], "rgbs": torch.rand(1, 256, 3, generator=g)}


def _counting(monkeypatch, name, log):
    from mvsnerf_amd import ops
    orig = getattr(ops, name)

    def wrapped(*a, **kw):
        log.append(kw.get("dilate"))
        return orig(*a, **kw)
    monkeypatch.setattr(ops, name, wrapped)


@pytest.mark.parametrize("use_amp", [False, True])
def test_finetune_with_the_switch(use_amp, monkeypatch):
    ft, batch = _finetune(use_amp, skip_empty_train=0.0, skip_empty_dilate=1, skip_empty_refresh=4)
    builds, steps = [], []
    _counting(monkeypatch, "node_density", builds)
    from mvsnerf_amd import ops
    orig = ops.raymarch_sparse_train

    def spy(*a, **kw):
        steps.append((ft.global_step, len(builds), ft.train_density.data_ptr()))
        return orig(*a, **kw)
    monkeypatch.setattr(ops, "raymarch_sparse_train", spy)
    v0 = ft.volume.feat_volume.detach().clone()
    w0 = ft.network_fn.nerf.pts_bias.weight.detach().clone()
    torch.manual_seed(0)
    losses = ft.fit_steps([batch] * 8)
    print(f"use_amp={use_amp}: losses {[round(l, 5) for l in losses]}, last live fraction {ft.last_live_fraction:.3f}")
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses[-1] < losses[0], losses
    assert 0 < ft.last_live_fraction <= 1
    assert builds == [1, 1]                                                                     # dilate = 1, twice:
    assert [(st, nb) for st, nb, _ in steps] == [(0, 1), (1, 1), (2, 1), (3, 1), (4, 2), (5, 2), (6, 2), (7, 2)]       # at steps 0 and 4
    assert tuple(ft.train_density.shape) == tuple(ft.volume.feat_volume.shape[-3:]) and ft.train_density.dtype == torch.float32
    assert ft.density_volume is None
    assert float((ft.volume.feat_volume.detach() - v0).abs().max()) > 0
    assert float((ft.network_fn.nerf.pts_bias.weight.detach() - w0).abs().max()) > 0


def test_finetune_without_the_switch_is_the_dense_step(monkeypatch):
    ft, batch = _finetune(False)
    calls = []
    _counting(monkeypatch, "live_samples", calls)
    _counting(monkeypatch, "node_density", calls)
    torch.manual_seed(0)
    losses = ft.fit_steps([batch] * 2)
    assert all(l == l for l in losses) and calls == []
    assert getattr(ft, "train_density", None) is None and not hasattr(ft, "last_live_fraction")


def test_fused_system_with_the_switch(monkeypatch):
    from mvsnerf_amd import ops
    from tests.test_gpu_fusion import fusion_views, fusion_system
    monkeypatch.setattr(ops, "MLP_PRECISION", "fp32")
    views, bbox, img_wh, focal = fusion_views()
    sysm, _ = fusion_system(views, bbox, img_wh, focal)
    splat = sysm.density_volume.clone()
    assert splat.shape == (1, 1, 10, 12, 14)
    sysm.args.skip_empty_train, sysm.args.skip_empty_dilate, sysm.args.skip_empty_refresh = 0.0, 1, 200
    from mvsnerf_amd import train
    g = torch.Generator().manual_seed(3)
    ro, rd = train.get_rays(train.get_ray_directions(64, 96, focal), views[1][4])
    pick = torch.randperm(ro.shape[0], generator=g)[:128]
    rays = torch.cat([ro[pick], rd[pick], torch.full((128, 1), 2.125), torch.full((128, 1), 4.525)], 1)
    batch = {"rays": rays[None], "rgbs": torch.rand((1, 128, 3), generator=g)}
    torch.manual_seed(4)
    opt = sysm.configure_optimizers()[0][0]
    losses = []
    for i in range(2):
        opt.zero_grad(set_to_none=True)
        out = sysm.training_step(batch, i)
        out["loss"].backward()
        opt.step()
        sysm.global_step += 1
        losses.append(float(out["loss"].detach()))
    print(f"fused system: losses {losses}, live fraction {sysm.last_live_fraction:.3f}")
    assert all(l == l and abs(l) != float("inf") for l in losses)
    assert 0 <= sysm.last_live_fraction <= 1
    assert tuple(sysm.train_density.shape) == (10, 12, 14)
    assert sysm.density_volume.shape == (1, 1, 10, 12, 14) and torch.equal(sysm.density_volume, splat)
    assert all(l.weight.grad is not None for l in sysm.network_fn.nerf._linears())
