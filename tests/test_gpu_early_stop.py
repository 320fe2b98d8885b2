"""Early ray termination on the GPU (csrc/sparse.hip's ray_transmittance / live_samples_range / scatter_rows, ops.raymarch_early_stop,
the systems' early_stop= keyword).

Yardsticks: a decided ray (tests/early_stop_refs.py) has the bits of ops.composite of the dense raw with the restatement's rows zeroed; against the
call without early_stop the frame moves by at most eps (+ S 2^-22 for the fp32 rounding of the two S-term sums), the depth by that times max|z|.

The scene is tests/test_gpu_sparse_render.py's; the networks' alpha_linear.bias is raised by the constants of BIAS so that rays do saturate.  Sigma is
relu(alpha_linear) and a uniform shift moves every ray of a shape together, so the constant that leaves a quarter of the rays on either side of
eps = 1e-2 depends on how many samples stand in front of the boundaries: one constant per (case, shape), chosen on the float64 transmittance of the
dense raw (v0: the CPU oracle's; the others: the dense launch sequence's, swept from 0 to 3).  _mixed() asserts the outcome wherever a constant is
used.  The shipped v0 network - the test network - meets all three conditions of non-vacuity (a quarter of the rays stop, at two or more boundaries, a
quarter never stop) on both shapes, and so do v2 on (37, 24) and the band density on (1030, 40).  On the other (case, shape) pairs no constant of the
sweep does: the seeded v2 / wide networks and the random colour volume give rays that are too much alike, and a shift that stops a quarter of them at
two boundaries stops nearly all of them.  Those pairs (strict = False in BIAS) assert what their best constant gives: some rays stop, some never do."""
import functools

import pytest
import torch

from tests import early_stop_refs as E
from tests import sparse_refs as R
from tests.test_gpu_sparse_render import GRID, _band, _dense, _rays

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-2
SHAPES = [(37, 24, 8), (1030, 40, 16)]          # (N, S, stop_every): three segments, N no multiple of 64 | across the 1024-sample compaction tile, short last segment
ONE_SEGMENT = (5, 7, 32)                        # stop_every > S: a single segment, equal to dense
# alpha_linear.bias += BIAS[kind][(N, S)]; "band": with the density of _band() (planes 4..8 occupied) only the band's samples carry sigma
# (constant, strict): what the sweep gave at eps = 1e-2, as rays that never stop / stop at the first / at the second boundary
BIAS = {"v0": {(37, 24): (0.25, True), (1030, 40): (0.05, True)},                    # 20 / 1 / 16 of 37; 600 / 83 / 347 of 1030
        "v2": {(37, 24): (0.0, True), (1030, 40): (0.0, False)},                      # 11 / 13 / 13; 104 / 744 / 182
        "wide": {(37, 24): (0.25, False), (1030, 40): (0.1, False)},                  # 24 / 0 / 13; 844 / 0 / 186
        "colour": {(37, 24): (0.0, False), (1030, 40): (0.0, False)},                 # 5 / 14 / 18; 31 / 755 / 244
        "band": {(37, 24): (0.5, False), (1030, 40): (0.3, True)}}                    # 16 / 0 / 21; 365 / 50 / 615
KEYS = ("raw", "rgb_map", "weights", "depth", "alpha", "disp", "acc")


@functools.lru_cache(maxsize=None)
def _net(kind, c):
    """(packed for the fp32 mode, model | None) of tests/test_gpu_sparse_render._net's networks with alpha_linear.bias raised by c (fresh objects: that
    module's cached networks stay as they are)."""
    from mvsnerf_amd import models, ops
    from tests.util import load_weights
    if kind == "wide":
        from tests import wide_refs
        ws, bs = wide_refs.weights(20)
        bs = list(bs)
        bs[8] = bs[8] + c                                            # ops.MLP_ORDER: alpha_linear
        return ops.mlp_pack_wide([w.to(DEV) for w in ws], [b.to(DEV) for b in bs], 20, wide_refs.WIDE, 0), None
    m = models.MVSNeRF(D=6, W=128, input_ch_pts=63, input_ch_views=3, input_ch_feat=20, skips=[4], net_type=kind)
    if kind == "v0":
        m.load_state_dict(load_weights()[0])
    else:
        torch.manual_seed(20)
        for p in m.parameters():
            torch.nn.init.uniform_(p, -0.15, 0.15)
    with torch.no_grad():
        m.nerf.alpha_linear.bias += c
    m = m.to(DEV)
    with ops.mlp_precision("fp32"):
        return m.packed(20), m


def _case(case, N, S):
    """case -> (network kind, colour volume?, density | None, thr | None, bias, strict)"""
    kind = case if case in ("v0", "v2", "wide") else "v0"
    density, thr = (_band(), 0.0) if case == "band" else (None, None)
    return (kind, case == "colour", density, thr, *BIAS[case].get((N, S), (0.25, False)))


def _dense_run(x, packed, density, thr, white, colour, **alt):
    """The march without early_stop as tests/test_gpu_sparse_render._dense spells it (gather -> mlp_forward on all N*S samples -> dead rows zeroed ->
    composite); without a density every sample is live."""
    if density is None:
        density, thr = torch.ones(GRID), -1.0
    return _dense(x, packed, density, thr, white, colour, **alt)[0]


def _early(x, packed, eps, G, density, thr, white, colour, **alt):
    from mvsnerf_amd import ops
    vol = x["cvol_cl"] if colour else x["vol_cl"]
    kw = {} if density is None else dict(density=density.to(DEV), thr=thr)
    return ops.raymarch_early_stop(vol, None if colour else x["imgs"], x["w2cs"], None if colour else x["Ks"], packed, x["pts"], x["ndc"], x["z"], x["dirs"],
                                   eps, stop_every=G, white_bkgd=white, want=("disp", "acc"), **kw, **alt)


def _mixed(raw, eps, G, strict=True):
    """The test is not vacuous: on the float64 T of the dense raw at least a quarter of the rays stop, at two or more different boundaries, at least a
    quarter never stop (strict; otherwise: some stop, some never do), and at most 2 % are undecided.  Returns the restatement's (zeroed raw, stop,
    undecided)."""
    zeroed, stop, und = E.early_stop(raw, eps, G)
    N = raw.shape[0]
    n_stop, n_go, where = int((stop >= 0).sum()), int((stop < 0).sum()), sorted(set(stop[stop >= 0].tolist()))
    print(f"(N,S)={tuple(raw.shape[:2])} G={G} eps={eps}: {n_stop} rays stop at boundaries {where}, {n_go} never, {int(und.sum())} undecided")
    assert n_stop > 0 and n_go > 0 and 50 * int(und.sum()) <= N
    if strict:
        assert 4 * n_stop >= N and 4 * n_go >= N and len(where) >= 2
    return zeroed, stop, und


def _check_exact(case, N, S, G, white=False):
    from mvsnerf_amd import ops
    kind, colour, density, thr, c, strict = _case(case, N, S)
    x, (packed, _) = _rays(N, S), _net(kind, c)
    with torch.no_grad(), ops.mlp_precision("fp32"):
        dense = _dense_run(x, packed, density, thr, white, colour)
        got = _early(x, packed, EPS, G, density, thr, white, colour)
        zeroed, stop, und = _mixed(dense["raw"], EPS, G, strict)
        rgb, disp, acc, weights, depth, alpha = ops.composite(zeroed.contiguous(), x["z"], white)
    want = {"raw": zeroed, "rgb_map": rgb, "disp": disp, "acc": acc, "weights": weights, "depth": depth, "alpha": alpha}
    ok = ~und
    for k in KEYS:
        assert got[k].shape == want[k].shape, k
        assert torch.equal(got[k][ok], want[k][ok]), (k, float((got[k][ok] - want[k][ok]).abs().max()))
    if not bool(und.any()):
        assert got["n_stopped"] == int((stop >= 0).sum())
        sent = torch.ones((N, S), dtype=torch.bool, device=DEV) if density is None else R.live_mask(density, x["ndc"].cpu(), thr).to(DEV).view(N, S)
        s = torch.arange(S, device=DEV)[None]
        assert got["n_live"] == int((sent & ~((stop[:, None] >= 0) & (s >= stop[:, None]))).sum())
    assert 0 < got["n_live"] < N * S and 0 < got["n_stopped"] < N


# ------------------------------------------------------------------ A. ops.raymarch_early_stop: decided rays have the bits of the restatement
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("N,S,G", SHAPES)
def test_early_stop_v0_equals_the_restatement(N, S, G, white):
    _check_exact("v0", N, S, G, white)


@pytest.mark.parametrize("N,S,G", SHAPES)
@pytest.mark.parametrize("case", ["v2", "wide", "colour", "band"])
def test_early_stop_other_networks_colour_volume_and_density(case, N, S, G):
    _check_exact(case, N, S, G)


@pytest.mark.parametrize("N,S,G", SHAPES + [ONE_SEGMENT])
def test_eps_zero_equals_raymarch(N, S, G):
    from mvsnerf_amd import ops
    x, (packed, _) = _rays(N, S), _net("v0", BIAS["v0"].get((N, S), (0.25,))[0])
    with torch.no_grad(), ops.mlp_precision("fp32"):
        want = ops.raymarch(x["vol_cl"], x["imgs"], x["w2cs"], x["Ks"], packed, x["pts"], x["ndc"], x["z"], x["dirs"], want=("disp", "acc"))
        got = _early(x, packed, 0.0, G, None, None, False, False)
        one = _early(x, packed, EPS, S + 5, None, None, False, False)               # a single segment stops nothing, whatever eps is
    assert got["n_stopped"] == 0 and got["n_live"] == N * S and one["n_stopped"] == 0 and one["n_live"] == N * S
    for k in KEYS:
        assert torch.equal(got[k], want[k]), (k, float((got[k] - want[k]).abs().max()))
        assert torch.equal(one[k], want[k]), k


@pytest.mark.parametrize("N,S,G", SHAPES)
def test_eps_zero_with_density_equals_raymarch_sparse(N, S, G):
    from mvsnerf_amd import ops
    x, (packed, _) = _rays(N, S), _net("v0", BIAS["band"][(N, S)][0])
    with torch.no_grad(), ops.mlp_precision("fp32"):
        want = ops.raymarch_sparse(x["vol_cl"], x["imgs"], x["w2cs"], x["Ks"], packed, x["pts"], x["ndc"], x["z"], x["dirs"], _band().to(DEV), 0.0,
                                   want=("disp", "acc"))
        got = _early(x, packed, 0.0, G, _band(), 0.0, False, False)
    assert got["n_stopped"] == 0 and got["n_live"] == want["n_live"]
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k


# ------------------------------------------------------------------ B. the bound against the call without early_stop
def _check_bound(got, dense, z, eps, S):
    tol = eps + S * 2.0 ** -22
    e_rgb, e_acc = float((got["rgb_map"] - dense["rgb_map"]).abs().max()), float((got["acc"] - dense["acc"]).abs().max())
    e_depth, zmax = float((got["depth"] - dense["depth"]).abs().max()), float(z.abs().max())
    print(f"eps {eps}: max |rgb diff| {e_rgb:.3g}, |acc diff| {e_acc:.3g} (bound {tol:.3g}); |depth diff| {e_depth:.3g} (bound {tol * zmax:.3g})")
    assert e_rgb <= tol and e_acc <= tol and e_depth <= tol * zmax


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("eps", [1e-3, 1e-2])
@pytest.mark.parametrize("N,S,G", SHAPES)
def test_bound_against_the_dense_frame(N, S, G, eps, white):
    from mvsnerf_amd import ops
    x, (packed, _) = _rays(N, S), _net("v0", BIAS["v0"][(N, S)][0])
    with torch.no_grad(), ops.mlp_precision("fp32"):
        dense = _dense_run(x, packed, None, None, white, False)
        got = _early(x, packed, eps, G, None, None, white, False)
    assert got["n_stopped"] > 0 or eps < EPS                                            # BIAS was chosen at EPS
    _check_bound(got, dense, x["z"], eps, S)


@pytest.mark.parametrize("eps", [1e-3, 1e-2])
@pytest.mark.parametrize("N,S,G", SHAPES)
def test_bound_in_auto_mode_against_the_dense_auto_frame(N, S, G, eps):
    from mvsnerf_amd import ops
    x, (_, m) = _rays(N, S), _net("v0", BIAS["v0"][(N, S)][0])
    with torch.no_grad(), ops.mlp_precision("auto"):
        n0 = ops.guard_fallbacks()
        alt = m.packed_alt(20)
        assert "guard" in alt
        dense = _dense_run(x, m.packed(20), None, None, False, False, **alt)
        got = _early(x, m.packed(20), eps, G, None, None, False, False, **alt)
        assert ops.guard_fallbacks() == n0
    assert got["n_stopped"] > 0 or eps < EPS                                            # BIAS was chosen at EPS
    _check_bound(got, dense, x["z"], eps, S)


# ------------------------------------------------------------------ C. the kernels against torch
@functools.lru_cache(maxsize=None)
def _raw(N, S):
    g = torch.Generator().manual_seed(N + S)
    raw = torch.rand((N, S, 4), generator=g)
    raw[..., 3] = torch.empty((N, S)).exponential_(1.0, generator=g) * (6.0 / S)          # rays saturate around the middle of the ray
    return raw


@pytest.mark.parametrize("N,S,s0,s1", [(37, 24, 0, 8), (37, 24, 8, 24), (1030, 40, 16, 32), (5, 7, 3, 4), (300, 128, 0, 128)])
def test_ray_transmittance_against_float64(N, S, s0, s1):
    from mvsnerf_amd import ops
    raw = _raw(N, S)
    start = torch.rand((N,), generator=torch.Generator().manual_seed(1)) + 0.5
    f = (1.0 - (1.0 - torch.exp(-raw[:, s0:s1, 3].double()))) + 1e-10
    want = start.double() * f.prod(1)
    runs = []
    for _ in range(2):
        T = start.clone().to(DEV)
        with torch.no_grad():
            assert ops.ray_transmittance(raw.to(DEV), s0, s1, T) is T
        runs.append(T.cpu())
    rel = float(((runs[0].double() - want).abs() / want).max())
    print(f"(N,S)=({N},{S}) window [{s0},{s1}): max relative error {rel:.3g}, allowed {(s1 - s0) * 2.0 ** -22:.3g}")
    assert rel <= (s1 - s0) * 2.0 ** -22
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))


def test_ray_transmittance_order_and_nan():
    """Consecutive windows give the bits of one left-to-right fp32 product; a NaN sigma gives a NaN transmittance for its ray alone."""
    from mvsnerf_amd import ops
    N, S = 37, 24
    raw = _raw(N, S).clone()
    raw[3, 10, 3] = float("nan")
    f = (1.0 - (1.0 - torch.exp(-raw[..., 3]))) + 1e-10                                  # fp32: the factor may differ from expf's in the last bit
    d = raw.to(DEV)
    whole, parts = torch.ones(N, device=DEV), torch.ones(N, device=DEV)
    with torch.no_grad():
        ops.ray_transmittance(d, 0, S, whole)
        for s0, s1 in ((0, 8), (8, 9), (9, 16), (16, 24)):
            ops.ray_transmittance(d, s0, s1, parts)
    assert torch.equal(whole.view(torch.int32), parts.view(torch.int32))
    assert bool(torch.isnan(whole[3])) and int(torch.isnan(whole).sum()) == 1
    seq = torch.ones(N)
    for s in range(S):
        seq = seq * f[:, s]
    ok = ~torch.isnan(seq)
    assert float(((whole.cpu()[ok] - seq[ok]).abs() / seq[ok]).max()) <= S * 2.0 ** -22


def _check_range(density, ndc, thr, s0, s1, ray_T, eps, pts, dirs):
    from mvsnerf_amd import ops
    N, S = ndc.shape[:2]
    sel = torch.zeros((N, S), dtype=torch.bool)
    sel[:, s0:s1] = True
    if ray_T is not None:
        sel &= ~(ray_T < torch.tensor(eps, dtype=torch.float32))[:, None]
    if density is not None:
        sel &= R.live_mask(density, ndc, thr).view(N, S)
    idx = torch.nonzero(sel.reshape(-1)).reshape(-1)
    n = idx.numel()
    d = lambda t: None if t is None else t.to(DEV)
    runs = []
    for _ in range(2):
        with torch.no_grad():
            runs.append(ops.live_samples_range(d(density), d(ndc), thr, s0, s1, d(ray_T), eps, d(pts), d(dirs)))
    for count, gidx, ndc_c, pts_c, dir_c in runs:
        assert count.dtype == torch.int32 and gidx.dtype == torch.int32 and int(count.item()) == n, (int(count.item()), n)
        assert gidx.numel() == N * (s1 - s0) and torch.equal(gidx[:n].cpu().long(), idx)
        assert torch.equal(ndc_c[:n].cpu().view(torch.int32), ndc.reshape(-1, 3)[idx].contiguous().view(torch.int32))
        assert (pts_c is None) == (pts is None) and (dir_c is None) == (dirs is None)
        if pts is not None:
            assert torch.equal(pts_c[:n].cpu(), pts.reshape(-1, 3)[idx])
        if dirs is not None:
            assert torch.equal(dir_c[:n].cpu(), dirs[idx // S])
    return n


@pytest.mark.parametrize("N,S,s0,s1", [(37, 24, 8, 16), (1030, 40, 32, 40), (1030, 40, 0, 16), (5, 7, 0, 7), (2100, 128, 0, 128)])
def test_live_samples_range_against_nonzero(N, S, s0, s1):
    """(2100, 128) over the whole ray: 263 workgroup counts, the scan's threads own runs of two."""
    from tests.test_gpu_sparse_render import _live_case
    grid = R.GRIDS[1]
    density, ndc, pts, dirs = _live_case(grid, N, S)
    ray_T = torch.rand((N,), generator=torch.Generator().manual_seed(N))
    ray_T[::7] = float("nan")                                                           # a NaN transmittance never stops its ray
    W = N * (s1 - s0)
    n = _check_range(density, ndc, 0.5, s0, s1, ray_T, 0.5, pts, dirs)
    assert 0 < n < W
    assert 0 < _check_range(None, ndc, 0.0, s0, s1, ray_T, 0.5, pts, dirs) < W          # early_stop alone: no density
    assert 0 < _check_range(density, ndc, 0.5, s0, s1, None, 0.5, None, dirs) < W       # segment 0: no ray_T; a colour volume: no world points
    assert _check_range(None, ndc, 0.0, s0, s1, None, 0.0, None, None) == W             # the whole window
    assert _check_range(None, ndc, 0.0, s0, s1, torch.zeros(N), 0.5, pts, dirs) == 0    # every ray dead
    assert _check_range(None, ndc, 0.0, s0, s1, torch.zeros(N), 0.0, pts, dirs) == W    # eps = 0 stops nothing: T < 0 never holds


@pytest.mark.parametrize("C", [1, 4])
def test_scatter_rows_leaves_other_rows_untouched(C):
    from mvsnerf_amd import ops
    P = 2500
    g = torch.Generator().manual_seed(C)
    mixed = torch.sort(torch.randperm(P, generator=g)[:777])[0]
    wild = mixed.clone()
    wild[5], wild[400] = -3, P                                                          # out of range: ignored
    for idx64, count in ((mixed, 777), (mixed, 300), (wild, 777), (torch.tensor([1500]), 1), (torch.arange(P), P), (mixed, 0)):
        n = idx64.numel()
        src, before = torch.randn((n, C), generator=g), torch.randn((P, C), generator=g)
        before[7] = float("nan")
        want = before.clone()
        keep = (idx64[:count] >= 0) & (idx64[:count] < P)
        want[idx64[:count][keep]] = src[:count][keep]
        outs = []
        for _ in range(2):
            dst = before.clone().to(DEV)
            with torch.no_grad():
                assert ops.scatter_rows(src.to(DEV), idx64.to(torch.int32).to(DEV), torch.tensor([count], dtype=torch.int32).to(DEV), dst) is dst
            outs.append(dst.cpu())
        assert torch.equal(outs[0].view(torch.int32), want.view(torch.int32)), (C, n, count)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


# ------------------------------------------------------------------ D. the systems (64 x 96 source views, 16 planes)
# alpha_linear.bias of the systems' v0 network, swept like BIAS on the two fractions.  0.3: 32 samples, stop_every 8 - render_view stops 46 % of its
# rays, render_rays 82 %; 0.2 with importance sampling (48 samples, stop_every 16): 85 %; 0.5 for the fused scene (16 samples, stop_every 4): 60 %
SYSTEM_BIAS = 0.3


def _raise_sigma(net, c=SYSTEM_BIAS):
    with torch.no_grad():
        net.nerf.alpha_linear.bias += c


def _check_frames(render, zmax, eps, S, sysm, n_rays):
    """render(**kw) -> (rgb, depth): the early_stop frame lies within the bound of the default call, does not depend on batch_rays, and the two
    fractions say that samples were saved and that some rays, not all, were stopped."""
    from mvsnerf_amd import ops
    tol = eps + S * 2.0 ** -22
    with torch.no_grad(), ops.mlp_precision("fp32"):
        dense_rgb, dense_depth = render()
        rgb, depth = render(early_stop=eps, batch_rays=1000)
        live, stopped = sysm.last_live_fraction, sysm.last_stopped_fraction
        rgb2, depth2 = render(early_stop=eps, batch_rays=max(n_rays // 3 + 1, 1))
        stopped2 = sysm.last_stopped_fraction
    e_rgb, e_depth = float((rgb - dense_rgb).abs().max()), float((depth - dense_depth).abs().max())
    print(f"live fraction {live:.4f}, stopped fraction {stopped:.4f}; max |rgb diff| {e_rgb:.3g} (bound {tol:.3g}), |depth diff| {e_depth:.3g} "
          f"(bound {tol * zmax:.3g})")
    assert rgb.shape == dense_rgb.shape and depth.shape == dense_depth.shape
    assert e_rgb <= tol and e_depth <= tol * zmax
    assert torch.equal(rgb, rgb2) and torch.equal(depth, depth2) and stopped == stopped2
    assert live < 1.0 and 0.0 < stopped < 1.0


def test_render_view_early_stop():
    from mvsnerf_amd import train
    from tests.util import load_weights
    mlp_sd, mvs_sd = load_weights()
    s = train.MVSSystem(train.default_args(pad=4, batch_size=64, N_samples=32, chunk=1024), n_depth_planes=16)
    s.render_kwargs_train["network_fn"].load_state_dict(mlp_sd)
    s.MVSNet.load_state_dict(mvs_sd)
    _raise_sigma(s.render_kwargs_train["network_fn"])
    s = s.to(DEV)
    batch = train.synthetic_batch(64, 96, seed=8, smooth=True)
    vol = s.encode_scene(batch)
    _, pose = s.decode_batch(dict(batch))
    zmax = float(pose["near_fars"].max())
    _check_frames(lambda **kw: s.render_view(batch, volume=vol, **({"stop_every": 8, **kw} if kw else {})), zmax, EPS, 32, s, 64 * 96)


def test_finetune_render_rays_early_stop_with_skip_empty():
    from tests.test_gpu_finetune_render import _system, _rays as scene_rays
    ft, _, _ = _system(V=3)
    _raise_sigma(ft.network_fn)
    ft.update_density_volume()
    rays = scene_rays(2500)
    zmax = float(rays[:, 7].max())

    def render(**kw):
        return ft.render_rays(rays, skip_empty=0.0, **({"stop_every": 8, **kw} if kw else {}))
    _check_frames(render, zmax, EPS, 32, ft, 2500)
    from mvsnerf_amd import ops
    with torch.no_grad(), ops.mlp_precision("fp32"):                                    # early_stop alone reads no density volume
        ft.density_volume = None
        alone, _ = ft.render_rays(rays, early_stop=EPS, stop_every=8)
        dense, _ = ft.render_rays(rays)
    assert float((alone - dense).abs().max()) <= EPS + 32 * 2.0 ** -22 and 0.0 < ft.last_stopped_fraction < 1.0


def test_finetune_render_rays_early_stop_with_importance_sampling():
    """N_importance > 0: the merged depths are a larger S (32 + 16 = 48 samples, stop_every 16: three segments)."""
    from mvsnerf_amd import ops
    from tests.test_gpu_finetune_render import _system, _rays as scene_rays
    ft, _, _ = _system(V=3, N_importance=16)
    _raise_sigma(ft.network_fn, 0.2)
    ft.update_density_volume()
    rays = scene_rays(1500, seed=3)
    u = torch.rand((1500, 16), generator=torch.Generator().manual_seed(5))
    with torch.no_grad(), ops.mlp_precision("fp32"):
        dense_rgb, dense_depth = ft.render_rays(rays, u=u)
        rgb, depth = ft.render_rays(rays, u=u, early_stop=EPS, stop_every=16, batch_rays=1000)
    tol = EPS + 48 * 2.0 ** -22
    assert float((rgb - dense_rgb).abs().max()) <= tol and float((depth - dense_depth).abs().max()) <= tol * float(rays[:, 7].max())
    assert ft.last_live_fraction < 1.0 and 0.0 < ft.last_stopped_fraction < 1.0


def test_fusion_render_rays_early_stop():
    from mvsnerf_amd import ops, train
    from tests.test_gpu_fusion import fusion_system, fusion_views
    views, bbox, img_wh, focal = fusion_views()
    with ops.mlp_precision("fp32"), torch.no_grad():
        sysm, _ = fusion_system(views, bbox, img_wh, focal)
    _raise_sigma(sysm.network_fn, 0.5)
    ro, rd = train.get_rays(train.get_ray_directions(64, 96, focal), views[1][4])
    pick = torch.randperm(ro.shape[0], generator=torch.Generator().manual_seed(3))[:300]
    rays = torch.cat([ro[pick], rd[pick], torch.full((300, 1), 2.125), torch.full((300, 1), 4.525)], 1)
    _check_frames(lambda **kw: sysm.render_rays(rays, **({"stop_every": 4, **kw} if kw else {})), 4.525, EPS, 16, sysm, 300)
