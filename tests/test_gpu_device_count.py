"""Counted launches and device_count= on the GPU: the gather and MLP kernels that take their row count from device memory, and the
sparse / early-stopped marches built on them.

The yardstick is torch.equal throughout, against the host-count call - the parent's own code path, which stays as it was: a counted launch on the
first n compact rows composes its tiles exactly as the host-count launch with N = n does, so no tolerance is needed in any mode."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 700
COUNTS = (0, 1, 127, 128, 129, 255, 256, 257, 512, 699, 700, 5000, -3)      # tile edges of 128 and 256, an empty launch, clamped counts
SENTINEL = -123.25
KEYS = ("raw", "rgb_map", "weights", "depth", "alpha", "disp", "acc")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _count(n):
    return torch.tensor([n], dtype=torch.int32, device=DEV)


def _untouched(buf, n):
    return bool((buf[n:] == SENTINEL).all())


# ------------------------------------------------------------------ 1. the counted MLP launches
@functools.lru_cache(maxsize=None)
def _rows(F):
    """CAP rows of random NDC, features and unit directions; shared, nobody writes to them."""
    g = torch.Generator().manual_seed(F)
    d = torch.randn((CAP, 3), generator=g)
    return (torch.rand((CAP, 3), generator=g).to(DEV), torch.randn((CAP, F), generator=g).to(DEV), (d / d.norm(dim=-1, keepdim=True)).to(DEV))


@functools.lru_cache(maxsize=None)
def _model(kind, width, F):
    from mvsnerf_amd import models
    from tests.util import load_weights
    m = models.MVSNeRF(D=6, W=width, input_ch_pts=63, input_ch_views=3, input_ch_feat=F, skips=[4], net_type=kind)
    if (kind, width, F) == ("v0", 128, 20):
        m.load_state_dict(load_weights()[0])
    else:
        torch.manual_seed(1000 * width + F)
        for p in m.parameters():
            torch.nn.init.uniform_(p, -0.15, 0.15)
    return m.to(DEV)


def _query(packed, F, rows, N, ao, **kw):
    from mvsnerf_amd import ops
    ndc, feat, dirs = rows
    return ops.mlp_forward(packed, F, ndc.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, N, 1, ao, ndc.device, **kw)


MLP_CASES = ([("fp32", kind, 128, F, ao) for kind in ("v0", "v2") for F in (12, 20) for ao in (0, 1)]
             + [(mode, "v0", 128, F, 0) for mode in ("auto", "fp16x3") for F in (12, 20)]
             + [("fp32", kind, 256, F, ao) for kind in ("v0", "v2") for F in (12, 20) for ao in (0, 1)])


@pytest.mark.parametrize("mode,kind,width,F,ao", MLP_CASES)
def test_counted_mlp_equals_the_host_count_launch(mode, kind, width, F, ao):
    from mvsnerf_amd import ops
    m, rows = _model(kind, width, F), _rows(F)
    with torch.no_grad(), ops.mlp_precision(mode):
        packed, alt = m.packed(F), m.packed_alt(F)
        assert ("guard" in alt) == (mode == "auto") and ("packed_split" in alt) == (mode in ("auto", "fp16x3"))
        fallbacks = ops.guard_fallbacks()
        for count in COUNTS:
            n = min(max(count, 0), CAP)
            buf = torch.full((CAP, 1 if ao else 4), SENTINEL, device=DEV)
            got = _query(packed, F, rows, CAP, ao, count=_count(count), out=buf, **alt)
            assert got is buf
            if n:
                want = _query(packed, F, rows, n, ao, **alt)                 # the parent's launch with N = n
                assert torch.equal(buf[:n], want), (count, float((buf[:n] - want).abs().max()))
                assert bool(torch.isfinite(want).all())
            assert _untouched(buf, n), count
        assert ops.guard_fallbacks() == fallbacks


def test_counted_guarded_sequence_falls_back_to_the_counted_fp32_kernel():
    from mvsnerf_amd import ops
    m, (ndc, feat, dirs) = _model("v0", 128, 20), _rows(20)
    feat = feat.clone()
    feat[5, 3] = float("inf")                                                 # a live row the fp16 kernel cannot represent
    rows, n = (ndc, feat, dirs), 300
    with torch.no_grad():
        with ops.mlp_precision("fp32"):
            want = torch.full((CAP, 4), SENTINEL, device=DEV)
            _query(m.packed(20), 20, rows, CAP, 0, count=_count(n), out=want)
        with ops.mlp_precision("auto"):
            before = ops.guard_fallbacks()
            got = torch.full((CAP, 4), SENTINEL, device=DEV)
            _query(m.packed(20), 20, rows, CAP, 0, count=_count(n), out=got, **m.packed_alt(20))
            assert ops.guard_fallbacks() == before + 1
            _query(m.packed(20), 20, rows, CAP, 0, count=_count(0), out=got, **m.packed_alt(20))      # an empty launch trips nothing
            assert ops.guard_fallbacks() == before + 1
    assert torch.equal(_bits(got), _bits(want)) and _untouched(got, n)        # bytes: the row with the inf holds NaNs


def test_mlp_forward_count_refusals():
    from mvsnerf_amd import ops
    m, rows = _model("v0", 128, 20), _rows(20)
    with torch.no_grad():
        for mode in ("bf16", "bf16x3", "bf16x6"):
            with ops.mlp_precision(mode), pytest.raises(NotImplementedError, match=f"'{mode}'"):
                _query(m.packed(20), 20, rows, CAP, 0, count=_count(5), **m.packed_alt(20))
        for bad in (_count(5).long(), torch.zeros(2, dtype=torch.int32, device=DEV), _count(5).cpu(), 5):
            with pytest.raises(RuntimeError, match="count"):
                _query(m.packed(20), 20, rows, CAP, 0, count=bad)
        with pytest.raises(RuntimeError, match="out must be"):
            _query(m.packed(20), 20, rows, CAP, 0, count=_count(5), out=torch.zeros((CAP, 1), device=DEV))


# ------------------------------------------------------------------ 2. the counted gathers
@functools.lru_cache(maxsize=None)
def _scene(V):
    """50 x 14 = CAP samples of tests/test_gpu_raymarch_onelaunch._inputs as rows, with a direction per row; both memory orders of both volumes."""
    from tests.test_gpu_raymarch_onelaunch import _inputs, _hwdc
    x = _inputs(50, 14, V=V, seed=V)
    g = torch.Generator().manual_seed(V)
    cvol = torch.randn((1, 20, 16, 24, 32), generator=g)
    d = torch.randn((CAP, 3), generator=g)
    return dict(x, pts=x["pts"].view(CAP, 1, 3), ndc=x["ndc"].view(CAP, 1, 3), dirs=(d / d.norm(dim=-1, keepdim=True)).to(DEV),
                vol={"hwdc": _hwdc(x["vol"]), "dhwc": x["vol"][0].permute(1, 2, 3, 0).contiguous().to(DEV)},
                cvol={"hwdc": _hwdc(cvol), "dhwc": cvol[0].permute(1, 2, 3, 0).contiguous().to(DEV)})


def _check_gather(run, F):
    """run(rows n | None, count, out) -> (feat, dirs)"""
    for count in COUNTS:
        n = min(max(count, 0), CAP)
        feat, dirs = torch.full((CAP, 1, F), SENTINEL, device=DEV), torch.full((CAP, 3), SENTINEL, device=DEV)
        got = run(None, _count(count), (feat, dirs))
        assert got[0] is feat and got[1] is dirs
        if n:
            wf, wd = run(n, None, None)                                      # the parent's launch on n rows
            assert torch.equal(_bits(feat[:n]), _bits(wf)) and torch.equal(_bits(dirs[:n]), _bits(wd)), count
        assert _untouched(feat, n) and _untouched(dirs, n), count


@pytest.mark.parametrize("layout", ["hwdc", "dhwc"])
@pytest.mark.parametrize("V", [1, 3, 5])
def test_counted_gather_equals_the_host_count_launch(V, layout):
    from mvsnerf_amd import ops
    x = _scene(V)
    vol = x["vol"][layout]
    assert ops.vol_ptr_layout(vol)[1] == (ops.VOL_HWDC if layout == "hwdc" else ops.VOL_DHWC)

    def run(n, count, out):
        s = slice(None) if n is None else slice(0, n)
        return ops.gather(vol, x["imgs"], x["w2cs"], x["Ks"], x["pts"][s], x["ndc"][s], x["dirs"][s], count=count, out=out)
    with torch.no_grad():
        _check_gather(run, 8 + 4 * V)


@pytest.mark.parametrize("wide_offsets", [False, True])
@pytest.mark.parametrize("layout", ["hwdc", "dhwc"])
def test_counted_colour_volume_gather_equals_the_host_count_launch(layout, wide_offsets):
    from mvsnerf_amd import ops
    x = _scene(3)
    vol = x["cvol"][layout]

    def run(n, count, out):
        s = slice(None) if n is None else slice(0, n)
        return ops.gather_colorvol(vol, x["ndc"][s], x["dirs"][s], x["w2cs"][0].contiguous(), force_offsets64=wide_offsets, count=count, out=out)
    with torch.no_grad():
        _check_gather(run, 20)


# ------------------------------------------------------------------ 3. raymarch_sparse(device_count=True)
def _densities(x):
    from tests import sparse_refs as R
    from tests.test_gpu_sparse_render import GRID, _band
    return {"dead": (torch.zeros(GRID), x), "live": (torch.ones(GRID), dict(x, ndc=x["ndc"].clamp(0, 1).contiguous())), "band": (_band(), x),
            "ragged": (R.sparse_density(GRID, torch.Generator().manual_seed(7)), x)}


def _march_pair(call):
    with torch.no_grad():
        want, got = call(device_count=False), call(device_count=True)
    torch.cuda.synchronize()
    assert isinstance(want["n_live"], int) and torch.is_tensor(got["n_live"]) and got["n_live"].dtype == torch.int32 and got["n_live"].is_cuda
    assert int(got["n_live"]) == want["n_live"]
    for k in KEYS:
        assert got[k].shape == want[k].shape and torch.equal(_bits(got[k]), _bits(want[k])), k
    return want


@pytest.mark.parametrize("mode", ["fp32", "auto"])
@pytest.mark.parametrize("N,S", [(1, 1), (37, 24), (300, 128)])
def test_raymarch_sparse_device_count_equals_host_count(N, S, mode):
    from mvsnerf_amd import ops
    from tests.test_gpu_sparse_render import _rays, _net
    x0 = _rays(N, S)
    seen = set()
    with ops.mlp_precision(mode):
        for kind, white, colour in (("v0", False, False), ("v0", True, False), ("v2", False, False), ("wide", False, False), ("v0", False, True)):
            packed, m = _net(kind)
            alt = {} if m is None else m.packed_alt(20)
            for name, (density, x) in _densities(x0).items():
                if (kind, white, colour) != ("v0", False, False) and name in ("dead", "live"):
                    continue                                                  # the two extremes once; every network on the two mixed volumes
                vol = x["cvol_cl"] if colour else x["vol_cl"]

                def call(device_count):
                    return ops.raymarch_sparse(vol, None if colour else x["imgs"], x["w2cs"], None if colour else x["Ks"], packed, x["pts"], x["ndc"],
                                               x["z"], x["dirs"], density.to(DEV), 0.0, white_bkgd=white, want=("disp", "acc"),
                                               device_count=device_count, **alt)
                n = _march_pair(call)["n_live"]
                seen.add((name, n))
                assert {"dead": n == 0, "live": n == N * S}.get(name, True), (name, n)
    if N * S > 100:
        assert any(0 < n < N * S and n % 128 for name, n in seen if name in ("band", "ragged"))      # a mixed count with a partial last tile


# ------------------------------------------------------------------ 4. raymarch_early_stop(device_count=True)
# alpha_linear.bias raised as tests/test_gpu_early_stop.py does (its BIAS table: 0.25 alone and 0.5 against the band at (37,24)), so that the
# host-count reference stops some rays and not all at eps = 1e-2; at 128 samples the shipped bias does that already (246 / 142 of 300 rays stop)
EARLY_BIAS = {(37, 24): (0.25, 0.5), (300, 128): (0.0, 0.0)}


@pytest.mark.parametrize("with_density", [False, True])
@pytest.mark.parametrize("N,S,G", [(37, 24, 5), (37, 24, 8), (37, 24, 24), (37, 24, 32), (300, 128, 32)])
def test_raymarch_early_stop_device_count_equals_host_count(N, S, G, with_density):
    from mvsnerf_amd import ops
    from tests.test_gpu_sparse_render import _rays, _band
    from tests.test_gpu_early_stop import _net
    x = _rays(N, S)
    packed, _ = _net("v0", EARLY_BIAS[(N, S)][int(with_density)])
    kw = dict(density=_band().to(DEV), thr=0.0) if with_density else {}
    with ops.mlp_precision("fp32"):
        for eps in (0.0, 1e-2, 0.5):
            def call(device_count):
                return ops.raymarch_early_stop(x["vol_cl"], x["imgs"], x["w2cs"], x["Ks"], packed, x["pts"], x["ndc"], x["z"], x["dirs"], eps, stop_every=G,
                                               want=("disp", "acc"), device_count=device_count, **kw)
            want = _march_pair(call)
            with torch.no_grad():
                got = call(device_count=True)
            assert torch.is_tensor(got["n_stopped"]) and got["n_stopped"].dtype == torch.int32 and int(got["n_stopped"]) == want["n_stopped"]
            print(f"(N,S,G)=({N},{S},{G}) eps {eps} density {with_density}: {want['n_live']} of {N * S} samples, {want['n_stopped']} of {N} rays stopped")
            if eps == 0.0:
                assert want["n_stopped"] == 0
            if eps == 1e-2 and G < S:
                assert 0 < want["n_stopped"] < N                               # the host-count reference itself stops some rays, not all


def test_raymarch_early_stop_device_count_auto_mode():
    from mvsnerf_amd import ops
    from tests.test_gpu_sparse_render import _rays
    from tests.test_gpu_early_stop import _net
    x = _rays(37, 24)
    _, m = _net("v0", 0.25)
    with ops.mlp_precision("auto"):
        before = ops.guard_fallbacks()

        def call(device_count):
            return ops.raymarch_early_stop(x["vol_cl"], x["imgs"], x["w2cs"], x["Ks"], m.packed(20), x["pts"], x["ndc"], x["z"], x["dirs"], 1e-2, stop_every=8,
                                           want=("disp", "acc"), device_count=device_count, **m.packed_alt(20))
        want = _march_pair(call)
        assert 0 < want["n_stopped"] < 37 and ops.guard_fallbacks() == before


# ------------------------------------------------------------------ 5. the count is read on the device: a captured graph follows the data
@pytest.mark.parametrize("mode", ["fp32", "auto"])
def test_a_captured_graph_follows_the_density(mode):
    """A graph freezes every launch argument: the replays below can only follow the density if the gather and MLP kernels take their row count
    from device memory.  One capture, four replays."""
    from mvsnerf_amd import ops
    from tests.test_gpu_sparse_render import GRID, _rays, _net, _band
    x = _rays(37, 24)
    _, m = _net("v0")
    density = _band().to(DEV)                                                  # static: the graph reads this tensor

    def call(d, device_count):
        return ops.raymarch_sparse(x["vol_cl"], x["imgs"], x["w2cs"], x["Ks"], m.packed(20), x["pts"], x["ndc"], x["z"], x["dirs"], d, 0.0,
                                   want=("disp", "acc"), device_count=device_count, **m.packed_alt(20))
    with torch.no_grad(), ops.mlp_precision(mode):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):                                                 # guard words, LDS caps and the image cache exist before the capture
                call(density, True)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                out = call(density, True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        counts = []
        for X in (_band(2, 13), torch.zeros(GRID), torch.ones(GRID), _band()):
            density.copy_(X.to(DEV))
            g.replay()
            torch.cuda.synchronize()
            want = call(X.to(DEV), False)
            torch.cuda.synchronize()
            assert int(out["n_live"]) == want["n_live"]
            for k in KEYS:
                assert torch.equal(_bits(out[k]), _bits(want[k])), (k, want["n_live"])
            counts.append(want["n_live"])
    assert counts[1] == 0 and counts[0] > counts[3] > 0 and counts[2] > counts[0]      # the replays did see different counts


# ------------------------------------------------------------------ 6. the systems
def _frames_equal(render, sysm, stopped=False):
    """render(device_count) -> tensors: equal outputs and equal fractions, which are Python floats either way."""
    with torch.no_grad():
        want = render(False)
        w_live, w_stop = sysm.last_live_fraction, getattr(sysm, "last_stopped_fraction", None)
        got = render(True)
        g_live, g_stop = sysm.last_live_fraction, getattr(sysm, "last_stopped_fraction", None)
    want, got = (want, got) if isinstance(want, tuple) else ((want,), (got,))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert type(g_live) is float and g_live == w_live and 0.0 < g_live < 1.0
    if stopped:
        assert type(g_stop) is float and g_stop == w_stop and 0.0 < g_stop < 1.0


@pytest.mark.parametrize("mode", ["fp32", "auto"])
def test_finetune_system_device_count(mode):
    from mvsnerf_amd import ops
    from tests.test_gpu_finetune_render import _system, _rays as scene_rays
    from tests.test_gpu_early_stop import _raise_sigma
    from tests.test_gpu_frames import _path_of
    ft, _, pose = _system(V=3)
    _raise_sigma(ft.network_fn)
    ft.update_density_volume()
    band = torch.zeros_like(ft.density_volume)
    band[4:9] = 1.0
    ft.density_volume = band
    rays = scene_rays(2500)
    with ops.mlp_precision(mode):
        _frames_equal(lambda dc: ft.render_rays(rays, skip_empty=0.0, batch_rays=1000, device_count=dc), ft)          # three sub-batches
        _frames_equal(lambda dc: ft.render_rays(rays, early_stop=1e-2, stop_every=8, batch_rays=1000, device_count=dc), ft, stopped=True)
        _frames_equal(lambda dc: ft.render_rays(rays, skip_empty=0.0, early_stop=1e-2, stop_every=8, batch_rays=1000, device_count=dc), ft, stopped=True)
        H, W = 20, 28
        focal = [float(pose["intrinsics"][0, 0, 0]) * W / 96, float(pose["intrinsics"][0, 1, 1]) * H / 64]
        _frames_equal(lambda dc: ft.render_path(_path_of(pose["c2ws"][:3]), (H, W), focal, skip_empty=0.0, batch_rays=200, device_count=dc), ft)


def test_finetune_colour_volume_system_device_count():
    from mvsnerf_amd import ops
    from tests.test_gpu_finetune_render import _system, _rays as scene_rays
    ft, _, _ = _system(V=3, use_color_volume=True)
    ft.update_density_volume()
    band = torch.zeros_like(ft.density_volume)
    band[4:9] = 1.0
    ft.density_volume = band
    rays = scene_rays(1200, seed=4)
    with ops.mlp_precision("fp32"):
        _frames_equal(lambda dc: ft.render_rays(rays, skip_empty=0.0, batch_rays=500, device_count=dc), ft)


def test_pretrained_system_device_count():
    from mvsnerf_amd import ops, train
    from tests.util import load_weights
    from tests.test_gpu_early_stop import _raise_sigma
    mlp_sd, mvs_sd = load_weights()
    s = train.MVSSystem(train.default_args(pad=4, batch_size=64, N_samples=32, chunk=1024), n_depth_planes=16)
    s.render_kwargs_train["network_fn"].load_state_dict(mlp_sd)
    s.MVSNet.load_state_dict(mvs_sd)
    _raise_sigma(s.render_kwargs_train["network_fn"])
    s = s.to(DEV)
    batch = train.synthetic_batch(64, 96, seed=8, smooth=True)
    with ops.mlp_precision("fp32"), torch.no_grad():
        vol = s.encode_scene(batch)
        band = torch.zeros(tuple(vol.shape[-3:]), device=DEV)
        band[4:9] = 1.0
        _frames_equal(lambda dc: s.render_view(batch, volume=vol, batch_rays=2500, skip_empty=0.0, density=band, device_count=dc), s)
        _frames_equal(lambda dc: s.render_view(batch, volume=vol, batch_rays=2500, early_stop=1e-2, stop_every=8, device_count=dc), s, stopped=True)
        from tests.test_gpu_frames import _path_of
        _, pose = s.decode_batch(dict(batch))
        H, W = 20, 28
        K = pose["intrinsics"][0] * torch.tensor([[W / 96], [H / 64], [1.0]], device=pose["intrinsics"].device)
        dens = s.scene_density(batch, volume=vol)
        thr = float(dens[dens > 0].median()) if bool((dens > 0).any()) else 0.0
        _frames_equal(lambda dc: s.render_path_skip_empty(batch, _path_of(pose["c2ws"][:2]), thr, dilate=1, hw=(H, W), intrinsic=K, volume=vol,
                                                          device_count=dc), s)


def test_fusion_system_device_count():
    from mvsnerf_amd import ops, train
    from tests.test_gpu_fusion import fusion_system, fusion_views
    from tests.test_gpu_early_stop import _raise_sigma
    views, bbox, img_wh, focal = fusion_views()
    with ops.mlp_precision("fp32"), torch.no_grad():
        sysm, _ = fusion_system(views, bbox, img_wh, focal)
    _raise_sigma(sysm.network_fn, 0.5)
    ro, rd = train.get_rays(train.get_ray_directions(64, 96, focal), views[1][4])
    pick = torch.randperm(ro.shape[0], generator=torch.Generator().manual_seed(3))[:300]
    rays = torch.cat([ro[pick], rd[pick], torch.full((300, 1), 2.125), torch.full((300, 1), 4.525)], 1)
    from tests.test_gpu_fusion import DIMS
    with ops.mlp_precision("fp32"):
        _frames_equal(lambda dc: sysm.render_rays(rays, early_stop=1e-2, stop_every=4, batch_rays=120, device_count=dc), sysm, stopped=True)
        band = torch.zeros(DIMS, device=DEV)
        band[3:6] = 1.0
        sysm.density_volume = band.view(1, 1, *DIMS)
        _frames_equal(lambda dc: sysm.render_rays(rays, skip_empty=0.0, batch_rays=120, device_count=dc), sysm)
