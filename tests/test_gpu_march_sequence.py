"""The C entries the compacted marches and the batched colour-volume march call, in order.

Every case runs once unrecorded (the one-off nchw_to_nhwc of ops.channels_last_images, the weight packing), then once with _lib.lib replaced by
a proxy that writes down the name of every entry it hands out a call to.  Size queries (*_workspace_bytes) enqueue nothing and are left out of
the record.  fp32 MLP mode, V = 3 (F = 20), an (8,6,6,8) volume or an (8,6,6,20) colour volume, a (4,4,4) density grid, N = 5 rays of S = 7 samples.

The density is 1 in its first depth plane and 0 elsewhere, the threshold 0, and sample s of every ray sits at NDC depth Z[s]: a sample is live iff
its cell touches plane 0, i.e. Z[s] * 3 < 1.  Samples 0-2 and 6 are live, 3-5 are not: with stop_every = 3 the segments [0,3), [3,6), [6,7) are
live, dead, live."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, S, G = 5, 7, 3
Z = (0.1, 0.15, 0.2, 0.8, 0.85, 0.9, 0.25)
SEGMENT_LIVE = (True, False, True)
N_LIVE = N * 4


@functools.lru_cache(maxsize=None)
def _scene():
    """Shared inputs; nobody writes to them."""
    from mvsnerf_amd import ops
    from tests.test_gpu_raymarch_onelaunch import _inputs
    from tests.test_gpu_sparse_render import _net
    x = _inputs(N, S, D=8, h=6, w=6, seed=S)
    g = torch.Generator().manual_seed(5)
    ndc = torch.rand((N, S, 3), generator=g)
    ndc[..., 2] = torch.tensor(Z)
    band = torch.zeros((4, 4, 4))
    band[0] = 1.0
    packed, _ = _net("v0")                                               # the fp32 buffer: no packed_alt keyword selects another kernel
    return dict(x, ndc=ndc.to(DEV), vol_cl=x["vol"][0].permute(1, 2, 3, 0).contiguous().to(DEV),
                cvol_cl=torch.randn((8, 6, 6, 20), generator=g).to(DEV), band=band.to(DEV), dead=torch.zeros((4, 4, 4), device=DEV), packed=packed)


class _Recorder:
    """Stands in for the loaded library: hands out every entry under its own name and notes each call."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            if not name.endswith("_workspace_bytes"):
                self.calls.append(name[len("mvsnerf_"):])
            return fn(*args)
        return call


def _record(monkeypatch, fn):
    """fn() once unrecorded, once recorded -> (the recorded run's result, the entries it called)."""
    from mvsnerf_amd import _lib, ops
    with torch.no_grad(), ops.mlp_precision("fp32"):
        fn()
        rec = _Recorder(_lib.lib())
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "lib", lambda: rec)
            out = fn()
    torch.cuda.synchronize()
    print(rec.calls)
    return out, rec.calls


def _sparse(x, density, colour, device_count):
    from mvsnerf_amd import ops
    return ops.raymarch_sparse(x["cvol_cl"] if colour else x["vol_cl"], None if colour else x["imgs"], x["w2cs"], None if colour else x["Ks"], x["packed"],
                               x["pts"], x["ndc"], x["z"], x["dirs"], density, 0.0, want=("disp", "acc"), device_count=device_count)


def _early(x, density, colour, device_count):
    from mvsnerf_amd import ops
    kw = {} if density is None else dict(density=density, thr=0.0)
    return ops.raymarch_early_stop(x["cvol_cl"] if colour else x["vol_cl"], None if colour else x["imgs"], x["w2cs"], None if colour else x["Ks"], x["packed"],
                                   x["pts"], x["ndc"], x["z"], x["dirs"], 0.0, stop_every=G, want=("disp", "acc"), device_count=device_count, **kw)


def _names(colour, counted):
    tail = "_counted" if counted else ""
    return ["gather_colorvol_fwd" + tail if colour else "gather_fwd" + tail, "mlp_fwd" + tail]


def _early_sequence(live, colour, counted):
    """live: per segment, whether the gather and the MLP are enqueued (always, under device counts)."""
    seq = []
    for k, has_rows in enumerate(live):
        seq.append("live_samples_range_fwd")
        if has_rows:
            seq += _names(colour, counted) + ["scatter_rows_fwd"]
        if k < len(live) - 1:
            seq.append("ray_transmittance_fwd")
    return seq + ["composite_fwd"]


@pytest.mark.parametrize("colour", [False, True])
def test_raymarch_sparse_host_count(monkeypatch, colour):
    x = _scene()
    out, calls = _record(monkeypatch, lambda: _sparse(x, x["band"], colour, False))
    assert out["n_live"] == N_LIVE                                      # some samples are live and some are not
    assert calls == ["live_samples_fwd", *_names(colour, False), "expand_rows_fwd", "composite_fwd"]


def test_raymarch_sparse_host_count_nothing_live(monkeypatch):
    x = _scene()
    out, calls = _record(monkeypatch, lambda: _sparse(x, x["dead"], False, False))
    assert out["n_live"] == 0
    assert calls == ["live_samples_fwd", "expand_rows_fwd", "composite_fwd"]


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("density", ["band", "dead"])
def test_raymarch_sparse_device_count(monkeypatch, density, colour):
    x = _scene()
    out, calls = _record(monkeypatch, lambda: _sparse(x, x[density], colour, True))
    assert int(out["n_live"]) == (N_LIVE if density == "band" else 0)
    assert calls == ["live_samples_fwd", *_names(colour, True), "expand_rows_fwd", "composite_fwd"]       # whatever the density


@pytest.mark.parametrize("colour", [False, True])
def test_raymarch_early_stop_host_count(monkeypatch, colour):
    x = _scene()
    assert [len(range(s, min(s + G, S))) for s in range(0, S, G)] == [3, 3, 1]
    out, calls = _record(monkeypatch, lambda: _early(x, None, colour, False))                             # no density: every segment has rows
    assert out["n_live"] == N * S and out["n_stopped"] == 0
    assert calls == _early_sequence((True, True, True), colour, False)
    out, calls = _record(monkeypatch, lambda: _early(x, x["band"], colour, False))                        # the middle segment has none
    assert out["n_live"] == N_LIVE
    assert calls == _early_sequence(SEGMENT_LIVE, colour, False)


@pytest.mark.parametrize("colour", [False, True])
def test_raymarch_early_stop_device_count(monkeypatch, colour):
    x = _scene()
    for density, n_live in ((None, N * S), (x["band"], N_LIVE), (x["dead"], 0)):
        out, calls = _record(monkeypatch, lambda: _early(x, density, colour, True))
        assert int(out["n_live"]) == n_live and int(out["n_stopped"]) == 0
        assert calls == _early_sequence((True, True, True), colour, True)


def test_raymarch_colorvol_batched_is_one_call(monkeypatch):
    """Two batches, (3,5) and (1,128), in one entry; the first one's outputs are those of gather_colorvol -> mlp_forward -> composite."""
    from mvsnerf_amd import ops
    x = _scene()
    g = torch.Generator().manual_seed(9)
    batches = []
    for n, s in ((3, 5), (1, 128)):
        d = torch.randn((n, 3), generator=g)
        batches.append((torch.rand((n, s, 3), generator=g).to(DEV), torch.sort(torch.rand((n, s), generator=g) + 0.5, dim=-1)[0].to(DEV),
                        (d / d.norm(dim=-1, keepdim=True)).to(DEV)))
    outs, calls = _record(monkeypatch, lambda: ops.raymarch_colorvol_batched(x["cvol_cl"], x["w2cs"], x["packed"], batches, want=("disp", "acc")))
    assert calls == ["raymarch_colorvol_fwd_batched"]
    assert [tuple(o["raw"].shape) for o in outs] == [(3, 5, 4), (1, 128, 4)]
    ndc, z, dirs = batches[0]
    with torch.no_grad(), ops.mlp_precision("fp32"):
        feat, dfeat = ops.gather_colorvol(x["cvol_cl"], ndc, dirs, x["w2cs"][0].contiguous())
        raw = ops.mlp_forward(x["packed"], 20, ndc.data_ptr(), 3, feat.data_ptr(), 20, dfeat.data_ptr(), 3, 3, 5, 0, ndc.device).view(3, 5, 4)
        rgb, disp, acc, weights, depth, alpha = ops.composite(raw, z)
    want = {"input_feat": feat, "raw": raw, "rgb_map": rgb, "disp": disp, "acc": acc, "weights": weights, "depth": depth, "alpha": alpha}
    for k, v in want.items():
        assert torch.equal(outs[0][k], v), k
