"""CPU-only: the surface of the netwidth-256 MLP - symbols, the size query against the documented layout, the model's state dict, and the
refusals that must come before any launch.  No compute (no GPU here)."""
import os
import re
import subprocess
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_SYMBOLS = ("mvsnerf_mlp_wide_packed_floats", "mvsnerf_mlp_pack_wide", "mvsnerf_mlp_fwd_wide")


def _layout_floats(F):
    """csrc/mlp_wide_layout.h from its description: a segment is steps x blocks x 64 lanes floats.  pts_bias: feat_steps(F) = F/2 rounded up to a
    multiple of 4 k-steps x 8 blocks; positional encoding (layer 0 and layer 5's skip part): 32 x 8; a 256-wide input: 128 x 8 (layers 1..4, layer
    5, feature_linear); views_linears.0: 132 x 4; then the vector block: 8 bias vectors of 256, the views bias (128), the alpha weight (256), the
    alpha bias + 3 flags / pad, the rgb weight (3 x 128), the rgb bias + 1 pad."""
    fsteps = (F // 2 + 3) & ~3
    seg = lambda steps, nb: steps * nb * 64
    vec = 8 * 256 + 128 + 256 + 4 + 3 * 128 + 4
    return seg(fsteps, 8) + 2 * seg(32, 8) + 6 * seg(128, 8) + seg(132, 4) + vec


def test_symbols_are_declared_exported_and_bound():
    from mvsnerf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    stable = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read(), flags=re.S)
    for name in WIDE_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert not re.search(rf"\b{name}\s*\(", stable), name            # internal tier only: the stable header and ABI 12 do not change
        assert name in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(WIDE_SYMBOLS) <= {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert _lib.lib().mvsnerf_abi_version() == 12


def test_size_query_follows_the_layout():
    from mvsnerf_amd import _lib
    q = _lib.lib().mvsnerf_mlp_wide_packed_floats
    assert _layout_floats(20) == 468744                     # 1.875 MB streamed per 128 points
    assert q(20, 256) == _layout_floats(20)
    for F in (4, 12, 36, 40):
        assert q(F, 256) == _layout_floats(F)
    for F, W in ((21, 256), (42, 256), (20, 128), (20, 192), (2, 256), (0, 256)):
        assert q(F, W) == 0, (F, W)


@pytest.mark.parametrize("net_type", ["v0", "v2"])
def test_state_dict_is_the_references_at_width_256(net_type):
    from mvsnerf_amd import models, ops
    from tests import wide_refs as R
    F = 20
    m = models.MVSNeRF(D=6, W=256, input_ch_pts=63, input_ch_views=3, input_ch_feat=F, skips=[4], net_type=net_type)
    want = {}
    for name, sh in zip(ops.MLP_ORDER, R.shapes_of(F, 256)):
        want[f"nerf.{name}.weight"], want[f"nerf.{name}.bias"] = sh, (sh[0],)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert m.wide and not models.MVSNeRF(D=6, W=128, input_ch_pts=63, input_ch_views=3, input_ch_feat=F, net_type=net_type).wide


def _no_library(monkeypatch):
    """Any touch of the library from here on fails the test: the refusals below must come first."""
    from mvsnerf_amd import _lib

    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "bf16x6", "fp16x3"])
@pytest.mark.parametrize("net_type", ["v0", "v2"])
def test_16bit_modes_are_refused_before_anything_is_packed(monkeypatch, net_type, mode):
    from mvsnerf_amd import models, ops
    m = models.MVSNeRF(D=6, W=256, input_ch_pts=63, input_ch_views=3, input_ch_feat=20, skips=[4], net_type=net_type)
    _no_library(monkeypatch)
    with ops.mlp_precision(mode), torch.no_grad():
        with pytest.raises(NotImplementedError, match="netwidth"):
            m.packed(20)
        with pytest.raises(NotImplementedError, match="netwidth"):
            m.packed_alt(20)
    for fn in (m.packed_bf16, m.packed_split):
        with pytest.raises(NotImplementedError, match="netwidth"):
            fn(20)


def test_gradients_are_refused_before_anything_is_enqueued(monkeypatch):
    from mvsnerf_amd import models, ops, renderer
    m = models.MVSNeRF(D=6, W=256, input_ch_pts=63, input_ch_views=3, input_ch_feat=20, skips=[4], net_type="v2")
    _no_library(monkeypatch)
    args = types.SimpleNamespace(feat_dim=20, use_color_volume=False, img_downscale=1.0, net_type="v2")
    qfn = lambda *a: None
    qfn._mvsnerf_fused = True
    vol = torch.zeros((1, 8, 4, 4, 4))
    z = torch.zeros((2, 3))
    call = lambda: renderer.rendering(args, {"w2cs": torch.eye(4)[None]}, torch.zeros((2, 3, 3)), torch.zeros((2, 3, 3)), z, None, torch.zeros((2, 3)),
                                      vol, torch.zeros((1, 3, 3, 8, 8)), network_fn=m, network_query_fn=qfn)
    with pytest.raises(NotImplementedError, match="training at netwidth 256"):
        call()                                                   # the parameters require gradients
    for p in m.parameters():
        p.requires_grad_(False)
    vol.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="training at netwidth 256"):
        call()                                                   # a learnable volume does
    with pytest.raises(NotImplementedError, match="netwidth"):
        ops.raymarch_train(vol, None, None, None, m, None, None, None, None)
    wp = ops.WidePacked(torch.zeros(4), 256, 20, 0)
    for op, a in (("raymarch", (None, None, None, None, wp, None, None, None, None)), ("raymarch_batched", (None, None, None, None, wp, [])),
                  ("raymarch_colorvol_batched", (None, None, wp, [])), ("render_pixels", (None, None, None, None, wp) + (None,) * 9),
                  ("render_rays", (None, None, None, wp) + (None,) * 5)):
        with pytest.raises(NotImplementedError, match="netwidth"):
            getattr(ops, op)(*a)
    wide_ws = [torch.zeros(sh) for sh in [(256, 63)] + [(256, 256)] * 10]
    for op in (ops.mlp_pack_bwd, ops.mlp_pack_bwd_bf16):
        with pytest.raises(NotImplementedError, match="netwidth"):
            op(wide_ws, 20)
    with pytest.raises(ValueError):
        ops.mlp_forward(wp, 20, 0, 3, 0, 20, 0, 3, 1, 1, False, "cpu", guard=torch.zeros(4))


@pytest.mark.parametrize("system", ["MVSSystemFinetune", "MVSSystemFusion"])
def test_training_systems_refuse_netwidth_256(system):
    from mvsnerf_amd import train
    args = types.SimpleNamespace(netwidth=256, n_views=3, pad=24, N_importance=0)
    with pytest.raises(NotImplementedError, match="training at netwidth 256"):
        if system == "MVSSystemFinetune":
            train.MVSSystemFinetune(args, None)
        else:
            train.MVSSystemFusion(args, None, None, None, None)
