"""CPU-only: the Python surface of net_type 'v2' (Renderer_linear, reference models.py:464-538) - the classes, their state_dict and the factory.
What the kernels compute for it is tests/test_gpu_net_v2.py."""
import inspect
import types

import pytest
import torch


def _mvsnerf(net_type, F=20):
    from mvsnerf_amd import models
    return models.MVSNeRF(D=6, W=128, input_ch_pts=63, input_ch_views=3, input_ch_feat=F, skips=[4], net_type=net_type)


def test_v2_builds_a_renderer_linear():
    from mvsnerf_amd import models
    m = _mvsnerf("v2")
    assert type(m.nerf) is models.Renderer_linear
    assert type(_mvsnerf("v0").nerf) is models.Renderer_ours
    assert not isinstance(m.nerf, models.Renderer_ours)
    # the reference's class default is v2 (models.py:541)
    assert type(models.MVSNeRF().nerf) is models.Renderer_linear


def test_v2_state_dict_is_v0s():
    a, b = _mvsnerf("v0").state_dict(), _mvsnerf("v2").state_dict()
    assert list(a) == list(b) and len(a) == 22
    assert {k: tuple(v.shape) for k, v in a.items()} == {k: tuple(v.shape) for k, v in b.items()}
    # a v2 network_fn_state_dict loads as the reference's does (models.py:619)
    m = _mvsnerf("v2")
    sd = {k: torch.full_like(v, 0.25) for k, v in b.items()}
    m.load_state_dict(sd)
    assert all(bool((p == 0.25).all()) for p in m.parameters())


def test_star_import_offers_the_name():
    ns = {}
    exec("from mvsnerf_amd.models import *", ns)
    assert "Renderer_linear" in ns and "Renderer_ours" in ns and "MVSNeRF" in ns


def test_constructor_signature_is_the_references():
    from mvsnerf_amd import models
    P, K = inspect.Parameter, inspect.Parameter.POSITIONAL_OR_KEYWORD
    want = inspect.Signature([P("self", K), P("D", K, default=8), P("W", K, default=256), P("input_ch", K, default=3),
                              P("input_ch_views", K, default=3), P("output_ch", K, default=4), P("input_ch_feat", K, default=8),
                              P("skips", K, default=[4]), P("use_viewdirs", K, default=False)])
    assert inspect.signature(models.Renderer_linear.__init__) == want
    assert inspect.signature(models.Renderer_ours.__init__) == want


def test_v1_still_raises():
    with pytest.raises(NotImplementedError):
        _mvsnerf("v1")


def test_create_nerf_mvs_with_v2():
    from mvsnerf_amd import models
    args = types.SimpleNamespace(feat_dim=20, img_downscale=1.0, use_color_volume=False, net_type="v2", multires=10, i_embed=0, pts_dim=3,
                                 multires_views=4, dir_dim=3, netdepth=6, netwidth=128, N_importance=0, netchunk=1024, ckpt=None, perturb=1.0,
                                 N_samples=32, use_viewdirs=True, white_bkgd=False, raw_noise_std=0.0)
    train, test, start, grad_vars = models.create_nerf_mvs(args, use_mvs=False, dir_embedder=False, pts_embedder=True)
    keys = {"network_query_fn", "perturb", "N_importance", "network_fine", "N_samples", "network_fn", "network_mvs", "use_viewdirs", "white_bkgd",
            "raw_noise_std"}
    assert set(train) == keys and set(test) == keys and start == 0 and len(grad_vars) == 22
    assert type(train["network_fn"].nerf) is models.Renderer_linear
    assert test["perturb"] is False and train["network_query_fn"]._mvsnerf_fused


def test_v2_refuses_the_16_bit_modes_before_packing():
    """No GPU involved: the refusal comes before anything is packed or launched."""
    from mvsnerf_amd import ops
    m = _mvsnerf("v2")
    for mode in ("bf16", "bf16x3", "bf16x6", "fp16x3"):
        with ops.mlp_precision(mode):
            for call in (lambda: m.packed(20), lambda: m.packed_alt(20)):
                with pytest.raises(NotImplementedError, match=r"net_type v2.*fp32"):
                    call()
