"""Yardsticks of the fine-tuning step that skips empty space (ops.compact_rows, ops.raymarch_sparse_train).  CPU only.

compact_rows: a torch restatement.  The step: autograd through the reference composition with the DEAD rows of raw zeroed before raw2outputs -
`raw * live[..., None]`, live = tests/sparse_refs.live_mask(band, ndc, 0.0) - which is the function the sparse step computes: a dead sample's raw is the
constant (0,0,0,0) and hands no gradient to anything.  The four compositions are those of tests/test_gpu_train_wide_feat.py (the oracle's rendering for
v0, the float64 composition for v2, the colour-volume lookup, the bf16 emulation) on that file's scenes and networks; every reference is computed once
and shared, nobody writes to it."""
import functools

import torch

from tests import sparse_refs as R
from tests.test_gpu_net_v2 import _state_dict
from tests.test_gpu_train_wide_feat import _scene, _sd_of, _loss, _rel, _net_v2, _renderer_bf16_emulation, _lists    # noqa: F401  (_rel: re-exported)

GRID = (16, 24, 32)
SHAPES = [(37, 16, True), (8, 128, False), (130, 3, False)]         # (rays, samples, white background): test_gradients_of_rendering's
COLOR_SCENE = (48, 24, 77)                                          # rays, samples, seed: test_color_volume_gradients'
AMP_SCENE = (96, 32, 3)


def band():
    d = torch.zeros(GRID)
    d[4:9] = 1.0
    return d


def sd_of(V, net_type):
    """_sd_of for every V: its v2 seeds start at F = 32; below, uniform(-0.15, 0.15) from torch.manual_seed(F), the same rule"""
    F = 8 + 4 * V
    if net_type == "v0" or F >= 32:
        return _sd_of(V, net_type)
    from mvsnerf_amd import models
    m = models.MVSNeRF(D=6, W=128, input_ch_pts=63, input_ch_views=3, input_ch_feat=F, skips=[4], net_type="v2")
    torch.manual_seed(F)
    for p in m.parameters():
        torch.nn.init.uniform_(p, -0.15, 0.15)
    lins = m.nerf._linears()
    return _state_dict([l.weight.detach().clone().contiguous() for l in lins], [l.bias.detach().clone().contiguous() for l in lins])


def compact_rows(src, idx, count, n_rows):
    """dst (n_rows,C): dst[j] = src[idx[j]] for j < min(count, n_rows) with idx[j] in [0, P); every other row zero."""
    P = src.shape[0]
    dst = torch.zeros((n_rows, src.shape[1]), dtype=src.dtype, device=src.device)
    n = max(0, min(int(count), n_rows))
    j = idx[:n].long()
    ok = (j >= 0) & (j < P)
    dst[:n][ok] = src[j[ok]]
    return dst


def live_of(s, density=None, thr=0.0):
    """bool (N,S): the live samples of a scene against the band"""
    return R.live_mask(band() if density is None else density, s["ndc"], thr).view(s["z"].shape)


def _angle(s, O):
    return O.gen_dir_feature(s["pose"]["w2cs"][0], s["dirs"] / torch.norm(s["dirs"], dim=-1, keepdim=True))


@functools.lru_cache(maxsize=None)
def masked_reference(V, net_type, n_rays, n_samples, white, mask=True):
    """(loss, {name: grad}, volume grad, live) on the CPU: reference_gradients of tests/test_gpu_train_wide_feat.py with the dead rows of raw zeroed
    (mask=False: every row kept - the dense step)"""
    from oracle import mvsnerf_oracle as O
    s = _scene(V, n_rays, n_samples, 5 + n_rays)
    live = live_of(s) if mask else torch.ones(s["z"].shape, dtype=torch.bool)
    sd0 = sd_of(V, net_type)
    if net_type == "v0":
        sd = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
        vol = s["vol"].clone().requires_grad_(True)
        feat = O.gen_pts_feats(s["imgs"], vol, s["pts"], s["pose"], s["ndc"])
        raw = O.run_network_mvs(s["ndc"], _angle(s, O), feat, sd)             # = O.rendering up to here
        rgb, _, _, w, depth, alpha = O.raw2outputs(raw * live[..., None], s["z"], white)
        loss = _loss(rgb, depth, w, alpha, s["G"])
    else:
        sd = {k: v.double().requires_grad_(True) for k, v in sd0.items()}
        vol = s["vol"].double().requires_grad_(True)
        ws, bs = _lists(sd)
        feat32 = O.gen_pts_feats(s["imgs"], s["vol"], s["pts"], s["pose"], s["ndc"])
        feat = torch.cat([O.index_point_feature(vol, s["ndc"].double()), feat32[..., 8:].double()], -1)
        raw = _net_v2(ws, bs, s["ndc"].double(), feat, _angle(s, O).double())
        rgb, _, _, w, depth, alpha = O.raw2outputs(raw * live[..., None], s["z"].double(), white)
        loss = _loss(rgb, depth, w, alpha, [t.double() for t in s["G"]])
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in sd.items()}, vol.grad, live


def color_volume(V):
    """the (1,8+4V,16,24,32) learnable colour volume of test_color_volume_gradients: the scene's 8 channels + uniform colours"""
    s = _scene(V, *COLOR_SCENE)
    return torch.cat([s["vol"], torch.rand((1, 4 * V, *s["vol"].shape[2:]), generator=torch.Generator().manual_seed(9))], 1)


@functools.lru_cache(maxsize=None)
def masked_color_reference(V):
    from oracle import mvsnerf_oracle as O
    s = _scene(V, *COLOR_SCENE)
    live = live_of(s)
    sd = {k: v.clone().requires_grad_(True) for k, v in _sd_of(V, "v0").items()}
    vol = color_volume(V).requires_grad_(True)
    feat = O.index_point_feature(vol, s["ndc"])
    raw = O.run_network_mvs(s["ndc"], _angle(s, O), feat, sd)
    rgb, _, _, w, depth, alpha = O.raw2outputs(raw * live[..., None], s["z"], False)
    loss = _loss(rgb, depth, w, alpha, s["G"])
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in sd.items()}, vol.grad, live


@functools.lru_cache(maxsize=None)
def masked_amp_reference():
    """the bf16 emulation of tests/test_gpu_backward.py on _scene(3, 96, 32, 3), dead rows zeroed"""
    from oracle import mvsnerf_oracle as O
    s = _scene(3, *AMP_SCENE)
    live = live_of(s)
    sd = {k: v.clone().requires_grad_(True) for k, v in _sd_of(3, "v0").items()}
    vol = s["vol"].clone().requires_grad_(True)
    feat = O.gen_pts_feats(s["imgs"], vol, s["pts"], s["pose"], s["ndc"])
    raw = _renderer_bf16_emulation(s["ndc"], _angle(s, O), feat, sd)
    rgb, _, _, w, depth, alpha = O.raw2outputs(raw * live[..., None], s["z"], False)
    loss = _loss(rgb, depth, w, alpha, s["G"])
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in sd.items()}, vol.grad, live
