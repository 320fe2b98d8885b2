"""What the netwidth-256 MLP tests share: the weight recipe, the inputs and the two networks restated in torch for any width W.

Weights: g = torch.Generator().manual_seed(seed); the 11 weights in ops.MLP_ORDER as (torch.rand(shape, generator=g) * 2 - 1) * a, then the 11
biases the same way.  a = 0.15 / sqrt(2) at W = 256: doubling the fan-in at uniform(-a, a) keeps the per-layer gain of the 128-wide tests'
uniform(-0.15, 0.15).  SEEDS[F] was chosen (float64, the (37, 24) inputs, v0 and v2) so that alpha_linear's output is below zero on >= 12 % and
above zero on >= 12 % of the points: both sides of the ReLU that v2's sigma-only query leaves out are exercised.
Inputs: tests/test_gpu_mlp_fold._inputs(N, S, F).
The network: reference models.py:176-222 (v0, h = relu(p * bias)) and :495-538 (v2, h = relu(p + bias), forward_alpha without the ReLU), written
with torch.nn.functional.linear - which reproduces the reference's fp32 output bit for bit (tests/test_wide_refs.py).
"""
import functools
import math

import torch

from tests.test_gpu_mlp_fold import _embed, _inputs          # noqa: F401  (_inputs is re-exported)

WIDE = 256
A_WIDE = 0.15 / math.sqrt(2.0)
A_128 = 0.15
SEEDS = {12: 0, 20: 0, 36: 1, 40: 1}
FS = (12, 20, 36, 40)
SHAPES = ((1, 1), (5, 7), (4, 32), (37, 24))     # one point, a partial wave, exactly one 128-point tile, seven tiles with a partial last one
VARIANTS = {"v0": 0, "v2": 1}
GOLDEN = "mlp_wide_ref.npz"


def shapes_of(F, W):
    """(out, in) of the 11 layers in ops.MLP_ORDER"""
    return [(W, 63)] + [(W, W)] * 4 + [(W, W + 63), (W, F), (W, W), (1, W), (W // 2, W + 3), (3, W // 2)]


def weights(F, W=WIDE, seed=None, a=None):
    """-> (11 weights, 11 biases), fp32 CPU"""
    seed = SEEDS[F] if seed is None else seed
    a = (A_WIDE if W == WIDE else A_128) if a is None else a
    g = torch.Generator().manual_seed(seed)
    sh = shapes_of(F, W)
    ws = [((torch.rand(s, generator=g) * 2 - 1) * a).contiguous() for s in sh]
    bs = [((torch.rand((s[0],), generator=g) * 2 - 1) * a).contiguous() for s in sh]
    return ws, bs


def trunk(ws, bs, ndc, feat, variant):
    """-> (h5, alpha_linear(h5) before any ReLU) in the dtype of the arguments"""
    lin = torch.nn.functional.linear
    pts = _embed(ndc)
    bias = lin(feat, ws[6], bs[6])
    h = pts
    for i in range(6):
        p = lin(h, ws[i], bs[i])
        h = torch.relu(p + bias if variant else p * bias)
        if i == 4:
            h = torch.cat([pts, h], -1)
    return h, lin(h, ws[8], bs[8])


def tail(ws, bs, h5, dirs):
    """rgb of models.py:210-217 for any width; dirs (N, 3) per ray or (N, S, 3) per point"""
    lin = torch.nn.functional.linear
    d = dirs[:, None, :].expand(*h5.shape[:-1], 3) if dirs.dim() == h5.dim() - 1 else dirs
    hv = lin(torch.cat([lin(h5, ws[7], bs[7]), d], -1), ws[9], bs[9])
    return torch.sigmoid(lin(torch.relu(hv), ws[10], bs[10]))


def forward(ws, bs, ndc, feat, dirs, variant):
    """MVSNeRF.forward: (..., 4) = [rgb, relu(sigma)]"""
    h5, s = trunk(ws, bs, ndc, feat, variant)
    return torch.cat([tail(ws, bs, h5, dirs), torch.relu(s)], -1)


def forward_alpha(ws, bs, ndc, feat, variant):
    """MVSNeRF.forward_alpha: (..., 1); v0 clamps, v2 does not"""
    s = trunk(ws, bs, ndc, feat, variant)[1]
    return s if variant else torch.relu(s)


def to64(ts):
    return [t.double() for t in ts]


@functools.lru_cache(maxsize=None)
def reference(N, S, F, net_type, W=WIDE):
    """Computed once per case and shared: {"x": inputs, "w": (ws, bs), "f32": (raw, alpha) from the fp32 restatement on the CPU,
    "f64": (raw, alpha, alpha_linear output before the ReLU) in float64}.  Nobody writes to these."""
    v = VARIANTS[net_type]
    ndc, feat, dirs = _inputs(N, S, F)
    ws, bs = weights(F, W)
    with torch.no_grad():
        f32 = (forward(ws, bs, ndc, feat, dirs, v), forward_alpha(ws, bs, ndc, feat, v))
        w64, b64 = to64(ws), to64(bs)
        f64 = (forward(w64, b64, ndc.double(), feat.double(), dirs.double(), v), forward_alpha(w64, b64, ndc.double(), feat.double(), v),
               trunk(w64, b64, ndc.double(), feat.double(), v)[1])
    return {"x": (ndc, feat, dirs), "w": (ws, bs), "f32": f32, "f64": f64}


def rows(ndc, feat, dirs):
    """The reference's concatenated rows [embed(63) | feat | dir] (N, S, 63 + F + 3), per-ray directions repeated per sample"""
    return torch.cat([_embed(ndc), feat, dirs[:, None, :].expand(*ndc.shape[:-1], 3)], -1).contiguous()
