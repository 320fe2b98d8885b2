"""Torch restatement of early ray termination for the tests: which samples of a dense raw (N,S,4) a march with `eps` and
stop_every = G zeroes, where each ray stops, and which rays' decisions a fp32 run may take differently.

The rule: alpha = 1 - exp(-sigma), T(b) = prod_{s < b} ((1 - alpha_s) + 1e-10), boundaries b_k = k G for k = 1 .. ceil(S / G) - 1; a ray stops at the
first boundary with T(b_k) < eps (a NaN T never stops) and every sample s >= b_k of it becomes (0,0,0,0).  The decision is taken here on the float64 T
of the fp32 raw; the kernels take it on the fp32 product, whose relative error is below S * 2^-23 < 1e-4 for every S the tests use - so a ray is
UNDECIDED when its float64 T lies within a relative 1e-4 of eps at some boundary up to and including the one it stops at, and the tests leave such
rays out of their bit-exact comparisons.  (Behind a stop the decision is moot: the zeroed samples leave T where it was.)"""
import torch

UNDECIDED_REL = 1e-4


def boundaries(S, G):
    return list(range(G, S, G))


def transmittance64(raw):
    """(N, S + 1) float64: T before sample b, b = 0 .. S, as compositing forms it from the fp32 sigma (expf's argument and 1 - alpha rounded in fp32
    would differ in the last bit only; float64 throughout is the yardstick)."""
    sigma = raw[..., 3].double()
    f = (1.0 - (1.0 - torch.exp(-sigma))) + 1e-10
    T = torch.ones((raw.shape[0], raw.shape[1] + 1), dtype=torch.float64, device=raw.device)
    T[:, 1:] = torch.cumprod(f, 1)
    return T


def early_stop(raw, eps, G):
    """raw (N,S,4), eps in [0,1), G >= 1 -> (zeroed raw, stop (N,) int64: the boundary b_k the ray stopped at or -1, undecided (N,) bool)."""
    N, S = raw.shape[:2]
    T = transmittance64(raw)
    stop = torch.full((N,), -1, dtype=torch.int64, device=raw.device)
    undecided = torch.zeros((N,), dtype=torch.bool, device=raw.device)
    for b in boundaries(S, G):
        going = stop < 0
        undecided |= going & ((T[:, b] - eps).abs() <= UNDECIDED_REL * eps) & (eps > 0)
        stop = torch.where(going & (T[:, b] < eps), torch.full_like(stop, b), stop)
    s = torch.arange(S, device=raw.device)[None, :]
    dropped = (stop[:, None] >= 0) & (s >= stop[:, None])
    return torch.where(dropped[..., None], torch.zeros_like(raw), raw), stop, undecided


def composite64(raw, z, white_bkgd=False):
    """renderer.py:65-92 in float64 (dist ignored, as the kernels): -> rgb (N,3), acc (N,), depth (N,), weights (N,S)."""
    raw, z = raw.double(), z.double()
    alpha = 1.0 - torch.exp(-raw[..., 3])
    f = (1.0 - alpha) + 1e-10
    T = torch.cat([torch.ones_like(f[:, :1]), torch.cumprod(f, 1)[:, :-1]], 1)
    w = alpha * T
    rgb, acc, depth = (w[..., None] * raw[..., :3]).sum(1), w.sum(1), (w * z).sum(1)
    if white_bkgd:
        rgb = rgb + (1.0 - acc)[:, None]
    return rgb, acc, depth, w
