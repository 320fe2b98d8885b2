"""TEST INFRASTRUCTURE: the definition of the order-independent volume-gradient scatter (csrc/sample.hip, mvsnerf_volume_sample_bwd_det), restated in CPU
torch with integers, so that the kernel's accumulators can be predicted exactly instead of approached with a tolerance.

  volume_sample_bwd_det_scatter_kernel   coordinates, bounds test, weights, index      -> corners
                                         the fp32 product rounded once to 2^(e - 40)   -> scatter_ints
  volume_sample_bwd_det_finish_kernel    the sum back in fp32                          -> finish

The coordinate arithmetic is fp32, operation for operation as in the kernel (which is compiled with `fp contract(off)`: plain IEEE operations, the ones
torch's CPU fp32 performs).  `inputs` builds the rows that tests/test_scatter_det_refs.py (CPU) and tests/test_gpu_scatter_det.py (GPU) share.
"""
import math

import torch

FRAC_BITS = 40                                  # a contribution resolves 2^-40 of 2^e > max |g|
MAX_POINTS = 1 << 22                            # the entry refuses more: 2^22 contributions of at most 2^40 keep |sum| <= 2^62

# (C, (D, H, W), P): the shapes both test files run
SHAPES = [(8, (6, 7, 9), 5000), (20, (5, 6, 7), 3001), (8, (16, 24, 32), 40000), (12, (5, 6, 7), 1), (12, (5, 6, 7), 37)]
N_EDGE_ROWS = 9


def inputs(C, dims, P, seed=None):
    """-> (ndc (P,3), g (P,C)) fp32: coordinates uniform in [-0.05, 1.05] with half of the points in ONE (x, y) column (many contributions per voxel).
    When P > 9 the last nine rows are edges: one coordinate exactly 0 and exactly 1 on each axis (six rows), then one NaN, one +inf and one -inf coordinate
    (the kernel forms an index only after its bounds test on the FLOAT corner, sample.hip, so these rows touch no memory)."""
    gen = torch.Generator().manual_seed(C * 1000 + dims[0] * 10 + P if seed is None else seed)
    ndc = torch.rand((P, 3), generator=gen) * 1.1 - 0.05
    ndc[: P // 2, :2] = ndc[:1, :2]
    g = torch.randn((P, C), generator=gen)
    if P > N_EDGE_ROWS:
        t = P - N_EDGE_ROWS
        for axis in range(3):
            ndc[t + 2 * axis, axis] = 0.0
            ndc[t + 2 * axis + 1, axis] = 1.0
        ndc[t + 6, 0] = float("nan")
        ndc[t + 7, 1] = float("inf")
        ndc[t + 8, 2] = float("-inf")
    return ndc.contiguous(), g.contiguous()


def corners(ndc, dims):
    """ndc (P,3) fp32 (x -> W, y -> H, z -> D), dims = (D, H, W) -> eight (in-bounds mask (P,) bool, weight (P,) fp32, voxel (P,) int64) in the kernel's
    corner order k = zc * 4 + yc * 2 + xc; voxel = (z * H + y) * W + x, 0 where the mask is False.  A NaN or infinite coordinate fails every bounds test."""
    D, H, W = dims
    ndc = ndc.reshape(-1, 3).to(torch.float32)
    one, two = torch.tensor(1.0), torch.tensor(2.0)
    i, f = [], []
    for axis, n in ((0, W), (1, H), (2, D)):
        gk = ndc[:, axis] * two - one                                     # gx = ndc * 2 - 1
        i.append(((gk + one) / two) * torch.tensor(float(n - 1)))         # ix = ((gx + 1) / 2) * (W - 1)
        f.append(torch.floor(i[-1]))
    (ix, iy, iz), (fx, fy, fz) = i, f
    out = []
    for zc in (0, 1):
        for yc in (0, 1):
            for xc in (0, 1):
                cx, cy, cz = fx + float(xc), fy + float(yc), fz + float(zc)
                ok = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1) & (cz >= 0) & (cz <= D - 1)          # on the float corner
                w = ((ix - fx) if xc else ((fx + one) - ix)) * ((iy - fy) if yc else ((fy + one) - iy)) * ((iz - fz) if zc else ((fz + one) - iz))
                zero = torch.zeros_like(cx)
                vox = (torch.where(ok, cz, zero).long() * H + torch.where(ok, cy, zero).long()) * W + torch.where(ok, cx, zero).long()
                out.append((ok, w, vox))
    return out


def exponent(g):
    """e of the fixed-point scale 2^(40 - e): the frexp exponent of max |g| (max |g| in [2^(e-1), 2^e)); 0 for an all-zero g."""
    m = float(g.abs().max()) if g.numel() else 0.0
    if not math.isfinite(m):
        raise ValueError("the integer form is defined for finite gradients only")
    return math.frexp(m)[1] if m else 0


def products(ndc, g, dims):
    """[(flat element index (K*C,) int64, fp32 product g * w (K*C,))] per corner: the contributions of the float-atomic and of the fixed-point scatter."""
    C = g.shape[1]
    ch = torch.arange(C)[None]
    return [((vox[ok, None] * C + ch).reshape(-1), (g[ok] * w[ok, None]).reshape(-1)) for ok, w, vox in corners(ndc, dims)]


def scatter_ints(ndc, g, dims, e=None):
    """-> (acc (D,H,W,C) int64, e): every fp32 product g * w rounded ONCE, round_half_even(double(prod) * 2^(40 - e)), and summed in int64.
    e: the exponent of max |g| over the elements of g, or the caller's (a part of a larger input is rounded on the whole input's grid)."""
    D, H, W = dims
    C = g.shape[1]
    g = g.to(torch.float32)
    if e is None:
        e = exponent(g)
    acc = torch.zeros(D * H * W * C, dtype=torch.int64)
    if float(g.abs().max() if g.numel() else 0.0) != 0.0:
        scale = 2.0 ** (FRAC_BITS - e)
        for idx, prod in products(ndc, g, dims):
            acc.index_add_(0, idx, torch.round(prod.double() * scale).long())         # torch.round: half to even, as __double2ll_rn
    return acc.view(D, H, W, C), e


def finish(acc, e):
    """float(double(acc) * 2^(e - 40)): what the finish pass adds to a zeroed volume gradient."""
    return (acc.double() * 2.0 ** (e - FRAC_BITS)).float()
