"""Torch oracles of the empty-space kernels (csrc/sparse.hip): the live predicate, the compaction and expand_rows.  Device-agnostic.

A sample with NDC coordinate (x, y, z) is live iff a coordinate is non-finite, or some IN-GRID corner of its trilinear cell holds a density v with
~(v <= thr).  The cell is floor(ix), floor(iy), floor(iz), ix = ((gx + 1) / 2) * (W - 1), gx = x * 2 - 1, in fp32 with every operation rounded on
its own - torch's elementwise ops on float32 tensors do exactly that."""
import torch

GRIDS = ((6, 5, 7), (16, 24, 32))


def cell_coord(c, n):
    g = c * 2.0 - 1.0
    return ((g + 1.0) / 2.0) * float(n - 1)


def live_mask(density, ndc, thr):
    """density (D,H,W) fp32, ndc (...,3) fp32 -> bool (P,), P the number of samples in flat order."""
    D, H, W = density.shape
    flat = ndc.reshape(-1, 3).to(torch.float32)
    x, y, z = flat.unbind(-1)
    thr32 = torch.tensor(float(thr), dtype=torch.float32, device=density.device)
    fx, fy, fz = torch.floor(cell_coord(x, W)), torch.floor(cell_coord(y, H)), torch.floor(cell_coord(z, D))
    live = ~torch.isfinite(flat).all(-1)
    zero = torch.zeros_like(fx)
    for k in range(8):
        cx, cy, cz = fx + float(k & 1), fy + float((k >> 1) & 1), fz + float(k >> 2)
        inside = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1) & (cz >= 0) & (cz <= D - 1)
        xi, yi, zi = (torch.where(inside, c, zero).long() for c in (cx, cy, cz))
        v = density[zi, yi, xi]
        live = live | (inside & ~(v <= thr32))
    return live


def live_samples(density, ndc, thr, pts=None, dirs=None):
    """-> (count int, idx int32 (count,), ndc_c, pts_c | None, dir_c | None), the live rows in ascending flat order (torch.nonzero's)."""
    S = ndc.shape[-2]
    idx = torch.nonzero(live_mask(density, ndc, thr)).flatten()
    ndc_c = ndc.reshape(-1, 3)[idx]
    pts_c = None if pts is None else pts.reshape(-1, 3)[idx]
    dir_c = None if dirs is None else dirs[torch.div(idx, S, rounding_mode="floor")]
    return int(idx.numel()), idx.to(torch.int32), ndc_c, pts_c, dir_c


def expand_rows(src, idx, count, P):
    dst = torch.zeros((P, src.shape[1]), dtype=src.dtype, device=src.device)
    dst[idx[:count].long()] = src[:count]
    return dst


def coords(N, S, grid, g, lo=-0.15, hi=1.15):
    """(N,S,3) NDC coordinates in [lo, hi): the first samples sit on exact voxel positions, then one at 0, one at 1, one NaN, +inf and -inf each -
    as many of them as N*S has room for."""
    D, H, W = grid
    ndc = torch.rand((N, S, 3), generator=g) * (hi - lo) + lo
    flat = ndc.view(-1, 3)
    nan, inf = float("nan"), float("inf")
    special = [[i / (W - 1), (i % H) / (H - 1), (i % D) / (D - 1)] for i in range(W)]
    special += [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [nan, 0.5, 0.5], [0.5, inf, 0.5], [0.5, 0.5, -inf], [1.0 + 1e-6, 0.5, 0.5], [3e38, -3e38, 0.5]]
    for i, c in enumerate(special[:flat.shape[0]]):
        flat[i] = torch.tensor(c)
    return ndc


def sparse_density(grid, g, empty=0.8, nan_voxel=False):
    """(D,H,W) densities in (0,1] with a share `empty` of exact zeros (and one NaN voxel on request)."""
    d = torch.rand(grid, generator=g) + 1e-3
    d = d * (torch.rand(grid, generator=g) >= empty)
    if nan_voxel:
        d[grid[0] // 2, grid[1] // 2, grid[2] // 2] = float("nan")
    return d.contiguous()
