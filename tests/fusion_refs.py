"""TEST INFRASTRUCTURE: restatements, in CPU torch, of the pieces of the reference's fusion script that csrc/fusion.hip implements.

  update_volume            train_mvs_nerf_fusion_finetuning_pl.py:35-76     -> splat_corners / splat_sums / splat_ints
  the normalisation        train_mvs_nerf_fusion_finetuning_pl.py:190-192   -> normalise
  dda                      data/ray_utils.py:143-150                         -> dda
  ray_marcher(bbox_3D=)    data/ray_utils.py:152-197 (+ the box coordinates of the script's :263)   -> ray_march_bbox

The index arithmetic is fp32 exactly as in the reference.  Where the reference is ill-defined - `vol[..., idx] += x` with repeated indices keeps ONE of
the colliding writes - the restatements ACCUMULATE (index_add_), which is what the product defines; on inputs whose eight passes are each free of
collisions the two agree, and tests/golden/caseD_fusion.npz (tests/gen_golden_fusion.py, the reference's own function) is such an input.
"""
import torch

SCALE = 2.0 ** 32
LIMIT = 2.0 ** 20
SHIFTS = [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]]       # :68


def splat_corners(ndc, dims):
    """ndc (P,3) fp32 box coordinates (x -> W, y -> H, z -> D), dims = (D, H, W) -> (kept (P,) bool, [(weight (K,) fp32, voxel (K,) int64)] per shift),
    voxel = (d * H + h) * W + w."""
    D, H, W = dims
    ndc = ndc.reshape(-1, 3).to(torch.float32)
    voxel_size = 1.0 / (torch.tensor([W, H, D]) - 1)                      # :43 (fp32: int64 tensor under a Python float)
    v = ndc / voxel_size.view(1, 3)                                       # :52 - a division
    local = v - torch.floor(v)                                            # :53
    finite = torch.isfinite(v).all(-1)                                    # .long() of a non-finite value is INT64_MIN on the CPU: dropped by :58
    idx = torch.where(finite[:, None], v, torch.full_like(v, -2.0)).long()    # :54 - truncation toward zero
    kept = ((idx[:, 0] >= 0) & (idx[:, 1] >= 0) & (idx[:, 2] >= 0) & (idx[:, 0] < W - 1) & (idx[:, 1] < H - 1) & (idx[:, 2] < D - 1))      # :58-59
    idx, local = idx[kept], local[kept]
    out = []
    for x, y, z in SHIFTS:
        wl = torch.abs(local - torch.tensor([x, y, z]).float().view(1, 3))                      # :70-71
        wl = (wl[:, 0] * wl[:, 1]) * wl[:, 2]                                                   # :72
        out.append((wl, ((idx[:, 2] + x) * H + (idx[:, 1] + y)) * W + (idx[:, 0] + z)))         # :74 - x and z swapped
    return kept, out


def splat_sums(ndc, feat, alpha, dims, dtype=torch.float64):
    """-> (feat sums (C,D,H,W), alpha sums (D,H,W), weight sums (D,H,W), contribution count (D,H,W) int64); fp32 products (:75-76) accumulated in `dtype`
    in the reference's order (pass by pass, points in order)."""
    D, H, W = dims
    C = feat.shape[-1]
    kept, corners = splat_corners(ndc, dims)
    feat, alpha = feat.reshape(-1, C).float()[kept], alpha.reshape(-1).float()[kept]
    n = D * H * W
    fs, as_, ws, cnt = torch.zeros((n, C), dtype=dtype), torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=torch.int64)
    for wl, vox in corners:
        ws.index_add_(0, vox, wl.to(dtype))
        fs.index_add_(0, vox, (wl[:, None] * feat).to(dtype))
        as_.index_add_(0, vox, (wl * alpha).to(dtype))
        cnt.index_add_(0, vox, torch.ones_like(vox))
    return fs.t().reshape(C, D, H, W).contiguous(), as_.view(D, H, W), ws.view(D, H, W), cnt.view(D, H, W)


def splat_ints(ndc, feat, alpha, dims):
    """The integer form: every fp32 product rounded once, round(double(prod) * 2^32) to nearest-even, summed in int64; a product with |prod| >= 2^20
    or not finite is left out and counted.  -> (words (D,H,W,C+4) int64: C feature sums, alpha, weight, 2 zero pads; refused count)."""
    D, H, W = dims
    C = feat.shape[-1]
    kept, corners = splat_corners(ndc, dims)
    feat, alpha = feat.reshape(-1, C).float()[kept], alpha.reshape(-1).float()[kept]
    acc = torch.zeros((D * H * W, C + 4), dtype=torch.int64)
    refused = 0
    for wl, vox in corners:
        prod = torch.cat([wl[:, None] * feat, (wl * alpha)[:, None], wl[:, None]], 1)           # fp32 products
        ok = prod.abs() < LIMIT                                                                  # False for NaN and inf
        refused += int((~ok).sum())
        q = torch.round(torch.where(ok, prod, torch.zeros_like(prod)).double() * SCALE).long()
        acc[:, :C + 2].index_add_(0, vox, q)
    return acc.view(D, H, W, C + 4), refused


def normalise(feat_sum, alpha_sum, weight_sum):
    """:190-192 in fp32: -> (feat volume (C,D,H,W), density volume (D,H,W))."""
    inv = 1.0 / (weight_sum.float() + 1e-6)
    return feat_sum.float() * inv, alpha_sum.float() * inv


def dda(rays_o, rays_d, bbox_3D):
    """data/ray_utils.py:143-150."""
    inv_ray_d = 1.0 / (rays_d + 1e-6)
    t_min = (bbox_3D[:1] - rays_o) * inv_ray_d
    t_max = (bbox_3D[1:] - rays_o) * inv_ray_d
    t = torch.stack((t_min, t_max))
    return torch.max(torch.min(t, dim=0)[0], dim=-1, keepdim=True)[0], torch.min(torch.max(t, dim=0)[0], dim=-1, keepdim=True)[0]


def ray_march_bbox(rays, bbox_3D, N_samples, lindisp=False, perturb=0, jitter=None):
    """data/ray_utils.py:166-197 with bbox_3D and the uniform draw of :190 supplied -> (pts (N,S,3), ndc (N,S,3), z (N,S)); ndc as the script's :263."""
    N = rays.shape[0]
    rays_o, rays_d = rays[:, 0:3], rays[:, 3:6]
    near, far = dda(rays_o, rays_d, bbox_3D)                                                    # :173
    z_steps = torch.linspace(0, 1, N_samples)
    z = near * (1 - z_steps) + far * z_steps if not lindisp else 1 / (1 / near * (1 - z_steps) + 1 / far * z_steps)      # :177-180
    z = z.expand(N, N_samples)
    if perturb > 0:                                                                             # :184-191
        mid = 0.5 * (z[:, :-1] + z[:, 1:])
        upper, lower = torch.cat([mid, z[:, -1:]], -1), torch.cat([z[:, :1], mid], -1)
        z = lower + (upper - lower) * (perturb * jitter)
    pts = rays_o.unsqueeze(1) + rays_d.unsqueeze(1) * z.unsqueeze(2)                            # :193-194
    ndc = (pts - bbox_3D[0].view(1, 1, 3)) / (bbox_3D[1] - bbox_3D[0]).view(1, 1, 3)            # script :263
    return pts, ndc, z.contiguous()
