"""Torch restatements of csrc/occupancy.hip: the node grid of a (D,H,W) volume, the inverse of get_ndc_coordinate in a chosen dtype, and the
grid-clipped maximum filter.  Device-agnostic; nothing here calls the library."""
import math

import torch
import torch.nn.functional as F


def node_grid(D, H, W, planes=None, dtype=torch.float32):
    """(n,3) rows (i/(W-1), j/(H-1), k/(D-1)) in [k][j][i] order for planes [d0, d1); an axis of size 1 gives 0.  In float32 arange(n) / (n-1) is the
    one correctly rounded division per coordinate the kernel does."""
    d0, d1 = (0, D) if planes is None else planes

    def axis(n, lo=0, hi=None):
        a = torch.arange(lo, n if hi is None else hi, dtype=dtype)
        return a / (n - 1) if n > 1 else torch.zeros_like(a)
    z, y, x = torch.meshgrid(axis(D, d0, d1), axis(H), axis(W), indexing="ij")
    return torch.stack((x, y, z), -1).reshape(-1, 3)


def ndc_to_world(ndc, K_ref, c2w_ref, near_far, ref_hw, pad=0, lindisp=False, dtype=torch.float64):
    """The inverse of utils.get_ndc_coordinate / mvsnerf_ray_points_fwd, every step in `dtype` (the camera inverse included): undo the pad,
    pixel = q * (size - 1), depth from z_ndc, K^-1 (u z, v z, z), then c2w."""
    ndc, K, c2w = ndc.to(dtype), K_ref.to(dtype), c2w_ref.to(dtype)
    near, far = (float(v) for v in torch.as_tensor(near_far).reshape(-1)[:2])
    H_img, W_img = ref_hw
    x, y, zn = ndc.unbind(-1)
    if pad > 0:
        wf, hf = W_img / 4.0, H_img / 4.0
        x = (x * (wf + 2 * pad) - pad) / wf
        y = (y * (hf + 2 * pad) - pad) / hf
    u, v = x * (W_img - 1), y * (H_img - 1)
    z = 1.0 / (1.0 / near + zn * (1.0 / far - 1.0 / near)) if lindisp else near + zn * (far - near)
    cam = torch.stack((u * z, v * z, z), -1) @ torch.linalg.inv(K).T
    return cam @ c2w[:3, :3].T + c2w[:3, 3]


def max_dilate3d(x, r):
    """(D,H,W) -> the maximum over the (2r+1)^3 window clipped to the grid; max_pool3d pads with -inf and propagates NaN on the CPU."""
    return F.max_pool3d(x[None, None], 2 * r + 1, 1, r)[0, 0]


def camera(seed=0, ref_hw=(64, 96), dtype=torch.float32):
    """A rotated and translated reference camera: (K (3,3), c2w (4,4), w2c (4,4), near_far (2,)).  w2c is the float64 inverse of the fp32 c2w, rounded."""
    g = torch.Generator().manual_seed(seed)
    H, W = ref_hw
    K = torch.tensor([[1.1 * W, 0.0, W / 2 - 0.7], [0.0, 1.05 * W, H / 2 + 0.4], [0.0, 0.0, 1.0]])
    ax = torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0).double()
    a = 0.6
    Kx = torch.tensor([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + math.sin(a) * Kx + (1 - math.cos(a)) * (Kx @ Kx)
    c2w = torch.eye(4, dtype=torch.float64)
    c2w[:3, :3], c2w[:3, 3] = R, torch.tensor([0.4, -0.3, 0.25], dtype=torch.float64)
    c2w = c2w.float()
    w2c = torch.linalg.inv(c2w.double()).float()
    return K.to(dtype), c2w.to(dtype), w2c.to(dtype), torch.tensor([2.125, 4.525], dtype=dtype)


def planted(shape, seed=0):
    """Random values with -inf, +inf and NaN planted in the interior, on a face and in a corner (as many as the shape has room for)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    D, H, W = shape
    spots = [((D // 2, H // 2, W // 2), float("nan")), ((0, H // 2, W // 3), float("inf")), ((D - 1, H - 1, W - 1), float("nan")),
             ((D // 2, 0, W - 1), -float("inf")), ((0, 0, 0), -float("inf")), ((D - 1, H // 3, 2 * W // 3), float("inf"))]
    if D * H * W > len(spots):
        for (k, j, i), v in spots:
            x[k, j, i] = v
    return x
