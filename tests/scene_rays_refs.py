"""Elementwise torch-CPU restatement of csrc/scene_rays.hip (mvsnerf_scene_rays_gather_fwd / _march_fwd): every operation of the kernels'
arithmetic is its own torch op, so every rounding is torch's.  What the reference computes in read_meta (data/dtu_ft.py:143-188,
data/blender.py:49-85: get_ray_directions, get_rays, the [o | d | near | far] rows, ToTensor, the blend onto white) and in ray_marcher
(data/ray_utils.py:152-197), per sampled index.  tests/golden/caseF_scene_rays.npz holds the reference's own outputs for a small scene."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caseF_scene_rays.npz")


def bank_f32(c2ws, intrinsics, near_far, M):
    """(c2ws (M,3,4), intrinsics (M,3,3), near_far (M,2)) fp32 CPU, broadcast as rays.SceneRays broadcasts them."""
    c2ws = torch.as_tensor(c2ws).to(torch.float32)[:, :3, :4]
    K = torch.as_tensor(intrinsics).to(torch.float32)
    K = K.expand(M, 3, 3) if K.dim() == 2 else K
    nf = torch.as_tensor(near_far).to(torch.float32)
    nf = nf.expand(M, 2) if nf.dim() == 1 else nf
    return c2ws, K, nf


def gather_ref(images, c2ws, intrinsics, near_far, depths, idx):
    """images (M,H,W,3|4) uint8, idx (B,) int64 -> rays (B,8), rgb (B,3), depth (B,) | None, mask (B,) bool; an index outside the bank: zero rows."""
    images = torch.as_tensor(images)
    M, H, W, C = images.shape
    c2ws, K, nf = bank_f32(c2ws, intrinsics, near_far, M)
    if C == 3:
        images = torch.cat((images, torch.full((M, H, W, 1), 255, dtype=torch.uint8)), -1)
    idx = torch.as_tensor(idx).to(torch.int64)
    valid = (idx >= 0) & (idx < M * H * W)
    i = torch.where(valid, idx, torch.zeros_like(idx))
    m, y, x = i // (H * W), (i % (H * W)) // W, i % W
    Km, Rm = K[m], c2ws[m]
    dx = (x.to(torch.float32) - Km[:, 0, 2]) / Km[:, 0, 0]                       # data/ray_utils.py:27
    dy = (y.to(torch.float32) - Km[:, 1, 2]) / Km[:, 1, 1]
    dz = torch.ones_like(dx)
    d = torch.stack([(dx * Rm[:, k, 0] + dy * Rm[:, k, 1]) + dz * Rm[:, k, 2] for k in range(3)], -1)
    rays = torch.cat([Rm[:, :, 3], d, nf[m]], 1)
    px = images.reshape(-1, 4)[i]
    c = px.to(torch.float32).div(255)                                            # ToTensor
    a = c[:, 3:]
    rgb = c[:, :3] * a + (1 - a)                                                 # data/blender.py:70
    mask = px[:, 3] > 0
    v = valid[:, None]
    zero = torch.zeros(())
    depth = None if depths is None else torch.where(valid, torch.as_tensor(depths).to(torch.float32).reshape(-1)[i], zero)
    return torch.where(v, rays, zero), torch.where(v, rgb, zero), depth, mask & valid


def march_depths(near, far, S, lindisp, perturb, jitter):
    """ray_marcher's z_vals (data/ray_utils.py:176-191) with the uniform draw supplied: near, far (B,1), jitter (B,S) | None -> (B,S)."""
    steps = torch.linspace(0, 1, S)
    z = near * (1 - steps) + far * steps if not lindisp else 1 / (1 / near * (1 - steps) + 1 / far * steps)
    z = z.expand(near.shape[0], S)
    if perturb > 0:
        mid = 0.5 * (z[:, :-1] + z[:, 1:])
        upper, lower = torch.cat([mid, z[:, -1:]], -1), torch.cat([z[:, :1], mid], -1)
        z = lower + (upper - lower) * (perturb * jitter)
    return z


def march_ref(images, c2ws, intrinsics, near_far, idx, S, jitter=None, perturb=0.0, lindisp=False):
    """-> rays (B,8), rgb (B,3), z (B,S); rows of an index outside the bank are zero."""
    rays, rgb, _, _ = gather_ref(images, c2ws, intrinsics, near_far, None, idx)
    M, H, W = torch.as_tensor(images).shape[:3]
    idx = torch.as_tensor(idx).to(torch.int64)
    valid = ((idx >= 0) & (idx < M * H * W))[:, None]
    one = torch.ones(())
    near, far = torch.where(valid, rays[:, 6:7], one), torch.where(valid, rays[:, 7:8], one)        # (no 1 / 0 in the rows that are zeroed below)
    z = march_depths(near, far, S, lindisp, perturb, jitter)
    return rays, rgb, torch.where(valid, z, torch.zeros(()))


def rays_d_bound(c2ws, intrinsics, H, W):
    """Per ray and component 6 * 2^-24 * sum_k |dir_k R[c][k]|: two fp32 evaluations of one 3-term dot product (the reference's is a matmul
    whose order and contraction are the BLAS's).  c2ws (3,4) | (4,4), intrinsics (3,3) of ONE view -> (H*W, 3)."""
    c2w, K = torch.as_tensor(c2ws).to(torch.float64), torch.as_tensor(intrinsics).to(torch.float64)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    dirs = torch.stack([(x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1], torch.ones_like(x)], -1).reshape(-1, 1, 3)
    return 6 * 2.0 ** -24 * (dirs.abs() * c2w[:3, :3].abs()[None]).sum(-1)


def golden():
    return {k: v for k, v in np.load(GOLDEN).items()}
