"""Writes tests/golden/caseF_scene_rays.npz from the reference's OWN get_ray_directions, get_rays and ray_marcher on the CPU (data/ray_utils.py;
needs the reference checkout, see oracle/ref_shim.py), composed as read_meta composes them (data/dtu_ft.py:173-183): two views of 6x7 pixels,
one with a rotated pose, each with its own intrinsics and near / far; S in {1, 5}, perturb in {0, 1} under torch.manual_seed (the draw is stored
too), lindisp both ways.  Only those inputs and outputs are stored (a few KB).

      python tests/gen_golden_scene_rays.py [--check]     (--check: regenerate and compare bit for bit)
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
H, W = 6, 7
SAMPLES, SEED = (1, 5), 11


def cameras():
    a, b = math.radians(17.0), math.radians(-8.0)
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    c2ws = np.stack([np.eye(4), np.eye(4)])
    c2ws[0, :3, 3] = [0.1, -0.2, 0.05]
    c2ws[1, :3, :3], c2ws[1, :3, 3] = Ry @ Rx, [-0.3, 0.15, 0.4]
    Ks = np.array([[[6.3, 0, 3.5], [0, 6.1, 3.0], [0, 0, 1]], [[5.9, 0, 3.25], [0, 6.4, 2.75], [0, 0, 1]]])
    near_far = np.array([[2.125, 4.525], [1.9, 5.3]])
    return c2ws.astype(np.float32), Ks.astype(np.float32), near_far.astype(np.float32)


def generate():
    from oracle import ref_shim
    ru = ref_shim.load_reference_ray_utils()
    c2ws, Ks, near_far = cameras()
    out = {"c2ws": c2ws, "intrinsics": Ks, "near_far": near_far}
    all_rays = []
    for m in range(2):
        K, c2w = Ks[m], torch.FloatTensor(c2ws[m])
        directions = ru.get_ray_directions(H, W, [K[0, 0], K[1, 1]], [K[0, 2], K[1, 2]])
        rays_o, rays_d = ru.get_rays(directions, c2w)
        all_rays += [torch.cat([rays_o, rays_d, near_far[m, 0] * torch.ones_like(rays_o[:, :1]), near_far[m, 1] * torch.ones_like(rays_o[:, :1])], 1)]
    all_rays = torch.cat(all_rays, 0)
    out["all_rays"] = all_rays.numpy().astype(np.float32)
    for S in SAMPLES:
        for lindisp in (0, 1):
            for perturb in (0, 1):
                torch.manual_seed(SEED + S)
                z = ru.ray_marcher(all_rays, N_samples=S, lindisp=bool(lindisp), perturb=perturb)[3]
                out[f"z_S{S}_l{lindisp}_p{perturb}"] = z.contiguous().numpy().astype(np.float32)
        torch.manual_seed(SEED + S)
        out[f"draw_S{S}"] = torch.rand((all_rays.shape[0], S)).numpy()
    return out


if __name__ == "__main__":
    from tests import scene_rays_refs as R
    out = generate()
    if "--check" in sys.argv:
        z = np.load(R.GOLDEN)
        assert sorted(z.files) == sorted(out), (z.files, sorted(out))
        for k in out:
            assert np.array_equal(z[k], out[k]), k
        print("golden matches bit for bit:", R.GOLDEN)
    else:
        np.savez_compressed(R.GOLDEN, **out)
        print("wrote", R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")
