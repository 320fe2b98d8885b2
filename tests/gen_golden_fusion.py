"""Writes tests/golden/caseD_fusion.npz from the reference's OWN functions on the CPU (needs the reference checkout, see oracle/ref_shim.py):

  * `update_volume` (train_mvs_nerf_fusion_finetuning_pl.py:35-76).  The script cannot be imported here (pytorch_lightning, the datasets, argument parsing
    at import), so the one function is cut out of its syntax tree and executed with `torch` in scope.  Inputs: a 10 x 12 x 14 volume, 20 channels, 300 points
    in 300 DISTINCT voxel cells - within each of the function's eight passes no two writes collide, so its `+=` is a true accumulation - the five edge points
    and one point in (-1, 0) voxel units.
  * `dda` / `ray_marcher(bbox_3D=)` (data/ray_utils.py:143-197) through oracle.ref_shim.load_reference_ray_utils(), with the uniform draw of :190 recorded.

Only inputs and outputs are stored.      python tests/gen_golden_fusion.py [--check]     (--check: regenerate and compare bit for bit)
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "caseD_fusion.npz")
DIMS = (10, 12, 14)            # D, H, W
C = 20
EDGE = [[-0.2, 0.5, 0.5], [0.5, 1.2, 0.5], [0.5, 0.5, 1.0], [1.0, 0.3, 0.3], [0.3, 1.0, 0.3]]
NEGATIVE = [-0.03, 0.52, 0.47]         # x in (-1, 0) voxel units: lands on voxel 0
MARCH_CASES = [(0.0, False), (1.0, False), (0.0, True), (0.5, True)]      # (perturb, lindisp)
MARCH_N, MARCH_S = 37, 16


def reference_update_volume():
    from oracle import ref_shim
    path = os.path.join(ref_shim.REF_ROOT, "train_mvs_nerf_fusion_finetuning_pl.py")
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "update_volume"]
    assert len(fn) == 1
    scope = {"torch": torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), scope)
    return scope["update_volume"]


def splat_inputs():
    D, H, W = DIMS
    g = torch.Generator().manual_seed(20)
    taken = {(12, 3, 2), (0, 5, 4)}            # the cells of the kept edge point [1.0, .3, .3] and of NEGATIVE
    cells = [(x, y, z) for z in range(D - 1) for y in range(H - 1) for x in range(W - 1) if (x, y, z) not in taken]
    pick = torch.randperm(len(cells), generator=g)[:300]
    idx = torch.tensor([cells[i] for i in pick.tolist()], dtype=torch.float32)
    u = torch.rand((300, 3), generator=g) * 0.9 + 0.05
    ndc = (idx + u) / torch.tensor([W - 1, H - 1, D - 1], dtype=torch.float32)
    ndc = torch.cat([ndc, torch.tensor(EDGE + [NEGATIVE], dtype=torch.float32)], 0)
    feat = torch.randn((ndc.shape[0], C), generator=g) * 2.0
    alpha = torch.rand((ndc.shape[0],), generator=g)
    return ndc, feat, alpha


def march_inputs():
    g = torch.Generator().manual_seed(21)
    bbox = torch.tensor([[-1.0, -0.8, 2.5], [1.0, 0.9, 4.5]])
    o = torch.cat([torch.rand((MARCH_N, 2), generator=g) * 0.6 - 0.3, torch.rand((MARCH_N, 1), generator=g) * 0.2], 1)
    d = torch.cat([torch.rand((MARCH_N, 2), generator=g) * 0.5 - 0.25, torch.ones((MARCH_N, 1))], 1)
    d[3, 0] = 0.0                              # a direction component of exactly 0
    d[4, 1] = 0.0
    d[5, :2] = torch.tensor([2.0, 1.5])        # misses the box: near > far
    d[6, :2] = torch.tensor([-1.7, 0.1])
    o[7] = torch.tensor([0.2, 0.1, 3.0])       # starts inside the box
    rays = torch.cat([o, d, torch.full((MARCH_N, 1), 2.0), torch.full((MARCH_N, 1), 6.0)], 1)
    return rays, bbox


def generate():
    from oracle import ref_shim
    out = {}
    ndc, feat, alpha = splat_inputs()
    D, H, W = DIMS
    vol, sig, wts = torch.zeros((1, C, D, H, W)), torch.zeros((1, 1, D, H, W)), torch.zeros((1, 1, D, H, W))
    P = ndc.shape[0]
    with torch.no_grad():
        reference_update_volume()(vol, sig, wts, feat.view(P, 1, C), ndc.view(P, 1, 3), alpha.view(P, 1, 1), torch.zeros((P, 1, 1)))
    out.update(splat_ndc=ndc, splat_feat=feat, splat_alpha=alpha, splat_dims=torch.tensor(DIMS), splat_volume=vol[0], splat_alpha_volume=sig[0, 0],
               splat_weight_volume=wts[0, 0])
    ru = ref_shim.load_reference_ray_utils()
    rays, bbox = march_inputs()
    out.update(march_rays=rays, march_bbox=bbox)
    with torch.no_grad():
        near, far = ru.dda(rays[:, :3], rays[:, 3:6], bbox)
        out.update(march_near=near, march_far=far)
        for k, (perturb, lindisp) in enumerate(MARCH_CASES):
            torch.manual_seed(100 + k)
            draw = torch.rand((MARCH_N, MARCH_S))
            torch.manual_seed(100 + k)                                   # ray_marcher draws the same numbers (:190)
            pts, _, _, z = ru.ray_marcher(rays, N_samples=MARCH_S, lindisp=lindisp, perturb=perturb, bbox_3D=bbox)
            nd = (pts - bbox[0].view(1, 1, 3)) / (bbox[1] - bbox[0]).view(1, 1, 3)                 # the script's :263
            assert torch.isfinite(pts).all() and torch.isfinite(z).all()
            out.update({f"march{k}_perturb": torch.tensor(perturb), f"march{k}_lindisp": torch.tensor(int(lindisp)), f"march{k}_draw": draw,
                        f"march{k}_pts": pts, f"march{k}_ndc": nd, f"march{k}_z": z})
    return {k: np.ascontiguousarray(v.numpy()) for k, v in out.items()}


def check():
    new, old = generate(), np.load(OUT)
    assert sorted(new) == sorted(old.files), sorted(set(new) ^ set(old.files))
    for k, v in new.items():
        assert v.dtype == old[k].dtype and v.shape == old[k].shape and v.tobytes() == old[k].tobytes(), f"{k} differs from the committed golden"
    return len(new)


if __name__ == "__main__":
    if "--check" in sys.argv:
        print(f"caseD_fusion.npz: {check()} arrays regenerate bit for bit")
    else:
        np.savez_compressed(OUT, **generate())
        print("wrote", OUT, os.path.getsize(OUT), "bytes")
