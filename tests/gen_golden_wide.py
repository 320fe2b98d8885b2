"""Writes tests/golden/mlp_wide_ref.npz from the reference's OWN MVSNeRF at netwidth 256 on the CPU (needs the reference checkout, see
oracle/ref_shim.py): MVSNeRF(D=6, W=256, net_type in {v0, v2}).forward and .forward_alpha on the (37, 24) rows [embed(63) | feat | dir] of
tests/wide_refs.py, for feat_dim 12, 20, 36, 40.  The weights are the seeded recipe of tests/wide_refs.py, loaded through the reference's own
state_dict keys.  Only fp32 outputs are stored (about 140 KB), never weights or inputs: the test rebuilds both from the seeds.

      python tests/gen_golden_wide.py [--check]     (--check: regenerate and compare bit for bit)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
N, S = 37, 24


def generate():
    from mvsnerf_amd.ops import MLP_ORDER
    from oracle import ref_shim
    from tests import wide_refs as R
    ref_models = ref_shim.load_reference()[0]
    out = {}
    for net_type in R.VARIANTS:
        for F in R.FS:
            ndc, feat, dirs = R._inputs(N, S, F)
            ws, bs = R.weights(F)
            net = ref_models.MVSNeRF(D=6, W=R.WIDE, input_ch_pts=63, input_ch_views=3, input_ch_feat=F, skips=[4], net_type=net_type)
            sd = {}
            for name, w, b in zip(MLP_ORDER, ws, bs):
                sd[f"nerf.{name}.weight"], sd[f"nerf.{name}.bias"] = w, b
            net.load_state_dict(sd)            # strict: the keys and shapes are the reference's
            x = R.rows(ndc, feat, dirs)
            with torch.no_grad():
                out[f"{net_type}_F{F}_raw"] = net(x).numpy().astype(np.float32)
                out[f"{net_type}_F{F}_alpha"] = net.forward_alpha(x[..., :63 + F].contiguous()).numpy().astype(np.float32)
    return out


if __name__ == "__main__":
    from tests import wide_refs as R
    path = os.path.join(ROOT, "tests", "golden", R.GOLDEN)
    out = generate()
    if "--check" in sys.argv:
        z = np.load(path)
        assert sorted(z.files) == sorted(out), (z.files, sorted(out))
        for k in out:
            assert np.array_equal(z[k], out[k]), k
        print("golden matches bit for bit:", path)
    else:
        np.savez(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes")
