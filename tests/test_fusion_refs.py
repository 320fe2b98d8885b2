"""CPU: the restatements of tests/fusion_refs.py against the reference's own outputs (tests/golden/caseD_fusion.npz, written by
tests/gen_golden_fusion.py from train_mvs_nerf_fusion_finetuning_pl.py:35-76 and data/ray_utils.py:143-197)."""
import os

import numpy as np
import pytest
import torch

from tests import fusion_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "caseD_fusion.npz")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _dims(gold):
    return tuple(int(v) for v in gold["splat_dims"])


def test_golden_points_cover_the_edges(gold):
    kept, _ = R.splat_corners(gold["splat_ndc"], _dims(gold))
    assert int(kept.sum()) >= 290
    # [-0.2,.5,.5] [.5,1.2,.5] outside; [.5,.5,1.0] at D = 10 and [.3,1.0,.3] at H = 12 divide to exactly dim - 1 and are dropped; [1.0,.3,.3] at W = 14
    # divides to just below 13 and is KEPT (a product with dim - 1 would drop it); the point in (-1, 0) voxel units is kept on voxel 0
    assert kept[-6:].tolist() == [False, False, False, True, False, True]
    v = gold["splat_ndc"][-3, 0] / (1.0 / (torch.tensor(14) - 1))
    assert float(v) < 13.0 and float(gold["splat_ndc"][-3, 0] * 13.0) == 13.0


def test_fp32_restatement_equals_the_reference_bit_for_bit(gold):
    f, a, w, cnt = R.splat_sums(gold["splat_ndc"], gold["splat_feat"], gold["splat_alpha"], _dims(gold), dtype=torch.float32)
    assert torch.equal(f, gold["splat_volume"]) and torch.equal(a, gold["splat_alpha_volume"]) and torch.equal(w, gold["splat_weight_volume"])
    assert int(cnt.sum()) == 8 * 302


def test_float64_and_integer_forms_agree_with_the_reference(gold):
    """Per voxel: n contributions summed sequentially in fp32 are within n * 2^-24 * (sum of magnitudes) of the exact sum; the integer form adds at most
    2^-33 per contribution."""
    dims = _dims(gold)
    f64, a64, w64, cnt = R.splat_sums(gold["splat_ndc"], gold["splat_feat"], gold["splat_alpha"], dims)
    fabs, aabs, _, _ = R.splat_sums(gold["splat_ndc"], gold["splat_feat"].abs(), gold["splat_alpha"].abs(), dims)
    n = cnt.double()
    assert bool(((f64 - gold["splat_volume"].double()).abs() <= n * 2.0 ** -24 * fabs).all())
    assert bool(((a64 - gold["splat_alpha_volume"].double()).abs() <= n * 2.0 ** -24 * aabs).all())
    assert bool(((w64 - gold["splat_weight_volume"].double()).abs() <= n * 2.0 ** -24 * w64).all())
    words, refused = R.splat_ints(gold["splat_ndc"], gold["splat_feat"], gold["splat_alpha"], dims)
    assert refused == 0 and not words[..., 22:].any()
    assert bool(((words[..., :20].permute(3, 0, 1, 2).double() / R.SCALE - f64).abs() <= n * 2.0 ** -33).all())
    assert bool(((words[..., 21].double() / R.SCALE - w64).abs() <= n * 2.0 ** -33).all())


def test_integer_form_refuses_large_and_non_finite_products(gold):
    ndc, feat, alpha = gold["splat_ndc"][:4].clone(), gold["splat_feat"][:4].clone(), gold["splat_alpha"][:4].clone()
    ndc[1] = torch.tensor([5.1 / 13, 4.1 / 11, 3.1 / 9])                   # local ~ (.1, .1, .1): the corner of shift (1, 1, 1) weighs 0.73
    feat[1, 3], feat[2, 5] = 2.0 ** 21, float("nan")
    words, refused = R.splat_ints(ndc, feat, alpha, _dims(gold))
    assert 9 <= refused <= 16                    # all eight corners of the NaN; of 2^21 at least the heaviest corner (0.73 * 2^21 >= 2^20)
    clean, none = R.splat_ints(ndc, torch.zeros_like(feat), alpha, _dims(gold))
    assert none == 0 and torch.equal(words[..., 20:], clean[..., 20:])       # a refused feature product leaves the point's alpha and weight sums alone


def test_ray_march_restatement_equals_the_reference_bit_for_bit(gold):
    near, far = R.dda(gold["march_rays"][:, :3], gold["march_rays"][:, 3:6], gold["march_bbox"])
    assert torch.equal(near, gold["march_near"]) and torch.equal(far, gold["march_far"])
    assert bool((near > far).any()) and bool((gold["march_rays"][:, 3:6] == 0).any())        # rays that miss, a zero direction component
    for k in range(4):
        perturb, lindisp = float(gold[f"march{k}_perturb"]), bool(int(gold[f"march{k}_lindisp"]))
        pts, ndc, z = R.ray_march_bbox(gold["march_rays"], gold["march_bbox"], gold[f"march{k}_z"].shape[1], lindisp, perturb, gold[f"march{k}_draw"])
        assert torch.equal(pts, gold[f"march{k}_pts"]) and torch.equal(ndc, gold[f"march{k}_ndc"]) and torch.equal(z, gold[f"march{k}_z"]), k


def test_normalise_leaves_untouched_voxels_zero(gold):
    f, d = R.normalise(gold["splat_volume"], gold["splat_alpha_volume"], gold["splat_weight_volume"])
    untouched = gold["splat_weight_volume"] == 0
    assert bool(untouched.any()) and not f[:, untouched].any() and not d[untouched].any()


def test_golden_regenerates_from_the_reference():
    from oracle import ref_shim
    if not os.path.isdir(ref_shim.REF_ROOT):
        pytest.skip("the reference checkout is not present")
    from tests import gen_golden_fusion
    assert gen_golden_fusion.check() == 35
