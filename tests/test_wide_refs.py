"""CPU-only: the torch restatement of the netwidth-256 networks (tests/wide_refs.py) against the real reference.

tests/golden/mlp_wide_ref.npz holds the fp32 outputs of the reference's own MVSNeRF(D=6, W=256, net_type in {v0, v2}).forward and .forward_alpha
on the (37, 24) rows, feat_dim 12 / 20 / 36 / 40 (tests/gen_golden_wide.py; outputs only).  The weights and inputs are rebuilt here from the seeds;
the fp32 restatement must equal the fixture within 2e-7 absolute on rgb and 1e-6 relative on sigma (it was bit-equal where the fixture was
written: the bounds leave room for another BLAS build's summation order, not for another network).  The GPU tests measure the kernel
against this restatement and its float64 twin.
"""
import os

import numpy as np
import pytest
import torch

from tests import wide_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S = 37, 24


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", R.GOLDEN))


def test_fixture_holds_outputs_only(golden):
    assert sorted(golden.files) == sorted(f"{nt}_F{F}_{k}" for nt in R.VARIANTS for F in R.FS for k in ("raw", "alpha"))
    for k in golden.files:
        assert golden[k].dtype == np.float32 and golden[k].shape == (N, S, 4 if k.endswith("raw") else 1)


@pytest.mark.parametrize("F", R.FS)
@pytest.mark.parametrize("net_type", list(R.VARIANTS))
def test_restatement_is_the_reference(golden, net_type, F):
    ref = R.reference(N, S, F, net_type)
    raw, alpha = (t.numpy() for t in ref["f32"])
    g_raw, g_alpha = golden[f"{net_type}_F{F}_raw"], golden[f"{net_type}_F{F}_alpha"]
    assert np.abs(raw[..., :3] - g_raw[..., :3]).max() <= 2e-7
    for got, want in ((raw[..., 3], g_raw[..., 3]), (alpha[..., 0], g_alpha[..., 0])):
        assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want))
    # forward clamps sigma in both variants; forward_alpha only in v0
    assert g_raw[..., 3].min() >= 0.0
    assert (g_alpha.min() < 0.0) == (net_type == "v2")


@pytest.mark.parametrize("F", R.FS)
@pytest.mark.parametrize("net_type", list(R.VARIANTS))
def test_seeds_put_alpha_on_both_sides_of_zero(net_type, F):
    s = R.reference(N, S, F, net_type)["f64"][2]
    assert float((s < 0).double().mean()) >= 0.05 and float((s > 0).double().mean()) >= 0.05
