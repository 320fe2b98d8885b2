"""CPU-only: the restatements of tests/occupancy_refs.py against the package's own forward map (utils.get_ndc_coordinate) and against themselves."""
import pytest
import torch

from tests import occupancy_refs as R

CASES = [((5, 6, 7), (24, 32), 0), ((4, 10, 12), (24, 32), 2), ((9, 20, 37), (64, 96), 4)]


@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("grid,ref_hw,pad", CASES)
def test_inverse_map_round_trips_through_get_ndc_coordinate(grid, ref_hw, pad, lindisp):
    """float64 nodes -> world (the restatement) -> utils.get_ndc_coordinate in float64 returns the nodes.  With the float64 inverse of c2w only
    float64 roundings remain: |error| <= 1e-12 (2^-53 times a few hundred for the division by a depth and the focal length).  With the fp32-rounded
    w2c a camera would be given in, its 2^-24 relative error shows: printed, bounded by 1e-6 (2^-24 x |pts| <= 6 x three terms ~ 1e-6 in camera space,
    times focal / depth / (size - 1) ~ 0.6 in NDC)."""
    from mvsnerf_amd import utils
    D, H, W = grid
    K, c2w, w2c32, nf = R.camera(seed=D, ref_hw=ref_hw)
    nodes = R.node_grid(D, H, W, dtype=torch.float64)
    world = R.ndc_to_world(nodes, K, c2w, nf, ref_hw, pad=pad, lindisp=lindisp, dtype=torch.float64)
    inv_scale = torch.tensor([ref_hw[1] - 1, ref_hw[0] - 1], dtype=torch.float64)
    errs = []
    for w2c in (torch.linalg.inv(c2w.double()), w2c32.double()):
        back = utils.get_ndc_coordinate(w2c, K.double(), world.view(1, -1, 3), inv_scale, near=float(nf[0]), far=float(nf[1]), pad=pad, lindisp=lindisp)
        errs.append(float((back.view(-1, 3) - nodes).abs().max()))
    print(f"grid {grid} pad {pad} lindisp {lindisp}: round trip {errs[0]:.3g} (float64 w2c), {errs[1]:.3g} (fp32 w2c)")
    assert errs[0] <= 1e-12
    assert errs[1] <= 1e-6


@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("grid,ref_hw,pad", CASES)
def test_fp32_restatement_is_a_few_ulps_from_float64(grid, ref_hw, pad, lindisp):
    """The yardstick of tests/test_gpu_occupancy.py: the fp32 restatement's own largest error.  A few ulps of coordinates up to ~6: below
    64 x 2^-24 x 6 = 2.3e-5, and far below the ~1e-2 of a voxel pitch a wrong pad or axis convention would cost."""
    D, H, W = grid
    K, c2w, _, nf = R.camera(seed=D, ref_hw=ref_hw)
    w64 = R.ndc_to_world(R.node_grid(D, H, W, dtype=torch.float64), K, c2w, nf, ref_hw, pad=pad, lindisp=lindisp, dtype=torch.float64)
    w32 = R.ndc_to_world(R.node_grid(D, H, W), K, c2w, nf, ref_hw, pad=pad, lindisp=lindisp, dtype=torch.float32)
    assert w32.dtype == torch.float32
    e = float((w32.double() - w64).abs().max())
    print(f"grid {grid} pad {pad} lindisp {lindisp}: fp32 restatement vs float64 {e:.3g} at |coordinate| <= {float(w64.abs().max()):.3g}")
    assert 0 < e < 2.3e-5
    pitch = float((w64.view(D, H, W, 3)[0, 0, 1] - w64.view(D, H, W, 3)[0, 0, 0]).norm())
    assert pitch > 100 * e


def test_node_grid_order_planes_and_unit_axes():
    g = R.node_grid(3, 4, 5)
    assert g.shape == (60, 3) and g.dtype == torch.float32
    assert torch.equal(g.view(3, 4, 5, 3)[2, 1, 3], torch.tensor([3 / 4, 1 / 3, 1.0]))
    assert torch.equal(R.node_grid(3, 4, 5, planes=(1, 3)), g[20:60]) and R.node_grid(3, 4, 5, planes=(2, 2)).shape == (0, 3)
    one = R.node_grid(1, 4, 1)
    assert torch.equal(one[:, 0], torch.zeros(4)) and torch.equal(one[:, 2], torch.zeros(4)) and torch.equal(one[:, 1], torch.arange(4.0) / 3)


@pytest.mark.parametrize("r", [0, 1, 2])
def test_dilation_restatement_clips_and_propagates_nan(r):
    x = R.planted((7, 9, 10), seed=r)
    got = R.max_dilate3d(x, r)
    D, H, W = x.shape
    want = torch.empty_like(x)
    for k in range(D):
        for j in range(H):
            for i in range(W):
                win = x[max(k - r, 0):k + r + 1, max(j - r, 0):j + r + 1, max(i - r, 0):i + r + 1]
                want[k, j, i] = float("nan") if bool(torch.isnan(win).any()) else win.max()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(want).any())
    assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))
    if r == 0:
        assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(x, nan=0.0))
