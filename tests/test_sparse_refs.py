"""CPU-only: the oracle of the empty-space predicate (tests/sparse_refs.py) has the two properties the feature rests on.

Conservative: for thr >= 0 a dead sample's trilinear density - F.grid_sample(align_corners=True, padding_mode='zeros'), what the renderer's lookups
compute - is <= thr: the interpolation is a convex combination of the in-grid corners (all <= thr for a dead sample) and of zeros.
Stable: the compact order is the ascending flat sample order."""
import pytest
import torch
import torch.nn.functional as F

from tests import sparse_refs as R


def _interp(density, ndc):
    grid = (ndc.reshape(1, 1, 1, -1, 3) * 2.0 - 1.0)
    return F.grid_sample(density[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(-1)


@pytest.mark.parametrize("grid", R.GRIDS)
def test_dead_samples_have_no_density_above_the_threshold(grid):
    g = torch.Generator().manual_seed(sum(grid))
    density = R.sparse_density(grid, g, empty=0.8)
    ndc = R.coords(400, 24, grid, g)
    finite = torch.isfinite(ndc.reshape(-1, 3)).all(-1)
    interp = _interp(density, torch.nan_to_num(ndc, nan=0.5, posinf=0.5, neginf=0.5))
    for thr in (0.0, 0.5, float(density.max())):
        live = R.live_mask(density, ndc, thr)
        assert bool(live[~finite].all())                                   # a non-finite coordinate is live: the dense march shows it too
        dead = ~live
        assert bool(dead.any())
        worst = float((interp[dead] - thr).max())
        print(f"grid {grid} thr {thr:.3g}: {int(live.sum())} of {live.numel()} live, max(interp - thr) over dead samples {worst:.3g}")
        assert worst <= 0.0
    assert not bool(R.live_mask(density, ndc, float(density.max()))[finite].any())      # nothing is strictly above the maximum
    assert bool(R.live_mask(density, ndc.clamp(0, 1).nan_to_num(0.5), -1.0).all())      # every in-grid cell is above -1


def test_a_nan_voxel_is_live_and_outside_is_dead():
    density = torch.zeros((4, 4, 4))
    density[1, 2, 3] = float("nan")
    ndc = torch.tensor([[[1.0, 2 / 3, 1 / 3], [0.9, 0.6, 0.3], [0.1, 0.1, 0.1], [-0.5, 0.5, 0.5], [1.4, 0.5, 0.5], [0.5, 0.5, 2.5]]])
    assert R.live_mask(density, ndc, 1e30).tolist() == [True, True, False, False, False, False]
    ones = torch.ones((4, 4, 4))
    assert R.live_mask(ones, ndc, 0.0).tolist() == [True, True, True, False, False, False]          # no corner in the grid: dead
    assert R.live_mask(ones, torch.tensor([[[-0.2, 0.5, 0.5]]]), 0.0).tolist() == [True]             # floor(-0.6) = -1: the x = 0 corners are in


def test_compact_order_is_ascending_and_rows_follow():
    grid = R.GRIDS[0]
    g = torch.Generator().manual_seed(1)
    density = R.sparse_density(grid, g, nan_voxel=True)
    N, S = 37, 24
    ndc, pts, dirs = R.coords(N, S, grid, g), torch.randn((N, S, 3), generator=g), torch.randn((N, 3), generator=g)
    n, idx, ndc_c, pts_c, dir_c = R.live_samples(density, ndc, 0.5, pts, dirs)
    assert 0 < n < N * S and idx.dtype == torch.int32
    assert bool((idx[1:] > idx[:-1]).all())
    for j in (0, n // 2, n - 1):
        t = int(idx[j])
        assert torch.equal(ndc_c[j], ndc.view(-1, 3)[t]) or bool(torch.isnan(ndc_c[j]).any())
        assert torch.equal(pts_c[j], pts.view(-1, 3)[t]) and torch.equal(dir_c[j], dirs[t // S])
    # expand_rows: the live rows back in place, zeros elsewhere
    src = torch.randn((n, 4), generator=g)
    dst = R.expand_rows(src, idx, n, N * S)
    dead = torch.ones(N * S, dtype=torch.bool)
    dead[idx.long()] = False
    assert torch.equal(dst[idx.long()], src) and not bool(dst[dead].any())
