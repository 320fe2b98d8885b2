"""CPU-only: the yardsticks of tests/test_gpu_sparse_train.py (tests/sparse_train_refs.py) and the conditions the GPU tests rely on, from the
references alone: every scene is a mixed case (live fraction in (0.1, 0.6)), no reference gradient is all zero (a bound relative to max |ref| would
be empty), the (130,3) scene has rays without a live sample, and zeroing the dead rows changes the function (the masked loss is not the dense one)."""
import pytest
import torch

from tests import sparse_refs as R
from tests import sparse_train_refs as T

FRACTIONS = {(3, 37, 16): 0.314, (3, 8, 128): 0.330, (3, 130, 3): 0.221, (7, 37, 16): 0.316}


def test_compact_rows_oracle():
    g = torch.Generator().manual_seed(0)
    src = torch.randn((9, 4), generator=g)
    idx = torch.tensor([1, 3, 4, 8, -1, 9, 0, 0, 0], dtype=torch.int32)
    got = T.compact_rows(src, idx, 6, 8)
    assert torch.equal(got[:4], src[[1, 3, 4, 8]]) and not bool(got[4:].any())                 # -1 and 9 are outside [0, 9): zero rows; rows 6, 7: past the count
    assert torch.equal(T.compact_rows(src, idx, 99, 3), src[[1, 3, 4]])                         # the count is clamped to the rows of dst
    assert T.compact_rows(src, idx, 0, 5).shape == (5, 4) and not bool(T.compact_rows(src, idx, 0, 5).any())
    assert T.compact_rows(src, idx, -2, 2).abs().sum() == 0 and T.compact_rows(src, idx, 4, 0).shape == (0, 4)
    # the inverse of expand_rows on the live rows
    live = torch.tensor([0, 2, 3, 7], dtype=torch.int32)
    rows = torch.randn((4, 4), generator=g)
    assert torch.equal(T.compact_rows(R.expand_rows(rows, live, 4, 9), live, 4, 4), rows)


@pytest.mark.parametrize("V,n,s", list(FRACTIONS))
def test_scenes_are_mixed_cases(V, n, s):
    sc = T._scene(V, n, s, 5 + n)
    live = T.live_of(sc)
    f = float(live.float().mean())
    dead_rays = int((~live.any(-1)).sum())
    print(f"V={V} ({n},{s}): live fraction {f:.3f}, {dead_rays} rays without a live sample")
    assert 0.1 < f < 0.6
    assert abs(f - FRACTIONS[(V, n, s)]) < 5e-4
    if (n, s) == (130, 3):
        assert dead_rays == 45
    assert bool(live.any(-1).any())


def test_other_scenes_are_mixed_cases():
    f_amp = float(T.live_of(T._scene(3, *T.AMP_SCENE)).float().mean())
    f_col = float(T.live_of(T._scene(3, *T.COLOR_SCENE)).float().mean())
    print(f"bf16 scene live fraction {f_amp:.3f}, colour-volume scene {f_col:.3f}")
    assert abs(f_amp - 0.322) < 5e-4
    assert 0.1 < f_amp < 0.6 and 0.1 < f_col < 0.6


def _nonzero(grads, gvol):
    return all(float(g.abs().max()) > 0 for g in grads.values()) and float(gvol.abs().max()) > 0


@pytest.mark.parametrize("net_type", ["v0", "v2"])
@pytest.mark.parametrize("V,n,s,white", [(3, *sh) for sh in T.SHAPES] + [(7, *T.SHAPES[0])])
def test_masked_references_reach_every_tensor(V, n, s, white, net_type):
    loss, grads, gvol, live = T.masked_reference(V, net_type, n, s, white)
    assert len(grads) == 22 and loss == loss and _nonzero(grads, gvol)
    assert gvol.shape == (1, 8, *T.GRID)
    if V == 7:
        assert float(grads["nerf.pts_bias.weight"][:, 32:].abs().max()) > 0                     # F > 32: the second feature block
    if (V, n) == (3, 37):                                                                       # the mask matters: not the dense function
        dense_loss = T.masked_reference(V, net_type, n, s, white, mask=False)[0]
        assert abs(dense_loss - loss) > 1e-2 * max(1.0, abs(dense_loss)), (dense_loss, loss)


def test_masked_colour_and_bf16_references_reach_every_tensor():
    loss, grads, gvol, _ = T.masked_color_reference(3)
    assert gvol.shape == (1, 20, *T.GRID) and _nonzero(grads, gvol) and float(gvol[:, 8:].abs().max()) > 0
    loss, grads, gvol, _ = T.masked_amp_reference()
    assert loss == loss and _nonzero(grads, gvol)
