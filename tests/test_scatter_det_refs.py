"""CPU-only: the integer restatement of the deterministic volume-gradient scatter (tests/scatter_det_refs.py) has the properties the GPU tests lean on -
and a float accumulation of the same products does not, which is what gives the permutation tests of tests/test_gpu_scatter_det.py their teeth."""
import functools

import pytest
import torch

from tests import scatter_det_refs as R


@functools.lru_cache(maxsize=None)
def _case(i):
    C, dims, P = R.SHAPES[i]
    ndc, g = R.inputs(C, dims, P)
    acc, e = R.scatter_ints(ndc, g, dims)
    return C, dims, P, ndc, g, acc, e


def _float_sum(ndc, g, dims, dtype):
    out = torch.zeros(dims[0] * dims[1] * dims[2] * g.shape[1], dtype=dtype)
    for idx, prod in R.products(ndc, g, dims):
        out.index_add_(0, idx, prod.to(dtype))
    return out


CASES = range(len(R.SHAPES))


@pytest.mark.parametrize("i", CASES)
def test_a_row_permutation_leaves_every_accumulator_unchanged(i):
    C, dims, P, ndc, g, acc, e = _case(i)
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(5))
    acc2, e2 = R.scatter_ints(ndc[perm], g[perm], dims)
    assert e2 == e and torch.equal(acc2, acc)


@pytest.mark.parametrize("i", CASES)
def test_three_parts_on_the_whole_inputs_grid_add_up_to_the_whole(i):
    """Integers add exactly - but only on ONE grid: a part that lacks the largest |g| has a smaller exponent of its own, is rounded on a finer grid and need
    not add up (which is why N ranks scatter their rows in one call)."""
    C, dims, P, ndc, g, acc, e = _case(i)
    cuts = [0, P // 3, P // 3 + (P + 2) // 4, P]                              # uneven; empty parts at P = 1
    total = torch.zeros_like(acc)
    for a, b in zip(cuts[:-1], cuts[1:]):
        part, pe = R.scatter_ints(ndc[a:b], g[a:b], dims, e=e)
        assert pe == e
        total += part
    assert torch.equal(total, acc)


@pytest.mark.parametrize("i", CASES)
def test_finish_is_the_float64_sum_to_the_roundings_of_the_definition(i):
    """Per element: every contribution is rounded once to the grid 2^(e - 40) (error <= half a step each), the sum is exact, and the conversion to fp32 rounds
    once more (half an ulp of the result).  Over the whole volume that stays within ONE fp32 ulp of the largest sum while an element has fewer than 2^15
    contributions: n * 2^(e - 41) < 2^(e - 26) <= half an ulp of any value >= 2^(e - 2)."""
    C, dims, P, ndc, g, acc, e = _case(i)
    exact = _float_sum(ndc, g, dims, torch.float64)
    cnt = torch.zeros(exact.numel(), dtype=torch.int64)
    for idx, _ in R.products(ndc, g, dims):
        cnt.index_add_(0, idx, torch.ones_like(idx))
    out = R.finish(acc, e).reshape(-1)
    ulp = lambda x: (torch.nextafter(x.float().abs(), torch.tensor(float("inf"))) - x.float().abs()).double()
    err = (out.double() - exact).abs()
    assert bool((err <= cnt.double() * 2.0 ** (e - 41) + 0.5 * ulp(out)).all())
    top = exact.abs().max()
    assert int(cnt.max()) < 2 ** 15 and float(top) >= 2.0 ** (e - 2)
    assert float(err.max()) <= float(ulp(top))


@pytest.mark.parametrize("i", [i for i in CASES if R.SHAPES[i][2] >= 3001])
def test_a_float32_sum_of_the_same_products_depends_on_the_order(i):
    """The teeth of the permutation tests: accumulated in fp32, the same products give other bits in at least 10 % of the elements once the rows are permuted
    (the crowded shapes: an element needs three or more contributions before the order of a sum matters)."""
    C, dims, P, ndc, g, acc, e = _case(i)
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(5))
    f1, f2 = _float_sum(ndc, g, dims, torch.float32), _float_sum(ndc[perm], g[perm], dims, torch.float32)
    frac = float((f1 != f2).double().mean())
    print(f"[C={C} dims={dims} P={P}] a float32 sum differs under a row permutation in {100 * frac:.0f} % of the elements")
    assert frac >= 0.10, frac


@pytest.mark.parametrize("i", CASES)
def test_accumulators_stay_far_inside_a_word(i):
    C, dims, P, ndc, g, acc, e = _case(i)
    assert int(acc.abs().max()) < 2 ** 62 and P <= R.MAX_POINTS
    assert int(acc.abs().max()) <= P * 2 ** R.FRAC_BITS                      # one contribution of at most 2^40 per point and element


def test_edge_rows_and_the_all_zero_gradient():
    C, dims, P, ndc, g, acc, e = _case(0)
    edge = ndc[P - R.N_EDGE_ROWS:]
    assert [float(edge[2 * a, a]) for a in range(3)] == [0.0] * 3 and [float(edge[2 * a + 1, a]) for a in range(3)] == [1.0] * 3
    for ok, w, vox in R.corners(edge[6:], dims):                             # NaN, +inf, -inf: out of bounds at every corner, index 0
        assert not bool(ok.any()) and int(vox.abs().max()) == 0
    D, H, W = dims
    for ok, w, vox in R.corners(ndc, dims):
        assert int(vox.min()) >= 0 and int(vox.max()) < D * H * W
    # a coordinate of exactly 1 sits ON the last voxel: its upper corner is out of bounds, its lower one carries weight 1 along that axis
    on_last = R.corners(torch.tensor([[1.0, 0.5, 0.5]]), dims)
    assert bool(on_last[0][0]) and not bool(on_last[1][0]) and int(on_last[0][2]) % W == W - 1
    zacc, ze = R.scatter_ints(ndc, torch.zeros_like(g), dims)
    assert ze == 0 and not bool(zacc.any()) and not bool(R.finish(zacc, ze).any())
    with pytest.raises(ValueError):
        R.exponent(torch.tensor([[1.0, float("inf")]]))
