"""CPU: the float64 reference of tests/mlp_train_refs.py pinned, and the conditions under which tests/test_gpu_mlp_train_f64.py may compare the
training kernels with it - for every (N, S, F) that file uses."""
import pytest
import torch

from tests import mlp16_refs as M
from tests import mlp_train_refs as R
from tests.util import record_err

A_FS = [4, 12, 20, 32, 34, 36, 40]
A_SHAPES = [(5, 7), (37, 24), (3, 300)]
B_CASES = [(65, 128, 20), (129, 128, 20), (517, 32, 40)]
C_CASES = [(5, 7, 20), (37, 24, 40), (517, 32, 40)]
GPU_CASES = sorted(set([(N, S, F) for F in A_FS for N, S in A_SHAPES] + B_CASES + C_CASES))


def test_autograd_of_the_reference_against_central_differences():
    """(raw * d_raw).sum() on 3 points in float64: for each of the 23 differentiated tensors, the directional derivative along a random direction of
    that tensor alone, by central differences with step 1e-6 of the tensor's largest entry, against <gradient, direction>.  Truncation is O(step^2)
    and rounding 2^-53 / step, both far below the 1e-6 (relative to the abs-sum of the inner product's terms) asked here; a point within the step
    of a ReLU kink would show as an O(1) miss and get another seed."""
    N, S, F = 3, 1, 20
    ws, bs = R.weights(F)
    ndc, feat, dirs = R.inputs(N, S, F)
    g_raw = R.d_raw(N, S, F)
    net = R.network(ws, bs, ndc, feat, dirs, g_raw=g_raw)
    gen = torch.Generator().manual_seed(5)

    def loss(ws_, bs_, feat_):
        return float((R.network(ws_, bs_, ndc, feat_, dirs).raw * g_raw.double()).sum())

    tensors = [feat.double()] + [t.double() for pair in zip(ws, bs) for t in pair]
    grads = [net.d_feat.reshape(feat.shape)] + net.grads
    for k, (t, g, name) in enumerate(zip(tensors, grads, R.tensor_names())):
        v = torch.randn(t.shape, generator=gen, dtype=torch.float64)
        eps = 1e-6 * max(float(t.abs().max()), 1e-3)
        vals = []
        for s in (+1, -1):
            moved = list(tensors)
            moved[k] = t + s * eps * v
            vals.append(loss(moved[1::2], moved[2::2], moved[0]))
        numeric, analytic, scale = (vals[0] - vals[1]) / (2 * eps), float((g * v).sum()), float((g * v).abs().sum())
        assert abs(numeric - analytic) <= 1e-6 * scale, (name, numeric, analytic, scale)


@pytest.mark.parametrize("F", [2, 20, 34])
def test_reference_forward_is_the_exact_network_of_mlp16_refs(F):
    """network() in float64 IS tests.mlp16_refs.exact (the same operations; 1e-12 allows another association), and in fp32 it is within fp32
    rounding of it: eight layers of dot products up to 191 long, each a random walk of about sqrt(191) roundings of 2^-24 relative to the
    abs-sum, which the kept activations (< 130) keep near the result's own size: 8 x 14 x 2^-24 = 7e-6 of a column's largest value; 2e-5 asked."""
    N, S = 37, 24
    ws, bs = R.weights(F)
    x = R.inputs(N, S, F)
    want = M.exact(ws, bs, *x)
    got64 = R.network(ws, bs, *x).raw
    got32 = R.network(ws, bs, *x, dtype=torch.float32).raw
    assert got32.dtype == torch.float32
    for c in range(4):
        top = max(1.0, float(want[:, c].abs().max()))
        assert float((got64[:, c] - want[:, c]).abs().max()) <= 1e-12 * top
        assert float((got32[:, c].double() - want[:, c]).abs().max()) <= 2e-5 * top, c


@pytest.mark.parametrize("N,S,F", GPU_CASES)
def test_conditions_of_a_gpu_case(N, S, F):
    c = R.case(N, S, F)
    print(f"mlp_train_refs:({N},{S},{F}): live {c.live:.3f}  dropped {c.dropped:.3f}  flips {c.flips}  "
          f"e_cpu {min(c.e_cpu):.2e} .. {max(c.e_cpu):.2e}")
    assert 0.40 <= c.live <= 0.90, c.live
    assert c.dropped <= 0.25, c.dropped                 # a condition: a case above it gets another seed (mlp_train_refs.SEEDS), not another cap
    assert c.flips == 0
    for name, e in zip(R.tensor_names(), c.e_cpu):
        record_err(f"mlp_train_f64:cpu_fp32:({N},{S},{F}):{name}", e)
        assert e == e and e != float("inf"), name
    # the dropped rows contribute exactly nothing on either side
    dropped = ~c.kept
    assert not bool(c.ref.d_feat[dropped].any()) and not bool(c.cpu32.d_feat[dropped].any())


def test_forward_error_in_margin_units_is_far_below_tau():
    """the CPU fp32 forward against float64, each ReLU argument in the units of its margin: tau = 2^-17 is 8 x the largest figure (2^-20)"""
    N, S, F = 37, 24, 34
    ws, bs = R.weights(F)
    x = R.inputs(N, S, F)
    a, b = R.network(ws, bs, *x, with_margin=True), R.network(ws, bs, *x, dtype=torch.float32)
    worst = 0.0
    for i, (p64, p32) in enumerate(zip(a.pre, b.pre)):
        if R.STAGES[i] == "alpha_linear":
            continue                                    # its unit (|w| . |h| + |b|) is larger than the stage's |p|: covered by the others' figure
        worst = max(worst, float(((p32.double() - p64).abs().max(-1).values / p64.abs().max(-1).values).max()))
    record_err("mlp_train_f64:cpu_fp32:forward_in_margin_units", worst, tol=R.TAU / 8)
    assert worst <= R.TAU / 8, worst


def test_a_lost_tile_breaks_the_summation_bound():
    """Teeth of summation_bound, emulated in float64: the gradients of (129, 128, 20) with the 32 points of one tile left out.  At least 8 of the
    11 weight gradients must move by more than 4 x summation_bound(3, 256, 3) x A somewhere, and so must the largest bias gradient."""
    N, S, F = 129, 128, 20
    c = R.case(N, S, F)
    ws, bs = R.weights(F)
    g = c.g_raw.clone()
    tile = 259                                          # the second tile of workgroup 86's three (per = 3): the odd-tile contract of the prefetch loop
    g[32 * tile:32 * tile + 32] = 0
    assert bool(c.kept[32 * tile:32 * tile + 32].any())
    lost = R.network(ws, bs, *c.x, g_raw=g)
    bound = 4 * R.summation_bound(3, 256, 3)
    seen = [bool(((a - b).abs() > bound * A).any()) for a, b, A in zip(lost.grads, c.ref.grads, c.ref.A)]
    names = R.tensor_names()[1:]
    print({n: s for n, s in zip(names, seen)})
    assert sum(seen[0::2]) >= 8, {n: s for n, s in zip(names[0::2], seen[0::2])}
    k = max(range(11), key=lambda i: float(c.ref.grads[2 * i + 1].abs().max()))
    assert seen[2 * k + 1], names[2 * k + 1]


def test_psum_depth_and_bound():
    assert R.psum_depth(1) == 4 and R.psum_depth(32) == 7 and R.psum_depth(256) == 4 + 7 and R.psum_depth(260) == 5 + 7
    assert R.summation_bound(1, 72, 0) == 2 * (32 + (1 + 3) + (3 + 3)) * 2.0 ** -24      # 72 partials: chunks of 3 -> 24 slices
    assert R.summation_bound(3, 256, 3) == 2 * (96 + 11 + 32 + 11) * 2.0 ** -24
