"""The plane-sweep edge references (tests/sweep_refs.py) checked on the CPU: every geometry produces the situation it exists for at every
shape it is paired with, the zero-tap reference is the oracle except where the oracle is NaN, the float64 restatement agrees with it, and
the resize reference agrees with F.interpolate."""
import pytest
import torch
import torch.nn.functional as F

from oracle import mvsnerf_oracle as O
from tests import sweep_refs as R

# max |costvar_f64 - costvar_zero_tap| over every forward case below, measured on the authoring host (ATen CPU fp32 against float64 sums) and
# asserted with 4x slack for another host's float64 summation:
#  * as a fraction of E[x^2] + mean^2: 5.41e-5.  Not the 1e-7 of an fp32 chain, because the bilinear blend cancels on its own: at (9, 17, 2, 6)
#    `sign_change` four taps of size 2..3 blend to 9.8e-4 on a padded voxel, the blend's fp32 rounding (u x 3) is 2e-4 of that value, and
#    E[x^2] + mean^2 there is the square of that value alone;
#  * as a fraction of the same scale formed from the blends of |tap|: 2.38e-7, which is the fp32 rounding of the oracle's blend, s, s2 and
#    inv chain and the figure that would notice a wrong weight or tap.
F64_VS_FP32_MEASURED = 5.41e-5
F64_VS_FP32_MEASURED_ABS = 2.38e-7


@pytest.mark.parametrize("name", list(R.GEOMETRIES))
def test_every_geometry_produces_its_situation(name):
    build, wanted = R.GEOMETRIES[name]
    for H, W, pad, D in R.paired_shapes(name):
        got = R.situations(build(H, W), R.depths(D), H, W, pad)
        for key in wanted:
            assert got[key] > 0, f"{name} at {(H, W, pad, D)}: no voxel with `{key}` ({got})"
    # a voxel behind the camera AND counted as in view needs an interior: the shapes that have one
    if name == "negated":
        assert all(R.situations(build(H, W), R.depths(D), H, W, pad)["behind_inside"] > 0 for H, W, pad, D in R.SHAPES if H > 2 and W > 2)


def test_the_backward_view_lists_cover_what_they_are_for():
    assert set(R.BWD_CORE) | set(R.BWD_FAR) | {"identity"} == set(R.GEOMETRIES) and len(R.BWD_START) == len(R.BWD_SHAPES)
    for V in range(1, 9):
        for k in range(len(R.BWD_SHAPES)):
            assert len(set(R.bwd_views(V, k))) == V - 1
    # every backward instantiation NSRC = 1..7 meets a non-finite view, a border-crossing view and partial taps at some shape
    for V in range(2, 9):
        seen = set()
        for k in range(len(R.BWD_SHAPES)):
            seen |= set(R.bwd_views(V, k))
        assert {"p2_zero", "fast_fit", "half"} <= seen, (V, seen)
    # the deepest shape (D = 33: three 16-plane geometry batches) changes its tap set beyond the first batch from its first view on (at D = 17 only
    # plane 16 lies beyond it, 0.03 depth units from plane 15: the taps it carries over the batch border are the case there)
    for k, (H, W, pad, D) in enumerate(R.BWD_SHAPES):
        if D > 32:
            name = R.bwd_views(2, k)[0]
            gx, gy = R.grid_of(R.GEOMETRIES[name][0](H, W), R.depths(D), H, W, pad)
            tp, _ = R.taps(gx, gy, H, W)
            tapset = torch.stack([i for _, i in tp], -1)
            assert bool((tapset[16:] != tapset[15:-1]).any()), (name, H, W, pad, D)


def _oracle(case, shape, with_img):
    pad = shape[2]
    f, P, dv = case["feats"][None], case["P"][None], case["dv"][None]
    if not with_img:
        var, cnt = O.build_volume_costvar(f, P, dv, pad)
        return var[0], cnt[0, 0]
    # imgs at the thumbnails' own size: F.interpolate to the same size is the identity
    cost, masks = O.build_volume_costvar_img(case["small"][None], f, P, dv, pad)
    return cost[0], masks[0]


@pytest.mark.parametrize("with_img", [0, 1])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_zero_tap_reference_is_the_oracle_except_where_it_is_nan(shape, with_img):
    n_zeroed = 0
    for cname, names in R.forward_cases(shape):
        case = R.forward_case(shape, names, with_img)
        V = 1 + len(names)
        cost_o, masks_o = _oracle(case, shape, with_img)
        assert torch.equal(masks_o, case["masks"]), cname                        # counts / masks never depend on the zeroing
        zero_any = case["zeroed"].any(0)                                          # (D, Hp, Wp)
        var_o, var_z = cost_o[-R.C:], case["cost"][-R.C:]
        # the oracle's variance is NaN exactly on the voxels with a zeroed view (all 32 channels), bit-equal elsewhere
        assert torch.equal(torch.isnan(var_o).any(0), zero_any) and torch.equal(torch.isnan(var_o).all(0), zero_any), cname
        keep = ~zero_any[None].expand_as(var_o)
        assert torch.equal(var_o[keep].view(torch.int32), var_z[keep].view(torch.int32)), cname
        assert not bool(torch.isnan(case["cost"]).any()), cname
        if with_img:
            for v in range(1, V):
                th_o, th_z, z = cost_o[3 * v:3 * v + 3], case["cost"][3 * v:3 * v + 3], case["zeroed"][v]
                assert torch.equal(torch.isnan(th_o).all(0), z) and torch.equal(torch.isnan(th_o).any(0), z), (cname, v)
                k = ~z[None].expand_as(th_o)
                assert torch.equal(th_o[k].view(torch.int32), th_z[k].view(torch.int32)), (cname, v)
                assert bool((th_z[z[None].expand_as(th_z)] == 0).all())
            assert torch.equal(cost_o[:3], case["cost"][:3])
        # a zeroed view is never counted
        if with_img:
            assert not bool((case["masks"].bool() & case["zeroed"]).any()), cname
        n_zeroed += int(case["zeroed"].sum())
    assert n_zeroed > 0


def test_homo_warp_oracle_is_nan_exactly_on_nonfinite_coordinates():
    """`warped` of O.homo_warp itself, per source view: NaN where the fp32 coordinate is not finite, finite elsewhere (this host's ATen)."""
    for shape in R.SHAPES:
        H, W, pad, D = shape
        for name, (build, _) in R.GEOMETRIES.items():
            feats, _ = R.make_inputs(2, H, W, seed=5)
            warped, grid = O.homo_warp(feats[None, 1], build(H, W)[None], R.depths(D)[None], pad=pad)
            g = grid.view(D, H + 2 * pad, W + 2 * pad, 2)
            nf = R.nonfinite(g[..., 0], g[..., 1], H, W)
            assert torch.equal(torch.isnan(warped[0]).all(0), nf) and torch.equal(torch.isnan(warped[0]).any(0), nf), (shape, name)
            assert bool(torch.isfinite(warped[0][:, ~nf]).all()), (shape, name)


def test_homo_warp_oracle_on_the_hand_filled_grid():
    H, W, pad, D = R.HAND_GRID_SHAPE
    grid = R.hand_grid(H, W, pad, D)
    feats, _ = R.make_inputs(2, H, W, seed=6)
    warped, g2 = O.homo_warp(feats[None, 1], None, None, src_grid=grid, pad=pad)
    assert g2 is grid
    g = grid.view(D, H + 2 * pad, W + 2 * pad, 2)
    nf = R.nonfinite(g[..., 0], g[..., 1], H, W)
    assert 0 < int(nf.sum()) < nf.numel() and int(torch.isinf(g).sum()) > 0 and int(torch.isnan(g).sum()) > 0 and int((g.abs() == 1).sum()) > 0
    assert torch.equal(torch.isnan(warped[0]).all(0), nf) and torch.equal(torch.isnan(warped[0]).any(0), nf)
    assert float(warped[0][:, ~nf].abs().max()) > 0


def test_float64_restatement_agrees_with_the_zero_tap_reference():
    worst = worst_abs = 0.0
    for shape in R.SHAPES:
        H, W, pad, D = shape
        for cname, names in R.forward_cases(shape):
            case = R.forward_case(shape, names, 0)
            var64, cnt64, scale, scale_abs = R.costvar_f64(case["feats"].double(), case["P"], case["dv"], pad)
            assert torch.equal(cnt64, case["masks"].double()), (shape, cname)    # the oracle's counts (zero_tap's are the oracle's, above)
            diff = (var64 - case["cost"].double()).abs()
            worst = max(worst, float((diff / scale.clamp_min(1e-30)).max()))
            worst_abs = max(worst_abs, float((diff / scale_abs.clamp_min(1e-30)).max()))
    print(f"costvar_f64 vs costvar_zero_tap: max |diff| / (E[x^2] + mean^2) = {worst:.3e}, with the blends of |tap| {worst_abs:.3e}")
    assert worst <= 4 * F64_VS_FP32_MEASURED, worst
    assert worst_abs <= 4 * F64_VS_FP32_MEASURED_ABS, worst_abs


def test_float64_restatement_is_differentiable_and_blind_to_nonfinite_views():
    H, W, pad, D = 6, 7, 1, 5
    names = ("half", "p2_zero")
    feats, _ = R.make_inputs(3, H, W, seed=9)
    f = feats.double().requires_grad_()
    P, dv = R.proj_stack(names, H, W), R.depths(D)
    var = R.costvar_f64(f, P, dv, pad)[0]
    gw = torch.randn(var.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    (g,) = torch.autograd.grad((var * gw).sum(), f, retain_graph=True)
    assert bool(torch.isfinite(g).all()) and float(g[1].abs().max()) > 0 and float(g[2].abs().max()) > 0
    # restricted to the voxels where view 2's coordinate is not finite, view 2 receives no gradient at all
    gx, gy = R.grid_of(P[2], dv, H, W, pad)
    nf = R.nonfinite(gx, gy, H, W)
    assert int(nf.sum()) > 0
    (g_nf,) = torch.autograd.grad((var * gw * nf.double()).sum(), f)
    assert float(g_nf[2].abs().max()) == 0.0 and float(g_nf[1].abs().max()) > 0


RESIZES = [((8, 12), (2, 3)), ((7, 9), (3, 4)), ((3, 5), (7, 11)), ((1, 1), (4, 4)), ((5, 1), (2, 3)), ((6, 6), (6, 6)), ((40, 52), (17, 23))]


@pytest.mark.parametrize("size_in,size_out", RESIZES)
def test_resize_reference_vs_interpolate(size_in, size_out):
    """resize_f64 forms the source coordinates in fp32 like the kernels; F.interpolate in float64 forms them in float64.  A coordinate error of
    e moves the value by at most e * (difference of neighbouring pixels) <= 2 e max|src| per axis; e <= 4 u max(coordinate) (three fp32
    roundings of a value <= the input size, one of the scale)."""
    g = torch.Generator().manual_seed(size_in[0] * 100 + size_out[1])
    src = torch.randn((2, 3, *size_in), generator=g)
    ref = F.interpolate(src.double(), size_out, mode="bilinear", align_corners=False)
    got = R.resize_f64(src, *size_out)
    assert got.shape == ref.shape and got.dtype == torch.float64
    bound = 2 * 2 * 4 * R.U * max(size_in) * float(src.abs().max())
    assert float((got - ref).abs().max()) <= bound
    if size_in == size_out:
        assert torch.equal(got, src.double())
