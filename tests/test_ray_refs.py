"""CPU-only checks of tests/ray_refs.py: every float64 reference, input family and bound that test_gpu_ray_edges.py and test_gpu_importance_f64.py hold the HIP
kernels to is exercised here against the fp32 oracle (torch eager on the CPU), and every condition on the inputs (exactness of the exact families, the shares of
left-out and weakly bounded samples) is asserted, so that a broken reference, a bound the reference arithmetic itself does not meet or a family that lost its
property fails without a GPU."""
import pytest
import torch

from tests import ray_refs as R

U = R.U


# ------------------------------------------------------------------------------------------------------------------ sample_pdf
@pytest.mark.parametrize("nb", R.PDF_NB)
def test_pdf_exact_family_is_exact(nb):
    from oracle import mvsnerf_oracle as O
    bins, w, u, d, pick = R.pdf_exact_case(nb)
    q = R.pdf_q(w)
    assert torch.equal(q, d)                                                       # the construction succeeded: fl32(w + 1e-5f) = d
    assert torch.equal(d * 16, (d * 16).round()) and torch.equal(bins * 256, (bins * 256).round())
    tot = d.double().sum(-1)
    assert torch.equal(torch.log2(tot), torch.log2(tot).round())                  # the row sum is a power of two ...
    assert torch.equal(R.kernel_order_sum32(q).double(), tot) and torch.equal(q.sum(-1).double(), tot)      # ... in the kernel's order and in torch's
    ref = R.sample_pdf_ref64(bins, q, u)
    assert torch.equal(ref["C"].to(torch.float32).double(), ref["C"]) and float(ref["C"][:, -1].min()) == 1.0     # every knot is an fp32 number
    assert torch.equal(O.sample_pdf(bins, w, u).double(), ref["z"])               # the fp32 oracle reproduces float64 bit for bit
    knot = pick < nb                                                              # candidates 0 .. nb-1 are the knots, 1.0 included
    assert torch.equal(ref["z"][knot], torch.gather(bins.double(), 1, pick.clamp(max=nb - 1))[knot])        # u = cdf[k] returns bins[k]
    seen = torch.zeros(3 * nb - 2, dtype=torch.bool)
    seen[pick.reshape(-1)] = True
    assert bool(seen.all())                                                       # u = 0, every knot, every 1/2 and 1/4 point
    assert bool((u[0::2, 0] == 0).all()) and bool((u[1::2, 0] == 1).all())
    if nb > 3:                                                                    # knots on top of a bin below the switch, where z(u) jumps
        thin_top = torch.cat([torch.zeros((d.shape[0], 1), dtype=torch.bool), (ref["C"][:, 1:] - ref["C"][:, :-1]) < R.SWITCH], -1)
        assert bool((knot & torch.gather(thin_top, 1, pick.clamp(max=nb - 1))).any())


@pytest.mark.parametrize("nb", R.PDF_NB)
@pytest.mark.parametrize("family", R.PDF_FAMILIES)
def test_pdf_conditioned_family_bound_holds_for_the_oracle(family, nb):
    from oracle import mvsnerf_oracle as O
    bins, w, u = R.pdf_conditioned_case(family, nb)
    ref = R.sample_pdf_ref64(bins, R.pdf_q(w), u)
    bound, left = R.sample_pdf_bound(ref, bins, u, nb)
    err = (O.sample_pdf(bins, w, u).double() - ref["z"]).abs()
    assert bool((err <= bound)[~left].all()), float((err / bound)[~left].max())
    assert float(left.float().mean()) <= 0.005
    weak = (bound > 0.01 * ref["width"]) & ~left & (ref["width"] > 0)
    assert float(weak.float().mean()) <= 0.005
    assert bool((u == 0).any()) and bool((u == 1 - 2.0 ** -24).any())


# ------------------------------------------------------------------------------------------------------------------ ray_marcher_fine
@pytest.mark.parametrize("S", [S for S in R.FINE_S if R.fine_is_exact_S(S)])
def test_fine_empty_rays_are_exact(S):
    dens, ndc, z, u = R.fine_empty_case(S)
    assert float(dens.abs().max()) == 0 and bool((z[:, 1:] >= z[:, :-1]).all()) and float(z.max()) <= 6.0
    q = R.C1E5.expand(z.shape[0], S - 2)
    tot = R.kernel_order_sum32(q)
    assert bool((tot.double() == float(R.C1E5) * (S - 2)).all()) and bool(((q / tot[:, None]).double() == 1.0 / (S - 2)).all())      # pdf = 1/(S-2) exactly
    ref, smp = R.fine_empty_ref64(z, u)
    assert torch.equal(R.fine_oracle32(dens, ndc, z, u).double(), ref)
    assert bool((u == 0).any()) and bool((u == 1).any())
    if S > 3:
        assert bool((z[:, 1:] == z[:, :-1]).any())
        bins = 0.5 * (z[:, :-1] + z[:, 1:]).double()
        tie = (smp["z"][:, :, None] == z.double()[:, None, :]).sum(-1)
        assert bool((tie >= 2).any())                                              # a sample equal to two coarse depths
        srt = torch.sort(u, -1)[0]
        assert bool((srt[:, 1:] == srt[:, :-1]).any())                             # repeated u
        assert torch.equal(bins.to(torch.float32).double(), bins)


@pytest.mark.parametrize("S", R.FINE_S)
def test_fine_binary_family_bound_holds_for_the_oracle(S):
    from oracle import mvsnerf_oracle as O
    dens, ndc, z, u, sigma = R.fine_binary_case(S)
    assert torch.equal(O.index_point_feature(dens[None, None], ndc * 2 - 1.0)[..., 0], sigma)      # voxel centres: the lookup is exact
    assert bool((ndc < 0.5).any()) and bool((sigma == 32).any()) and bool((sigma == 0).any())
    run = (sigma[:, 1:6] == 32).all(-1) if S >= 7 else torch.ones(1, dtype=torch.bool)
    assert bool(run.any())                                                        # several opaque samples in a row
    ref, bound, left = R.fine_binary_ref64(sigma, z, u)
    assert float(left.float().mean()) <= 0.01
    assert not bool(((bound > 0.01 * ref["width"]) & ~left).any())
    out = R.fine_oracle32(dens, ndc, z, u)
    assert bool((out[:, 1:] >= out[:, :-1]).all())
    lo, hi = R.order_stat_band(ref["z"], bound, left, float(z.min()), float(z.max()))
    rest, ok = R.remove_multiset(out, z)
    assert bool(ok.all())
    assert bool((rest.double() >= lo).all()) and bool((rest.double() <= hi).all())


def test_remove_multiset():
    rows = torch.tensor([[1.0, 2.0, 2.0, 2.0, 3.0, 4.0, 4.0]]).repeat(3, 1)
    rest, ok = R.remove_multiset(rows, torch.tensor([[2.0, 2.0, 4.0], [2.0, 2.5, 4.0], [3.0, 3.0, 4.0]]))
    assert ok.tolist() == [True, False, False] and rest[0].tolist() == [1.0, 2.0, 3.0, 4.0]


# ------------------------------------------------------------------------------------------------------------------ ray points, ray generation
@pytest.mark.parametrize("ref_hw", R.REF_HW)
@pytest.mark.parametrize("geometry", R.GEOMETRIES)
def test_ray_points_reference_and_bound(geometry, ref_hw):
    cam = R.camera_case(geometry, ref_hw)
    Hr, Wr = ref_hw
    worst = 0.0
    for i, (N, S) in enumerate(R.RAY_SHAPES):
        for pad in (0, 4):
            for lindisp in (False, True):
                per_ray = bool((i + pad // 4 + lindisp) % 2)
                o, d, z, xs, ys = R.ray_points_case(cam, N, S, per_ray)
                assert float(z.min()) == float(cam["nf"][0]) and float(z.max()) <= float(cam["nf"][1]) and (N == 1 or float(z.max()) == float(cam["nf"][1]))
                pts = R.points_ref64(o, d, z)
                ndc = R.ndc_ref64(pts, cam["w2c"], cam["Kr"], cam["nf"], Wr, Hr, pad, lindisp)
                p32 = o.unsqueeze(1) + d.unsqueeze(1) * z.unsqueeze(2)
                worst = max(worst, R.within(p32, pts), R.within(R.ndc_oracle32(cam, p32, pad, lindisp), ndc))
                if geometry == "same" and pad == 0 and not per_ray:                 # the reference camera is the target camera (d was rounded to fp32)
                    assert float((ndc.v[..., 0] * (Wr - 1) - xs.double()[:, None]).abs().max()) < 16 * U * (Wr + Hr)
                    assert float((ndc.v[..., 1] * (Hr - 1) - ys.double()[:, None]).abs().max()) < 16 * U * (Wr + Hr)
                    zn = (z.double() - float(cam["nf"][0])) / (float(cam["nf"][1]) - float(cam["nf"][0]))
                    if not lindisp:
                        assert float((ndc.v[..., 2] - zn).abs().max()) < 1e-12
                    assert float(ndc.v[..., 2].min()) > -1e-12 and float(ndc.v[..., 2].max()) < 1 + 1e-12
    assert worst <= 1.0, worst


@pytest.mark.parametrize("ref_hw", R.REF_HW)
@pytest.mark.parametrize("geometry", R.GEOMETRIES)
def test_raygen_reference_and_bound(geometry, ref_hw):
    cam = R.camera_case(geometry, ref_hw)
    Hr, Wr = ref_hw
    worst = 0.0
    g = torch.Generator().manual_seed(3)
    for N, S in R.RAY_SHAPES:
        xs, ys = R.pixel_ids(cam, N)
        if N >= 2:
            assert (xs[0], ys[0]) == (cam["W"] - 1, cam["H"] - 1) and (xs[1], ys[1]) == (0, 0)
        for pad in (0, 4):
            for lindisp in (False, True):
                for t_rand in (None, torch.rand((N, S), generator=g)):
                    ref = R.raygen_ref64(xs, ys, cam["Kt"], cam["c2w"], cam["nf"], S, lindisp, t_rand)
                    ndc = R.ndc_ref64(ref["pts"], cam["w2c"], cam["Kr"], cam["nf"], Wr, Hr, pad, lindisp)
                    p32, d32, n32, z32 = R.raygen_oracle32(cam, xs, ys, S, pad, lindisp, t_rand)
                    worst = max(worst, R.within(p32, ref["pts"]), R.within(d32, ref["dirs"]), R.within(z32, ref["z"]), R.within(n32, ndc))
                    if geometry == "same" and pad == 0:
                        assert float((ndc.v[..., 0] * (Wr - 1) - xs.double()[:, None]).abs().max()) < 1e-9
                        assert float((ndc.v[..., 1] * (Hr - 1) - ys.double()[:, None]).abs().max()) < 1e-9
                        if t_rand is None and S > 1:
                            assert float(ndc.v[:, 0, 2].abs().max()) < 1e-12 and float((ndc.v[:, -1, 2] - 1).abs().max()) < 1e-12
    assert worst <= 1.0, worst


@pytest.mark.parametrize("near,far", [(2.125, 4.525), (2.0, 6.0), (1.0, 4.0)])
def test_jitter_edge_rows_stay_ordered_and_inside(near, far):
    """t_rand rows of all 0 and all 1 - 2^-24 in the oracle's arithmetic: non-decreasing depths inside [near, far], z_0 = near for t_rand = 0."""
    from oracle import mvsnerf_oracle as O
    for S in (1, 2, 3, 64, 128):
        for tr in (0.0, 1.0 - 2.0 ** -24):
            n32, f32 = torch.tensor(near), torch.tensor(far)
            z = O.stratified_depths(n32, f32, 3, S, torch.full((3, S), tr))
            assert bool((z[:, 1:] >= z[:, :-1]).all()) and bool((z >= n32).all()) and bool((z <= f32).all())
            if tr == 0.0:
                assert bool((z[:, 0] == n32).all())


# ------------------------------------------------------------------------------------------------------------------ positional encoding
@pytest.mark.parametrize("d", R.PE_D)
def test_posenc_reference(d):
    for P in R.PE_P:
        x = R.posenc_inputs(P, d)
        assert float(x.abs().max()) <= 1.5
        for L in R.PE_L:
            ref, a = R.posenc_ref64(x, L)
            assert ref.shape == (P, d * (1 + 2 * L)) and torch.equal(ref[:, :d], x.double())
            if L:
                # f-major: column d + f d + c holds sin(x_c 2^f)
                assert torch.equal(ref[:, d + (L - 1) * d + (d - 1)], torch.sin(x[:, d - 1].double() * 2.0 ** (L - 1)))
                e = max(float((torch.sin(a).double() - torch.sin(a.double())).abs().max()), float((torch.cos(a).double() - torch.cos(a.double())).abs().max()))
                assert e <= 2 * U, e                                               # torch's fp32 sin / cos on the CPU: below two units of the last place of 1
