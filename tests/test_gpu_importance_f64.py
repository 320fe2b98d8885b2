"""sample_pdf_kernel and ray_marcher_fine_kernel (csrc/importance.hip) against float64, on inputs where the float64 value is either exact in fp32 (asserted bit for
bit) or well conditioned (asserted within an operation-count bound).  References, families and bounds live in tests/ray_refs.py; test_ray_refs.py holds every one of
them against the fp32 oracle on the CPU, with the shares of left-out and weakly bounded samples.

1a. sample_pdf, exact family: dyadic weights, bins and u - every knot, u = 0 and u = 1 among them, and knots on top of bins below the `denom < 1e-5` switch.
1b. sample_pdf, conditioned families (dense, sparse, one-hot, zero weights): |z - z64| <= width (den < 1e-5 ? 1 : 2 g C_a / den) + 4 u max|bins| + 4 u width.
2a. ray_marcher_fine on empty rays: the output is sort(cat(samples64, z_vals)) bit for bit, with samples that equal two coarse depths, repeated u, u = 0.
2b. ray_marcher_fine on a binary density (alpha exactly 0 or 1, samples on voxel centres): every coarse depth present bit for bit, rows ascending, the
    remaining samples inside the order-statistic band of width (den < 1e-5 ? dC : min(1, 2 dC / den)) + 48 u, dC = (2 S + 16) u.
2c. Random densities stay with test_gpu_importance.py::test_ray_marcher_fine_vs_oracle and its allowances (1 % of rays outside a 1 % band, 10 % in the saturated
    family).  A float64 bound on the whole chain is vacuous there: where alpha is tiny the empty bins' pdf ~1e-5 / sum amplifies the expf and trilinear roundings
    of the weights by ~1e4, and the CPU prototype of such a bound came out wider than 1 % of the bin for 3-84 % of the samples.  Do not reopen this with a
    tighter tolerance on random densities; tighten the binary family instead."""
import pytest
import torch

from tests import ray_refs as R
from tests.util import record_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _poison(*shape):
    """The ops allocate their outputs with torch.empty: leave NaNs in the block the caching allocator hands out next, so that an element the kernel
    does not write cannot hold a correct value left by an earlier call."""
    torch.full(shape, float("nan"), device=DEV)


# ------------------------------------------------------------------------------------------------------------------ 1. sample_pdf
@pytest.mark.parametrize("nb", R.PDF_NB)
def test_sample_pdf_exact_family_bit_for_bit(nb):
    """u = cdf[k] returns bins[k], u = 0 bins[0], u = 1 the last bin edge, the 1/2 and 1/4 points their exact interpolants: every bit of the float64 value."""
    from mvsnerf_amd import ops
    bins, w, u, d, pick = R.pdf_exact_case(nb)
    ref = R.sample_pdf_ref64(bins, d, u)["z"].to(DEV)
    knot_ref = torch.gather(bins.double(), 1, pick.clamp(max=nb - 1)).to(DEV)
    knot = (pick < nb).to(DEV)
    bins_d, w_d, u_d = bins.to(DEV), w.to(DEV), u.to(DEV)
    with torch.no_grad():
        for N in R.PDF_N:
            for NI in R.PDF_NI:
                _poison(N, NI)
                out = ops.sample_pdf(bins_d[:N].contiguous(), w_d[:N].contiguous(), u_d[:N, :NI].contiguous()).double()
                assert torch.equal(out, ref[:N, :NI]), (N, NI, float((out - ref[:N, :NI]).abs().max()))
                assert torch.equal(out[knot[:N, :NI]], knot_ref[:N, :NI][knot[:N, :NI]])


@pytest.mark.parametrize("nb", R.PDF_NB)
@pytest.mark.parametrize("family", R.PDF_FAMILIES)
def test_sample_pdf_conditioned_families_vs_float64(family, nb):
    from mvsnerf_amd import ops
    bins, w, u = R.pdf_conditioned_case(family, nb)
    ref = R.sample_pdf_ref64(bins, R.pdf_q(w), u)
    bound, left = R.sample_pdf_bound(ref, bins, u, nb)
    z64, bound, keep = ref["z"].to(DEV), bound.to(DEV), (~left).to(DEV)
    bins_d, w_d, u_d = bins.to(DEV), w.to(DEV), u.to(DEV)
    worst = 0.0
    with torch.no_grad():
        for N in R.PDF_N:
            for NI in R.PDF_NI:
                _poison(N, NI)
                out = ops.sample_pdf(bins_d[:N].contiguous(), w_d[:N].contiguous(), u_d[:N, :NI].contiguous()).double()
                assert bool(torch.isfinite(out).all())
                share = ((out - z64[:N, :NI]).abs() / bound[:N, :NI])[keep[:N, :NI]]
                if share.numel():
                    worst = max(worst, float(share.max()))
                assert bool((out >= bins_d[:N, :1].double()).all()) and bool((out <= bins_d[:N, -1:].double()).all())      # left-out samples included
    print(f"sample_pdf {family} nb={nb}: largest error {worst:.3f} of the bound")
    record_err(f"sample_pdf_f64:{family}:{nb}", worst, tol=1.0)
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------ 2. ray_marcher_fine
@pytest.mark.parametrize("S", [S for S in R.FINE_S if R.fine_is_exact_S(S)])
def test_ray_marcher_fine_empty_rays_bit_for_bit(S):
    from mvsnerf_amd import ops
    dens, ndc, z, u = R.fine_empty_case(S)
    _, smp = R.fine_empty_ref64(z, u)
    zs64, z64 = smp["z"].to(DEV), z.double().to(DEV)
    dens_d, ndc_d, z_d, u_d = dens.to(DEV), ndc.to(DEV), z.to(DEV), u.to(DEV)
    with torch.no_grad():
        for N in R.FINE_N:
            for NI in R.FINE_NI:
                ref = torch.sort(torch.cat([zs64[:N, :NI], z64[:N]], -1), -1)[0]
                _poison(N, S + NI)
                out = ops.ray_marcher_fine_z(dens_d, ndc_d[:N].contiguous(), z_d[:N].contiguous(), u_d[:N, :NI].contiguous()).double()
                assert torch.equal(out, ref), (N, NI)


@pytest.mark.parametrize("S", R.FINE_S)
def test_ray_marcher_fine_binary_density_vs_float64(S):
    from mvsnerf_amd import ops
    dens, ndc, z, u, sigma = R.fine_binary_case(S)
    ref, bound, left = R.fine_binary_ref64(sigma, z, u)
    dens_d, ndc_d, z_d, u_d = dens.to(DEV), ndc.to(DEV), z.to(DEV), u.to(DEV)
    zlo, zhi = float(z.min()), float(z.max())
    worst = 0.0                                                                     # largest error / bound on the rows where sample i can be paired with its reference
    with torch.no_grad():
        for N in R.FINE_N:
            for NI in R.FINE_NI:
                _poison(N, S + NI)
                out = ops.ray_marcher_fine_z(dens_d, ndc_d[:N].contiguous(), z_d[:N].contiguous(), u_d[:N, :NI].contiguous()).cpu()
                assert bool((out[:, 1:] >= out[:, :-1]).all()), (N, NI)
                rest, ok = R.remove_multiset(out, z[:N])
                assert bool(ok.all()), (N, NI)                                      # every coarse depth is there, bit for bit
                lo, hi = R.order_stat_band(ref["z"][:N, :NI], bound[:N, :NI], left[:N, :NI], zlo, zhi)
                inside = (rest.double() >= lo) & (rest.double() <= hi)
                assert bool(inside.all()), (N, NI, int((~inside).sum()))
                # a figure for the record: rows without left-out samples whose reference order is separated by more than the bounds pair up rank by rank
                zr, order = torch.sort(ref["z"][:N, :NI], -1)
                br = torch.gather(bound[:N, :NI], 1, order)
                paired = ~left[:N, :NI].any(-1) & ((zr[:, 1:] - zr[:, :-1]) > (br[:, 1:] + br[:, :-1])).all(-1)
                if bool(paired.any()):
                    worst = max(worst, float(((rest.double() - zr).abs() / br)[paired].max()))
    print(f"ray_marcher_fine binary S={S}: largest error {worst:.3f} of the bound on the rows that pair up")
    record_err(f"ray_marcher_fine_f64:binary:{S}", worst, tol=1.0)
    assert worst <= 1.0, worst
