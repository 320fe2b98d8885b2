"""The compositing kernels of csrc/composite.hip / composite_wave.h against float64 (references and bounds: tests/edge_refs.py, run without a GPU by
test_edge_refs.py; u = 2^-24).

D. mvsnerf_composite_fwd: every composite_kernel<CHUNK> instantiation (S <= 64: 1, <= 128: 2, <= 192: 3, <= 256: 4, above: the run-time path), each with a full and
   a ragged last lane, N in {1, 5, 9} (four rays per workgroup), white_bkgd on and off, on densities that are small, mixed, dense (alpha = 1 exactly, t = 1e-10),
   sparse (70 % exact zeros), all zero on one ray, saturating on a ray's first sample.  Reference: float64 raw2alpha / raw2outputs on the fp32 inputs, the +1e-10
   included; per-output bounds in edge_refs.composite_ref64.
   A ray without density: the reference forms disp = 1 / max(1e-10, 0/0) = NaN (torch.max propagates it); the kernels' fmaxf(1e-10f, NaN) is 1e-10, so they return the
   finite 1e10.  That value is asserted here and documented in ops.composite; raymarch_fused_kernel's epilogue shares composite_wave and is driven with an MLP
   whose parameters are all zero (density 0 everywhere).
E. mvsnerf_composite_bwd: the same S and densities without the all-dense family; g_rgb, g_depth, g_acc, g_weights, g_alpha each alone (the other pointers NULL) and
   all together.  Reference: float64 autograd.  S_i / t_i is ill-conditioned behind a saturated sample, so the density gradient is held to a yardstick: per ray
   e = max_j |d_sigma_j - ref| / R with R = sum_j |G_j| w_j + max_j |G_j| T_j + max_j |g_alpha,j|, and e_kernel <= 4 e_torch + 16 u where e_torch is torch's fp32 CPU
   autograd of the same forward on the same inputs.  The colour gradients w g_rgb get the forward's weight bound times |g_rgb|.
   Measured on an MI355X: largest e_kernel / e_torch over the cases 1.68 (S = 63, white_bkgd off: 2.10e-07 against 1.25e-07); largest per-ray share of
   4 e_torch + 16 u: 0.23 (S = 1); colour gradients at most 0.15 of their bound; forward outputs at most 0.22 (alpha) of theirs."""
import pytest
import torch

from tests import edge_refs as E
from tests.util import record_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = E.U

def _forward(raw, z, white):
    from mvsnerf_amd import ops
    with torch.no_grad():
        return tuple(t.cpu() for t in ops.composite(raw.to(DEV), z.to(DEV), white_bkgd=white))


def _assert_empty_ray(outs, ray, white, tag):
    rgb, disp, acc, w, depth, alpha = outs
    assert bool((rgb[ray] == (1.0 if white else 0.0)).all()), tag
    assert float(acc[ray]) == 0.0 and float(depth[ray]) == 0.0 and bool((w[ray] == 0).all()) and bool((alpha[ray] == 0).all()), tag
    assert float(disp[ray]) == 1e10, (tag, float(disp[ray]))            # finite where the reference has NaN (module docstring)


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("S", E.S_LIST)
def test_composite_forward_vs_float64(S, white):
    """composite_kernel<1> (S = 1, 2, 63, 64), <2> (65, 128), <3> (129, 192), <4> (193, 256), <0> (257, 300) through ops.composite: alpha, weights, rgb, depth, acc and
    disp (rays with acc > 1e-3) within the float64 bounds; the ray without density exactly rgb = 0 (1 with white_bkgd), acc = depth = weights = alpha = 0, disp = 1e10."""
    worst = {}
    cases = [(f"{f}:N{N}", E.composite_inputs(f, N, S)) for f in E.FAMILIES for N in (1, 5, 9)]
    cases += [("zero_ray", E.zero_ray_inputs(S)), ("saturated_first", E.saturated_ray_inputs(S))]
    for tag, (raw, z) in cases:
        outs = _forward(raw, z, white)
        ref = E.composite_ref64(raw, z, white)
        sh = E.composite_shares(outs, ref)
        for k, v in sh.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert all(v <= 1.0 for v in sh.values()), f"S={S} white={white} {tag}: shares of the bounds {sh}"
        if tag == "zero_ray":
            _assert_empty_ray(outs, 0, white, tag)
        elif raw.shape[0] >= 5:
            _assert_empty_ray(outs, 1, white, tag)
    for k, v in worst.items():
        record_err(f"composite_fwd_share:{k}:S{S}:white{int(white)}", v, tol=1.0)


def _backward(raw, z, white, grads):
    from mvsnerf_amd import _lib
    from mvsnerf_amd.ops import stream_ptr
    N, S = z.shape
    keep = {k: v.to(DEV).contiguous() for k, v in grads.items()}
    raw_d, z_d = raw.to(DEV).contiguous(), z.to(DEV).contiguous()
    d_raw = torch.full((N, S, 4), float("nan"), device=DEV)
    ptr = [keep[k].data_ptr() if k in keep else 0 for k in E.GRAD_NAMES]
    rc = _lib.lib().mvsnerf_composite_bwd(raw_d.data_ptr(), z_d.data_ptr(), N, S, int(white), *ptr, d_raw.data_ptr(), stream_ptr())
    assert rc == 0
    return d_raw.cpu()


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("S", E.S_LIST)
def test_composite_backward_vs_float64_autograd(S, white):
    """composite_bwd_kernel (chunk = ceil(S / 64) = 1 .. 5) on nine rays of small, mixed and sparse densities (ray 1 without density, ray 3 saturating on its first
    sample), every gradient alone - each NULL-pointer branch of the kernel - and all together: per ray e_kernel <= 4 e_torch + 16 u, colour gradients within the
    forward's weight bound times |g_rgb|."""
    N = 9
    grads = E.composite_grads(N, S)
    worst = {"e_kernel": 0.0, "e_torch": 0.0, "ratio": 0.0, "colour": 0.0}
    for fam in ("small", "mixed", "sparse"):
        raw, z = E.composite_inputs(fam, N, S)
        for combo in E.GRAD_COMBOS:
            sel = {k: grads[k] for k in combo}
            d_raw = _backward(raw, z, white, sel)
            assert bool(torch.isfinite(d_raw).all()), (fam, combo)
            r = E.composite_bwd_errors(d_raw, raw, z, white, sel)
            ek, et = r["e"], r["e_torch"]
            worst["e_kernel"], worst["e_torch"] = max(worst["e_kernel"], float(ek.max())), max(worst["e_torch"], float(et.max()))
            worst["ratio"] = max(worst["ratio"], float((ek / (4 * et + 16 * U)).max()))
            worst["colour"] = max(worst["colour"], r["col"])
            assert bool((ek <= 4 * et + 16 * U).all()), f"S={S} white={white} {fam} {combo}: e_kernel {ek.tolist()} e_torch {et.tolist()}"
            assert r["col"] <= 1.0, f"S={S} white={white} {fam} {combo}: colour gradients at {r['col']:.3f} of the bound"
    record_err(f"composite_bwd:e_kernel:S{S}:white{int(white)}", worst["e_kernel"], tol=4 * worst["e_torch"] + 16 * U)
    record_err(f"composite_bwd:e_torch:S{S}:white{int(white)}", worst["e_torch"])
    record_err(f"composite_bwd_share:S{S}:white{int(white)}", worst["ratio"], tol=1.0)
    record_err(f"composite_bwd_colour_share:S{S}:white{int(white)}", worst["colour"], tol=1.0)


@pytest.mark.parametrize("N,S", [(37, 16), (20, 128)])
def test_raymarch_epilogue_on_rays_without_density(N, S):
    """raymarch_fused_kernel (ops.raymarch, fp32 mode, depth-fastest volume, whole rays per tile: its epilogue is composite_wave) with an MLP whose parameters are all
    zero: every ray is empty, and the outputs are those of the stand-alone kernel - rgb = 0 (1 with white_bkgd), acc = depth = weights = alpha = 0, disp = 1e10."""
    from mvsnerf_amd import models, ops
    from tests.test_gpu_raymarch_onelaunch import _hwdc, _inputs
    m = models.MVSNeRF(D=6, W=128, input_ch_pts=63, input_ch_views=3, input_ch_feat=20, skips=[4], net_type="v0")
    for p in m.parameters():
        torch.nn.init.zeros_(p)
    packed = m.to(DEV).packed(20)
    x = _inputs(N, S, seed=S)
    vol_cl = _hwdc(x["vol"])
    for white in (False, True):
        with ops.mlp_precision("fp32"), torch.no_grad():
            o = ops.raymarch(vol_cl, x["imgs"], x["w2cs"], x["Ks"], packed, x["pts"], x["ndc"], x["z"], x["dirs"], white_bkgd=white, want=("disp", "acc"))
        assert bool((o["raw"][..., 3] == 0).all())
        outs = tuple(o[k].cpu() for k in ("rgb_map", "disp", "acc", "weights", "depth", "alpha"))
        for ray in range(N):
            _assert_empty_ray(outs, ray, white, f"raymarch N={N} S={S} ray {ray}")
