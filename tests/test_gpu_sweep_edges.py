"""Degenerate geometry and tiny shapes for the encode head: the plane sweep (csrc/planesweep.hip, four store layouts), its two backward
kernels (csrc/planesweep_bwd.hip), the stand-alone homo_warp and the image-prep helpers (csrc/encoder_prep.hip), through the C ABI.  References, geometries and
shapes: tests/sweep_refs.py (checked on the CPU by test_sweep_refs.py).

What is pinned here and nowhere else: a source view whose fp32 sample coordinate is not finite has four zero weights in the sweep and in
both backward kernels (no contribution, not counted, no gradient), while homo_warp returns the CPU reference's NaN; voxels behind a camera,
coordinates beyond the int range, taps with one or two pixels inside, tap sets that cross the image border along a column; Hp < 8 (empty
row bands), a single partial chunk, D < 4, H = W = 2; V = 1 forward and backward, every backward instantiation NSRC = 1..7; the blocked
stores without thumbnails; and that the backward entries ACCUMULATE into g_feats_cl.

Outputs sit inside a larger allocation filled with a sentinel and are themselves pre-filled with NaN: a store outside the buffer or a voxel
that is never written shows."""
import pytest
import torch
import torch.nn.functional as F

from tests import sweep_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -1024.0            # exact in fp32, bf16 and fp16; no output can take it (|feats| <= 6)
FENCE = 64                # elements on either side: the inner buffer stays 16-byte aligned for every dtype used


def _fenced(n, dtype=torch.float32, fill=float("nan")):
    big = torch.full((n + 2 * FENCE,), SENT, device=DEV, dtype=dtype)
    inner = big[FENCE:FENCE + n]
    inner.fill_(fill)
    return big, inner


def _fence_intact(big):
    return bool((big[:FENCE] == SENT).all()) and bool((big[-FENCE:] == SENT).all())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _round4(n):
    return (n + 3) // 4 * 4


def _lib():
    from mvsnerf_amd import _lib
    return _lib.lib()


def _sp():
    from mvsnerf_amd.ops import stream_ptr
    return stream_ptr()


LAYOUTS = {"plain": ("mvsnerf_planesweep_costvar_fwd", torch.float32), "blocked": ("mvsnerf_planesweep_costvar_blocked_fwd", torch.float32),
           "bf16": ("mvsnerf_planesweep_costvar_bf16_fwd", torch.bfloat16), "f16x2": ("mvsnerf_planesweep_costvar_f16x2_fwd", torch.float16)}


def _cp(V, with_img):
    """One more channel than the sweep produces, rounded up to four: every case has zero-filled pad channels."""
    return _round4((3 * V if with_img else 0) + R.C + 1)


def _sweep(layout, case, shape, with_img):
    """Run one forward entry on a case of sweep_refs.forward_case.  Returns (cost (flat, its dtype), masks (flat), CP): both fenced, checked
    for an intact fence and for no NaN left inside."""
    H, W, pad, D = shape
    V = case["feats"].shape[0]
    nvox = D * (H + 2 * pad) * (W + 2 * pad)
    CP = _cp(V, with_img)
    nb16 = (CP + 15) // 16
    entry, dtype = LAYOUTS[layout]
    n_cost = {"plain": nvox * CP, "blocked": nvox * CP, "bf16": nb16 * nvox * 16, "f16x2": 2 * nb16 * nvox * 16}[layout]
    feats_cl = case["feats"].permute(0, 2, 3, 1).contiguous().to(DEV)
    imgs_cl = F.pad(case["small"].permute(0, 2, 3, 1), (0, 1)).contiguous().to(DEV)
    proj, depth = case["P"].contiguous().to(DEV), case["dv"].contiguous().to(DEV)
    cbig, cost = _fenced(n_cost, dtype)
    mbig, masks = _fenced((V if with_img else 1) * nvox)
    rc = getattr(_lib(), entry)(feats_cl.data_ptr(), imgs_cl.data_ptr() if with_img else 0, proj.data_ptr(), depth.data_ptr(), V, R.C, H, W, D, pad,
                                cost.data_ptr(), CP, masks.data_ptr(), int(with_img), _sp())
    torch.cuda.synchronize()
    assert rc == 0, (layout, rc)
    assert _fence_intact(cbig) and _fence_intact(mbig), f"{layout}: a store outside the buffer"
    assert not bool(torch.isnan(cost).any()) and not bool(torch.isnan(masks).any()), f"{layout}: an element was never written (or is NaN)"
    return cost.clone(), masks.clone(), CP


def _plain_vs_reference(case, shape, with_img, tag):
    H, W, pad, D = shape
    V = case["feats"].shape[0]
    Hp, Wp = H + 2 * pad, W + 2 * pad
    n_ch = (3 * V if with_img else 0) + R.C
    cost, masks, CP = _sweep("plain", case, shape, with_img)
    cost = cost.view(D, Hp, Wp, CP).cpu()
    masks = masks.view(-1, D, Hp, Wp).cpu()
    assert torch.equal(masks if with_img else masks[0], case["masks"]), f"{tag}: masks / view counts"
    got = cost[..., :n_ch].permute(3, 0, 1, 2)
    if with_img:
        bad = got[:3 * V] != case["cost"][:3 * V]
        assert not bool(bad.any()), f"{tag}: {int(bad.sum())} thumbnail values differ"
    bad = got[-R.C:] != case["cost"][-R.C:]
    assert not bool(bad.any()), f"{tag}: {int(bad.sum())} variance values differ, max {float((got[-R.C:] - case['cost'][-R.C:]).abs().max()):.3e}"
    assert bool((cost[..., n_ch:] == 0).all()), f"{tag}: pad channels are not zero"
    return cost, masks


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("with_img", [0, 1])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_sweep_forward_equals_the_zero_tap_reference(shape, with_img):
    """Plain layout, V = 1, every geometry alone (V = 2) and the mixed V = 4 and 8: masks and counts equal, variance and thumbnail channels equal by
    value (the project's convention: equality up to the sign of zero), pad channels zero, no NaN, nothing written outside."""
    for cname, names in R.forward_cases(shape):
        _plain_vs_reference(R.forward_case(shape, names, with_img), shape, with_img, f"{cname} {shape}")


@pytest.mark.parametrize("with_img", [0, 1])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_sweep_forward_single_view(shape, with_img):
    """V = 1 (the geometry rows are sized from V - 1 = 0 source views): variance exactly 0, count 1, thumbnails the zero-padded reference image."""
    H, W, pad, D = shape
    case = R.forward_case(shape, (), with_img)
    cost, masks = _plain_vs_reference(case, shape, with_img, f"V1 {shape}")
    c0 = 3 if with_img else 0
    assert bool((cost[..., c0:c0 + R.C] == 0).all()) and bool((masks == 1).all())
    if with_img:
        want = F.pad(case["small"][0], (pad, pad, pad, pad)).permute(1, 2, 0)[None].expand(D, -1, -1, -1)
        assert torch.equal(cost[..., :3], want)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_sweep_behind_the_camera_gives_the_bits_of_in_front(shape):
    """-[I|0] puts every voxel behind the source camera at the same image coordinates as [I|0]: the same bits, masks included."""
    for with_img in (0, 1):
        a = _sweep("plain", R.forward_case(shape, ("identity",), with_img), shape, with_img)
        b = _sweep("plain", R.forward_case(shape, ("negated",), with_img), shape, with_img)
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])


@pytest.mark.parametrize("with_img", [0, 1])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_sweep_blocked_stores_are_their_definitions_of_the_plain_volume(shape, with_img):
    """The blocked-fp32, bf16 and two-piece-fp16 entries on the same inputs (V = 1 and thumbnail-free calls included), each held to its storage
    definition applied to the plain entry's output: the same bits permuted into channel blocks of four; every value rounded to bf16 (nearest
    even) in channel blocks of sixteen; hi = fp16(x / 16), lo = fp16(x / 16 - hi) in those blocks, hi plane then lo plane.  Channels beyond CP
    are zero; the masks are the plain entry's."""
    H, W, pad, D = shape
    nvox = D * (H + 2 * pad) * (W + 2 * pad)
    for cname, names in R.forward_cases(shape):
        case = R.forward_case(shape, names, with_img)
        plain, masks, CP = _sweep("plain", case, shape, with_img)
        plain = plain.view(nvox, CP)
        nb = (CP + 15) // 16
        got, m, _ = _sweep("blocked", case, shape, with_img)
        assert _same_bits(got.view(CP // 4, nvox, 4), plain.view(nvox, CP // 4, 4).permute(1, 0, 2)) and _same_bits(m, masks), f"blocked fp32 {cname}"
        ref = torch.zeros((nb * 16, nvox), device=DEV)
        ref[:CP] = plain.t()
        blocks = ref.reshape(nb, 16, nvox).permute(0, 2, 1)
        got, m, _ = _sweep("bf16", case, shape, with_img)
        assert torch.equal(got.view(nb, nvox, 16), blocks.to(torch.bfloat16)) and _same_bits(m, masks), f"bf16 {cname}"
        got, m, _ = _sweep("f16x2", case, shape, with_img)
        scaled = blocks * 0.0625
        hi = scaled.to(torch.float16)
        lo = (scaled - hi.float()).to(torch.float16)
        got = got.view(2, nb, nvox, 16)
        assert torch.equal(got[0], hi) and torch.equal(got[1], lo) and _same_bits(m, masks), f"two-piece fp16 {cname}"


# ------------------------------------------------------------------------------------------------------------------ backward
def _bwd(det, feats_cl, proj, depth, V, shape, g_cost, CP, with_img, prefill=None):
    H, W, pad, D = shape
    L = _lib()
    big, gf = _fenced(V * H * W * R.C, fill=0.0)
    if prefill is not None:
        gf.copy_(prefill.reshape(-1))
    args = (feats_cl.data_ptr(), proj.data_ptr(), depth.data_ptr(), V, R.C, H, W, D, pad, g_cost.data_ptr(), CP, int(with_img), gf.data_ptr())
    if det:
        ws = torch.zeros(L.mvsnerf_planesweep_costvar_bwd_det_workspace_words(V, R.C, H, W), device=DEV, dtype=torch.int64)
        rc = L.mvsnerf_planesweep_costvar_bwd_det(*args, ws.data_ptr(), _sp())
    else:
        rc = L.mvsnerf_planesweep_costvar_bwd(*args, _sp())
    torch.cuda.synchronize()
    assert rc == 0 and _fence_intact(big), ("det" if det else "atomic", rc)
    return gf.clone().view(V, H, W, R.C)


@pytest.mark.parametrize("V", range(1, 9))
@pytest.mark.parametrize("si", range(len(R.BWD_SHAPES)))
def test_sweep_backward_vs_float64_autograd(si, V):
    """mvsnerf_planesweep_costvar_bwd and _bwd_det for every V = 1..8 (V = 1: the per-voxel scatter kernel, the only way it is reached; V >= 2: the column
    kernel's NSRC = V - 1) on mixed degenerate views, against torch.autograd.grad through the float64 restatement - whose view counts are the
    reference's own, not the forward kernel's.  Bound: the project's err < 2e-5 max|g_ref|.  A view whose coordinate is not finite gets no
    gradient from that voxel (the reference's definition).  Three deterministic runs are bit-identical; V = 1 gives exactly zero; and both entries
    ADD to g_feats_cl (float atomics for the source views, `g_feat[refoff] += racc` for view 0): handed a non-zero buffer they return buffer +
    gradient, which is why the Python caller hands in zeros."""
    shape = R.BWD_SHAPES[si]
    H, W, pad, D = shape
    names = R.bwd_views(V, si)
    with_img = (V + si) % 2
    feats, _ = R.make_inputs(V, H, W, seed=77 + 10 * si + V)
    P, dv = R.proj_stack(names, H, W), R.depths(D)
    CP, c_var = _cp(V, with_img), (3 * V if with_img else 0)
    g = torch.Generator().manual_seed(V * 100 + D)
    g_cost = torch.randn((D, H + 2 * pad, W + 2 * pad, CP), generator=g)
    f = feats.double().requires_grad_()
    var = R.costvar_f64(f, P, dv, pad)[0]
    (gref,) = torch.autograd.grad((var * g_cost[..., c_var:c_var + R.C].double().permute(3, 0, 1, 2)).sum(), f)
    gref = gref.permute(0, 2, 3, 1)
    scale = float(gref.abs().max())
    feats_cl = feats.permute(0, 2, 3, 1).contiguous().to(DEV)
    dev = (feats_cl, P.contiguous().to(DEV), dv.to(DEV), V, shape, g_cost.to(DEV), CP, with_img)
    pre = torch.randn((V, H, W, R.C), generator=g) * max(scale, 1.0)
    for det in (False, True):
        tag = f"{'det' if det else 'atomic'} V={V} {shape} {names}"
        got = _bwd(det, *dev)
        err = float((got.cpu().double() - gref).abs().max())
        print(f"[planesweep bwd {tag}] max err {err:.2e}, max|g_ref| {scale:.2e}")
        if V == 1:
            assert scale == 0.0 and bool((got == 0).all()), tag
        assert err < 2e-5 * scale if scale > 0 else err == 0.0, f"{tag}: {err:.3e} vs {scale:.3e}"
        acc = _bwd(det, *dev, prefill=pre.to(DEV))
        if det:
            for _ in range(2):
                assert _same_bits(_bwd(True, *dev), got), f"{tag}: two runs differ"
            # one fixed-point sum per element, converted once and added once: exactly fl(buffer + gradient)
            assert torch.equal(acc, pre.to(DEV) + got), f"{tag}: not buffer + gradient"
        err_acc = float((acc.cpu().double() - pre.double() - gref).abs().max())
        assert err_acc <= 2e-5 * (scale + float(pre.abs().max())), f"{tag}: buffer + gradient off by {err_acc:.3e}"
    assert V == 1 or scale > 0, (names, shape)


# ------------------------------------------------------------------------------------------------------------------ homo_warp
def _nan_or_same_bits(got, want):
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))


@pytest.mark.parametrize("shape", R.SHAPES)
def test_homo_warp_reproduces_the_oracle_nan_included(shape):
    """utils.homo_warp per geometry: the grid is the oracle's bits on every voxel (NaN where it is NaN), `warped` the oracle's bits where the sample
    coordinate is finite and NaN elsewhere - homo_warp deliberately returns the CPU reference's NaN where the sweep gives zero weights."""
    from mvsnerf_amd import utils as U
    from oracle import mvsnerf_oracle as O
    H, W, pad, D = shape
    feats, _ = R.make_inputs(2, H, W, seed=5)
    src, dv = feats[None, 1], R.depths(D)[None]
    for name, (build, _) in R.GEOMETRIES.items():
        P = build(H, W)[None]
        w_ref, g_ref = O.homo_warp(src, P, dv, pad=pad)
        with torch.no_grad():
            w, g = U.homo_warp(src.to(DEV), P.to(DEV), dv.to(DEV), pad=pad)
        assert g.shape == g_ref.shape and _nan_or_same_bits(g.cpu(), g_ref), f"{name}: grid"
        gg = g_ref.view(D, H + 2 * pad, W + 2 * pad, 2)
        nf = R.nonfinite(gg[..., 0], gg[..., 1], H, W)
        w = w.cpu()
        assert torch.equal(torch.isnan(w[0]).all(0), nf) and torch.equal(torch.isnan(w[0]).any(0), nf), f"{name}: NaN voxels"
        assert _nan_or_same_bits(w, w_ref), f"{name}: warped"


def test_homo_warp_on_a_hand_filled_grid():
    """The src_grid= path on a grid holding +-1 exactly, their neighbours, +-1e30, +-inf and NaN in every pairing."""
    from mvsnerf_amd import utils as U
    from oracle import mvsnerf_oracle as O
    H, W, pad, D = R.HAND_GRID_SHAPE
    grid = R.hand_grid(H, W, pad, D)
    feats, _ = R.make_inputs(2, H, W, seed=6)
    w_ref, _ = O.homo_warp(feats[None, 1], None, None, src_grid=grid, pad=pad)
    with torch.no_grad():
        w, g = U.homo_warp(feats[None, 1].to(DEV), None, None, src_grid=grid.to(DEV), pad=pad)
    assert _nan_or_same_bits(g.cpu(), grid)
    gg = grid.view(D, H + 2 * pad, W + 2 * pad, 2)
    nf = R.nonfinite(gg[..., 0], gg[..., 1], H, W)
    w = w.cpu()
    assert torch.equal(torch.isnan(w[0]).all(0), nf) and torch.equal(torch.isnan(w[0]).any(0), nf)
    assert _nan_or_same_bits(w, w_ref)


# ------------------------------------------------------------------------------------------------------------------ image prep
RESIZES = [((8, 12), (2, 3)),       # the production ratio of 4
           ((7, 9), (3, 4)),
           ((3, 5), (7, 11)),       # upscaling: the clamp at 0 and the y1 / x1 clamp
           ((1, 1), (4, 4)),
           ((5, 1), (2, 3)),
           ((6, 6), (6, 6)),        # the identity, bit for bit
           ((40, 52), (17, 23))]    # more than 256 outputs: a second workgroup


@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("size_in,size_out", RESIZES)
def test_resize_bilinear_both_forms(size_in, size_out, N):
    """mvsnerf_resize_bilinear (planes) and mvsnerf_resize_bilinear_nhwc4 (three-channel images, channel-last with a zero fourth channel) against
    resize_f64: within 8 u max|src| (six roundings of a convex combination, and weights that sum to 1 + 2u); the channel-last form holds the
    bits of the planar one.  (It did not when this test was written: left to the compiler, the one source expression was contracted differently in
    the two kernels and per channel - 11 of 48 green values at (7, 9) -> (3, 4) differed in the last bit.  Both kernels now share resize_axis /
    resize_blend in csrc/encoder_prep.hip, every operation spelled out.)"""
    (Hi, Wi), (Ho, Wo) = size_in, size_out
    L = _lib()
    src = torch.randn((N, 3, Hi, Wi), generator=torch.Generator().manual_seed(Hi * 100 + Wo + N))
    ref = R.resize_f64(src, Ho, Wo)
    s = src.to(DEV)
    pbig, planar = _fenced(N * 3 * Ho * Wo)
    assert L.mvsnerf_resize_bilinear(s.data_ptr(), planar.data_ptr(), N * 3, Hi, Wi, Ho, Wo, _sp()) == 0
    cbig, cl = _fenced(N * Ho * Wo * 4)
    assert L.mvsnerf_resize_bilinear_nhwc4(s.data_ptr(), cl.data_ptr(), N, Hi, Wi, Ho, Wo, _sp()) == 0
    torch.cuda.synchronize()
    assert _fence_intact(pbig) and _fence_intact(cbig)
    planar, cl = planar.view(N, 3, Ho, Wo).cpu(), cl.view(N, Ho, Wo, 4).cpu()
    assert not bool(torch.isnan(planar).any()) and not bool(torch.isnan(cl).any())
    err = float((planar.double() - ref).abs().max())
    assert err <= 8 * R.U * float(src.abs().max()), err
    assert _same_bits(cl[..., 3], torch.zeros(N, Ho, Wo))
    assert _same_bits(cl[..., :3].permute(0, 3, 1, 2), planar)
    if size_in == size_out:
        assert _same_bits(planar, src)


@pytest.mark.parametrize("N,C,Cpad,H,W", [(1, 3, 4, 5, 7), (2, 41, 44, 3, 5), (3, 8, 8, 2, 9), (4, 3, 4, 9, 31)])
def test_nchw_to_nhwc_is_permute_and_pad(N, C, Cpad, H, W):
    src = torch.randn((N, C, H, W), generator=torch.Generator().manual_seed(C)).to(DEV)
    big, dst = _fenced(N * H * W * Cpad)
    assert _lib().mvsnerf_nchw_to_nhwc(src.data_ptr(), dst.data_ptr(), N, C, H, W, Cpad, _sp()) == 0
    torch.cuda.synchronize()
    assert _fence_intact(big)
    assert _same_bits(dst.view(N, H, W, Cpad), F.pad(src.permute(0, 2, 3, 1), (0, Cpad - C)))


@pytest.mark.parametrize("C,D,H,W", [(1, 1, 1, 1), (8, 3, 5, 7), (5, 2, 3, 47), (41, 3, 7, 13)])
def test_volume_transposes_are_permutes_and_inverse_to_each_other(C, D, H, W):
    L = _lib()
    src = torch.randn((C, D, H, W), generator=torch.Generator().manual_seed(C + W)).to(DEV)
    big1, cl = _fenced(src.numel())
    assert L.mvsnerf_ncdhw_to_ndhwc(src.data_ptr(), cl.data_ptr(), C, D, H, W, _sp()) == 0
    big2, back = _fenced(src.numel())
    assert L.mvsnerf_ndhwc_to_ncdhw(cl.data_ptr(), back.data_ptr(), C, D, H, W, _sp()) == 0
    torch.cuda.synchronize()
    assert _fence_intact(big1) and _fence_intact(big2)
    assert _same_bits(cl.view(D, H, W, C), src.permute(1, 2, 3, 0))
    assert _same_bits(back.view(C, D, H, W), src)
