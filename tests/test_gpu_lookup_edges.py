"""The gather and scatter kernels of csrc/sample.hip / sample_dev.h against float64 on the inputs where such kernels go wrong: border planes, size-1
axes, exact knots, half cells, samples one cell outside, partial tail quads, samples in ray order.  References, input families and bounds live in
tests/edge_refs.py (test_edge_refs.py runs them without a GPU); u = 2^-24 and the "fp32 chain" are defined there.

A. trilinear lookup, every route: hard bound |out - ref| <= 9 u S + 1e-30 against the float64 sum over the fp32-chain weights, exact zeros outside the volume,
   ATen's float64 grid_sample as the independent reference, and torch.equal between the routes documented as bit-identical.
B. colour lookup (border padding, strict mask), the zero-padded feature channels of color_feat_sample, and the direction feature.
C. trilinear scatter: the float-atomic kernels within (n_v + 2) u Sabs and the fixed-point variant within 2 u Sabs + n_v 2^(e-40) of the exact float64 sum of the
   kernels' own fp32 contributions, voxels that receive nothing exactly 0.0; ray-ordered samples so that the depth hand-off of volume_sample_c8_bwd_kernel fires
   on three of four neighbour pairs; the hand-off key collision of volumes wider than 4091 voxels.  (These bounds need the scatter's weights to be the forward's:
   compiled with fp contraction, (ix - fx) skipped the rounding of ix and the ragged volume sat at 480 x the bound; the kernels now switch contraction off.)

Out of scope: the 64-bit-offset instantiations of the C = 8 kernels (volume_sample_c8_kernel<1, false>, volume_sample_c8_zfast_kernel<false>,
gather_fused_kernel<false, .>) need a volume of 2 GB; the wide kernel's 64-bit form is reached through force_offsets64.  NaN, Inf and huge coordinates are not fed:
the float64 reference is undefined there, the kernels' handling of them (float compares before any int conversion) stays a matter of code reading."""
import pytest
import torch

from tests import edge_refs as E
from tests.util import record_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = E.U


def _dev64(t):
    return t.to(DEV, torch.float64)


# ------------------------------------------------------------------------------------------------------------------ A. trilinear lookup
_GATHER_RIG = {}


def _gather_rig():
    """Images, cameras and points for ops.gather (only its volume part is looked at in section A)."""
    if not _GATHER_RIG:
        imgs, _, w2cs, Ks, pts = E.exact_geometry_case(3)
        _GATHER_RIG["r"] = (imgs.to(DEV), w2cs.to(DEV), Ks.to(DEV), pts[torch.arange(E.P_POOL) % pts.shape[0]].contiguous().to(DEV))
    return _GATHER_RIG["r"]


def _lookup_routes(vol40, ndc_pool, P, check):
    """Every lookup route at the first P samples of the pool.  check(tag, out (P, C)) holds one result to the references."""
    from mvsnerf_amd import ops
    ndc = ndc_pool[:P].contiguous()
    D, H, W, _ = vol40.shape
    two_orders = D > 1 and H * W > 1          # with D == 1 or H * W == 1 the two memory orders are the same bytes
    imgs, w2cs, Ks, pts = _gather_rig()
    per_c = {}
    for C in (4, 8, 12, 20, 40):
        vd = vol40[..., :C].contiguous()
        vh = E.hwdc_view(vd)
        assert ops.vol_ptr_layout(vd)[1] == ops.VOL_DHWC
        if two_orders:
            assert ops.vol_ptr_layout(vh)[1] == ops.VOL_HWDC
        a, b = ops.volume_sample(vd, ndc), ops.volume_sample(vh, ndc)       # C == 8: volume_sample_c8_kernel<1, true> / volume_sample_c8_zfast_kernel<true>; else generic
        check(f"C{C}:dhwc", a)
        check(f"C{C}:hwdc", b)
        assert torch.equal(a, b), f"C{C}: HWDC != DHWC"
        per_c[C] = a
        if C == 8:
            for v, tag in ((vd, "dhwc"), (vh, "hwdc")):
                o = torch.zeros((P, 10), device=DEV)                         # out_stride % 4 != 0: volume_sample_generic_kernel, both layouts
                ops.volume_sample(v, ndc, out=o, out_stride=10)
                check(f"C8:generic:{tag}", o[:, :8])
                assert torch.equal(o[:, :8], a) and bool((o[:, 8:] == 0).all()), f"generic C8 {tag} != c8 kernel"
                f, _ = ops.gather(v, imgs, w2cs, Ks, pts[:P].view(P, 1, 3), ndc.view(P, 1, 3))      # gather_fused_kernel<true, ZFAST>
                check(f"C8:fused:{tag}", f[:, 0, :8])
                assert torch.equal(f[:, 0, :8], a), f"fused {tag} != stand-alone"
        if C > 8:
            rd = torch.randn((P, 3), device=DEV)
            for v, tag in ((vd, "dhwc"), (vh, "hwdc")):
                for f64 in (False, True):                                   # volume_sample_wide_kernel<!f64, ZFAST>
                    f, _ = ops.gather_colorvol(v, ndc.view(P, 1, 3), force_offsets64=f64)
                    check(f"C{C}:wide:{tag}:{int(f64)}", f[:, 0])
                    assert torch.equal(f[:, 0], a), f"wide C{C} {tag} offsets64={f64} != generic"
                fd, dirs = ops.gather_colorvol(v, ndc.view(P, 1, 3), rays_dir=rd, w2c_ref=w2cs[0])
                assert torch.equal(fd[:, 0], a), "gather_colorvol with directions != lookup only"
                assert torch.equal(dirs, ops.dir_feature(rd, w2cs[0]))
    return per_c


@pytest.mark.parametrize("dims,family", [(d, "random") for d in E.VOLUMES] + [(d, "dyadic") for d in E.VOLUMES if E.is_dyadic_volume(d)])
def test_trilinear_lookup_every_route_vs_float64(dims, family):
    """volume_sample_c8_kernel<1, true>, volume_sample_c8_zfast_kernel<true>, volume_sample_generic_kernel (C = 8 with out_stride 10, C = 4, 12, 20, 40; both
    layouts), volume_sample_wide_kernel (C = 12, 20, 40; both layouts; 32- and 64-bit offsets) and gather_fused_kernel<true, false / true>, at
    P in {1, 3, 63, 64, 65, 1021}.  dyadic (ndc = k/64; volumes whose size - 1 is 0 or a power of two): exact knots, border planes, ix = -1 and ix = size, half
    cells, the band -1 < ix < 0; random: uniform(-0.15, 1.15), also on the ragged (7, 12, 28)."""
    seed = sum(dims)
    vol = E.make_volume(dims, seed)
    ndc = E.dyadic_pool(seed) if family == "dyadic" else E.random_pool(seed)
    ref, S = E.lookup_ref(vol, ndc)
    gs = E.lookup_gs64(vol, ndc)
    M = float(vol.abs().max())
    if family == "dyadic":
        assert E.chain_is_exact(ndc, dims)
        assert float((gs - ref).abs().max()) <= 1e-12 * M
        gs_bound = E.lookup_hard_bound(S) + 1e-12 * M
    else:
        gs_bound = E.lookup_hard_bound(S) + E.lookup_coord_slack(vol)
    R = {"ref": _dev64(ref), "S": _dev64(S), "bound": _dev64(E.lookup_hard_bound(S)), "gs": _dev64(gs), "gs_bound": _dev64(gs_bound)}
    worst = {"hard": 0.0, "gs": 0.0}
    vol_d, ndc_d = vol.to(DEV), ndc.to(DEV)
    with torch.no_grad():
        for P in E.P_LIST:
            def check(tag, out):
                C = out.shape[1]
                o = out.double()
                hard = float(((o - R["ref"][:P, :C]).abs() / R["bound"][:P, :C]).max())
                ind = float(((o - R["gs"][:P, :C]).abs() / R["gs_bound"][:P, :C]).max())
                worst["hard"], worst["gs"] = max(worst["hard"], hard), max(worst["gs"], ind)
                assert hard <= 1.0, f"{dims} {family} P={P} {tag}: {hard:.3f} of 9 u S"
                assert bool((out[R["S"][:P, :C] == 0] == 0).all()), f"{dims} {family} P={P} {tag}: non-zero outside the volume"
                assert ind <= 1.0, f"{dims} {family} P={P} {tag}: {ind:.3f} of the grid_sample bound"
            _lookup_routes(vol_d, ndc_d, P, check)
    record_err(f"lookup_hard_share:{dims}:{family}", worst["hard"], tol=1.0)
    record_err(f"lookup_gridsample_share:{dims}:{family}", worst["gs"], tol=1.0)


# ------------------------------------------------------------------------------------------------------------------ B. colour lookup, direction feature
def _color_outputs(imgs, feats, w2cs, Ks, pts):
    """{route: (P, V, channels)} of color_sample_kernel, color_feat_sample_kernel and the colour part of gather_fused_kernel (both layouts)."""
    from mvsnerf_amd import ops
    V = imgs.shape[0]
    P = pts.reshape(-1, 3).shape[0]
    d = [t.to(DEV) for t in (imgs, w2cs, Ks, pts.reshape(-1, 3).contiguous())]
    out = {}
    with torch.no_grad():
        out["color_sample"] = ops.color_sample(d[0], d[1], d[2], d[3]).view(P, V, 4)
        assert torch.equal(ops.color_sample(d[0], d[1], d[2], d[3], with_mask=False).view(P, V, 3), out["color_sample"][..., :3])
        if feats is not None:
            out["color_feat_sample"] = ops.color_feat_sample(d[0], feats.to(DEV), d[1], d[2], d[3]).view(P, V, -1)
        vol = E.make_volume((3, 4, 5), 1, 8).to(DEV)
        ndc = torch.rand((P, 1, 3), device=DEV)
        for v, tag in ((vol, "dhwc"), (E.hwdc_view(vol), "hwdc")):
            f, _ = ops.gather(v, d[0], d[1], d[2], d[3].view(P, 1, 3), ndc)
            out[f"gather_fused:{tag}"] = f[:, 0, 8:].reshape(P, V, 4)
            assert torch.equal(out[f"gather_fused:{tag}"], out["color_sample"]), f"fused colour lookup ({tag}) != color_sample"
    return {k: v.cpu().double() for k, v in out.items()}


@pytest.mark.parametrize("V", [1, 3, 5, 6])
def test_colour_lookup_exact_geometry(V):
    """color_sample_kernel, color_feat_sample_kernel (feature maps 5 x 9 next to 9 x 17 images) and gather_fused_kernel<true, false / true> for V views (V > 4: a lane
    owns views q and q + 4).  Identity w2c, power-of-two focal lengths, points with z in {1, 2, 4} and dyadic x, y: the fp32 projection is exact (asserted), so the
    samples sit exactly on pixel centres, on the last row and column, on g = +-1 (mask 0; 1 one dyadic step inside) and outside the image (colours border-clamped,
    feature channels zero).  Bound 5 u S_c per channel against float64 grid_sample; masks equal."""
    imgs, feats, w2cs, Ks, pts = E.exact_geometry_case(V)
    H, W = imgs.shape[2:]
    ref = E.color_ref64(imgs, w2cs, Ks, pts, feats)
    for v in range(V):
        assert torch.equal(E.project32(pts, w2cs[v], Ks[v], W, H).double(), ref["grid"][:, v])
    worst = 0.0
    for route, o in _color_outputs(imgs, feats, w2cs, Ks, pts).items():
        share = float(((o[..., :3] - ref["col"]).abs() / (5 * U * ref["col_S"] + 1e-30)).max())
        assert torch.equal(o[..., -1], ref["mask"]), f"{route}: mask"
        if route == "color_feat_sample":
            share = max(share, float(((o[..., 3:5] - ref["feat"]).abs() / (5 * U * ref["feat_S"] + 1e-30)).max()))
            assert bool((o[..., 3:5][ref["feat_S"] == 0] == 0).all())
        worst = max(worst, share)
        assert share <= 1.0, f"{route} V={V}: {share:.3f} of 5 u S_c"
    record_err(f"colour_exact_share:V{V}", worst, tol=1.0)


def test_colour_lookup_general_rig():
    """color_sample_kernel and gather_fused_kernel on make_rig(64, 96) (four rotated views), (N, S) = (37, 5), all points in front of every camera.  Colours within
    5 u S_c + 2 max|img| delta_pix of float64, delta_pix (edge_refs.delta_pix) the bound on the fp32 pixel coordinates from color_project's operation count:
    4 roundings per camera coordinate, 3 per row of K, the division, and 4 for / (W-1), * 2 - 1, + 1, * (W-1).  The kernel's largest error stays within 5 x the fp32 CPU
    oracle's + 4 u.  Masks are compared except where |g| is within 1e-5 of 1 (at most 1 % of the samples)."""
    imgs, w2cs, Ks, pts = E.rig_case()
    p = pts.reshape(-1, 3)
    ref = E.color_ref64(imgs, w2cs, Ks, p)
    assert float(ref["camz"].min()) >= 0.5
    near = E.near_mask_edge(ref["grid"])
    assert int(near.sum()) <= 0.01 * near.numel()
    bound = 5 * U * ref["col_S"] + 2 * float(imgs.abs().max()) * ref["dpix"][..., None]
    err_o = float((E.oracle_colors(imgs, w2cs, Ks, p).double()[..., :3] - ref["col"]).abs().max())
    for route, o in _color_outputs(imgs, None, w2cs, Ks, pts).items():
        d = (o[..., :3] - ref["col"]).abs()
        err_k = float(d.max())
        record_err(f"colour_rig:{route}:kernel", err_k, tol=5 * err_o + 4 * U)
        record_err(f"colour_rig:{route}:oracle", err_o)
        record_err(f"colour_rig_share:{route}", float((d / bound).max()), tol=1.0)
        assert bool((d <= bound).all()), f"{route}: {float((d / bound).max()):.3f} of the bound"
        assert err_k <= 5 * err_o + 4 * U, (route, err_k, err_o)
        assert torch.equal(o[..., 3][~near], ref["mask"][~near]), f"{route}: mask"


def test_direction_feature_vs_float64():
    """dir_feature_kernel with and without the rotation, normalised and not: 64 directions - the six axis directions, scaled ones, one with ||d|| = 2^-20, random ones -
    within 8 u sum_j |R_ij| |d_j| / ||d|| of float64 (edge_refs.dir_ref64 counts the operations)."""
    from mvsnerf_amd import ops
    d = E.dir_cases()
    _, w2cs, _, _ = E.rig_case()
    worst = 0.0
    for R, nrm in ((None, True), (w2cs[0], True), (None, False), (w2cs[0], False)):
        ref, b = E.dir_ref64(d, R, nrm)
        with torch.no_grad():
            o = ops.dir_feature(d.to(DEV), None if R is None else R.to(DEV), normalize=nrm).cpu().double()
        diff = (o - ref).abs()
        assert bool((diff <= b).all()), (R is not None, nrm, float((diff / (b + 1e-300)).max()))
        worst = max(worst, float((diff / (b + 1e-300)).max()))
    record_err("dir_feature_share", worst, tol=1.0)


# ------------------------------------------------------------------------------------------------------------------ C. trilinear scatter
def _scatter(kind, dims, C, ndc_d, g_d):
    """mvsnerf_volume_sample_bwd ('atomic') or _bwd_det ('det') into a zeroed (D,H,W,C) volume; g_d (P, g_stride >= C)."""
    from mvsnerf_amd import _lib
    from mvsnerf_amd.ops import stream_ptr
    L = _lib.lib()
    D, H, W = dims
    P, stride = g_d.shape
    gv = torch.zeros((D, H, W, C), device=DEV)
    if kind == "atomic":
        rc = L.mvsnerf_volume_sample_bwd(D, H, W, C, ndc_d.data_ptr(), P, g_d.data_ptr(), stride, gv.data_ptr(), stream_ptr())
    else:
        ws = torch.zeros(L.mvsnerf_volume_sample_bwd_det_workspace_words(D, H, W, C), device=DEV, dtype=torch.int64)
        rc = L.mvsnerf_volume_sample_bwd_det(D, H, W, C, ndc_d.data_ptr(), P, g_d.data_ptr(), stride, gv.data_ptr(), ws.data_ptr(), stream_ptr())
    assert rc == 0
    return gv.cpu()


def _check_scatter(tag, dims, ndc, C, stride, seed, kinds=("atomic", "det")):
    """Both scatters of one (ndc, C, g_stride) case against the exact float64 scatter.  -> largest share of the bounds {kind: share}."""
    g = torch.Generator().manual_seed(seed)
    gfull = torch.randn((ndc.shape[0], stride), generator=g)
    gf = gfull[:, :C].contiguous()
    ref, sabs, nv = E.scatter_ref(ndc, gf, dims)
    ndc_d, g_d = ndc.to(DEV).contiguous(), gfull.to(DEV).contiguous()
    shares = {}
    for kind in kinds:
        out = _scatter(kind, dims, C, ndc_d, g_d)
        bound = E.scatter_atomic_bound(sabs, nv) if kind == "atomic" else E.scatter_det_bound(sabs, nv, gf)
        diff = (out.double() - ref).abs()
        shares[kind] = float((diff / (bound + 1e-300)).max())
        assert bool((out[sabs == 0] == 0).all()), f"{tag} {kind}: a voxel that receives nothing is not 0.0"
        assert bool((diff <= bound).all()), f"{tag} {kind} C={C} stride={stride}: {shares[kind]:.3f} of the bound"
        if kind == "det":
            assert torch.equal(_scatter(kind, dims, C, ndc_d, g_d), out), f"{tag}: the fixed-point scatter does not repeat bit for bit"
    return shares


def _record_scatter(tag, worst):
    for kind, v in worst.items():
        record_err(f"scatter_share:{kind}:{tag}", v, tol=1.0)


def _merge(worst, shares):
    for k, v in shares.items():
        worst[k] = max(worst.get(k, 0.0), v)


@pytest.mark.parametrize("N,S", E.RAY_SHAPES)
def test_scatter_ray_ordered_samples(N, S):
    """volume_sample_c8_bwd_kernel (C = 8; g_stride 8 and 12), volume_sample_bwd_kernel (C = 20, g_stride 24) and the fixed-point variant on N rays x S samples in ray
    order on a (9, 17, 33) volume, dyadic coordinates: z advancing by exactly one plane per sample (the hand-off fires on three of four neighbour pairs, also across
    the boundary of two rays that share a cell), by 1/2 and by 2 planes; rays entering from z < 0 and leaving through z = D - 1; rays on the x = W - 1 column, with
    fy = -1 and with fy = H - 1; a partial last 16-lane row."""
    worst = {}
    for step in E.RAY_STEPS:
        ndc = E.ray_ordered_ndc(N, S, step)
        assert E.chain_is_exact(ndc, E.RAY_DIMS)
        for C, stride in ((8, 8), (8, 12), (20, 24)):
            _merge(worst, _check_scatter(f"rays {N}x{S} step {step}", E.RAY_DIMS, ndc, C, stride, seed=N * 100 + S + C))
    _record_scatter(f"rays:{N}x{S}", worst)


@pytest.mark.parametrize("dims", [(1, 1, 2), (1, 5, 9), (5, 1, 9), (5, 9, 1), (2, 2, 2), (7, 12, 28)])
def test_scatter_small_and_ragged_volumes(dims):
    """Size-1 axes, (2, 2, 2) and a ragged volume, 1021 samples uniform in (-0.15, 1.15) (up to thousands of contributions per voxel): volume_sample_c8_bwd_kernel
    (g_stride 8, 12), volume_sample_bwd_kernel at C = 4, 12, 20 (g_stride 24), 40, and the fixed-point variant at each."""
    ndc = E.random_pool(sum(dims) + 1)
    worst = {}
    for C, stride in ((8, 8), (8, 12), (4, 4), (12, 12), (20, 24), (40, 40)):
        _merge(worst, _check_scatter(f"{dims}", dims, ndc, C, stride, seed=sum(dims) * 10 + C))
    _record_scatter(f"{dims}", worst)


def test_scatter_handoff_key_collision():
    """mvsnerf_volume_sample_bwd on a (3, 3, 4100) C = 8 volume, eight samples alternating (fy = 0, fx = 4097, fz = 0) and (fy = 1, fx = 1, fz = 1): the two cells have the
    same hand-off key fy * 4096 + cx in volume_sample_c8_bwd_kernel and the second lies one plane further, so that kernel moves the first sample's z1 contributions to
    the second sample's voxels.  The launcher therefore sends volumes with W > 4091 (or H >= 2^18) to volume_sample_bwd_kernel.  The widest volume the hand-off kernel
    still takes, (3, 3, 4091) with fx = 4088, is checked next to it."""
    dims, ndc = E.collision_case()
    fx, fy, fz = E.cell_of(ndc, dims)
    assert len(set((fy * 4096 + fx).tolist())) == 1 and fz.tolist() == [0, 1] * 4
    worst = _check_scatter("key collision W=4100", dims, ndc, 8, 8, seed=41)
    dims2, ndc2 = E.collision_case(4091, 4088)
    _merge(worst, _check_scatter("W=4091", dims2, ndc2, 8, 8, seed=42))
    _record_scatter("collision", worst)
