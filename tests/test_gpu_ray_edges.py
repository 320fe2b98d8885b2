"""raygen_kernel (csrc/sample.hip), ray_points_kernel (csrc/importance.hip) and posenc_kernel against float64, at the edges the suite did not reach: the first and
last pixel, z = near and z = far, S = 1, a W_ref that is no multiple of 4 with pad > 0, a reference size that differs from the image, launches whose N * S ends on
and next to a block edge, the 64-bit pixel-id branch, jitter rows of all 0 and all 1 - 2^-24, and the two entry points against each other.

References and bounds live in tests/ray_refs.py (test_ray_refs.py holds them against the fp32 oracle on the CPU): float64 on the fp32 inputs with a running
first-order error bound, u |result| per fp32 operation, doubled.  The bit-level tests need no bound.

Out of scope: the 64-bit SAMPLE-id branch of raygen_kernel (N * S >= 2^32 needs 48 GB of outputs); the 64-bit pixel-id branch is reached with first_pixel = 2^32 + 5."""
import pytest
import torch

from tests import ray_refs as R
from tests.util import record_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
NEAR_FAR = ((2.125, 4.525), (2.0, 6.0), (1.0, 4.0))


def _cam_dev(cam):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in cam.items()}


def _variants():
    """(shape index, N, S, pad, lindisp, flag): every shape with both pads and both depth forms; `flag` alternates (per-ray origin / jitter)."""
    for i, (N, S) in enumerate(R.RAY_SHAPES):
        for pad in (0, 4):
            for lindisp in (False, True):
                yield i, N, S, pad, lindisp, bool((i + pad // 4 + lindisp) % 2)


# ------------------------------------------------------------------------------------------------------------------ float64 bounds
@pytest.mark.parametrize("ref_hw", R.REF_HW)
@pytest.mark.parametrize("geometry", R.GEOMETRIES)
def test_ray_points_vs_float64(geometry, ref_hw):
    from mvsnerf_amd import ops
    cam = R.camera_case(geometry, ref_hw)
    cd = _cam_dev(cam)
    Hr, Wr = ref_hw
    worst = 0.0
    with torch.no_grad():
        for i, N, S, pad, lindisp, per_ray in _variants():
            o, d, z, xs, ys = R.ray_points_case(cam, N, S, per_ray)
            pts_ref = R.points_ref64(o, d, z)
            ndc_ref = R.ndc_ref64(pts_ref, cam["w2c"], cam["Kr"], cam["nf"], Wr, Hr, pad, lindisp)
            pts, ndc = ops.ray_points(o.to(DEV), d.to(DEV), z.to(DEV), cd["w2c"], cd["Kr"], cd["nf"], ref_hw=ref_hw, pad=pad, lindisp=lindisp)
            assert pts.shape == (N, S, 3) and ndc.shape == (N, S, 3)
            worst = max(worst, R.within(pts.cpu(), pts_ref), R.within(ndc.cpu(), ndc_ref))
            only_pts, none = ops.ray_points(o.to(DEV), d.to(DEV), z.to(DEV))
            assert none is None and torch.equal(only_pts, pts)
            if geometry == "same" and pad == 0 and not per_ray:                     # ndc.xy gives back pixel / (W-1, H-1); ndc.z runs from 0 to 1
                tol = 2 * ndc_ref.e + 16 * U * (Wr + Hr) / torch.tensor([Wr - 1.0, Hr - 1.0, 1.0], dtype=torch.float64)
                want = torch.stack([xs.double()[:, None].expand(N, S) / (Wr - 1), ys.double()[:, None].expand(N, S) / (Hr - 1),
                                    ndc_ref.v[..., 2]], -1)
                assert bool(((ndc.cpu().double() - want).abs() <= tol).all())
                ends = ndc.cpu().double()[..., 2]
                first, last = (ends[:, 0], ends[:, -1]) if S > 1 else (ends[0::2, 0], ends[1::2, 0])
                assert bool((first.abs() <= 2 * ndc_ref.e[..., 2].max()).all()) and bool(((last - 1).abs() <= 2 * ndc_ref.e[..., 2].max()).all())
    record_err(f"ray_points_f64:{geometry}:{ref_hw}", worst, tol=1.0)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("ref_hw", R.REF_HW)
@pytest.mark.parametrize("geometry", R.GEOMETRIES)
def test_raygen_vs_float64(geometry, ref_hw):
    from mvsnerf_amd import ops
    cam = R.camera_case(geometry, ref_hw)
    cd = _cam_dev(cam)
    Hr, Wr = ref_hw
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    with torch.no_grad():
        for i, N, S, pad, lindisp, jitter in _variants():
            xs, ys = R.pixel_ids(cam, N)
            t_rand = torch.rand((N, S), generator=g) if jitter else None
            ref = R.raygen_ref64(xs, ys, cam["Kt"], cam["c2w"], cam["nf"], S, lindisp, t_rand)
            ndc_ref = R.ndc_ref64(ref["pts"], cam["w2c"], cam["Kr"], cam["nf"], Wr, Hr, pad, lindisp)
            same_size = (cam["H"], cam["W"]) == tuple(ref_hw)
            pts, dirs, ndc, z, pix = ops.raygen(cam["H"], cam["W"], cd["Kt"], cd["c2w"], cd["Kr"], cd["w2c"], cd["nf"], cd["nf"], S, pad=pad, lindisp=lindisp,
                                                xs=xs.to(DEV), ys=ys.to(DEV), t_rand=None if t_rand is None else t_rand.to(DEV),
                                                ref_hw=None if (same_size and i % 2) else ref_hw)
            assert torch.equal(pix.cpu(), torch.stack([ys, xs]))
            worst = max(worst, R.within(pts.cpu(), ref["pts"]), R.within(dirs.cpu(), ref["dirs"]), R.within(z.cpu(), ref["z"]), R.within(ndc.cpu(), ndc_ref))
            if geometry == "same" and pad == 0:                                     # the reference camera is the target camera
                want = torch.stack([xs.double()[:, None].expand(N, S) / (Wr - 1), ys.double()[:, None].expand(N, S) / (Hr - 1), ndc_ref.v[..., 2]], -1)
                assert bool(((ndc.cpu().double() - want).abs() <= 2 * ndc_ref.e + 1e-9).all())
                if t_rand is None and S > 1:
                    nz = ndc.cpu().double()[..., 2]
                    assert bool((nz[:, 0].abs() <= 2 * ndc_ref.e[:, 0, 2]).all()) and bool(((nz[:, -1] - 1).abs() <= 2 * ndc_ref.e[:, -1, 2]).all())
    record_err(f"raygen_f64:{geometry}:{ref_hw}", worst, tol=1.0)
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------ raygen: entry forms, jitter rows, train extras
def _all_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_raygen_first_pixel_form_equals_pixel_list_form():
    """Row-major ids first_pixel + n and the same pixels as xs / ys: bit-identical outputs.  first_pixel = 2^32 + 5 on a 70001 x 70001 target takes the 64-bit
    division (the plain entry reads no image)."""
    from mvsnerf_amd import ops
    cd = _cam_dev(R.camera_case("rig", (64, 96)))
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for H, W, first, N, S, pad, lindisp, jitter in ((64, 96, 0, 257, 3, 0, False, False), (64, 96, 95, 128, 2, 4, True, True), (64, 96, 64 * 96 - 4, 4, 64, 4, False, True),
                                                       (70001, 70001, 2 ** 32 + 5, 300, 3, 0, False, False), (70001, 70001, 2 ** 32 - 150, 300, 2, 4, True, True)):
            t_rand = torch.rand((N, S), generator=g).to(DEV) if jitter else None
            kw = dict(pad=pad, lindisp=lindisp, t_rand=t_rand, ref_hw=(64, 96))
            a = ops.raygen(H, W, cd["Kt"], cd["c2w"], cd["Kr"], cd["w2c"], cd["nf"], cd["nf"], S, first_pixel=first, n_rays=N, **kw)
            p = first + torch.arange(N, dtype=torch.int64)
            assert torch.equal(a[4].cpu(), torch.stack([(p // W).float(), (p % W).float()])), (H, first)
            b = ops.raygen(H, W, cd["Kt"], cd["c2w"], cd["Kr"], cd["w2c"], cd["nf"], cd["nf"], S, xs=a[4][1].contiguous(), ys=a[4][0].contiguous(), **kw)
            assert _all_equal(a, b), (H, first)


@pytest.mark.parametrize("near,far", NEAR_FAR)
def test_raygen_jitter_rows_of_zeros_and_of_almost_ones(near, far):
    """t_rand = 0 and t_rand = 1 - 2^-24 in every sample: depths non-decreasing along the ray and inside [near, far]; t_rand = 0 gives z_0 = near exactly."""
    from mvsnerf_amd import ops
    cd = _cam_dev(R.camera_case("rig", (64, 96)))
    nf = torch.tensor([near, far], device=DEV)
    with torch.no_grad():
        for S in (1, 2, 3, 64, 128):
            for tr in (0.0, 1.0 - 2.0 ** -24):
                z = ops.raygen(64, 96, cd["Kt"], cd["c2w"], cd["Kr"], cd["w2c"], nf, cd["nf"], S, first_pixel=0, n_rays=5, t_rand=torch.full((5, S), tr, device=DEV))[3]
                assert bool((z[:, 1:] >= z[:, :-1]).all()), (S, tr)
                assert bool((z >= nf[0]).all()) and bool((z <= nf[1]).all()), (S, tr, float(z.min()), float(z.max()))
                if tr == 0.0:
                    assert bool((z[:, 0] == nf[0]).all())


def test_raygen_train_gathers_and_depth_modes():
    """depth_mode 0: colours and ground-truth depth bit-exact (the four corner pixels among them); 1: near = d - 0.1f, far = d + 0.1f; 2: S == 1, z from z_map."""
    from mvsnerf_amd import ops
    cam = R.camera_case("rig", (64, 96))
    cd = _cam_dev(cam)
    H, W, N, S = 64, 96, 37, 5
    g = torch.Generator().manual_seed(11)
    img = torch.rand((3, H, W), generator=g).to(DEV)
    depth = (torch.rand((H, W), generator=g) * 2 + 2).to(DEV)
    zmap = (torch.rand((H, W), generator=g) * 2 + 2).to(DEV)
    xs, ys = R.pixel_ids(cam, N)
    assert [(int(x), int(y)) for x, y in zip(xs[:4], ys[:4])] == [(W - 1, H - 1), (0, 0), (W - 1, 0), (0, H - 1)]
    xl, yl = xs.long().to(DEV), ys.long().to(DEV)
    args = (H, W, cd["Kt"], cd["c2w"], cd["Kr"], cd["w2c"], cd["nf"], cd["nf"], S, xs.to(DEV), ys.to(DEV))
    with torch.no_grad():
        plain = ops.raygen(H, W, cd["Kt"], cd["c2w"], cd["Kr"], cd["w2c"], cd["nf"], cd["nf"], S, xs=xs.to(DEV), ys=ys.to(DEV))
        out0 = ops.raygen_train(*args, None, img, depth_map=depth, depth_mode=0)
        assert _all_equal(out0[:5], plain)
        assert torch.equal(out0[5], img[:, yl, xl].t()) and torch.equal(out0[6], depth[yl, xl])
        assert ops.raygen_train(*args, None, img, depth_mode=0)[6] is None
        out1 = ops.raygen_train(*args, None, img, depth_map=depth, depth_mode=1)
        d = depth[yl, xl]
        assert torch.equal(out1[3][:, 0], d - 0.1) and torch.equal(out1[3][:, -1], d + 0.1)
        assert bool((out1[3][:, 1:] >= out1[3][:, :-1]).all()) and torch.equal(out1[5], out0[5]) and torch.equal(out1[6], d)
        out2 = ops.raygen_train(*args, None, img, depth_map=depth, z_map=zmap, depth_mode=2)
        assert out2[3].shape == (N, 1) and torch.equal(out2[3][:, 0], zmap[yl, xl]) and out2[0].shape == (N, 1, 3)
        o = cd["c2w"][:3, 3].reshape(1, 3).contiguous()
        pts2, ndc2 = ops.ray_points(o, out2[1], out2[3], cd["w2c"], cd["Kr"], cd["nf"], ref_hw=(H, W))
        assert torch.equal(pts2, out2[0]) and torch.equal(ndc2, out2[2])


# ------------------------------------------------------------------------------------------------------------------ the two entry points against each other
@pytest.mark.parametrize("geometry", R.GEOMETRIES)
def test_ray_points_reproduces_raygen_bit_for_bit(geometry):
    """ops.ray_points on raygen's own (o, dirs, z) returns raygen's pts and ndc in every bit: both kernels form o + d z and the NDC chain the same way."""
    from mvsnerf_amd import ops
    g = torch.Generator().manual_seed(13)
    with torch.no_grad():
        for ref_hw in R.REF_HW:
            cam = R.camera_case(geometry, ref_hw)
            cd = _cam_dev(cam)
            o = cd["c2w"][:3, 3].reshape(1, 3).contiguous()
            for i, N, S, pad, lindisp, jitter in _variants():
                xs, ys = R.pixel_ids(cam, N)
                t_rand = torch.rand((N, S), generator=g).to(DEV) if jitter else None
                pts, dirs, ndc, z, _ = ops.raygen(cam["H"], cam["W"], cd["Kt"], cd["c2w"], cd["Kr"], cd["w2c"], cd["nf"], cd["nf"], S, pad=pad, lindisp=lindisp,
                                                  xs=xs.to(DEV), ys=ys.to(DEV), t_rand=t_rand, ref_hw=ref_hw)
                p2, n2 = ops.ray_points(o, dirs, z, cd["w2c"], cd["Kr"], cd["nf"], ref_hw=ref_hw, pad=pad, lindisp=lindisp)
                dp, dn = int((p2 != pts).sum()), int((n2 != ndc).sum())
                assert dp == 0 and dn == 0, (ref_hw, N, S, pad, lindisp, dp, dn, pts.numel())


def _ulp_distance(a, b):
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs()


@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("near,far", NEAR_FAR)
def test_raygen_depths_equal_eager_torch(near, far, lindisp):
    """raygen's coarse depths are those of eager torch on the device - near (1 - t) + far t (or the lindisp form) with every operation rounded, t =
    torch.linspace(0, 1, S) - which is what train.ray_marcher and the depth-forming ray_points kernel (coarse_depth) give: a frame rendered from pixels and
    one rendered from explicit rays march the same depths.  The stratified jitter lower + (upper - lower) t_rand is held to the same arithmetic."""
    from mvsnerf_amd import ops
    cd = _cam_dev(R.camera_case("rig", (64, 96)))
    nf = torch.tensor([near, far], device=DEV)
    g = torch.Generator().manual_seed(17)
    bad = []
    with torch.no_grad():
        for S in (1, 2, 3, 64, 128):
            want = R.coarse_depths32(nf[0], nf[1], S, lindisp).expand(5, S)
            z = ops.raygen(64, 96, cd["Kt"], cd["c2w"], cd["Kr"], cd["w2c"], nf, cd["nf"], S, lindisp=lindisp, first_pixel=7, n_rays=5)[3]
            checks = [("plain", z, want)]
            if S > 1:
                t_rand = torch.rand((5, S), generator=g).to(DEV)
                mid = 0.5 * (want[:, :-1] + want[:, 1:])
                upper, lower = torch.cat([mid, want[:, -1:]], -1), torch.cat([want[:, :1], mid], -1)
                zj = ops.raygen(64, 96, cd["Kt"], cd["c2w"], cd["Kr"], cd["w2c"], nf, cd["nf"], S, lindisp=lindisp, first_pixel=7, n_rays=5, t_rand=t_rand)[3]
                checks.append(("jitter", zj, lower + (upper - lower) * t_rand))
            for tag, got, ref in checks:
                dist = _ulp_distance(got, ref)
                share = float((dist > 0).float().mean())
                print(f"raygen depths near={near} far={far} lindisp={lindisp} S={S} {tag}: {share:.3f} of the depths differ from eager torch, by at most {int(dist.max())} ulp")
                if not torch.equal(got, ref):
                    bad.append((S, tag, share, int(dist.max())))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ positional encoding
@pytest.mark.parametrize("d", R.PE_D)
def test_posenc_layout_and_values_vs_float64(d):
    """[x | sin(x 2^f), f-major | cos(x 2^f)] with x copied bit for bit, values against float64 sin / cos of the exact fp32 argument x 2^f.  The allowance is
    measured in the test: the largest error of torch.sin / torch.cos on the device for the same arguments, plus 1 u.  Measured on an MI355X: allowance 2.01 u
    (d = 1), 2.12 u (d = 3), 2.13 u (d = 4); the kernel's own error 1.01 / 1.12 / 1.13 u (it calls the same sinf / cosf)."""
    from mvsnerf_amd import ops
    worst = allow_max = 0.0
    with torch.no_grad():
        for P in R.PE_P:
            x = R.posenc_inputs(P, d)
            xd = x.to(DEV)
            for L in R.PE_L:
                ref, a = R.posenc_ref64(x, L)
                out = ops.posenc(xd, L)
                assert out.shape == (P, d * (1 + 2 * L))
                assert torch.equal(out[:, :d], xd)
                if L == 0:
                    continue
                ad, refd = a.to(DEV), ref.to(DEV)
                e_torch = max(float((torch.sin(ad).double() - refd[:, d:d + d * L]).abs().max()), float((torch.cos(ad).double() - refd[:, d + d * L:]).abs().max()))
                allow = e_torch + U
                err = float((out.double() - refd).abs().max())
                worst, allow_max = max(worst, err), max(allow_max, allow)
                assert err <= allow, (P, L, err, allow)
    print(f"posenc d={d}: kernel error {worst / U:.3f} u, allowance (torch.sin / cos on the device + 1 u) {allow_max / U:.3f} u")
    record_err(f"posenc_f64:{d}", worst, tol=allow_max)
