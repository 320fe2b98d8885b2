"""Float64 references, input families and error bounds of the edge-case tests for the kernels between the volume and the MLP
(test_gpu_lookup_edges.py, test_gpu_composite_f64.py; test_edge_refs.py runs every reference and every input condition without a GPU,
against torch's fp32 emulation of the same operation).

Notation: u = 2^-24.  The "fp32 chain" is the kernels' un-normalisation ((n*2 - 1 + 1)/2) * (size - 1) with floor, the weights (x1 - ix) /
(ix - x0) and w = (wx*wy)*wz, evaluated with torch float32 on the CPU: IEEE operations with nothing to contract, so these are the values
the kernels form.  Everything here is CPU-only and deterministic (seeded CPU generators)."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24

# ------------------------------------------------------------------------------------------------------------------ trilinear lookup
VOLUMES = [(1, 1, 2), (1, 5, 9), (5, 1, 9), (5, 9, 1), (2, 2, 2), (5, 9, 17), (9, 17, 33), (7, 12, 28)]       # (D, H, W)
P_LIST = (1, 3, 63, 64, 65, 1021)
P_POOL = 1021
C_POOL = 40
EDGE_VALUES = (-1 / 2, -1 / 64, 0.0, 1 / 64, 1 / 2, 63 / 64, 1.0, 65 / 64, 3 / 2)


def is_dyadic_volume(dims):
    """size - 1 is 0 or a power of two on every axis: the fp32 chain is exact for ndc = k/64."""
    return all(((n - 1) & (n - 2)) == 0 or n == 1 for n in dims)


def make_volume(dims, seed=0, C=C_POOL):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn((*dims, C), generator=g)


def dyadic_pool(seed=0):
    """P_POOL samples ndc = k/64, k in [-32, 96]: the full product of EDGE_VALUES over the three axes (729) and random k for the rest, shuffled so
    that every prefix of the pool mixes inside, border and outside samples."""
    g = torch.Generator().manual_seed(2000 + seed)
    e = torch.tensor(EDGE_VALUES, dtype=torch.float32)
    prod = torch.cartesian_prod(e, e, e)
    rest = torch.randint(-32, 97, (P_POOL - prod.shape[0], 3), generator=g).to(torch.float32) / 64.0
    pool = torch.cat([prod, rest])
    return pool[torch.randperm(P_POOL, generator=g)].contiguous()


def random_pool(seed=0):
    g = torch.Generator().manual_seed(3000 + seed)
    return (torch.rand((P_POOL, 3), generator=g) * 1.3 - 0.15).contiguous()


def chain(n, size, dtype=torch.float32):
    n = n.to(dtype)
    return ((n * 2.0 - 1.0 + 1.0) / 2.0) * float(size - 1)


def chain_is_exact(ndc, dims):
    D, H, W = dims
    return all(torch.equal(chain(ndc[:, k], n).double(), chain(ndc[:, k], n, torch.float64)) for k, n in ((0, W), (1, H), (2, D)))


def corners(ndc, dims):
    """The eight corners in the kernels' order k = 4 zc + 2 yc + xc: (fp32 weight (P,), in-range (P,) bool, voxel index (P,), clamped where out)."""
    D, H, W = dims
    ndc = ndc.reshape(-1, 3).to(torch.float32)
    ix, iy, iz = chain(ndc[:, 0], W), chain(ndc[:, 1], H), chain(ndc[:, 2], D)
    fx, fy, fz = ix.floor(), iy.floor(), iz.floor()
    out = []
    for zc in (0, 1):
        for yc in (0, 1):
            for xc in (0, 1):
                cx, cy, cz = fx + xc, fy + yc, fz + zc
                ok = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1) & (cz >= 0) & (cz <= D - 1)
                wx = (ix - fx) if xc else ((fx + 1.0) - ix)
                wy = (iy - fy) if yc else ((fy + 1.0) - iy)
                wz = (iz - fz) if zc else ((fz + 1.0) - iz)
                idx = (cz.long().clamp(0, D - 1) * H + cy.long().clamp(0, H - 1)) * W + cx.long().clamp(0, W - 1)
                out.append(((wx * wy) * wz, ok, idx))
    return out


def lookup_ref(vol, ndc):
    """vol (D,H,W,C) fp32, ndc (P,3) fp32 -> (ref, S) float64 (P,C): sum of (fp32-chain weight) x value over the in-range corners, and the same sum of
    |value| |weight|."""
    dims, C = tuple(vol.shape[:3]), vol.shape[3]
    v = vol.reshape(-1, C).double()
    P = ndc.reshape(-1, 3).shape[0]
    ref, S = torch.zeros((P, C), dtype=torch.float64), torch.zeros((P, C), dtype=torch.float64)
    for w, ok, idx in corners(ndc, dims):
        t = v[idx] * (w.double() * ok.double())[:, None]
        ref += t
        S += t.abs()
    return ref, S


def lookup_emul32(vol, ndc):
    """The kernels' fold in torch fp32: every product rounded, corners added in the order k = 0..7 from 0, out-of-range corners skipped."""
    dims, C = tuple(vol.shape[:3]), vol.shape[3]
    v = vol.reshape(-1, C)
    acc = torch.zeros((ndc.reshape(-1, 3).shape[0], C), dtype=torch.float32)
    for w, ok, idx in corners(ndc, dims):
        acc = torch.where(ok[:, None], acc + v[idx] * w[:, None], acc)
    return acc


def lookup_gs64(vol, ndc):
    """The independent reference: ATen's float64 grid_sample on the CPU, zeros padding, align_corners."""
    P = ndc.reshape(-1, 3).shape[0]
    g = (ndc.reshape(-1, 3).double() * 2 - 1).view(1, 1, 1, P, 3)
    o = F.grid_sample(vol.permute(3, 0, 1, 2)[None].double(), g, mode="bilinear", padding_mode="zeros", align_corners=True)
    return o[0, :, 0, 0].t().contiguous()


def lookup_hard_bound(S):
    return 9 * U * S + 1e-30                 # eight rounded products and eight additions


def lookup_coord_slack(vol):
    """2 M delta: Lipschitz bound for the roundings of the fp32 coordinates, M = max |vol|, delta = 12 u ((W-1) + (H-1) + (D-1))."""
    D, H, W = vol.shape[:3]
    return 2 * float(vol.abs().max()) * 12 * U * ((W - 1) + (H - 1) + (D - 1))


def hwdc_view(vol_dhwc):
    """The same logical (D,H,W,C) tensor on depth-fastest memory vol[y][x][d][c]."""
    return vol_dhwc.permute(1, 2, 0, 3).contiguous().permute(2, 0, 1, 3)


# ------------------------------------------------------------------------------------------------------------------ colour lookup
def project64(pts, w2c, K, W, H):
    """float64 projection of world points (P,3) into one view: (grid (P,2) in [-1,1] units as grid_sample takes it, camera z (P,), pixel (P,2))."""
    p, M, K = pts.double(), w2c.double(), K.double()
    cam = p @ M[:3, :3].t() + M[:3, 3]
    q = cam @ K.t()
    pix = q[:, :2] / q[:, 2:]
    n = pix / torch.tensor([W - 1, H - 1], dtype=torch.float64)
    return n * 2.0 - 1.0, cam[:, 2], pix


def project32(pts, w2c, K, W, H):
    """The same projection in the kernels' fp32 arithmetic (the CPU oracle's fma chains): grid (P,2)."""
    from oracle import mvsnerf_oracle as O
    n = O.get_ndc_coordinate(w2c, K, pts.reshape(-1, 1, 3), torch.tensor([W - 1, H - 1], dtype=torch.float32))
    return n.reshape(-1, 3)[:, :2] * 2.0 - 1.0


def delta_pix(pts, w2c, K, W, H):
    """Bound (P,) on the fp32 error of a sample's pixel coordinates, |d ix| + |d iy|, from color_project's operation count (first order, x 1.01):
    camera coordinate c = fma(z, m2, fma(y, m1, x m0)) + m3: four roundings of partial sums <= A_c = sum |terms|      -> e_c <= 4 u A_c
    q_r = fma(cz, k2, fma(cy, k1, cx k0)): the inherited errors and three roundings                               -> E_r <= sum |k_j| e_j + 3 u sum |k_j c_j|
    pix = q_r / q_z                                                                                                -> (E_r + |pix| E_z) / |q_z| + u |pix|
    / (W-1), * 2 - 1, + 1, / 2, * (W-1): four more roundings of values below |pix| + (W-1)/2 in pixel units          -> 4 u (|pix| + W)."""
    p, M, Kd = pts.double(), w2c.double(), K.double()
    A = p.abs() @ M[:3, :3].abs().t() + M[:3, 3].abs()
    cam = p @ M[:3, :3].t() + M[:3, 3]
    e = 4 * U * A
    E = e @ Kd.abs().t() + 3 * U * (cam.abs() @ Kd.abs().t())
    q = cam @ Kd.t()
    pix = q[:, :2] / q[:, 2:]
    size = torch.tensor([W, H], dtype=torch.float64)
    d = (E[:, :2] + pix.abs() * E[:, 2:]) / q[:, 2:].abs() + U * pix.abs() + 4 * U * (pix.abs() + size)
    return 1.01 * d.sum(-1)


def color_ref64(imgs, w2cs, Ks, pts, feats=None):
    """float64 border-padded bilinear colours (and zero-padded feature channels at their own resolution) of every view.
    imgs (V,3,H,W); pts (P,3) -> dict of col (P,V,3), col_S (P,V,3) = sum |tap| weight, mask (P,V), grid (P,V,2), camz (P,V), dpix (P,V) [, feat (P,V,Cf), feat_S]."""
    V, _, H, W = imgs.shape
    P = pts.shape[0]
    out = {k: [] for k in ("col", "col_S", "mask", "grid", "camz", "dpix", "feat", "feat_S")}
    for v in range(V):
        grid, camz, _ = project64(pts, w2cs[v], Ks[v], W, H)
        g4 = grid.view(1, 1, P, 2)
        smp = lambda img, pad: F.grid_sample(img[None].double(), g4, mode="bilinear", padding_mode=pad, align_corners=True)[0, :, 0].t()
        out["col"].append(smp(imgs[v], "border"))
        out["col_S"].append(smp(imgs[v].abs(), "border"))
        out["mask"].append(((grid > -1.0) & (grid < 1.0)).all(-1).double())
        out["grid"].append(grid)
        out["camz"].append(camz)
        out["dpix"].append(delta_pix(pts, w2cs[v], Ks[v], W, H))
        if feats is not None:
            out["feat"].append(smp(feats[v], "zeros"))
            out["feat_S"].append(smp(feats[v].abs(), "zeros"))
    return {k: torch.stack(v, 1) for k, v in out.items() if v}


def exact_geometry_case(V, seed=0):
    """Identity w2c, K = [[f,0,cx],[0,f,cy],[0,0,1]] with f a power of two and integer cx, cy, 9 x 17 images (H-1, W-1 powers of two), 5 x 9 feature maps;
    points with z in {1, 2, 4} and dyadic x, y whose pixels in view 0 are the product of
        px: pixel centres, half pixels, the last column 16 (g = +1, the +1 taps must not be read), one dyadic step inside it, column 0 (g = -1) and one step
            inside, and columns outside the image on both sides
        py: the same for the rows (last row 8).
    Every fma and division of the projection is then exact in fp32 (asserted by the tests: project32 == project64)."""
    g = torch.Generator().manual_seed(4000 + seed)
    H, W = 9, 17
    f = [8.0, 16.0, 4.0, 8.0, 2.0, 32.0][:V]
    cx = [8.0, 3.0, 12.0, 8.0, 0.0, 16.0][:V]
    cy = [4.0, 2.0, 7.0, 8.0, 4.0, 0.0][:V]
    Ks = torch.tensor([[[f[v], 0, cx[v]], [0, f[v], cy[v]], [0, 0, 1]] for v in range(V)], dtype=torch.float32)
    w2cs = torch.eye(4).repeat(V, 1, 1)
    px = torch.tensor([0.0, 1 / 64, 0.5, 1.0, 7.25, 15.5, 16 - 1 / 64, 16.0, -1.0, -0.5, 17.5, 20.0])
    py = torch.tensor([0.0, 1 / 64, 3.5, 8 - 1 / 64, 8.0, 8.25, -2.0, 11.0])
    zs = torch.tensor([1.0, 2.0, 4.0])
    grid = torch.cartesian_prod(px, py, zs)
    pts = torch.stack([(grid[:, 0] - 8.0) * grid[:, 2] / 8.0, (grid[:, 1] - 4.0) * grid[:, 2] / 8.0, grid[:, 2]], -1)
    pts = pts[torch.randperm(pts.shape[0], generator=g)].contiguous()
    imgs = torch.randn((V, 3, H, W), generator=g)
    feats = torch.randn((V, 2, 5, 9), generator=g)
    return imgs, feats, w2cs, Ks, pts


RIG_SEED = 7          # chosen so that the reference leaves <= 1 % of the samples within 1e-5 of |g| = 1 (test_edge_refs.py asserts it)


def rig_case():
    """make_rig(64, 96) (four rotated views), (N, S) = (37, 5) points in front of every camera, a part of them outside some image."""
    from mvsnerf_amd.synth import make_rig, pose_ref_of
    rig = make_rig(64, 96, seed=RIG_SEED, rot_deg=2.0)
    pose = pose_ref_of(rig)
    g = torch.Generator().manual_seed(5000 + RIG_SEED)
    r = torch.rand((37, 5, 3), generator=g)
    pts = torch.stack([r[..., 0] * 2.4 - 1.2, r[..., 1] * 1.8 - 0.9, r[..., 2] * 3.0 + 1.5], -1).contiguous()
    return rig["images_raw"][0, :, :3].contiguous(), pose["w2cs"].contiguous(), pose["intrinsics"].contiguous(), pts


def oracle_colors(imgs, w2cs, Ks, pts, feats=None):
    """The fp32 CPU oracle's build_color_volume: (P, V, 3 [+ Cf] + 1)."""
    from oracle import mvsnerf_oracle as O
    V = imgs.shape[0]
    o = O.build_color_volume(pts.reshape(-1, 1, 3), {"w2cs": w2cs, "intrinsics": Ks}, imgs[None], with_mask=True, img_feat=None if feats is None else feats[None])
    return o.reshape(pts.reshape(-1, 3).shape[0], V, -1)


def near_mask_edge(grid):
    """(P,V) bool: |g| within 1e-5 of 1 on either axis - left out of the mask comparison of the general rig."""
    return ((grid.abs() - 1.0).abs() < 1e-5).any(-1)


# ------------------------------------------------------------------------------------------------------------------ direction feature
def dir_cases(seed=0):
    g = torch.Generator().manual_seed(6000 + seed)
    eye = torch.eye(3)
    small = torch.tensor([[2.0, 1.0, 2.0]]) / 3.0 * 2.0 ** -20           # ||d|| = 2^-20
    return torch.cat([eye, -eye, 3.0 * eye, small, torch.randn((54, 3), generator=g)]).contiguous()     # 64 directions, none zero


def dir_ref64(d, R=None, normalize=True):
    """-> (ref (n,3), bound (n,3)) in float64.  Operation count of dir_feature_of: the norm carries 2.5 u (three roundings under the square root, one
    of it), the division one more, the rotation's three-term chain 3 u of sum_j |R_ij| |u_j|: below 8 u sum_j |R_ij| |d_j| / ||d||."""
    d = d.double()
    n = d.norm(dim=-1, keepdim=True) if normalize else torch.ones((d.shape[0], 1), dtype=torch.float64)
    un = d / n
    if R is None:
        return un, 8 * U * un.abs()
    R = R.double()[:3, :3]
    return un @ R.t(), 8 * U * (un.abs() @ R.abs().t())


def dir_emul32(d, R=None, normalize=True):
    n = d.norm(dim=-1, keepdim=True) if normalize else torch.ones((d.shape[0], 1))
    un = d / n
    return un if R is None else un @ R[:3, :3].t()


# ------------------------------------------------------------------------------------------------------------------ trilinear scatter
def scatter_ref(ndc, g, dims):
    """Exact scatter of the kernels' own fp32 contributions g * ((wx*wy)*wz) (fp32 chain on the CPU), accumulated in float64.
    ndc (P,3), g (P,C) fp32 -> ref (D,H,W,C), Sabs (D,H,W,C) = sum |contribution|, n_v (D,H,W,1) = number of non-zero-weight contributions per voxel."""
    D, H, W = dims
    C = g.shape[1]
    ref = torch.zeros((D * H * W, C), dtype=torch.float64)
    sabs = torch.zeros_like(ref)
    nv = torch.zeros((D * H * W,), dtype=torch.float64)
    for w, ok, idx in corners(ndc, dims):
        c = (g * w[:, None])[ok].double()
        ref.index_add_(0, idx[ok], c)
        sabs.index_add_(0, idx[ok], c.abs())
        nv.index_add_(0, idx[ok], (w[ok] != 0).double())
    return ref.view(D, H, W, C), sabs.view(D, H, W, C), nv.view(D, H, W, 1)


def scatter_emul32(ndc, g, dims):
    """The float-atomic scatter in one (sequential) order, fp32 accumulation."""
    D, H, W = dims
    out = torch.zeros((D * H * W, g.shape[1]), dtype=torch.float32)
    for w, ok, idx in corners(ndc, dims):
        out.index_add_(0, idx[ok], (g * w[:, None])[ok])
    return out.view(D, H, W, -1)


def scatter_atomic_bound(sabs, nv):
    return (nv + 2) * U * sabs


def scatter_det_bound(sabs, nv, g):
    e = math.frexp(float(g.abs().max()))[1]            # max |g| < 2^e
    return 2 * U * sabs + nv * 2.0 ** (e - 40)


RAY_DIMS = (9, 17, 33)
RAY_SHAPES = ((16, 16), (5, 7), (1, 1), (33, 3))
RAY_STEPS = (1.0, 0.5, 2.0)


def ray_ordered_ndc(N, S, step, dims=RAY_DIMS):
    """N rays x S samples in ray order on a volume with power-of-two size - 1 (all coordinates dyadic: the fp32 chain is exact).  A ray keeps one (x, y)
    inside a cell and advances z by `step` planes per sample.  Rays 2k and 2k+1 share the cell; ray 2k ends on fz = -1 (it enters from z < 0: only its z1
    corners are inside) and ray 2k+1 continues the same depth sequence, leaving through z = D - 1, so the hand-off of volume_sample_c8_bwd_kernel also crosses a ray
    boundary (where |ndc| <= 2 allows it; the longest rays with step 2 all start at -15.75 instead).  Pair k % 4 == 1 walks the x = W - 1 column (ix = W - 1
    exactly: the x1 lanes are dead), k % 4 == 2 has fy = -1 (iy = -0.5), k % 4 == 3 has fy = H - 1 (iy = H - 1 exactly)."""
    D, H, W = dims
    rows = []
    for r in range(N):
        k = r // 2
        ix = float((3 + 5 * k) % (W - 2)) + 0.25
        iy = float((2 + 3 * k) % (H - 2)) + 0.75
        if k % 4 == 1:
            ix = float(W - 1)
        elif k % 4 == 2:
            iy = -0.5
        elif k % 4 == 3:
            iy = float(H - 1)
        z0 = max(-0.75 - step * (S - 1), -15.75)
        if r % 2 == 1 and z0 + step * S + step * (S - 1) <= 15.75:
            z0 = z0 + step * S
        for s in range(S):
            rows.append((ix / (W - 1), iy / (H - 1), (z0 + step * s) / (D - 1)))
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32).contiguous()


def collision_case(W=4100, first_fx=4097):
    """Eight samples that alternate (fy = 0, fx = first_fx, fz = 0) and (fy = 1, fx = 1, fz = 1) on a (3, 3, W) volume, fractional parts ~1/4.  With
    W = 4100 and first_fx = 4097 the two cells have equal keys fy * 4096 + cx (both x corners), and the second sample lies one depth plane further."""
    dims = (3, 3, W)
    a = (float(first_fx) + 0.25, 0.25, 0.25)
    b = (1.25, 1.25, 1.25)
    rows = [[c[0] / (W - 1), c[1] / 2.0, c[2] / 2.0] for c in (a, b) * 4]
    return dims, torch.tensor(rows, dtype=torch.float64).to(torch.float32).contiguous()


def cell_of(ndc, dims):
    """(fx, fy, fz) of the fp32 chain, as integer tensors."""
    D, H, W = dims
    return tuple(chain(ndc[:, k], n).floor().long() for k, n in ((0, W), (1, H), (2, D)))


# ------------------------------------------------------------------------------------------------------------------ compositing
S_LIST = (1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 300)          # CHUNK 1, 2, 3, 4 and the run-time path, each with a full and a ragged last lane
FAMILIES = ("small", "mixed", "dense", "sparse")


def composite_inputs(family, N, S, seed=0, special_rays=True):
    """raw (N,S,4) (randn colours, sigma >= 0 of the family), z (N,S) sorted.  special_rays (N >= 5): ray 1 has all-zero densities, ray 3 a saturating first sample."""
    g = torch.Generator().manual_seed(7000 + 131 * S + 17 * N + seed + 1000 * FAMILIES.index(family))
    r = torch.rand((N, S), generator=g)
    pick = torch.rand((N, S), generator=g)
    if family == "small":
        sig = r * 0.05
    elif family == "mixed":
        sig = torch.where(pick < 0.1, r * 30.0, r)
    elif family == "dense":
        sig = r * 40.0
    else:
        sig = torch.where(pick < 0.7, torch.zeros_like(r), r)
    if special_rays and N >= 5:
        sig[1] = 0.0
        sig[3, 0] = 100.0
    raw = torch.cat([torch.randn((N, S, 3), generator=g), sig[..., None]], -1).contiguous()
    z = torch.sort(torch.rand((N, S), generator=g) + 2.0, -1)[0].contiguous()
    return raw, z


def zero_ray_inputs(S, seed=0):
    raw, z = composite_inputs("small", 1, S, seed, special_rays=False)
    raw[..., 3] = 0.0
    return raw, z


def saturated_ray_inputs(S, seed=0):
    raw, z = composite_inputs("small", 1, S, seed + 1, special_rays=False)
    raw[0, 0, 3] = 100.0
    return raw, z


def composite_forward(raw, z, white_bkgd=False):
    """raw2alpha / raw2outputs (renderer.py:18-26, 65-92) in the dtype of `raw`, the +1e-10 included: rgb, disp, acc, weights, depth, alpha, T."""
    sig = raw[..., 3]
    alpha = 1.0 - torch.exp(-sig)
    t = 1.0 - alpha + 1e-10
    T = torch.cumprod(torch.cat([torch.ones_like(t[:, :1]), t], -1), -1)[:, :-1]
    w = alpha * T
    rgb = torch.sum(w[..., None] * raw[..., :3], -2)
    depth = torch.sum(w * z, -1)
    acc = torch.sum(w, -1)
    disp = 1.0 / torch.max(1e-10 * torch.ones_like(depth), depth / acc)
    if white_bkgd:
        rgb = rgb + (1.0 - acc[..., None])
    return rgb, disp, acc, w, depth, alpha, T


def composite_ref64(raw, z, white_bkgd=False):
    """float64 forward on the fp32 inputs and the bounds of every output (dict of (value, bound) pairs; disp's bound is relative, for rays with acc > 1e-3):
        alpha 4 u;  B_T,i = 4 u T_i sum_{j<i} 1/t_j + (i + 8) u T_i;  weights a_i B_T,i + 4 u T_i + u w_i + 1e-30;
        rgb / depth / acc  sum_i B_w,i |c_i| + (ceil(S/64) + 8) u sum_i w_i |c_i|  (c = 1 for acc; white_bkgd adds the acc bound + u to rgb);
        disp 4 u + B_depth / depth + B_acc / acc."""
    r, zz = raw.double(), z.double()
    rgb, disp, acc, w, depth, alpha, T = composite_forward(r, zz, white_bkgd)
    S = r.shape[1]
    t = 1.0 - alpha + 1e-10
    inv = 1.0 / t
    excl = torch.cumsum(inv, -1) - inv
    i = torch.arange(S, dtype=torch.float64)
    BT = 4 * U * T * excl + (i + 8) * U * T
    Bw = alpha * BT + 4 * U * T + U * w + 1e-30
    red = (math.ceil(S / 64) + 8) * U
    c = r[..., :3].abs()
    Bacc = Bw.sum(-1) + red * w.sum(-1)
    Bdepth = (Bw * zz.abs()).sum(-1) + red * (w * zz.abs()).sum(-1)
    Brgb = (Bw[..., None] * c).sum(-2) + red * (w[..., None] * c).sum(-2)
    if white_bkgd:
        Brgb = Brgb + Bacc[..., None] + U
    with torch.no_grad():
        Bdisp = 4 * U + Bdepth / depth + Bacc / acc
    return {"rgb": (rgb, Brgb), "disp": (disp, Bdisp), "acc": (acc, Bacc), "weights": (w, Bw), "depth": (depth, Bdepth),
            "alpha": (alpha, torch.full_like(alpha, 4 * U)), "T": (T, BT)}


def composite_shares(outs, ref):
    """Largest |out - ref| / bound per output name; outs = (rgb, disp, acc, weights, depth, alpha) as ops.composite returns them (CPU tensors).
    disp is compared relatively and on rays with acc > 1e-3 only."""
    shares = {}
    for name, o in zip(("rgb", "disp", "acc", "weights", "depth", "alpha"), outs):
        v, b = ref[name]
        if name == "disp":
            sel = ref["acc"][0] > 1e-3
            shares[name] = float(((o.double() - v).abs() / v / b)[sel].max()) if bool(sel.any()) else 0.0
        else:
            shares[name] = float(((o.double() - v).abs() / b).max())
    return shares


GRAD_NAMES = ("g_rgb", "g_depth", "g_acc", "g_weights", "g_alpha")
GRAD_COMBOS = tuple((n,) for n in GRAD_NAMES) + (GRAD_NAMES,)


def composite_grads(N, S, seed=0):
    g = torch.Generator().manual_seed(8000 + 7 * S + seed)
    return {"g_rgb": torch.randn((N, 3), generator=g), "g_depth": torch.randn((N,), generator=g), "g_acc": torch.randn((N,), generator=g),
            "g_weights": torch.randn((N, S), generator=g), "g_alpha": torch.randn((N, S), generator=g)}


def composite_autograd(raw, z, white_bkgd, grads, dtype):
    """d loss / d raw (N,S,4) by torch autograd of composite_forward in `dtype` on the CPU; grads: the subset of GRAD_NAMES that flows in."""
    r = raw.to(dtype).clone().requires_grad_(True)
    rgb, _, acc, w, depth, alpha, _ = composite_forward(r, z.to(dtype), white_bkgd)
    terms = {"g_rgb": rgb, "g_depth": depth, "g_acc": acc, "g_weights": w, "g_alpha": alpha}
    loss = sum((terms[k] * v.to(dtype)).sum() for k, v in grads.items())
    loss.backward()
    return r.grad


def composite_bwd_scale(raw, z, white_bkgd, grads):
    """Per ray R = sum_j |G_j| w_j + max_j |G_j| T_j + max_j |g_alpha,j| in float64, G_j the total gradient reaching w_j."""
    r, zz = raw.double(), z.double()
    _, _, _, w, _, _, T = composite_forward(r, zz, white_bkgd)
    N, S = zz.shape
    z0 = torch.zeros((), dtype=torch.float64)
    g_rgb = grads["g_rgb"].double() if "g_rgb" in grads else torch.zeros((N, 3), dtype=torch.float64)
    ga = (grads["g_acc"].double() if "g_acc" in grads else z0.expand(N)) - (g_rgb.sum(-1) if white_bkgd else 0.0)
    G = (r[..., :3] * g_rgb[:, None]).sum(-1) + ga[:, None]
    if "g_depth" in grads:
        G = G + grads["g_depth"].double()[:, None] * zz
    if "g_weights" in grads:
        G = G + grads["g_weights"].double()
    R = (G.abs() * w).sum(-1) + (G.abs() * T).max(-1)[0]
    if "g_alpha" in grads:
        R = R + grads["g_alpha"].double().abs().max(-1)[0]
    return R


def composite_bwd_errors(d_raw, raw, z, white_bkgd, grads):
    """-> dict: e (N,) = max_j |d_sigma - ref| / R of `d_raw`, e_torch (N,) the same for torch fp32 CPU autograd, col = largest share of the colour
    gradients' bound (the forward's weight bound times |g_rgb|; 0 without g_rgb)."""
    ref = composite_autograd(raw, z, white_bkgd, grads, torch.float64)
    t32 = composite_autograd(raw, z, white_bkgd, grads, torch.float32)
    R = composite_bwd_scale(raw, z, white_bkgd, grads)
    e = ((d_raw.double()[..., 3] - ref[..., 3]).abs().max(-1)[0]) / R
    et = ((t32.double()[..., 3] - ref[..., 3]).abs().max(-1)[0]) / R
    Bw = composite_ref64(raw, z, white_bkgd)["weights"][1]
    if "g_rgb" in grads:
        bc = Bw[..., None] * grads["g_rgb"].double().abs()[:, None]
        col = float(((d_raw.double()[..., :3] - ref[..., :3]).abs() / (bc + 1e-300)).max())
    else:
        col = 0.0 if float(d_raw[..., :3].abs().max()) == 0.0 else float("inf")          # no colour gradient flows: exactly zero
    return {"e": e, "e_torch": et, "col": col}
