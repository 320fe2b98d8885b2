"""The yardstick of the TSDF kernels (csrc/tsdf.hip): the definition restated in numpy, node by node and view by view, on the analytic rig of
tests/depth_fusion_refs.py (the plane z = 150 and a sphere of radius 120, cameras on an arc at distance 600).

integrate(..., dtype=np.float64) is the yardstick; dtype=np.float32 runs the same statements in single precision, one rounding per operation - what the kernel
computes - so that the fp32 noise floor of the definition itself is measured on the CPU and the GPU tests take their margins from it.  Both read the SAME
fp32 cameras, depths and box.  Every intermediate is returned per (view, node).

masked_mesh is the node mask of the mesher stated as a post-filter of mesh_refs.extract; vertex_colors is the numpy statement of tsdf_vertex_colors.
"""
import numpy as np
import torch

import depth_fusion_refs as F
import mesh_refs as MR

BOX = np.array([[-160.0, -150.0, -140.0], [160.0, 150.0, 170.0]], np.float32)
TRUNC = 30.0


def corrupt(g):
    """float32 depths of a rig with holes of every kind, a valid mask and an RGBA bank with an alpha-0 region (test_gpu_depth_fusion._corrupt's recipe
    without the scaled block) -> (depths (M,H,W) fp32, valid (M,H,W) uint8, rgba (M,H,W,4) uint8)"""
    M, H, W = g["depth"].shape
    d = g["depth"].astype(np.float32)
    v = 1 % M
    for k, hole in enumerate((0.0, -1.0, np.nan, np.inf, -np.inf)):
        y, x = (3 + 4 * k) % (H - 1), (5 + 7 * k) % (W - 1)
        d[v, y:y + 2, x:x + 2] = hole
        d[(v + 2) % M, (y + 2) % H, (x + 3) % W] = hole
    valid = np.ones((M, H, W), np.uint8)
    valid[3 % M, H // 2:H // 2 + 3, W // 2 - 2:W // 2 + 4] = 0
    valid[3 % M, 1, 1] = 7                                   # any non-zero byte is valid
    alpha = np.full((M, H, W), 255, np.uint8)
    alpha[0, :H // 3, W // 2:W // 2 + W // 4] = 0
    alpha[0, H - 2, 2] = 1                                   # alpha > 0 is foreground
    return d, valid, np.concatenate([g["images"], alpha[..., None]], -1)


def node_positions(box, dims, dtype=np.float64):
    """X, Y, Z (D,H,W) `dtype`: lo + (i/(W-1), j/(H-1), k/(D-1)) * (hi - lo), mesh_refs.extract's box mapping (box is rounded to fp32 first)"""
    t = np.dtype(dtype).type
    D, H, W = dims
    b = np.asarray(box, np.float32).reshape(2, 3).astype(t)
    k, j, i = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    size = b[1] - b[0]
    return tuple(b[0, a] + (idx.astype(t) / t(n - 1)) * size[a] for a, (idx, n) in enumerate(((i, W), (j, H), (k, D))))


def integrate(depth, w2c, K, images, box, dims, trunc, valid=None, alpha=None, views=None, z_min=0.0, dtype=np.float64):
    """depth (M,H,W) fp32, w2c (M,3,4) and K (M,3,3) fp32 (what the device receives), images (M,H,W,>=3) uint8, valid / alpha (M,H,W) or None, views a list
    of view ids (integrated in ascending order) or None ->
        tsdf (D,H,W) dtype, weight (D,H,W) int32, colors (D,H,W,4) uint8, tsum, csum (D,H,W,3) int64, cw (D,H,W) int64, views (the ids used, ascending) and,
        per used view (n_views,D,H,W): qz, u, v (u + 0.5 and v + 0.5 are `up`, `vp`), front, inside, x, y, usable, sdf, hit (step 5 ran), near (step 6 ran)"""
    t = np.dtype(dtype).type
    ref = F.Reference(depth, np.zeros_like(np.asarray(w2c)), w2c, K, valid, alpha, dtype=dtype)      # its to_camera and its usable rule
    M, Hi, Wi = ref.M, ref.H, ref.W
    D, H, W = dims
    X = node_positions(box, dims, dtype)
    views = list(range(M)) if views is None else sorted(int(v) for v in views)
    tr, zm, half, one = t(trunc), t(z_min), t(0.5), t(1)
    tsum = np.zeros((D, H, W), t)
    wsum = np.zeros((D, H, W), np.int64)
    csum = np.zeros((D, H, W, 3), np.int64)
    cw = np.zeros((D, H, W), np.int64)
    rec = {k: [] for k in ("qz", "u", "v", "up", "vp", "front", "inside", "x", "y", "usable", "sdf", "hit", "near")}
    for m in views:
        with np.errstate(all="ignore"):
            q = ref.to_camera(m, X)
            front = q[2] > zm
            Km = ref.K[m]
            u, v = Km[0, 0] * q[0] / q[2] + Km[0, 2], Km[1, 1] * q[1] / q[2] + Km[1, 2]
            up, vp = u + half, v + half
            inside = front & (up >= 0) & (up < t(Wi)) & (vp >= 0) & (vp < t(Hi))
            x = np.where(inside, np.floor(np.where(inside, up, 0)), 0).astype(np.int64)
            y = np.where(inside, np.floor(np.where(inside, vp, 0)), 0).astype(np.int64)
            usable = inside & ref.usable[m][y, x]
            d = np.where(usable, ref.depth[m][y, x], t(0))
            sdf = d - q[2]
            hit = usable & (sdf >= -tr)
            near = hit & (sdf <= tr)
            tsum = tsum + np.where(hit, np.minimum(sdf / tr, one), t(0))
        wsum += hit
        csum += np.where(near[..., None], np.asarray(images)[m][y, x, :3].astype(np.int64), 0)
        cw += near
        for k, a in (("qz", q[2]), ("u", u), ("v", v), ("up", up), ("vp", vp), ("front", front), ("inside", inside), ("x", x), ("y", y), ("usable", usable),
                     ("sdf", sdf), ("hit", hit), ("near", near)):
            rec[k].append(a)
    with np.errstate(all="ignore"):
        tsdf = np.where(wsum > 0, tsum / wsum.astype(t), one)
    colors = np.zeros((D, H, W, 4), np.uint8)
    has = cw > 0
    den = np.where(has, 2 * cw, 1)
    colors[..., :3] = np.where(has[..., None], (2 * csum + cw[..., None]) // den[..., None], 0)
    colors[..., 3] = np.where(has, 255, 0)
    out = {k: np.stack(a) for k, a in rec.items()}
    out.update(tsdf=tsdf, weight=wsum.astype(np.int32), colors=colors, tsum=tsum, csum=csum, cw=cw, views=views)
    return out


def noise(o64, o32):
    """(the largest |uv32 - uv64|, the largest |z32 - z64|) over the (view, node) entries in front of the camera in both runs"""
    both = o64["front"] & o32["front"] & np.isfinite(o64["u"]) & np.isfinite(o32["u"]) & np.isfinite(o64["v"]) & np.isfinite(o32["v"])
    n_uv = max(float(np.abs(o32["u"][both] - o64["u"][both]).max()), float(np.abs(o32["v"][both] - o64["v"][both]).max())) if both.any() else 0.0
    fin = np.isfinite(o64["qz"]) & np.isfinite(o32["qz"])
    n_z = float(np.abs(o32["qz"][fin].astype(np.float64) - o64["qz"][fin]).max()) if fin.any() else 0.0
    return n_uv, n_z


def decided(o64, trunc, m_px, m_z, hw, z_min=0.0):
    """(D,H,W) bool: the nodes of a float64 integrate() result none of whose verdicts single-precision noise can flip.  For every view:
        |q.z - z_min| > 1e-3 (the sign of step 1; z_min = 0 in every GPU test);
        when the projection is within one pixel of the image, u + 0.5 and v + 0.5 are further than m_px from every integer (the pixel and the border);
        for a usable tap, |sdf + trunc| and |sdf - trunc| exceed 2 m_z (sdf = d - q.z: the noise of q.z and a little room)."""
    Hi, Wi = hw
    with np.errstate(invalid="ignore"):
        ok = np.abs(o64["qz"] - z_min) > 1e-3
        up, vp = o64["up"], o64["vp"]
        close = o64["front"] & ~((up < -1) | (up > Wi + 1) | (vp < -1) | (vp > Hi + 1))          # NaN positions: close, and undecided below
        fr = lambda a: np.abs(a - np.round(a))
        ok &= ~close | ((fr(up) > m_px) & (fr(vp) > m_px))
        ok &= ~o64["usable"] | ((np.abs(o64["sdf"] + trunc) > 2 * m_z) & (np.abs(o64["sdf"] - trunc) > 2 * m_z))
    return ok.all(0)


def masked_mesh(field, level, valid, positions=None, box=None, dtype=torch.float64):
    """The mesher's node mask as a post-filter: mesh_refs.extract, then every vertex whose edge has an invalid end and every face that uses a dropped vertex
    removed, and the rest renumbered.  valid: (D,H,W), non-zero = valid.  The same keys as mesh_refs.extract."""
    r = MR.extract(field, level, positions=positions, box=box, dtype=dtype)
    ok = torch.as_tensor(np.asarray(valid) != 0).reshape(-1)
    keep = ok[r["node"]] & ok[r["upper"]]
    new = torch.cumsum(keep.to(torch.int64), 0) - 1
    f = r["faces"].to(torch.int64)
    fkeep = keep[f].all(1) if f.numel() else torch.zeros((0,), dtype=torch.bool)
    out = {k: r[k][keep] for k in ("vertices", "ndc", "grid", "t", "vertex_edge", "node", "upper")}
    out["faces"] = new[f[fkeep]].to(torch.int32).reshape(-1, 3)
    out["count"] = torch.tensor([int(keep.sum()), int(fkeep.sum())], dtype=torch.int64)
    return out


def vertex_colors(tsdf, colors, vertex_edge, count, rows=None):
    """The statement of tsdf_vertex_colors in numpy fp32: tsdf (D,H,W) fp32, colors (D,H,W,4) uint8, vertex_edge (rows,) int64 -> (rows,3) uint8; rows past
    min(count, rows) are 0."""
    tsdf = np.asarray(tsdf, np.float32)
    D, H, W = tsdf.shape
    key = np.asarray(vertex_edge, np.int64)
    rows = len(key) if rows is None else rows
    live = min(int(count), rows)
    out = np.zeros((rows, 3), np.uint8)
    key = key[:live]
    n, e = key >> 3, key & 7
    d = np.array(MR.EDGES, np.int64)[e]
    up = n + d[:, 0] + d[:, 1] * W + d[:, 2] * H * W
    f = (-tsdf).reshape(-1)
    c = np.asarray(colors).reshape(-1, 4)
    f0, f1, c0, c1 = f[n], f[up], c[n], c[up]
    with np.errstate(all="ignore"):
        t = np.where(np.isfinite(f0) & np.isfinite(f1), (np.float32(0) - f0) / (f1 - f0), np.float32(0.5)).astype(np.float32)
        a, b = c0[:, :3].astype(np.float32), c1[:, :3].astype(np.float32)
        mix = np.floor((a + t[:, None] * (b - a)) + np.float32(0.5))
        mix = np.fmin(np.fmax(mix, np.float32(0)), np.float32(255)).astype(np.uint8)         # fmax / fmin: a NaN gives 0
    h0, h1 = c0[:, 3] == 255, c1[:, 3] == 255
    res = np.where((h0 & h1)[:, None], mix, np.where(h0[:, None], c0[:, :3], np.where(h1[:, None], c1[:, :3], 0)))
    out[:live] = res
    return out


class Case:
    """A rig, its corrupted inputs and the float64 / float32 restatements over one grid, computed once and shared; margins measured on the rig itself."""

    def __init__(self, hw, dims, M=5, look_at=True, views=None, do_corrupt=True, box=BOX, trunc=TRUNC):
        self.hw, self.dims, self.box, self.trunc, self.views = hw, dims, np.asarray(box, np.float32), trunc, views
        g = self.g = F.make_rig(hw[0], hw[1], M, look_at)
        self.M = M
        if do_corrupt:
            self.d32, self.valid, self.rgba = corrupt(g)
        else:
            self.d32, self.valid = g["depth"].astype(np.float32), None
            self.rgba = np.concatenate([g["images"], np.full((M,) + tuple(hw) + (1,), 255, np.uint8)], -1)
        self.c2w32, self.w2c32 = F.rounded_cameras(g["c2w"])
        self.K32 = g["K"].astype(np.float32)
        kw = dict(valid=self.valid, alpha=self.rgba[..., 3], views=views)
        self.o64 = integrate(self.d32, self.w2c32, self.K32, self.rgba, self.box, dims, trunc, dtype=np.float64, **kw)
        self.o32 = integrate(self.d32, self.w2c32, self.K32, self.rgba, self.box, dims, trunc, dtype=np.float32, **kw)
        self.n_uv, self.n_z = noise(self.o64, self.o32)
        self.m_px, self.m_z = 8.0 * self.n_uv, 8.0 * self.n_z
        self.decided = decided(self.o64, trunc, self.m_px, self.m_z, hw)
        dec = self.decided
        self.weights_agree = bool((self.o32["weight"][dec] == self.o64["weight"][dec]).all())
        self.tsdf_noise = float(np.abs(self.o32["tsdf"][dec].astype(np.float64) - self.o64["tsdf"][dec]).max()) if dec.any() else 0.0

    def undecided_fraction(self):
        return 1.0 - float(self.decided.mean())

    def describe(self):
        o = self.o64
        return (f"[{self.hw[0]} x {self.hw[1]}, {self.dims}] uv noise {self.n_uv:.1e} px, z noise {self.n_z:.1e}, undecided {100 * self.undecided_fraction():.2f} %, "
                f"|tsdf32 - tsdf64| {self.tsdf_noise:.1e}, weights agree {self.weights_agree}, observed {100 * float((o['weight'] > 0).mean()):.0f} %, "
                f"tsdf < 0 {100 * float((o['tsdf'] < 0).mean()):.0f} %")
