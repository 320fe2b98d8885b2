"""The yardstick of the depth-fusion kernels (csrc/depth_fusion.hip): a numpy restatement of the definition in
include/mvsnerf_hip_internal.h, written pair by pair, and an analytic test rig.

Reference(...).pairs(r, s) evaluates every pixel of view r against source view s and returns every intermediate quantity; consistency() and compact()
assemble the kernels' outputs from it.  dtype=np.float64 is the yardstick; dtype=np.float32 runs the same statements in single precision, one rounding per
operation, so that the fp32 noise floor of the definition itself can be measured on the CPU (the GPU tests take their margins from it).

The rig is ray-cast in float64, so its depth maps are truly consistent wherever a surface point is visible in both views:
    scene   the plane z = 150 and a sphere of radius 120 at the origin
    views   M OpenCV-convention cameras (x right, y down, z forward) on an arc of +-14 degrees at distance 600 on the z < 0 side, each with a vertical
            offset and a roll about its optical axis.  look_at=False: every optical axis is the world's z axis, so the plane is fronto-parallel in every
            view and bilinear interpolation of its depth is exact; look_at=True: every camera looks at the origin (dense rotations, a tilted plane).
    K       fx = fy = 1.1 W, the principal point off-centre by a fraction of a pixel
"""
import numpy as np

PLANE_Z, SPHERE_R, DIST = 150.0, 120.0, 600.0


def _rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def rig_cameras(H, W, M=5, look_at=False):
    """c2w (M,4,4), K (M,3,3), float64."""
    c2w = np.zeros((M, 4, 4))
    K = np.zeros((M, 3, 3))
    for m in range(M):
        a = np.deg2rad(14.0) * (2.0 * m / max(M - 1, 1) - 1.0) if M > 1 else 0.0
        pos = np.array([DIST * np.sin(a), 25.0 * ((m % 3) - 1) + 4.0 * m, -DIST * np.cos(a)])
        f = -pos / np.linalg.norm(pos) if look_at else np.array([0.0, 0.0, 1.0])
        x = np.cross(np.array([0.0, 1.0, 0.0]), f)
        x /= np.linalg.norm(x)
        y = np.cross(f, x)
        R = np.stack([x, y, f], 1) @ _rot_z(np.deg2rad(3.0 * (m - (M - 1) / 2.0)))       # a roll about the optical axis
        c2w[m, :3, :3], c2w[m, :3, 3], c2w[m, 3, 3] = R, pos, 1.0
        K[m] = [[1.1 * W, 0.0, 0.5 * (W - 1) + 0.3 - 0.1 * m], [0.0, 1.1 * W, 0.5 * (H - 1) - 0.2 + 0.07 * m], [0.0, 0.0, 1.0]]
    return c2w, K


def analytic_depth(o, d):
    """Ray parameter t >= 0 of the first hit of o + t d with the sphere or the plane, float64; (t, label) with label 1 on the sphere, 0 on the plane and t = 0,
    label -1 for a ray that hits neither in front of it.  o, d: (...,3)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tp = (PLANE_Z - o[..., 2]) / d[..., 2]
        a, b, c = (d * d).sum(-1), (o * d).sum(-1), (o * o).sum(-1) - SPHERE_R ** 2
        disc = b * b - a * c
        ts = (-b - np.sqrt(np.where(disc >= 0, disc, np.nan))) / a
    tp = np.where(np.isfinite(tp) & (tp > 0), tp, np.inf)
    ts = np.where(np.isfinite(ts) & (ts > 0), ts, np.inf)
    t = np.minimum(tp, ts)
    label = np.where(ts < tp, 1, 0)
    miss = ~np.isfinite(t)
    return np.where(miss, 0.0, t), np.where(miss, -1, label).astype(np.int8)


def view_rays(c2w, K, H, W):
    """o (3,), d (H,W,3) of a view in the bank's convention: d = R ((x - cx) / fx, (y - cy) / fy, 1)."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dc = np.stack([(x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1], np.ones_like(x)], -1)
    return c2w[:3, 3], dc @ c2w[:3, :3].T


def make_rig(H, W, M=5, look_at=False):
    """{'c2w' (M,4,4), 'K' (M,3,3), 'depth' (M,H,W) float64 ray-cast, 'label' (M,H,W) int8, 'images' (M,H,W,3) uint8}."""
    c2w, K = rig_cameras(H, W, M, look_at)
    depth, label = np.zeros((M, H, W)), np.zeros((M, H, W), np.int8)
    for m in range(M):
        o, d = view_rays(c2w[m], K[m], H, W)
        depth[m], label[m] = analytic_depth(np.broadcast_to(o, d.shape), d)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    images = np.stack([np.stack([(37 * xx + 11 * m) % 256, (53 * yy + 5 * m) % 256, np.where(label[m] == 1, 200, 40) + (xx + yy) % 7], -1)
                       for m in range(M)]).astype(np.uint8)
    return {"c2w": c2w, "K": K, "depth": depth, "label": label, "images": images}


def rounded_cameras(c2w64):
    """What the device receives: c2w [M][3][4] and w2c [M][3][4] (inverted in float64, rounded once), float32."""
    c2w64 = np.asarray(c2w64, np.float64)
    return (np.ascontiguousarray(c2w64[:, :3, :4], np.float32), np.ascontiguousarray(np.linalg.inv(c2w64)[:, :3, :4], np.float32))


class Reference:
    """The definition, evaluated in `dtype` on exactly the arrays given (hand it the float32-rounded cameras and depths to judge a kernel that received those).
        depth (M,H,W); c2w, w2c (M,3,4); K (M,3,3); valid (M,H,W) or None; alpha (M,H,W) uint8 or None"""

    def __init__(self, depth, c2w, w2c, K, valid=None, alpha=None, dtype=np.float64):
        t = self.dtype = np.dtype(dtype).type
        self.depth = np.asarray(depth).astype(t)
        self.c2w, self.w2c, self.K = np.asarray(c2w).astype(t), np.asarray(w2c).astype(t), np.asarray(K).astype(t)
        self.M, self.H, self.W = self.depth.shape
        assert self.H >= 2 and self.W >= 2
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(self.depth) & (self.depth > 0)
        if valid is not None:
            ok &= np.asarray(valid) != 0
        if alpha is not None:
            ok &= np.asarray(alpha) != 0
        self.usable = ok
        y, x = np.meshgrid(np.arange(self.H), np.arange(self.W), indexing="ij")
        self.x, self.y = x.astype(t), y.astype(t)

    def lift(self, m, px, py, z):
        K, c = self.K[m], self.c2w[m]
        dx, dy = (px - K[0, 2]) / K[0, 0], (py - K[1, 2]) / K[1, 1]
        return [c[k, 3] + ((dx * c[k, 0] + dy * c[k, 1]) + c[k, 2]) * z for k in range(3)]

    def to_camera(self, m, P):
        w = self.w2c[m]
        return [((w[k, 0] * P[0] + w[k, 1] * P[1]) + w[k, 2] * P[2]) + w[k, 3] for k in range(3)]

    def cell_ok(self, s, x0, y0):
        """all four taps of the cell (x0, y0) of view s usable; x0, y0 int arrays inside [0, W-2] x [0, H-2]"""
        u = self.usable[s]
        return u[y0, x0] & u[y0, x0 + 1] & u[y0 + 1, x0] & u[y0 + 1, x0 + 1]

    def pairs(self, r, s):
        """Every pixel of view r against source view s -> dict of (H,W) arrays:
            ref_ok   the reference depth is usable           front    q.z > 0 in view s
            u, v     image position in view s                inside   front and (u, v) in [0, W-1] x [0, H-1]
            x0, y0   the bilinear cell (0 where not inside)  taps_ok  inside and all four taps usable
            zs       the bilinear depth                      xp, yp, zp   the way back: (x', y', z') in view r
            err      hypot(x' - x, y' - y)                   rel      |z' - z| / z
        Quantities are NaN (or arbitrary) where the steps before them failed; `consistent(p, ...)` combines them."""
        t, H, W = self.dtype, self.H, self.W
        z = np.where(self.usable[r], self.depth[r], t(1))
        with np.errstate(all="ignore"):
            q = self.to_camera(s, self.lift(r, self.x, self.y, z))
            front = q[2] > 0
            Ks = self.K[s]
            u, v = Ks[0, 0] * q[0] / q[2] + Ks[0, 2], Ks[1, 1] * q[1] / q[2] + Ks[1, 2]
            inside = front & (u >= 0) & (u <= t(W - 1)) & (v >= 0) & (v <= t(H - 1))
            uc, vc = np.where(inside, u, t(0)), np.where(inside, v, t(0))
            x0, y0 = np.minimum(np.floor(uc).astype(np.int64), W - 2), np.minimum(np.floor(vc).astype(np.int64), H - 2)
            ax, ay = uc - x0.astype(t), vc - y0.astype(t)
            taps_ok = inside & self.cell_ok(s, x0, y0)
            d = np.where(self.usable[s], self.depth[s], t(1))
            one = t(1)
            zs = (d[y0, x0] * (one - ax) + d[y0, x0 + 1] * ax) * (one - ay) + (d[y0 + 1, x0] * (one - ax) + d[y0 + 1, x0 + 1] * ax) * ay
            b = self.to_camera(r, self.lift(s, uc, vc, zs))
            Kr = self.K[r]
            xp, yp, zp = Kr[0, 0] * b[0] / b[2] + Kr[0, 2], Kr[1, 1] * b[1] / b[2] + Kr[1, 2], b[2]
            ex, ey = xp - self.x, yp - self.y
            err = np.sqrt(ex * ex + ey * ey)
            rel = np.abs(zp - z) / z
        return {"ref_ok": self.usable[r], "front": front, "qz": q[2], "u": u, "v": v, "inside": inside, "x0": x0, "y0": y0, "taps_ok": taps_ok, "zs": zs,
                "xp": xp, "yp": yp, "zp": zp, "err": err, "rel": rel, "z": z}

    def consistent(self, p, pix_thr, rel_thr):
        t = self.dtype
        with np.errstate(invalid="ignore"):
            return p["ref_ok"] & p["taps_ok"] & (p["zp"] > 0) & (p["err"] < t(pix_thr)) & (p["rel"] < t(rel_thr))

    def consistency(self, src_ids, pix_thr=1.0, rel_thr=0.01, min_views=3):
        """seen (M,H,W) uint32, fused (M,H,W) dtype, mask (M,H,W) uint8 for src_ids (M,n_src), -1 = no view."""
        t = self.dtype
        src_ids = np.asarray(src_ids)
        seen = np.zeros((self.M, self.H, self.W), np.uint32)
        fused = np.zeros((self.M, self.H, self.W), t)
        for r in range(self.M):
            total = np.where(self.usable[r], self.depth[r], t(0))
            n = np.zeros((self.H, self.W), np.int64)
            for j, s in enumerate(src_ids[r]):
                if s < 0:
                    continue
                assert s != r and s < self.M
                p = self.pairs(r, int(s))
                c = self.consistent(p, pix_thr, rel_thr)
                seen[r] |= np.where(c, np.uint32(1 << j), np.uint32(0))
                total = total + np.where(c, p["zp"], t(0))
                n += c
            fused[r] = np.where(self.usable[r], total / (n + 1).astype(t), t(0))
        pop = popcount(seen)
        return seen, fused, ((pop >= min_views) & self.usable).astype(np.uint8)

    def compact(self, mask, fused, seen, images):
        """The cloud of the pixels with mask != 0, visited view by view, row by row (the flat-ray-index order): points (N,3) dtype, colors (N,3) uint8,
        n_views (N,) uint8, index (N,) int64.  images (M,H,W,>=3) uint8."""
        t = self.dtype
        pts, col, nv, idx = [], [], [], []
        fused = np.asarray(fused).astype(t)
        for m in range(self.M):
            P = self.lift(m, self.x, self.y, fused[m])
            keep = np.asarray(mask[m]) != 0
            for y in range(self.H):                       # (spelt out: the order is part of the definition)
                for x in np.nonzero(keep[y])[0]:
                    pts.append([P[0][y, x], P[1][y, x], P[2][y, x]])
                    col.append(images[m, y, x, :3])
                    nv.append(bin(int(seen[m, y, x])).count("1"))
                    idx.append((m * self.H + y) * self.W + x)
        return (np.asarray(pts, t).reshape(-1, 3), np.asarray(col, np.uint8).reshape(-1, 3), np.asarray(nv, np.uint8), np.asarray(idx, np.int64))


def popcount(a):
    a = np.asarray(a).astype(np.uint32)
    return sum(((a >> np.uint32(k)) & np.uint32(1)).astype(np.int64) for k in range(32))


def default_src_ids(M, n_src):
    """every other view, in ascending order of |m - r| (ties: the lower id first), the first n_src of them, -1 padded: a fixed choice for tests that do not
    test the selection"""
    ids = np.full((M, n_src), -1, np.int32)
    for r in range(M):
        o = sorted((m for m in range(M) if m != r), key=lambda m: (abs(m - r), m))[:n_src]
        ids[r, :len(o)] = o
    return ids


def decided(ref64, p, pix_thr, rel_thr, m_px, m_rel, s):
    """Which pixels of a float64 pairs() result have a verdict that single-precision noise cannot flip (True = decided).  m_px: the margin in pixels for
    err, for (u, v) against the image border and against an integer grid line whose crossing changes the validity of the taps; m_rel: the margin for rel.
    Pixels whose reference depth is unusable are decided (their verdict does not depend on arithmetic)."""
    H, W = ref64.H, ref64.W
    with np.errstate(invalid="ignore"):
        ok = np.abs(p["qz"]) > 1e-3 * np.abs(p["z"])                                    # the sign of q.z
        u, v = p["u"], p["v"]
        border = np.minimum(np.minimum(np.abs(u), np.abs(u - (W - 1))), np.minimum(np.abs(v), np.abs(v - (H - 1))))
        ok &= ~p["front"] | (border > m_px)                                             # NaN positions compare False: undecided
        ins = p["inside"]
        # tap validity on the other side of a near grid line
        uc, vc = np.where(ins, u, 0.0), np.where(ins, v, 0.0)
        same = np.ones_like(ins)
        for du in (-1, 0, 1):
            for dv in (-1, 0, 1):
                x0 = np.clip(np.floor(uc + du * m_px).astype(np.int64), 0, W - 2)
                y0 = np.clip(np.floor(vc + dv * m_px).astype(np.int64), 0, H - 2)
                same &= ref64.cell_ok(s, x0, y0) == p["taps_ok"]
        ok &= ~ins | same
        live = ins & p["taps_ok"]
        thr = (np.abs(p["err"] - pix_thr) > m_px) & (np.abs(p["rel"] - rel_thr) > m_rel) & (np.abs(p["zp"]) > 1e-3 * np.abs(p["z"]))
        ok &= ~live | thr
    return ok | ~p["ref_ok"]
