"""The yardstick of the mesh rasteriser (csrc/raster.hip): the definition restated in numpy, face by face, with int64 edge functions.

render(..., dtype=np.float64) is the yardstick; dtype=np.float32 runs the same statements in single precision, one rounding per operation - what the kernels
compute - so the GPU is compared with it EXACTLY (face, depth bits, colours).  render_pixels is a second, independent formulation: pixel by pixel over all
faces, no bounding box, the winner chosen as the lexicographic minimum of (z, face).  face_views and filter_mesh restate the two mesh tools.

Meshes for the tests: the sphere of tests/depth_fusion_refs.py meshed by tests/mesh_refs.py over box = +-160, and hand-made triangles in front of a camera at
the origin whose focal length and depths are powers of two, so that their corners land on exact sub-pixel positions.
"""
import numpy as np
import torch

import depth_fusion_refs as DF
import mesh_refs as MR

SUB = 256
MAX_SNAP = 2 ** 23


def project(V, w2c, K, dtype, z_min=0.0):
    """Per vertex: (ok, X, Y int64 snapped positions (0 where not ok), iz)."""
    t = np.dtype(dtype).type
    V, w2c, K = np.asarray(V).astype(t).reshape(-1, 3), np.asarray(w2c).astype(t), np.asarray(K).astype(t)
    q = [((w2c[k, 0] * V[:, 0] + w2c[k, 1] * V[:, 1]) + w2c[k, 2] * V[:, 2]) + w2c[k, 3] for k in range(3)]
    with np.errstate(all="ignore"):
        u = K[0, 0] * q[0] / q[2] + K[0, 2]
        v = K[1, 1] * q[1] / q[2] + K[1, 2]
        X = np.floor(u * t(SUB) + t(0.5))
        Y = np.floor(v * t(SUB) + t(0.5))
        iz = t(1) / q[2]
        ok = (q[2] > t(z_min)) & np.isfinite(u) & np.isfinite(v) & (np.abs(X) <= MAX_SNAP) & (np.abs(Y) <= MAX_SNAP)
    return ok, np.where(ok, X, 0).astype(np.int64), np.where(ok, Y, 0).astype(np.int64), iz


def setup(f, F, nv, ok, X, Y, cull):
    """The setup of face f -> None (dropped whole) or (a, b, c after the swap, the three corners as ints, A > 0, the signed A before the swap)."""
    a, b, c = (int(i) for i in F[f])
    if min(a, b, c) < 0 or max(a, b, c) >= nv or not (ok[a] and ok[b] and ok[c]):
        return None
    x0, y0, x1, y1, x2, y2 = (int(w) for w in (X[a], Y[a], X[b], Y[b], X[c], Y[c]))
    A = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    if A == 0 or (cull > 0 and A > 0) or (cull < 0 and A < 0):
        return None
    signed = A
    if A < 0:
        b, c, x1, y1, x2, y2, A = c, b, x2, y2, x1, y1, -A
    return a, b, c, (x0, y0, x1, y1, x2, y2), A, signed


def _edge(xa, ya, xb, yb, px, py):
    """(e, the inner-side verdict) of the edge a -> b at the sub-pixel positions px, py (int64 arrays)"""
    dx, dy = xb - xa, yb - ya
    e = dx * (py - ya) - dy * (px - xa)
    top_left = dy < 0 or (dy == 0 and dx > 0)
    return e, (e > 0) | ((e == 0) & top_left)


def _fragment(e1, e2, A, iz, abc, C, t, z_min):
    """(z, counts, byte colours | None) of covered positions: e1, e2 int64 arrays"""
    a, b, c = abc
    with np.errstate(all="ignore"):
        b1 = e1.astype(t) / t(A)
        b2 = e2.astype(t) / t(A)
        b0 = (t(1) - b1) - b2
        t0, t1, t2 = b0 * iz[a], b1 * iz[b], b2 * iz[c]
        invz = (t0 + t1) + t2
        z = t(1) / invz
        good = np.isfinite(z) & (z > t(z_min))
        rgb = None
        if C is not None:
            col = ((t0[..., None] * C[a].astype(t) + t1[..., None] * C[b].astype(t)) + t2[..., None] * C[c].astype(t)) * z[..., None]
            rgb = np.clip(np.floor(np.where(good[..., None], col, 0) + t(0.5)), 0, 255).astype(np.uint8)
    return z, good, rgb


def _live(V, F, count):
    V, F = np.asarray(V).reshape(-1, 3), np.asarray(F).reshape(-1, 3).astype(np.int64)
    if count is not None:
        V, F = V[:min(max(int(count[0]), 0), len(V))], F[:min(max(int(count[1]), 0), len(F))]
    return V, F


def render(V, F, C, w2c, K, H, W, dtype=np.float64, z_min=0.0, cull=0, background=(255, 255, 255), count=None):
    """One view, face by face -> {'depth' (H,W) dtype (0 = nothing), 'face' (H,W) int32 (-1 = nothing), 'colors' (H,W,3) uint8 | None,
    'hits' (H,W) int32: the faces whose fragment counts at the pixel, 'area' (T,) int64: the signed snapped area of every face that was set up, else 0}.
    count: (vertices, faces) that are meaningful; rows past them are not read."""
    t = np.dtype(dtype).type
    V, F = _live(V, F, count)
    C = None if C is None else np.asarray(C)
    ok, X, Y, iz = project(V, w2c, K, dtype, z_min)
    depth, face, best = np.zeros((H, W), t), np.full((H, W), -1, np.int32), np.full((H, W), np.inf, t)
    rgb = None if C is None else np.empty((H, W, 3), np.uint8)
    if rgb is not None:
        rgb[:] = np.asarray(background, np.uint8)
    hits, area = np.zeros((H, W), np.int32), np.zeros((len(F),), np.int64)
    for f in range(len(F)):
        s = setup(f, F, len(V), ok, X, Y, cull)
        if s is None:
            continue
        a, b, c, (x0, y0, x1, y1, x2, y2), A, area[f] = s
        xs, xe = max(0, -(-min(x0, x1, x2) // SUB)), min(W - 1, max(x0, x1, x2) // SUB)
        ys, ye = max(0, -(-min(y0, y1, y2) // SUB)), min(H - 1, max(y0, y1, y2) // SUB)
        if xs > xe or ys > ye:
            continue
        py, px = np.meshgrid(np.arange(ys, ye + 1, dtype=np.int64) * SUB, np.arange(xs, xe + 1, dtype=np.int64) * SUB, indexing="ij")
        e0, i0 = _edge(x1, y1, x2, y2, px, py)
        e1, i1 = _edge(x2, y2, x0, y0, px, py)
        e2, i2 = _edge(x0, y0, x1, y1, px, py)
        z, good, col = _fragment(e1, e2, A, iz, (a, b, c), C, t, z_min)
        good &= i0 & i1 & i2
        box = (slice(ys, ye + 1), slice(xs, xe + 1))
        hits[box] += good
        win = good & (z < best[box])                                                    # strictly nearer: the lower face number keeps an equal z
        best[box][win] = z[win]
        depth[box][win] = z[win]
        face[box][win] = f
        if rgb is not None:
            rgb[box][win] = col[win]
    return {"depth": depth, "face": face, "colors": rgb, "hits": hits, "area": area}


def render_views(V, F, C, w2cs, Ks, H, W, views=None, **kw):
    """render per view of the list (default every view), stacked: depth (n,H,W), face (n,H,W), colors (n,H,W,3) | None"""
    views = range(len(w2cs)) if views is None else views
    out = [render(V, F, C, w2cs[m], Ks[m], H, W, **kw) for m in views]
    return {"depth": np.stack([o["depth"] for o in out]), "face": np.stack([o["face"] for o in out]),
            "colors": None if C is None else np.stack([o["colors"] for o in out]), "hits": np.stack([o["hits"] for o in out]),
            "area": np.stack([o["area"] for o in out])}


def render_pixels(V, F, C, w2c, K, H, W, dtype=np.float64, z_min=0.0, cull=0, background=(255, 255, 255)):
    """The second formulation: every pixel against ALL faces at once (no bounding box), the winner = the lexicographic minimum of (z, face)."""
    t = np.dtype(dtype).type
    V, F = _live(V, F, None)
    ok, X, Y, iz = project(V, w2c, K, dtype, z_min)
    S = [(f, s) for f, s in ((f, setup(f, F, len(V), ok, X, Y, cull)) for f in range(len(F))) if s is not None]
    depth, face = np.zeros((H, W), t), np.full((H, W), -1, np.int32)
    rgb = None if C is None else np.tile(np.asarray(background, np.uint8), (H, W, 1))
    if not S:
        return {"depth": depth, "face": face, "colors": rgb}
    fid = np.array([f for f, _ in S], np.int64)
    abc = np.array([s[:3] for _, s in S], np.int64)
    P = np.array([s[3] for _, s in S], np.int64)                                         # (n,6)
    A = np.array([s[4] for _, s in S], np.int64)
    Cn = None if C is None else np.asarray(C)

    def edge(xa, ya, xb, yb, px, py):
        dx, dy = xb - xa, yb - ya
        e = dx * (py - ya) - dy * (px - xa)
        return e, (e > 0) | ((e == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
    for y in range(H):
        for x in range(W):
            px, py = np.int64(x * SUB), np.int64(y * SUB)
            e0, i0 = edge(P[:, 2], P[:, 3], P[:, 4], P[:, 5], px, py)
            e1, i1 = edge(P[:, 4], P[:, 5], P[:, 0], P[:, 1], px, py)
            e2, i2 = edge(P[:, 0], P[:, 1], P[:, 2], P[:, 3], px, py)
            with np.errstate(all="ignore"):
                b1, b2 = e1.astype(t) / A.astype(t), e2.astype(t) / A.astype(t)
                b0 = (t(1) - b1) - b2
                t0, t1, t2 = b0 * iz[abc[:, 0]], b1 * iz[abc[:, 1]], b2 * iz[abc[:, 2]]
                z = t(1) / ((t0 + t1) + t2)
                good = i0 & i1 & i2 & np.isfinite(z) & (z > t(z_min))
            if not good.any():
                continue
            zmin = z[good].min()
            k = int(np.nonzero(good & (z == zmin))[0][0])                                # fid ascends: the lowest face number
            depth[y, x], face[y, x] = z[k], fid[k]
            if rgb is not None:
                ca, cb, cc = (Cn[abc[k, j]].astype(t) for j in range(3))
                rgb[y, x] = np.clip(np.floor(((t0[k] * ca + t1[k] * cb) + t2[k] * cc) * z[k] + t(0.5)), 0, 255).astype(np.uint8)
    return {"depth": depth, "face": face, "colors": rgb}


def face_views(face, n_faces, views=None, n_bank=None):
    """face (n,H,W) int -> (n_views (T,) int32, seen (T, ceil(M / 32)) int32 bit masks); map a shows view views[a] (default a)"""
    face = np.asarray(face)
    n = face.shape[0]
    views = list(range(n)) if views is None else list(views)
    M = n if n_bank is None else n_bank
    seen = np.zeros((n_faces, (M + 31) // 32), np.uint32)
    for a, m in enumerate(views):
        if not 0 <= m < M:
            continue
        ids = np.unique(face[a])
        ids = ids[(ids >= 0) & (ids < n_faces)]
        seen[ids, m >> 5] |= np.uint32(1 << (m & 31))
    return DF.popcount(seen).sum(1).astype(np.int32) if n_faces else np.zeros((0,), np.int32), seen.view(np.int32)


def filter_mesh(V, F, keep, count=None, **rows):
    """The kept faces in order and the vertices they use in order -> {'vertices', 'faces' int32, 'vertex_index', 'face_index' int64, and every keyword
    array (ndc=, vertex_edge=, colors=) cut to the kept vertices}.  A kept face with a vertex number outside the mesh is dropped."""
    V, F = np.asarray(V).reshape(-1, 3), np.asarray(F).reshape(-1, 3).astype(np.int64)
    nv, nf = (len(V), len(F)) if count is None else (min(max(int(count[0]), 0), len(V)), min(max(int(count[1]), 0), len(F)))
    k = np.asarray(keep).astype(bool).copy()
    k[nf:] = False
    k &= ((F >= 0) & (F < nv)).all(1)
    used = np.zeros(len(V), bool)
    used[F[k].reshape(-1)] = True
    remap = np.where(used, np.cumsum(used) - 1, -1)
    out = {"vertices": V[used], "faces": remap[F[k]].astype(np.int32).reshape(-1, 3), "vertex_index": np.nonzero(used)[0].astype(np.int64),
           "face_index": np.nonzero(k)[0].astype(np.int64)}
    out.update({name: np.asarray(a)[used] for name, a in rows.items() if a is not None})
    return out


# ------------------------------------------------------------------ meshes and cameras for the tests
BOX160 = np.array([[-160.0, -160.0, -160.0], [160.0, 160.0, 160.0]], np.float32)


def sphere_mesh(shape, seed=0):
    """The rig's sphere (radius 120) meshed over box = +-160 on a (D,H,W) grid, fp32 -> (vertices (V,3) fp32, faces (T,3) int32, colors (V,3) uint8 seeded)."""
    D, H, W = shape
    i, j, k = MR._xyz(*shape)
    x, y, z = -160 + i / (W - 1) * 320, -160 + j / (H - 1) * 320, -160 + k / (D - 1) * 320
    field = (DF.SPHERE_R - np.sqrt(x * x + y * y + z * z)).astype(np.float32)
    m = MR.extract(field, 0.0, box=BOX160, dtype=torch.float32)
    V, F = m["vertices"].numpy().astype(np.float32), m["faces"].numpy().astype(np.int32)
    C = np.random.default_rng(seed).integers(0, 256, (len(V), 3)).astype(np.uint8)
    return V, F, C


def rig(H, W, M=5, look_at=True):
    """(c2w (M,4,4) float64, K (M,3,3) float64, w2c32 (M,3,4), K32 (M,3,3): what the device receives) of the depth-fusion rig"""
    g = DF.make_rig(H, W, M, look_at)
    return g["c2w"], g["K"], DF.rounded_cameras(g["c2w"])[1], g["K"].astype(np.float32), g


FOCAL, CX, CY = 64.0, 8.0, 4.0
EYE_C2W = np.eye(4)[None]
EYE_K = np.array([[[FOCAL, 0.0, CX], [0.0, FOCAL, CY], [0.0, 0.0, 1.0]]])


def at(u, v, z):
    """The world point that the camera at the origin (EYE_C2W, EYE_K) sees at pixel (u, v) and depth z; exact for z a power of two and u, v multiples of
    1/256 well inside fp32."""
    return [(u - CX) / FOCAL * z, (v - CY) / FOCAL * z, z]


def quad():
    """A quad with corners on pixel centres (2,2) (10,2) (10,10) (2,10), split along the diagonal (2,2)-(10,10), which runs through pixel centres"""
    V = np.array([at(2, 2, 4.0), at(10, 2, 4.0), at(10, 10, 4.0), at(2, 10, 4.0)], np.float32)
    F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)          # face 0: above / right of the diagonal (x >= y), face 1: below / left of it
    return V, F


# world units: the median |mesh depth - analytic depth| of the CPU chain, measured by test_raster_refs.test_chain_figure (which asserts that it still stands)
CHAIN_MEDIAN = 1.1783
