"""Brute-force restatements of DESIGN.md 4p (csrc/cloud_metrics.hip) in numpy, for the tests: the nearest neighbour within a radius, the cloud scores and
the points on a mesh - each once in float32, operation for operation what the kernels are defined to compute (numpy rounds every float32 operation on its
own), and once in float64.  Plus `grid_nearest32`, the kernel's ring search over a uniform grid restated on the host: it must give the bits of the brute
force for every grid, which is what makes the search exact and not merely close.  No GPU, no library."""
import numpy as np

F = np.float32
INT_MAX = 2 ** 31 - 1


def _finite_rows(a):
    return np.isfinite(a).all(axis=1)


def nearest32(targets, queries, max_dist, chunk=256):
    """(dist (N,) float32, index (N,) int32): per query the minimum of d2 = (dx dx + dy dy) + dz dz in float32 over the finite targets with d2 <= r2 =
    fl(max_dist max_dist), the LOWEST index among equal d2 (np.argmin returns the first), dist = sqrt(d2); +inf, -1 when there is none or the query row is
    not finite."""
    t = np.ascontiguousarray(targets, dtype=F).reshape(-1, 3)
    q = np.ascontiguousarray(queries, dtype=F).reshape(-1, 3)
    r2 = F(max_dist) * F(max_dist)
    dist = np.full(len(q), np.inf, dtype=F)
    index = np.full(len(q), -1, dtype=np.int32)
    ok_t = _finite_rows(t)
    if len(t) == 0 or not ok_t.any():
        return dist, index
    for b in range(0, len(q), chunk):
        qq = q[b:b + chunk]
        with np.errstate(invalid="ignore", over="ignore"):
            d = t[None, :, :] - qq[:, None, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        d2[:, ~ok_t] = np.inf
        d2[~_finite_rows(qq)] = np.inf
        j = np.argmin(d2, axis=1)
        best = d2[np.arange(len(qq)), j]
        hit = best <= r2
        dist[b:b + chunk][hit] = np.sqrt(best[hit])
        index[b:b + chunk][hit] = j[hit]
    return dist, index


def nearest64(targets, queries, max_dist, chunk=256):
    """The same in float64 from the float32 inputs -> (dist, index, near, second): dist and index with the radius applied (d <= max_dist), near and second
    the smallest and second smallest distance to a finite target without any radius (inf when there is none)."""
    t = np.asarray(targets, dtype=F).reshape(-1, 3).astype(np.float64)
    q = np.asarray(queries, dtype=F).reshape(-1, 3).astype(np.float64)
    r = float(F(max_dist))
    dist = np.full(len(q), np.inf)
    near = np.full(len(q), np.inf)
    second = np.full(len(q), np.inf)
    index = np.full(len(q), -1, dtype=np.int32)
    ok_t = _finite_rows(t)
    if len(t) == 0 or not ok_t.any():
        return dist, index, near, second
    for b in range(0, len(q), chunk):
        qq = q[b:b + chunk]
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.sqrt(((t[None, :, :] - qq[:, None, :]) ** 2).sum(-1))
        d[:, ~ok_t] = np.inf
        d[~_finite_rows(qq)] = np.inf
        j = np.argmin(d, axis=1)
        rows = np.arange(len(qq))
        best = d[rows, j].copy()
        d[rows, j] = np.inf
        near[b:b + chunk] = best
        second[b:b + chunk] = d.min(axis=1)
        hit = best <= r
        dist[b:b + chunk][hit] = best[hit]
        index[b:b + chunk][hit] = j[hit]
    return dist, index, near, second


def uniform_case(seed=0, n_target=2500, n_query=3000):
    """The uniform inputs of the GPU test: targets uniform in the unit box, queries uniform in the box grown by a quarter on every side (so that a
    good share of them has nothing within max_dist = a tenth of the box, and many lie outside the grid) -> (targets, queries, max_dist)."""
    g = np.random.default_rng(seed)
    return g.uniform(0.0, 1.0, (n_target, 3)).astype(F), g.uniform(-0.25, 1.25, (n_query, 3)).astype(F), 0.1


def noise_and_decided(targets, queries, max_dist):
    """What the float32 definition itself loses against float64 on these inputs, and which queries float64 decides beyond it ->
    (d32, i32, d64, i64, noise, decided): noise = the largest |dist32 - dist64| over the queries where both found a neighbour; decided = the gap between
    the nearest and the second nearest distance, and |nearest - max_dist|, both exceed 8 noise."""
    d32, i32 = nearest32(targets, queries, max_dist)
    d64, i64, near, second = nearest64(targets, queries, max_dist)
    both = np.isfinite(d32) & np.isfinite(d64)
    noise = float(np.abs(d32[both].astype(np.float64) - d64[both]).max()) if both.any() else 0.0
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(second), second - near, np.inf)
        edge = np.where(np.isfinite(near), np.abs(near - float(F(max_dist))), np.inf)
    decided = (gap > 8 * noise) & (edge > 8 * noise)
    return d32, i32, d64, i64, noise, decided


# ---- the kernel's search, restated: grid_build + grid_nearest_kernel of csrc/cloud_metrics.hip

def grid_layout(lo, hi, cell):
    lo = np.asarray(lo, dtype=F)
    ext = np.maximum(np.asarray(hi, dtype=np.float64) - lo.astype(np.float64), 0.0)
    return lo, F(cell), tuple(int(e // float(F(cell))) + 1 for e in ext)


def _cell_axis(p, lo, inv_cell, dim):
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((F(p) - lo) * inv_cell)
    return int(min(max(c, F(0)), F(dim - 1))) if not np.isnan(c) else 0


def grid_build(targets, lo, cell, dims):
    """cells: dict flat cell -> list of (x, y, z, original index), finite rows only."""
    t = np.asarray(targets, dtype=F).reshape(-1, 3)
    inv = F(1) / F(cell)
    cells = {}
    for i in np.nonzero(_finite_rows(t))[0]:
        c = [_cell_axis(t[i, a], lo[a], inv, dims[a]) for a in range(3)]
        cells.setdefault((c[2] * dims[1] + c[1]) * dims[0] + c[0], []).append((t[i, 0], t[i, 1], t[i, 2], int(i)))
    return cells


def grid_nearest32(targets, queries, max_dist, lo, cell, dims, visited=None):
    """The ring search of grid_nearest_kernel, statement for statement, in float32.  visited: a list that receives the number of rings of every query."""
    lo, cell = np.asarray(lo, dtype=F), F(cell)
    inv = F(1) / cell
    cells = grid_build(targets, lo, cell, dims)
    q = np.asarray(queries, dtype=F).reshape(-1, 3)
    r2 = F(max_dist) * F(max_dist)
    dist = np.full(len(q), np.inf, dtype=F)
    index = np.full(len(q), -1, dtype=np.int32)
    dx, dy, dz = dims
    for n in range(len(q)):
        best, best_i = r2, INT_MAX
        if not np.isfinite(q[n]).all():
            continue
        c = [_cell_axis(q[n, a], lo[a], inv, dims[a]) for a in range(3)]
        r = 0
        while True:
            x0, x1 = max(c[0] - r, 0), min(c[0] + r, dx - 1)
            for z in range(max(c[2] - r, 0), min(c[2] + r, dz - 1) + 1):
                for y in range(max(c[1] - r, 0), min(c[1] + r, dy - 1) + 1):
                    row = (z * dy + y) * dx
                    if abs(z - c[2]) == r or abs(y - c[1]) == r:
                        run = range(row + x0, row + x1 + 1)
                    else:
                        run = [row + x for x in (c[0] - r, c[0] + r) if 0 <= x < dx]
                    for cc in run:
                        for (px, py, pz, i) in cells.get(cc, ()):
                            with np.errstate(over="ignore"):
                                ex, ey, ez = px - q[n, 0], py - q[n, 1], pz - q[n, 2]
                                d2 = (ex * ex + ey * ey) + ez * ez
                            if d2 < best or (d2 == best and i < best_i):
                                best, best_i = d2, i
            L = F(np.inf)
            with np.errstate(over="ignore"):
                for a in range(3):
                    if c[a] + r + 1 <= dims[a] - 1:
                        e = F(c[a] + r + 1) * cell
                        B = (lo[a] + e) - q[n, a]
                        L = min(L, max(B - F(2e-6) * ((abs(e) + abs(lo[a])) + abs(q[n, a])), F(0)))
                    if c[a] - r - 1 >= 0:
                        e = F(c[a] - r) * cell
                        B = q[n, a] - (lo[a] + e)
                        L = min(L, max(B - F(2e-6) * ((abs(e) + abs(lo[a])) + abs(q[n, a])), F(0)))
                stop = (L * L) * F(0.999999) > best
            r += 1
            if stop:
                break
        if visited is not None:
            visited.append(r)
        if best_i != INT_MAX:
            dist[n], index[n] = np.sqrt(best), best_i
    return dist, index


# ---- the scores

def metrics64(dist_pred, dist_gt, taus):
    """numpy float64 on float32 distances: evaluate.cloud_metrics's table.  tau is rounded to float32 and compared in float32."""
    out = {}
    t32 = np.asarray(taus, dtype=np.float64).astype(F)
    for d, mean, n, share in ((np.asarray(dist_pred, dtype=F), "accuracy", "n_accuracy", "precision"),
                              (np.asarray(dist_gt, dtype=F), "completeness", "n_completeness", "recall")):
        fin = np.isfinite(d)
        out[n] = float(fin.sum())
        out[mean] = float(d[fin].astype(np.float64).sum() / fin.sum()) if fin.any() else float("nan")
        out[share] = np.array([(d < t).sum() / len(d) if len(d) else 0.0 for t in t32], dtype=np.float64)
    out["overall"] = (out["accuracy"] + out["completeness"]) / 2.0
    s = out["precision"] + out["recall"]
    out["fscore"] = np.where(s > 0, 2.0 * out["precision"] * out["recall"] / np.where(s > 0, s, 1.0), 0.0)
    return out


# ---- points on a mesh

def lattice_weights(n):
    """The (wb, wc) numerators over 3n of the n n centroids, in the documented order: rows j = 0..n-1, in a row i = 0..n-1-j, up then (i < n-1-j) down."""
    out = []
    for j in range(n):
        for i in range(n - j):
            out.append((3 * i + 1, 3 * j + 1))
            if i < n - 1 - j:
                out.append((3 * i + 2, 3 * j + 2))
    return out


def lattice_weight_of(n, s):
    """(wb, wc) of output row s of a face, by the arithmetic of sample_points_kernel: the row j is the largest with j (2n - j) <= s, found from a float32
    square root of n n - s with an integer correction."""
    rest = n * n - s
    h = int(np.ceil(np.sqrt(F(rest))))
    while h * h < rest:
        h += 1
    while h > 1 and (h - 1) * (h - 1) >= rest:
        h -= 1
    j = n - h
    pos = s - j * (2 * n - j)
    i, down = pos >> 1, pos & 1
    return 3 * i + 1 + down, 3 * j + 1 + down


def _sample(vertices, faces, spacing, T, max_n):
    v = np.asarray(vertices, dtype=F).reshape(-1, 3).astype(T)
    f = np.asarray(faces).reshape(-1, 3)
    sp = T(F(spacing))
    points, face, ns, ratio, weights = [], [], [], [], {}
    for k, (ia, ib, ic) in enumerate(f):
        n, rho = 0, float("nan")
        if min(ia, ib, ic) >= 0 and max(ia, ib, ic) < len(v) and np.isfinite(v[[ia, ib, ic]]).all():
            A, B, C = v[ia], v[ib], v[ic]
            with np.errstate(over="ignore"):
                def length(a, b):
                    d = b - a
                    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                L = max(max(length(A, B), length(B, C)), length(C, A))
                rho = L / sp
            n = int(min(max(np.ceil(rho), 1.0), 2.0 ** 30))
        ns.append(n)
        ratio.append(float(rho))
        if 1 <= n <= max_n:
            den = T(3 * n)
            if n not in weights:
                weights[n] = np.asarray(lattice_weights(n), dtype=T)
            wb, wc = weights[n][:, 0:1], weights[n][:, 1:2]                           # (n n, 1) against the (3,) corners: the same operations per element
            wa = (den - wb) - wc
            points.append(((wa * A + wb * B) + wc * C) / den)
            face.append(np.full(n * n, k, dtype=np.int32))
    pts = np.concatenate(points).astype(T) if points else np.zeros((0, 3), dtype=T)
    fcs = np.concatenate(face) if face else np.zeros((0,), dtype=np.int32)
    return pts, fcs, np.asarray(ns, dtype=np.int64), np.asarray(ratio)


def sample32(vertices, faces, spacing, max_n=1024):
    """(points (P,3) float32, face (P,) int32, n per face) - operation for operation sample_points_kernel."""
    return _sample(vertices, faces, spacing, F, max_n)[:3]


def sample64(vertices, faces, spacing, max_n=1024):
    """The same in float64 from the float32 inputs -> (points, face, n per face, L / spacing per face)."""
    return _sample(vertices, faces, spacing, np.float64, max_n)


def barycentric64(p, A, B, C):
    """Least-squares barycentric coordinates (wa, wb, wc) of p in the plane of ABC (float64), and the distance of p from that plane's point."""
    M = np.stack([B - A, C - A], axis=1)
    uv, *_ = np.linalg.lstsq(M, p - A, rcond=None)
    return np.array([1.0 - uv.sum(), uv[0], uv[1]]), float(np.linalg.norm(A + M @ uv - p))
