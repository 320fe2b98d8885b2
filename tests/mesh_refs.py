"""The definition of geometry.extract_mesh restated in torch, for the tests and for bench_mesh.py's baseline: marching tetrahedra over the
Kuhn (Freudenthal) split of every cell of a (D,H,W) scalar field.  `extract(..., dtype=torch.float64)` is the yardstick; `dtype=torch.float32` is the
restatement whose every operation is rounded on its own, the bits the kernels of csrc/mesh.hip must give.  Both read the SAME fp32 field, level, box and
node table.  Vectorised, so it runs on the GPU as well.

The faces a tetrahedron emits are DERIVED here by a parity rule, not copied from a table (tet_case_triangles), so that the literal table of the kernel is
held to something independent.  With corners c0..c3 of a tetrahedron and s the sign of det(c1-c0, c2-c0, c3-c0) (the sign of the axis permutation of the
Kuhn split), the oriented volume of the simplex (c_p, c_q, c_r, c_w) is s times the sign of the permutation (p,q,r,w) of (0,1,2,3); a triangle on the three
edges leaving corner p towards q, r, w has its normal pointing away from p exactly when that volume is positive.
"""
import itertools
import math

import numpy as np
import torch

EDGES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))      # owned edge e -> (dx, dy, dz)
EDGE_ID = {d: e for e, d in enumerate(EDGES)}
PERMS = tuple(itertools.permutations(range(3)))                                            # xyz, xzy, yxz, yzx, zxy, zyx
U = 2.0 ** -24


def perm_sign(seq):
    inv = sum(1 for a in range(len(seq)) for b in range(a + 1, len(seq)) if seq[a] > seq[b])
    return -1 if inv & 1 else 1


def tet_case_triangles(case, s):
    """The triangles of a tetrahedron whose corner c is inside iff bit c of `case` is set, s = +-1 its orientation: a list of triangles, each three
    edges, each edge a (lower corner, upper corner) pair.  The normal points from the inside corners to the outside ones."""
    ins = [c for c in range(4) if case >> c & 1]
    out = [c for c in range(4) if not case >> c & 1]
    edge = lambda a, b: (min(a, b), max(a, b))
    if len(ins) in (0, 4):
        return []
    if len(ins) in (1, 3):
        i = ins[0] if len(ins) == 1 else out[0]                     # the lone corner; the triangle cuts its three edges
        a, b, c = [x for x in range(4) if x != i]
        sigma = s * perm_sign((i, a, b, c)) * (1 if len(ins) == 1 else -1)
        tris = [[edge(i, a), edge(i, b), edge(i, c)]]
    else:
        (i, j), (k, l) = ins, out                                   # the quad ik, il, jl, jk, split along ik - jl
        sigma = s * perm_sign((i, k, l, j))
        tris = [[edge(i, k), edge(i, l), edge(j, l)], [edge(i, k), edge(j, l), edge(j, k)]]
    if sigma < 0:
        tris = [[t[0], t[2], t[1]] for t in tris]
    return [tuple(t) for t in tris]


def _cell_tables():
    """n[6][16] triangles of tetrahedron p in case c; off[6][16][2][3][3], e[6][16][2][3]: per triangle vertex the owner node's offset from the cell's
    origin and the owned edge."""
    n = np.zeros((6, 16), np.int64)
    off = np.zeros((6, 16, 2, 3, 3), np.int64)
    e = np.zeros((6, 16, 2, 3), np.int64)
    for p, perm in enumerate(PERMS):
        corners = [np.zeros(3, np.int64)]
        for axis in perm:
            corners.append(corners[-1] + np.eye(3, dtype=np.int64)[axis])
        s = perm_sign(perm)
        for case in range(16):
            tris = tet_case_triangles(case, s)
            n[p, case] = len(tris)
            for ti, tri in enumerate(tris):
                for vi, (lo, hi) in enumerate(tri):
                    off[p, case, ti, vi] = corners[lo]
                    e[p, case, ti, vi] = EDGE_ID[tuple(int(v) for v in corners[hi] - corners[lo])]
    return n, off, e, corners


_TN, _TOFF, _TE, _ = _cell_tables()
_POP = np.array([bin(m).count("1") for m in range(128)], np.int64)


def extract(field, level, positions=None, box=None, dtype=torch.float64):
    """field (D,H,W) fp32, level a float (rounded to fp32 first, as the library takes it), positions (D,H,W,3) fp32 | None, box (2,3) | None ->
    dict(vertices, ndc, grid (V,3) `dtype`; t (V,) `dtype`; vertex_edge (V,) int64; faces (T,3) int32; count (2,) int64; node, upper (V,) int64)."""
    s32 = torch.as_tensor(field, dtype=torch.float32)
    dev = s32.device
    D, H, W = s32.shape
    HW = H * W
    lv32 = torch.tensor(float(level), dtype=torch.float32, device=dev)
    inside = s32 >= lv32                                            # NaN: outside
    mask = torch.zeros((D, H, W), dtype=torch.int64, device=dev)
    for e, (dx, dy, dz) in enumerate(EDGES):
        lo, up = inside[:D - dz, :H - dy, :W - dx], inside[dz:, dy:, dx:]
        mask[:D - dz, :H - dy, :W - dx] |= (lo != up).to(torch.int64) << e
    mask = mask.reshape(-1)
    POP = torch.from_numpy(_POP).to(dev)
    pop = POP[mask]
    vbase = torch.cumsum(pop, 0) - pop
    nodes = torch.nonzero(mask)[:, 0]
    bits = (mask[nodes, None] >> torch.arange(7, device=dev)) & 1
    nn, e = torch.nonzero(bits, as_tuple=True)                      # row-major: node ascending, then edge ascending = key order
    n = nodes[nn]
    d = torch.tensor(EDGES, dtype=torch.int64, device=dev)[e]
    up = n + d[:, 0] + d[:, 1] * W + d[:, 2] * HW
    s, lv = s32.reshape(-1).to(dtype), lv32.to(dtype)
    s0, s1 = s[n], s[up]
    t = (lv - s0) / (s1 - s0)
    t = torch.where(torch.isfinite(s0) & torch.isfinite(s1), t, torch.full_like(t, 0.5))
    ijk = torch.stack((n % W, (n // W) % H, n // HW), 1).to(dtype)
    grid = ijk + t[:, None] * d.to(dtype)
    ndc = grid / torch.tensor([W - 1, H - 1, D - 1], dtype=dtype, device=dev)
    if box is not None and positions is not None:
        raise ValueError("positions and box exclude each other")
    if box is not None:
        b = torch.as_tensor(box, dtype=torch.float32).to(dev).reshape(2, 3).to(dtype)
        vertices = b[0] + ndc * (b[1] - b[0])
    elif positions is not None:
        P = torch.as_tensor(positions, dtype=torch.float32).to(dev).reshape(-1, 3).to(dtype)
        vertices = P[n] + t[:, None] * (P[up] - P[n])
    else:
        vertices = grid

    ci = inside.to(torch.int64)
    corner = lambda c: ci[c[2]:D - 1 + c[2], c[1]:H - 1 + c[1], c[0]:W - 1 + c[0]].reshape(-1)
    cases = []
    for perm in PERMS:
        c, case = [0, 0, 0], corner((0, 0, 0))
        for b, axis in enumerate(perm):
            c[axis] = 1
            case = case | corner(c) << (b + 1)
        cases.append(case)
    cases = torch.stack(cases, 1)                                   # (cells, 6)
    TN, TOFF, TE = (torch.from_numpy(a).to(dev) for a in (_TN, _TOFF, _TE))
    p6 = torch.arange(6, device=dev)
    ntri = TN[p6, cases]
    sel = torch.nonzero(ntri.sum(1))[:, 0]                          # cells with faces, ascending
    origin = torch.arange(D * H * W, device=dev).reshape(D, H, W)[:D - 1, :H - 1, :W - 1].reshape(-1)[sel]
    cs, nt = cases[sel], ntri[sel]
    off, te = TOFF[p6, cs], TE[p6, cs]                              # (M,6,2,3,3), (M,6,2,3)
    node = origin[:, None, None, None] + off[..., 0] + off[..., 1] * W + off[..., 2] * HW
    vnum = vbase[node] + POP[mask[node] & ((1 << te) - 1)]
    valid = torch.arange(2, device=dev) < nt[..., None]             # (M,6,2): row-major = cell, tetrahedron, triangle
    faces = vnum[valid].to(torch.int32).reshape(-1, 3)
    count = torch.tensor([n.numel(), faces.shape[0]], dtype=torch.int64, device=dev)
    return dict(vertices=vertices, ndc=ndc, grid=grid, t=t, vertex_edge=n * 8 + e, faces=faces, count=count, node=n, upper=up)


# ---------------------------------------------------------------- analytic fields (float64, then cast to fp32); indices [k][j][i]
def _xyz(D, H, W):
    k, j, i = np.meshgrid(np.arange(D, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return i, j, k


def sphere_field(shape=(9, 11, 13), centre=(6.2, 5.1, 3.9), radius=3.3):
    x, y, z = _xyz(*shape)
    return (radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(np.float32)


def torus_field(shape=(12, 17, 19)):
    x, y, z = _xyz(*shape)
    q = np.sqrt((x - 9.1) ** 2 + (y - 8.2) ** 2) - 5.0
    return (1.6 - np.sqrt(q ** 2 + (z - 5.4) ** 2)).astype(np.float32)


def integer_sphere_field(shape=(9, 11, 13)):
    x, y, z = _xyz(*shape)
    return (10 - ((x - 6) ** 2 + (y - 5) ** 2 + (z - 4) ** 2)).astype(np.float32)


def nonfinite_field():
    s = sphere_field()
    s[4, 5, 6], s[3, 5, 6], s[0, 0, 0] = np.nan, np.inf, -np.inf
    return s


def single_cell_field():
    s = np.zeros((2, 2, 2), np.float32)
    s[0, 0, 0] = 1.0
    return s


def spheres_field(shape, spheres):
    """max over (cx, cy, cz, radius) of radius - r: a union of spheres."""
    x, y, z = _xyz(*shape)
    s = np.full(shape, -np.inf)
    for cx, cy, cz, r in spheres:
        s = np.maximum(s, r - np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2))
    return s.astype(np.float32)


# name -> (field builder, level, V, T, closed, Euler characteristic)
CASES = {
    "sphere": (sphere_field, 0.0, 618, 1232, True, 2),
    "sphere_037": (sphere_field, 0.37, 462, 920, True, 2),
    "torus": (torus_field, 0.0, 1334, 2668, True, 0),
    "integer_sphere": (integer_sphere_field, 0.0, 614, 1224, True, 2),
    "nonfinite": (nonfinite_field, 0.0, 632, 1256, True, 4),
    "single_cell": (single_cell_field, 0.5, 7, 6, False, None),
}


def node_table(D, H, W):
    """A sheared perspective grid with coordinates of a few hundred: (D,H,W,3) fp32 node positions (right-handed, so the winding is kept)."""
    x, y, z = _xyz(D, H, W)
    depth = 200.0 + 35.0 * z
    X = (x - 0.5 * (W - 1)) * depth * 0.021 + 0.3 * y + 17.0
    Y = (y - 0.5 * (H - 1)) * depth * 0.019 - 0.2 * z - 40.0
    Z = depth + 0.7 * x
    return np.stack((X, Y, Z), -1).astype(np.float32)


BOX = np.array([[-1.3, 0.4, 2.1], [2.2, 3.9, 4.6]], np.float32)


# ---------------------------------------------------------------- invariants of a closed, oriented surface
def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def surface_invariants(n_vertices, faces):
    """(closed and consistently oriented, Euler characteristic V - E + T, every vertex used) of a face list."""
    f = np.asarray(faces, np.int64)
    directed = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    code = directed[:, 0] * (n_vertices + 1) + directed[:, 1]
    rev = directed[:, 1] * (n_vertices + 1) + directed[:, 0]
    once = len(np.unique(code)) == len(code)                                            # every directed edge once ...
    paired = once and np.array_equal(np.sort(code), np.sort(rev))                       # ... and its reverse once
    und = np.sort(directed, 1)
    _, mult = np.unique(und[:, 0] * (n_vertices + 1) + und[:, 1], return_counts=True)
    closed = bool(paired and (mult == 2).all())                                         # every undirected edge in exactly two faces
    euler = n_vertices - len(mult) + len(f)
    used = len(np.unique(f)) == n_vertices
    return closed, euler, used
