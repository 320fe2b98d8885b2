"""CPU-only: the restatements of tests/cloud_refs.py pinned on cases a person can compute, against each other, and - for the host restatement
of the kernel's ring search - against the brute force, bit for bit, over the grids and the awkward inputs the GPU test uses.  Also the share of
undecided queries of the GPU test's uniform inputs (measured: 1284 of 3000 queries have a neighbour, noise 8.1e-9, 0 of 3000 undecided)."""
import numpy as np
import pytest

import cloud_refs as R

F = np.float32


def _lattice():
    """27 targets at the integer points of [0,2]^3, index (z 3 + y) 3 + x."""
    z, y, x = np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij")
    return np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(F)


def _lattice_queries():
    """-> (queries, expected dist^2, expected index): the 8 cell centres (8 corners tie at d2 = 3/4, the lowest index is the corner (i,j,k)) and the 54 edge
    midpoints (two ends tie at d2 = 1/4)."""
    q, d2, idx = [], [], []
    for k in range(2):
        for j in range(2):
            for i in range(2):
                q.append((i + .5, j + .5, k + .5)); d2.append(.75); idx.append((k * 3 + j) * 3 + i)
    for axis in range(3):
        for a in range(2):
            for b in range(3):
                for c in range(3):
                    p = [0.0, 0.0, 0.0]
                    p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = a + .5, b, c
                    lo = [int(np.floor(v)) for v in p]
                    q.append(tuple(p)); d2.append(.25); idx.append((lo[2] * 3 + lo[1]) * 3 + lo[0])
    return np.asarray(q, dtype=F), np.asarray(d2, dtype=F), np.asarray(idx, dtype=np.int32)


GRIDS = [((0, 0, 0), (2, 2, 2), 0.25), ((0, 0, 0), (2, 2, 2), 1.0), ((0, 0, 0), (2, 2, 2), 7.0), ((-3, -1, -2), (5, 4, 9), 0.6),
         ((0.5, 0.5, 0.5), (1.5, 1.5, 1.5), 0.3)]                                     # the last box is SMALLER than the cloud: points clamp into border cells


def test_integer_lattice_ties_take_the_lowest_index():
    t = _lattice()
    q, d2, idx = _lattice_queries()
    assert len(q) == 8 + 54
    d32, i32 = R.nearest32(t, q, 1.0)
    assert (i32 == idx).all() and d32.tobytes() == np.sqrt(d2).tobytes()
    d64, i64, near, second = R.nearest64(t, q, 1.0)
    assert (i64 == idx).all() and (d64 == np.sqrt(d2.astype(np.float64))).all() and (second == near).all()      # exact ties
    # the radius is inclusive and rounded in float32: sqrt(3)/2 just reaches the centres, the next float32 below does not
    r = np.sqrt(F(.75))
    assert (R.nearest32(t, q[:8], r)[1] == idx[:8]).all() if F(r) * F(r) >= F(.75) else (R.nearest32(t, q[:8], r)[1] == -1).all()
    assert (R.nearest32(t, q[:8], 0.8)[1] == -1).all() and (R.nearest32(t, q[8:], 0.5)[1] == idx[8:]).all()
    for lo, hi, cell in GRIDS:
        g_lo, g_cell, dims = R.grid_layout(lo, hi, cell)
        dg, ig = R.grid_nearest32(t, q, 1.0, g_lo, g_cell, dims)
        assert (ig == idx).all() and dg.tobytes() == d32.tobytes(), (lo, hi, cell)


def test_shuffled_repeats_still_take_the_lowest_index():
    g = np.random.default_rng(3)
    base = g.uniform(0, 1, (40, 3)).astype(F)
    order = g.permutation(120)
    t = np.tile(base, (3, 1))[order]                                                 # every target three times, shuffled
    q = g.uniform(-.2, 1.2, (60, 3)).astype(F)
    d, i = R.nearest32(t, q, 0.3)
    found = i >= 0
    assert found.sum() > 20 and (~found).sum() > 3
    for n in np.nonzero(found)[0]:
        same = np.nonzero((t == t[i[n]]).all(axis=1))[0]
        assert len(same) == 3 and i[n] == same.min()
    _, _, dims = R.grid_layout((0, 0, 0), (1, 1, 1), 0.1)
    dg, ig = R.grid_nearest32(t, q, 0.3, (0, 0, 0), 0.1, dims)
    assert dg.tobytes() == d.tobytes() and (ig == i).all()


def _awkward(seed):
    g = np.random.default_rng(seed)
    t = g.uniform(0, 1, (150, 3)).astype(F)
    t[5] = (np.nan, .5, .5); t[17] = (.2, np.inf, .1); t[33] = (-np.inf, 0, 0)       # never anyone's neighbour
    t[40:44] = (1.0, 1.0, 1.0)                                                       # on the upper faces of the computed box, and identical
    t[50] = (0.0, 0.0, 0.0)
    q = g.uniform(-.4, 1.4, (110, 3)).astype(F)
    q[0] = (np.nan, 0, 0); q[1] = (.5, .5, np.inf)
    q[2] = (1.05, 1.05, 1.05); q[3] = (3.0, .5, .5); q[4] = (-.05, .5, .5); q[5] = (.5, -40.0, .5)      # outside: nearer and farther than max_dist
    q[6] = t[70]                                                                                        # distance 0
    return t, q


@pytest.mark.parametrize("seed", [0, 1])
def test_ring_search_gives_the_brute_force_bits_for_every_grid(seed):
    t, q = _awkward(seed)
    max_dist = 0.15
    d, i = R.nearest32(t, q, max_dist)
    assert (i[:2] == -1).all() and 40 <= i[2] <= 43 and i[3] == -1 and i[5] == -1 and i[6] == 70 and d[6] == 0
    outside = ((q < 0) | (q > 1)).any(axis=1)
    assert (i[outside] >= 0).sum() >= 5 and (i[outside] < 0).sum() >= 5 and (i[~outside] >= 0).sum() >= 5
    assert not np.isin(i, (5, 17, 33)).any()
    fin = t[np.isfinite(t).all(axis=1)]
    lo, hi = fin.min(0), fin.max(0)
    for cell in (max_dist / 8, max_dist / 3, max_dist, 5 * max_dist, 10.0):
        for b_lo, b_hi in ((lo, hi), (lo - 1.5, hi + 0.7), (lo + .3, hi - .3)):      # computed, larger, smaller than the cloud
            g_lo, g_cell, dims = R.grid_layout(b_lo, b_hi, cell)
            rings = []
            dg, ig = R.grid_nearest32(t, q, max_dist, g_lo, g_cell, dims, visited=rings)
            assert dg.tobytes() == d.tobytes() and (ig == i).all(), (cell, b_lo, b_hi)
            assert max(rings) <= max(dims) + 1
    # the search really stops early on a fine grid: a query with a neighbour looks at a few rings, not at the grid
    g_lo, g_cell, dims = R.grid_layout(lo, hi, max_dist / 3)
    rings = []
    R.grid_nearest32(t, q[6:40], max_dist, g_lo, g_cell, dims, visited=rings)
    assert max(dims) >= 18 and max(rings) <= 6


def test_degenerate_grids():
    g = np.random.default_rng(5)
    q = g.uniform(-.1, 1.1, (50, 3)).astype(F)
    q[:3] = [(.55, .5, .45), (.5, .5, .5), (.5, .62, .5)]
    flat =g.uniform(0, 1, (80, 3)).astype(F)
    flat[:, 2] = 0.25                                                                # coplanar: one axis has dimension 1
    same = np.tile(np.asarray([[.5, .5, .5]], dtype=F), (30, 1))                     # all targets identical: a box of zero size
    for t in (flat, same, flat[:1], flat[:0]):
        d, i = R.nearest32(t, q, 0.2)
        if len(t):
            lo, hi = t.min(0), t.max(0)
        else:
            lo = hi = np.zeros(3, dtype=F)
        g_lo, g_cell, dims = R.grid_layout(lo, hi, 0.1)
        dg, ig = R.grid_nearest32(t, q, 0.2, g_lo, g_cell, dims)
        assert dg.tobytes() == d.tobytes() and (ig == i).all()
        if len(t) == 30:
            assert set(i.tolist()) <= {-1, 0} and (i == 0).any()
        if len(t) == 0:
            assert (i == -1).all() and np.isinf(d).all()


def test_float32_and_float64_agree_where_float64_decides():
    t, q, max_dist = R.uniform_case()
    d32, i32, d64, i64, noise, decided = R.noise_and_decided(t, q, max_dist)
    found = i32 >= 0
    print(f"uniform case: {found.sum()} of {len(q)} queries have a neighbour, noise {noise:.3e}, undecided {(~decided).sum()} of {len(q)}")
    assert found.sum() >= 300 and (~found).sum() >= 300                               # both outcomes in quantity
    assert 0 < noise < 4 * 2.0 ** -24 * max_dist                                      # a few ulps of the largest distance
    assert (~decided).mean() <= 0.01
    assert (i32[decided] == i64[decided]).all()
    both = np.isfinite(d32) & np.isfinite(d64)
    assert (np.isfinite(d32) == np.isfinite(d64))[decided].all() and np.abs(d32[both] - d64[both]).max() <= noise


def test_metrics_on_a_hand_case():
    dp = np.asarray([0.5, 1.0, np.inf, 2.0], dtype=F)
    dg = np.asarray([np.inf, np.inf], dtype=F)
    m = R.metrics64(dp, dg, (1.0, 2.5))
    assert m["accuracy"] == 3.5 / 3 and m["n_accuracy"] == 3 and np.isnan(m["completeness"]) and m["n_completeness"] == 0 and np.isnan(m["overall"])
    assert m["precision"].tolist() == [0.25, 0.75] and m["recall"].tolist() == [0.0, 0.0] and m["fscore"].tolist() == [0.0, 0.0]      # strict <: 1.0 is not below 1.0
    m = R.metrics64(dp[:0], dp, (1.0,))
    assert np.isnan(m["accuracy"]) and m["precision"].tolist() == [0.0] and m["fscore"].tolist() == [0.0] and m["recall"].tolist() == [0.25]
    m = R.metrics64(dp, dp, (3.0,))
    assert m["precision"].tolist() == [0.75] and m["fscore"].tolist() == [0.75]


TRI_V = np.asarray([[0, 0, 0], [4, 0, 0], [0, 3, 0]], dtype=F)                        # a 3-4-5 right triangle: L = 5 exactly
TRI_F = np.asarray([[0, 1, 2]], dtype=np.int32)


def test_right_triangle_lattice_by_hand():
    assert R.lattice_weights(1) == [(1, 1)] and R.lattice_weights(2) == [(1, 1), (2, 2), (4, 1), (1, 4)]
    for spacing, n in ((5.0, 1), (2.5, 2), (1.25, 4), (8.0, 1), (4.99, 2)):
        for fn in (R.sample32, R.sample64):
            p, f, ns = fn(TRI_V, TRI_F, spacing)[:3]
            assert ns.tolist() == [n] and len(p) == n * n and (f == 0).all()
    p = R.sample32(TRI_V, TRI_F, 5.0)[0]
    assert p.dtype == F and p.tobytes() == np.asarray([[F(4) / F(3), 1, 0]], dtype=F).tobytes()
    # n = 2: the centroids of (0,0)(2,0)(0,1.5) | (2,0)(2,1.5)(0,1.5) | (2,0)(4,0)(2,1.5) | (0,1.5)(2,1.5)(0,3)
    want = np.asarray([[2 / 3, .5, 0], [4 / 3, 1, 0], [8 / 3, .5, 0], [2 / 3, 2, 0]])
    assert np.abs(R.sample64(TRI_V, TRI_F, 2.5)[0] - want).max() < 1e-15
    assert R.sample32(TRI_V, TRI_F, 2.5)[0].tobytes() == want.astype(F).tobytes()     # integer vertices: one rounding, in the division
    # n = 4: 16 distinct points, all strictly inside, their mean the triangle's centroid, every sub-triangle of one size
    p = R.sample64(TRI_V, TRI_F, 1.25)[0]
    assert len(np.unique(p.round(12), axis=0)) == 16
    assert (p[:, 0] > 0).all() and (p[:, 1] > 0).all() and (p[:, 0] / 4 + p[:, 1] / 3 < 1).all() and (p[:, 2] == 0).all()
    assert np.abs(p.mean(0) - TRI_V.astype(np.float64).mean(0)).max() < 1e-14
    assert R.sample32(TRI_V, TRI_F, 1.25)[0].tobytes() == p.astype(F).tobytes()
    assert p[0].tolist() == [1 / 3, .25, 0] and np.allclose(p[1], [2 / 3, .5, 0]) and np.allclose(p[7], [1 / 3, 1.0, 0])      # row 1 starts at s = 7


def test_output_row_to_lattice_point():
    """One thread per output point: the kernel's way from a row number to its sub-triangle gives the documented order, for every row of small n and for the
    rows around every row boundary of the largest n."""
    for n in list(range(1, 40)) + [255, 256, 257]:
        assert [R.lattice_weight_of(n, s) for s in range(n * n)] == R.lattice_weights(n), n
    n = 1024
    want = R.lattice_weights(n)
    starts = [j * (2 * n - j) for j in range(n)]
    for s in sorted({min(max(b + d, 0), n * n - 1) for b in starts for d in (-2, -1, 0, 1, 2)}):
        assert R.lattice_weight_of(n, s) == want[s], s
    wa_min = min(3 * n - wb - wc for wb, wc in want)
    assert wa_min == 1 and len(want) == n * n and len(set(want)) == n * n


def test_sampler_conventions():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [2, 0, 0], [5000, 0, 0]], dtype=F)
    f = np.asarray([[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 1], [0, 5, 2], [0, 1, 9]], dtype=np.int32)
    p, face, ns = R.sample32(v, f, 0.5)
    # face 1: a NaN vertex; face 2: collinear (zero area), n = 4; face 3: two equal vertices, n = 2; face 4: n = 10000 > 1024 refused; face 5: no such vertex
    assert ns.tolist() == [3, 0, 4, 2, 10000, 0]
    assert np.bincount(face, minlength=6).tolist() == [9, 0, 16, 4, 0, 0] and (np.diff(face) >= 0).all()
    assert (p[face == 2][:, 1:] == 0).all() and p[face == 2][:, 0].min() > 0 and p[face == 2][:, 0].max() < 2


def test_float32_and_float64_samplers_agree():
    g = np.random.default_rng(11)
    v = g.uniform(-1, 1, (40, 3)).astype(F)
    f = g.integers(0, 40, (60, 3)).astype(np.int32)
    p32, f32, n32 = R.sample32(v, f, 0.21)
    p64, f64, n64, ratio = R.sample64(v, f, 0.21)
    assert (n32 == n64).all() and (f32 == f64).all() and len(p32) == (n64 ** 2).sum() > 1000
    assert np.abs(p32 - p64).max() < 8 * 2.0 ** -24
