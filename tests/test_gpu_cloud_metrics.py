"""GPU: the point grid, the exact nearest neighbour within a radius, the cloud scores and the mesh sampler (csrc/cloud_metrics.hip) against the
restatements of tests/cloud_refs.py.

Exact means exact: `dist` bits and `index` of geometry.PointGrid.nearest equal the float32 brute force on every input below, for every grid.  Against
float64 the fixture measures, on every run, what the float32 DEFINITION loses on the uniform inputs (cloud_refs.noise_and_decided): the largest
|dist32 - dist64| is 8.1e-9 at distances up to 0.1 (half an ulp of 0.1 is 3.7e-9), and 0 of the 3000 queries are undecided at 8x that noise (bound: 1 %).
The device must stay within 4x the measured noise and agree on the index of every decided query.
For the sampler the test measures the same way on its random mesh: the float32 restatement's points are within 1.0e-7 of float64 and its L / spacing within
1.2e-6, and 0 of 60 faces are left out of the count comparison."""
import numpy as np
import pytest
import torch

import cloud_refs as R
from mvsnerf_amd import evaluate, geometry, ops

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda"


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _nearest(t, q, max_dist, **kw):
    grid = geometry.PointGrid(_t(t), max_dist, **kw)
    dist, index = grid.nearest(_t(q))
    assert dist.dtype == torch.float32 and index.dtype == torch.int32 and dist.shape == index.shape == (len(q),)
    return dist.cpu().numpy(), index.cpu().numpy(), grid


def _same(got_d, got_i, want_d, want_i, what=""):
    bad = np.nonzero((got_i != want_i) | (got_d.view(np.uint32) != want_d.view(np.uint32)))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want_i)} queries differ, first {bad[:5]}: got {got_d[bad[:5]]} {got_i[bad[:5]]}, want {want_d[bad[:5]]} {want_i[bad[:5]]}"


def _lattice_case():
    z, y, x = np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij")
    t = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(F)
    g = np.random.default_rng(2)
    base = g.integers(0, 5, (400, 3)).astype(F)
    q = base.copy()
    q[:150] += 0.5                                                                   # cell centres: eight corners tie
    q[150:, 0] += 0.5                                                                # edge midpoints along x: two ends tie
    q[300:, 0] -= 0.5
    q[300:, 1] += 0.5                                                                # ... and along y
    q[370:] += 50.0                                                                  # and some with nothing in reach
    return t, q, 1.0


def _cases():
    g = np.random.default_rng(7)
    out = {}
    out["uniform"] = R.uniform_case()
    base = g.uniform(0, 1, (800, 3)).astype(F)
    out["repeats"] = (np.tile(base, (3, 1))[g.permutation(2400)], g.uniform(-.1, 1.1, (1000, 3)).astype(F), 0.1)
    out["lattice"] = _lattice_case()
    t = g.uniform(0, 1, (1500, 3)).astype(F)
    t[5] = (np.nan, .5, .5); t[17] = (.2, np.inf, .1); t[33] = (-np.inf, 0, 0); t[700:710, 2] = np.nan
    t[40:60] = np.where(g.uniform(size=(20, 3)) < .5, F(1.0), t[40:60])              # on the upper faces of the box (and on its far corner)
    t[60] = (1.0, 1.0, 1.0); t[61] = (0.0, 0.0, 0.0)
    q = g.uniform(-.3, 1.3, (1200, 3)).astype(F)
    q[0] = (np.nan, 0, 0); q[1] = (.5, .5, np.inf); q[2] = (-np.inf, np.nan, 0)
    q[3] = (1.02, 1.02, 1.02); q[4] = (3.0, .5, .5); q[5] = (.5, -40.0, .5); q[6] = (1e30, 0, 0); q[7] = t[70]; q[8:28] = t[40:60]
    out["nonfinite_outside_faces"] = (t, q, 0.1)
    flat = g.uniform(0, 1, (1200, 3)).astype(F)
    flat[:, 1] = 0.25
    out["coplanar"] = (flat, g.uniform(0, 1, (600, 3)).astype(F) * F([1, .5, 1]), 0.12)
    one = np.asarray([[.5, .25, .75]], dtype=F)
    out["identical"] = (np.tile(one, (300, 1)), one + g.uniform(-.15, .15, (500, 3)).astype(F), 0.1)
    out["single_cell"] = (g.uniform(0, .05, (5000, 3)).astype(F), g.uniform(-.03, .08, (300, 3)).astype(F), 0.02)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_nearest_is_the_float32_brute_force(name):
    t, q, max_dist = CASES[name]
    kw = {"cell": 1.0} if name == "single_cell" else {}
    want_d, want_i = R.nearest32(t, q, max_dist)
    got_d, got_i, grid = _nearest(t, q, max_dist, **kw)
    _same(got_d, got_i, want_d, want_i, name)
    found = want_i >= 0
    assert found.sum() >= 20 and (~found).sum() >= 20, (found.sum(), (~found).sum())   # both outcomes occur
    if name == "uniform":
        assert found.sum() >= 300 and (~found).sum() >= 300
    if name == "single_cell":
        assert grid.dims == (1, 1, 1) and int(grid.cell_start[-1]) == 5000
    if name == "coplanar":
        assert grid.dims[1] == 1
    if name == "nonfinite_outside_faces":
        assert int(grid.cell_start[-1]) == 1500 - 13 and not np.isin(got_i, (5, 17, 33)).any() and (got_i[:3] == -1).all() and (got_i[4:7] == -1).all()
        assert got_i[3] >= 0 and got_d[7] == 0 and (got_d[8:28] == 0).all()
    if name == "repeats":
        assert all(got_i[n] == np.nonzero((t == t[got_i[n]]).all(axis=1))[0].min() for n in np.nonzero(found)[0][:100])


@pytest.mark.parametrize("n_target", [0, 1])
@pytest.mark.parametrize("n_query", [1, 63, 65, 257])
def test_tiny_clouds(n_target, n_query):
    g = np.random.default_rng(n_query)
    t = np.full((n_target, 3), .5, dtype=F)
    q = g.uniform(.3, .7, (n_query, 3)).astype(F)
    q[0] = (.5, .5, .55)
    got_d, got_i, grid = _nearest(t, q, 0.1)
    _same(got_d, got_i, *R.nearest32(t, q, 0.1))
    assert grid.dims == (1, 1, 1) and int(grid.cell_start[-1]) == n_target
    assert got_i[0] == (0 if n_target else -1)
    assert geometry.PointGrid(_t(t), 0.1).nearest(_t(q[:0]))[0].shape == (0,)       # no query: nothing is launched


def test_results_do_not_depend_on_the_grid():
    t, q, max_dist = CASES["nonfinite_outside_faces"]
    want_d, want_i = R.nearest32(t, q, max_dist)
    fin = t[np.isfinite(t).all(axis=1)]
    lo, hi = fin.min(0), fin.max(0)
    seen = set()
    for cell in (max_dist / 8, max_dist / 3, max_dist, 5 * max_dist, 10.0, None):
        for box in (None, (lo, hi), (lo - 2.0, hi + 0.7), (lo + 0.3, hi - 0.3)):       # computed, the same given, larger, SMALLER than the cloud
            got_d, got_i, grid = _nearest(t, q, max_dist, cell=cell, box=box)
            _same(got_d, got_i, want_d, want_i, f"cell {cell} box {box}")
            seen.add(grid.dims)
    assert (1, 1, 1) in seen and max(max(d) for d in seen) >= 80 and len(seen) >= 12
    # two builds, two queries: identical bytes (the order inside a cell may differ, no output may)
    a = _nearest(t, q, max_dist)
    b = _nearest(t, q, max_dist)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and torch.equal(a[2].cell_start, b[2].cell_start)
    d2, i2 = a[2].nearest(_t(q))
    assert d2.cpu().numpy().tobytes() == a[0].tobytes() and i2.cpu().numpy().tobytes() == a[1].tobytes()
    # the records are the finite rows, each once, in their cells
    rec = a[2].records[:int(a[2].cell_start[-1])].cpu().numpy()
    idx = rec[:, 3].copy().view(np.int32)
    assert sorted(idx.tolist()) == np.nonzero(np.isfinite(t).all(axis=1))[0].tolist() and rec[:, :3].tobytes() == t[idx].tobytes()
    # the cell table is capped by growing the edge
    grid = geometry.PointGrid(_t(t), max_dist, cell=1e-4)
    assert np.prod(grid.dims) <= geometry.GRID_CELL_CAP and grid.cell > 1e-4
    _same(*(x.cpu().numpy() for x in grid.nearest(_t(q))), want_d, want_i, "capped")


def test_cell_start_where_the_top_scan_owns_runs_of_two():
    """128 x 128 x 129 = 2113536 cells: the cells + 1 counts make 1033 scan workgroups of 2048 entries, so the 1024 threads of the one-workgroup scan over
    their sums (in place; csrc/scan_dev.h) own runs of c = 2 and threads 517..1023 own nothing.  Integers throughout: compared exactly."""
    dims = (128, 128, 129)
    cells = dims[0] * dims[1] * dims[2]
    assert (cells + 1 + 2047) // 2048 == 1033
    g = np.random.default_rng(129)
    t = g.uniform(-0.02, 1.02, (5000, 3)).astype(F)                                  # some rows outside the box: they land in its border cells
    t[::97, g.integers(0, 3)] = np.nan
    t[5] = (np.inf, 0.5, 0.5)
    lo, cell = np.zeros(3, dtype=F), F(1.0 / 128)
    ref = R.grid_build(t, lo, cell, dims)
    ids = torch.tensor([c for c, rows in ref.items() for _ in rows], dtype=torch.int64)
    n_finite = int(np.isfinite(t).all(axis=1).sum())
    assert len(ids) == n_finite and 4900 < n_finite < 5000 and int(ids.max()) > cells - dims[0] * dims[1]      # the last z-layer is used
    counts = torch.bincount(ids, minlength=cells + 1)
    want = (torch.cumsum(counts, 0) - counts).to(torch.int32)
    cell_start, records = ops.grid_build(_t(t), lo.tolist(), float(cell), dims)
    assert cell_start.dtype == torch.int32 and cell_start.shape == (cells + 1,)
    assert torch.equal(cell_start.cpu(), want) and int(cell_start[-1]) == n_finite
    idx = records[:n_finite, 3].cpu().numpy().copy().view(np.int32)
    assert sorted(idx.tolist()) == np.nonzero(np.isfinite(t).all(axis=1))[0].tolist()


@pytest.fixture(scope="module")
def uniform():
    t, q, max_dist = CASES["uniform"]
    d32, i32, d64, i64, noise, decided = R.noise_and_decided(t, q, max_dist)
    got_d, got_i, _ = _nearest(t, q, max_dist)
    print(f"uniform: noise {noise:.3e}, undecided {(~decided).sum()} of {len(q)}")
    return dict(t=t, q=q, max_dist=max_dist, d64=d64, i64=i64, noise=noise, decided=decided, d=got_d, i=got_i)


def test_nearest_against_float64(uniform):
    u = uniform
    assert (~u["decided"]).mean() <= 0.01
    dec = u["decided"]
    assert (u["i"][dec] == u["i64"][dec]).all()
    both = np.isfinite(u["d"]) & np.isfinite(u["d64"])
    assert (np.isfinite(u["d"]) == np.isfinite(u["d64"]))[dec].all() and both.sum() >= 300
    assert np.abs(u["d"][both].astype(np.float64) - u["d64"][both]).max() <= 4 * u["noise"]


def _check_metrics(m, taus, n_pred, n_gt):
    dp, dg = m["dist_pred"].cpu().numpy(), m["dist_gt"].cpu().numpy()
    want = R.metrics64(dp, dg, taus)
    for key in ("accuracy", "completeness", "overall", "n_accuracy", "n_completeness", "precision", "recall", "fscore"):
        assert m[key].dtype == torch.float64 and m[key].is_cuda, key
    for key, n in (("accuracy", n_pred), ("completeness", n_gt)):
        got = float(m[key])
        assert (np.isnan(got) and np.isnan(want[key])) or abs(got - want[key]) <= max(n, 1) * 2.0 ** -52 * abs(want[key]), (key, got, want[key])
    ov = float(m["overall"])
    assert (np.isnan(ov) and np.isnan(want["overall"])) or abs(ov - want["overall"]) <= (n_pred + n_gt) * 2.0 ** -52 * want["overall"]
    assert float(m["n_accuracy"]) == want["n_accuracy"] and float(m["n_completeness"]) == want["n_completeness"]
    assert m["precision"].cpu().numpy().tolist() == want["precision"].tolist() and m["recall"].cpu().numpy().tolist() == want["recall"].tolist()
    assert np.abs(m["fscore"].cpu().numpy() - want["fscore"]).max() <= 4 * 2.0 ** -52
    return want


def test_metrics_against_numpy_float64(uniform):
    u = uniform
    pred, gt = _t(u["q"]), _t(u["t"])
    tie = float(u["d"][np.isfinite(u["d"])][11])                                     # a tau that IS some distance, bit for bit: that query is not below it
    taus = (0.03, tie, 0.1, 1e9)
    m = evaluate.cloud_metrics(pred, gt, u["max_dist"], taus=taus)
    assert m["dist_pred"].cpu().numpy().tobytes() == u["d"].tobytes() and m["index_pred"].cpu().numpy().tobytes() == u["i"].tobytes()
    want = _check_metrics(m, taus, len(u["q"]), len(u["t"]))
    assert 0 < want["precision"][0] < want["precision"][2] < 1 and int((m["dist_pred"] == tie).sum()) >= 1
    assert float(m["precision"][3]) == want["n_accuracy"] / len(u["q"]) and 0 < float(m["fscore"][1]) < 1
    # the same from a PointCloud-like object, and with the grids of an earlier call: the same bits
    grids = (geometry.PointGrid(gt, u["max_dist"]), geometry.PointGrid(pred, u["max_dist"], cell=0.3))
    cloud = geometry.PointCloud(pred, None, None, None, None, None, None, None, None)
    m2 = evaluate.cloud_metrics(cloud, gt, u["max_dist"], taus=taus, grids=grids)
    for key in m:
        assert m[key].cpu().numpy().tobytes() == m2[key].cpu().numpy().tobytes(), key


def test_metrics_empty_sets_and_many_workgroups():
    g = np.random.default_rng(4)
    a = _t(g.uniform(0, 1, (500, 3)).astype(F))
    empty = torch.zeros((0, 3), device=DEV)
    far = a + 50.0
    m = evaluate.cloud_metrics(empty, a, 0.1, taus=(0.05,))
    assert np.isnan(float(m["accuracy"])) and np.isnan(float(m["completeness"])) and np.isnan(float(m["overall"]))
    assert float(m["n_accuracy"]) == 0 and m["precision"].tolist() == [0.0] and m["recall"].tolist() == [0.0] and m["fscore"].tolist() == [0.0]
    assert m["dist_pred"].shape == (0,) and bool(torch.isinf(m["dist_gt"]).all()) and bool((m["index_gt"] == -1).all())
    m = evaluate.cloud_metrics(a, far, 0.1, taus=(0.05, 1e9))
    _check_metrics(m, (0.05, 1e9), 500, 500)
    assert np.isnan(float(m["accuracy"])) and m["precision"].tolist() == [0.0, 0.0] and m["fscore"].tolist() == [0.0, 0.0]
    m = evaluate.cloud_metrics(a, a, 0.1, taus=(1e-6,))
    assert float(m["accuracy"]) == 0 and m["precision"].tolist() == [1.0] and m["fscore"].tolist() == [1.0] and float(m["n_completeness"]) == 500
    # the reduction alone over several workgroups' worth of distances (8192 per workgroup), +inf and NaN among them
    d = g.uniform(0, 2, 20001).astype(F)
    d[g.integers(0, 20001, 3000)] = np.inf
    d[77] = np.nan
    taus = (0.5, float(d[5]), 2.5)
    row = ops.cloud_metrics_row(_t(d), taus).cpu().numpy()
    fin = np.isfinite(d)
    want_sum = d[fin].astype(np.float64).sum()
    assert abs(row[0] - want_sum) <= 20001 * 2.0 ** -52 * want_sum and row[1] == fin.sum()
    assert row[2:5].tolist() == [float((d < F(t)).sum()) for t in taus] and (row[5:] == 0).all()
    assert ops.cloud_metrics_row(_t(d), taus).cpu().numpy().tobytes() == row.tobytes()


def _mesh(v, f, count=None):
    return geometry.TriangleMesh(_t(v), None, _t(f, torch.int32), None, count)


def test_sample_mesh_is_the_float32_restatement():
    g = np.random.default_rng(9)
    v = g.integers(-8, 9, (120, 3)).astype(F)
    f = g.integers(0, 120, (700, 3)).astype(np.int32)                                # three workgroups of faces, degenerate ones among them
    f[3] = (5, 5, 5); f[4] = (5, 6, 5)
    for spacing in (4.0, 1.0, 0.5):
        want_p, want_f, want_n = R.sample32(v, f, spacing)
        got = geometry.sample_mesh(_mesh(v, f), spacing)
        p, face = got
        assert p.dtype == torch.float32 and face.dtype == torch.int32 and got.count.tolist() == [len(want_p), int(want_n.max())]
        assert face.cpu().numpy().tobytes() == want_f.tobytes() and p.cpu().numpy().tobytes() == want_p.tobytes(), spacing
        again = geometry.sample_mesh(_mesh(v, f), spacing)
        assert torch.equal(again.points, p) and torch.equal(again.face, face)
    assert len(want_p) > 100000 and want_n[3] == 1 and (want_f == 3).sum() == 1
    # one face, by hand: the 3-4-5 triangle of tests/test_cloud_refs.py
    v1, f1 = np.asarray([[0, 0, 0], [4, 0, 0], [0, 3, 0]], dtype=F), np.asarray([[0, 1, 2]], dtype=np.int32)
    for spacing, n in ((5.0, 1), (2.5, 2), (1.25, 4)):
        p, face = geometry.sample_mesh(_mesh(v1, f1), spacing)
        assert p.shape == (n * n, 3) and p.cpu().numpy().tobytes() == R.sample32(v1, f1, spacing)[0].tobytes()
    # a NaN vertex, a zero-area face, a vertex number outside the mesh, no face at all
    v2 = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [2, 0, 0]], dtype=F)
    f2 = np.asarray([[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 1], [0, 1, 9], [-1, 0, 1]], dtype=np.int32)
    got = geometry.sample_mesh(_mesh(v2, f2), 0.5)
    want_p, want_f, want_n = R.sample32(v2, f2, 0.5)
    assert np.bincount(want_f, minlength=6).tolist() == [9, 0, 16, 4, 0, 0]
    assert got.face.cpu().numpy().tobytes() == want_f.tobytes() and got.points.cpu().numpy().tobytes() == want_p.tobytes()
    got = geometry.sample_mesh(_mesh(v2, f2[:0]), 0.5)
    assert got.points.shape == (0, 3) and got.count.tolist() == [0, 0]
    # a mesh extracted with a capacity: rows past its counts are not read
    got = geometry.sample_mesh(_mesh(v2, f2, count=_t(np.asarray([5, 3]), torch.int64)), 0.5)
    assert got.count.tolist() == [25, 4] and got.face.cpu().numpy().tolist() == want_f[:25].tolist()


def test_sample_mesh_where_the_scan_owns_runs_of_two():
    """1024 x 256 + 300 faces: 1026 workgroup sums, so the 1024 threads of the int64 scan (csrc/scan_dev.h) own runs of c = 2 and threads 513..1023 own
    nothing.  The spacing is above every edge, so a face emits one point or none.  The float32 restatement runs once on 400 distinct faces (a face's point
    depends on its own corners alone); the mesh draws its faces from those."""
    g = np.random.default_rng(1026)
    T = 1024 * 256 + 300
    assert (T + 255) // 256 == 1026
    v = g.integers(-8, 9, (300, 3)).astype(F)                                        # edges <= 16 sqrt(3) < 28
    v[17] = (np.nan, 0, 0)
    base = g.integers(0, 300, (400, 3)).astype(np.int32)
    base[0] = (5, 5, 5); base[1] = (5, 6, 5)                                         # zero area: a point like any other
    base[2] = (0, 1, 300); base[3] = (-1, 0, 1); base[4] = (17, 1, 2)                # outside the mesh, a NaN corner: nothing
    base_p, base_f, base_n = R.sample32(v, base, 32.0)
    assert set(base_n.tolist()) == {0, 1} and base_n[:5].tolist() == [1, 1, 0, 0, 0] and len(base_p) == int(base_n.sum())
    row = np.cumsum(base_n) - base_n                                                 # the restatement's row of a base face that emits
    pick = g.integers(0, 400, T)
    pick[:256] = 2                                                                   # a workgroup that emits nothing
    keep = base_n[pick] == 1
    want_f = np.nonzero(keep)[0].astype(np.int32)
    want_p = base_p[row[pick[keep]]]
    got = geometry.sample_mesh(_mesh(v, base[pick]), 32.0)
    assert got.count.tolist() == [len(want_f), 1] and 0.9 * T < len(want_f) < T - 256
    assert torch.equal(got.face.cpu(), torch.from_numpy(want_f)) and got.points.cpu().numpy().tobytes() == want_p.tobytes()
    cut = geometry.sample_mesh(_mesh(v, base[pick]), 32.0, capacity=1000)            # the scan's total does not depend on the capacity
    assert cut.count.tolist() == got.count.tolist() and torch.equal(cut.face, got.face[:1000])


def test_sample_mesh_capacity_and_refusal():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5000, 0, 0]], dtype=F)
    f = np.asarray([[0, 1, 2], [0, 3, 2], [1, 0, 2]], dtype=np.int32)                # the middle face needs n = 10000 at spacing 0.5
    with pytest.raises(RuntimeError, match="unsupported shape.*10000 subdivisions"):
        geometry.sample_mesh(_mesh(v, f), 0.5)
    got = geometry.sample_mesh(_mesh(v, f), 0.5, capacity=64)                        # no host read: the face emits nothing and count[1] says so
    assert got.points.shape == (64, 3) and got.count.tolist() == [18, 10000]
    want_p, want_f, _ = R.sample32(v, f, 0.5)
    assert got.face[:18].cpu().numpy().tolist() == want_f.tolist() == [0] * 9 + [2] * 9 and got.points[:18].cpu().numpy().tobytes() == want_p.tobytes()
    full = geometry.sample_mesh(_mesh(v, f[::2]), 0.01)                              # n = 142: 2 x 20164 points
    assert full.count.tolist() == [2 * 142 * 142, 142]
    cut = geometry.sample_mesh(_mesh(v, f[::2]), 0.01, capacity=30000)               # the true count is above the capacity: the first rows, and the count
    assert cut.count.tolist() == full.count.tolist() and cut.points.shape == (30000, 3)
    assert torch.equal(cut.points, full.points[:30000]) and torch.equal(cut.face, full.face[:30000])
    assert geometry.sample_mesh(_mesh(v, f[::2]), 0.01, capacity=0).count.tolist() == full.count.tolist()


def test_sample_mesh_against_float64():
    g = np.random.default_rng(11)
    v = g.uniform(-1, 1, (40, 3)).astype(F)
    f = g.integers(0, 40, (60, 3)).astype(np.int32)
    spacing = 0.21
    p32, f32, n32, ratio32 = R._sample(v, f, spacing, F, 1024)
    p64, f64, n64, ratio64 = R.sample64(v, f, spacing)
    v64 = v.astype(np.float64)

    def bary(points, faces):
        out = np.empty((len(points), 3))
        for k in np.unique(faces):
            A, B, C = v64[f[k, 0]], v64[f[k, 1]], v64[f[k, 2]]
            if np.linalg.matrix_rank(np.stack([B - A, C - A])) < 2:
                out[faces == k] = np.nan                                            # a degenerate face has no barycentric coordinates
                continue
            for r in np.nonzero(faces == k)[0]:
                out[r] = R.barycentric64(points[r].astype(np.float64), A, B, C)[0]
        return out
    b64 = bary(p64, f64)
    ok = ~np.isnan(b64).any(axis=1)
    noise_b = float(np.abs(bary(p32, f32) - b64)[ok].max())                          # what the float32 definition itself loses
    noise_r = float(np.abs(ratio32 - ratio64).max())
    decided = np.abs(ratio64 - np.round(ratio64)) > noise_r
    print(f"sampler: barycentric noise {noise_b:.3e}, ratio noise {noise_r:.3e}, faces left out {(~decided).sum()} of {len(f)}")
    assert (~decided).mean() <= 0.01 and 0 < noise_b < 1e-5
    got = geometry.sample_mesh(_mesh(v, f), spacing)
    p, face = got.points.cpu().numpy(), got.face.cpu().numpy()
    per_face = np.bincount(face, minlength=len(f))
    assert (per_face[decided] == (n64 ** 2)[decided]).all()
    b = bary(p, face)
    live = ~np.isnan(b).any(axis=1)
    assert live.sum() > 1000 and b[live].min() >= -noise_b and np.abs(b[live].sum(axis=1) - 1).max() < 1e-12
    assert b[live].min() > 0.2 / (3 * n64.max())                                     # centroids: strictly inside, a third of a sub-triangle from every edge
    assert len(p) == len(p64) and np.abs(p - p64).max() <= 4 * np.abs(p32 - p64).max()


def test_chain_sphere_mesh_to_scores():
    """extract_mesh of an analytic distance field -> sample_mesh -> cloud_metrics against points on the exact sphere.  Marching tetrahedra interpolate
    linearly inside a cell, so every surface point lies within one cell diagonal of the sphere, and the nearest of the sphere's samples (0.011 apart at
    most, a tenth of the diagonal) within little more; the bound asserted is the derived one, one cell diagonal."""
    n, radius = 32, 0.6
    h = 2.0 / (n - 1)
    diag = h * 3 ** 0.5
    ax = torch.linspace(-1, 1, n, device=DEV)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    field = radius - torch.sqrt(x * x + y * y + z * z)
    mesh = geometry.extract_mesh(field, 0.0, box=((-1, -1, -1), (1, 1, 1)))
    k = np.arange(40000) + 0.5                                                       # a Fibonacci sphere: 40000 points, 4 pi r^2 / 40000 = (0.0106)^2 each
    phi, zz = k * np.pi * (3 - 5 ** 0.5), 1 - 2 * k / 40000
    rr = np.sqrt(1 - zz * zz)
    sphere = _t((radius * np.stack([rr * np.cos(phi), rr * np.sin(phi), zz], axis=1)).astype(F))
    m = evaluate.cloud_metrics(mesh, sphere, 4 * diag, taus=(diag,), spacing=h / 2)
    samples = geometry.sample_mesh(mesh, h / 2)
    assert samples.points.shape[0] == m["dist_pred"].shape[0] >= mesh.faces.shape[0] > 1000
    print(f"sphere chain: accuracy {float(m['accuracy']):.4e}, completeness {float(m['completeness']):.4e}, cell diagonal {diag:.4e}")
    assert float(m["accuracy"]) <= diag and float(m["completeness"]) <= diag and float(m["n_accuracy"]) == samples.points.shape[0]
    assert float(m["precision"][0]) == 1.0 and float(m["recall"][0]) == 1.0 and float(m["fscore"][0]) == 1.0
    r = samples.points.double().norm(dim=1)
    assert float((r - radius).abs().max()) <= diag


def test_refusals():
    import test_cloud_metrics_surface as S
    S.test_c_entries_refuse_on_the_host()                                            # every refusal of the C entries comes before a launch
    a = torch.zeros((4, 3), device=DEV)
    with pytest.raises(ValueError, match="max_dist"):
        geometry.PointGrid(a, 0.0)
    with pytest.raises(ValueError, match="float32"):
        geometry.PointGrid(a.double(), 1.0)
    with pytest.raises(ValueError, match="grid's device"):
        geometry.PointGrid(a, 1.0).nearest(torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="spacing="):
        evaluate.cloud_metrics(geometry.TriangleMesh(a, None, torch.zeros((1, 3), device=DEV, dtype=torch.int32), None, None), a, 1.0)
    with pytest.raises(RuntimeError, match="at most 8"):
        ops.cloud_metrics_row(torch.zeros((4,), device=DEV), (1.0,) * 9)
    with pytest.raises(RuntimeError, match="2\\^24 cells"):
        ops.grid_build(a, (0, 0, 0), 1.0, (4096, 4096, 2))
