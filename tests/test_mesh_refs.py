"""CPU-only: the yardstick of the mesh extraction (tests/mesh_refs.py) held to what a level-set mesh must be - the pinned vertex and face
counts of the analytic cases, closed and consistently oriented surfaces of the right Euler characteristic, a positive signed volume close to the
sphere's - and the fp32 restatement (the bits the kernels must give) held to the float64 form within bounds that follow from one rounding per operation."""
import math

import numpy as np
import pytest
import torch

import mesh_refs as R

U = R.U


@pytest.fixture(scope="module")
def meshes():
    return {name: R.extract(torch.from_numpy(case[0]()), case[1]) for name, case in R.CASES.items()}


def test_the_faces_of_a_tetrahedron_follow_from_the_parity_rule():
    """Geometry, not parity: on a positively and a negatively oriented Kuhn tetrahedron every derived triangle's normal points from the inside corners to the
    outside ones, wherever the vertices sit on their edges."""
    g = np.random.default_rng(0)
    for perm in R.PERMS:
        c = [np.zeros(3)]
        for axis in perm:
            c.append(c[-1] + np.eye(3)[axis])
        c = np.array(c)
        s = R.perm_sign(perm)
        assert np.sign(np.linalg.det(c[1:] - c[0])) == s
        for case in range(16):
            ins = [k for k in range(4) if case >> k & 1]
            tris = R.tet_case_triangles(case, s)
            assert len(tris) == (0, 1, 2, 1, 0)[len(ins)]
            for tri in tris:
                for _ in range(8):
                    P = [c[a] + g.uniform(0.05, 0.95) * (c[b] - c[a]) for a, b in tri]
                    assert all((a in ins) != (b in ins) for a, b in tri)
                    outward = c[[k for k in range(4) if k not in ins]].mean(0) - c[ins].mean(0)
                    assert np.cross(P[1] - P[0], P[2] - P[0]) @ outward > 0
            if len(tris) == 2:                                      # a quad: four distinct edges, split along a shared diagonal
                assert len(set(tris[0]) | set(tris[1])) == 4 and len(set(tris[0]) & set(tris[1])) == 2


@pytest.mark.parametrize("name", list(R.CASES))
def test_pinned_counts_and_surface_invariants(meshes, name):
    _, _, V, T, closed, chi = R.CASES[name]
    m = meshes[name]
    faces, ve = m["faces"].numpy(), m["vertex_edge"].numpy()
    assert m["count"].tolist() == [V, T] and tuple(m["vertices"].shape) == (V, 3) and tuple(faces.shape) == (T, 3)
    assert faces.dtype == np.int32 and ve.dtype == np.int64 and (np.diff(ve) > 0).all()
    assert float(m["t"].min()) >= 0.0 and float(m["t"].max()) <= 1.0
    is_closed, euler, used = R.surface_invariants(V, faces)
    assert used
    assert R.signed_volume(m["grid"].numpy(), faces) > 0
    if closed:
        assert is_closed and euler == chi
    else:
        assert not is_closed


def test_float32_and_float64_agree_on_the_topology(meshes):
    for name, case in R.CASES.items():
        m32 = R.extract(torch.from_numpy(case[0]()), case[1], dtype=torch.float32)
        assert torch.equal(m32["faces"], meshes[name]["faces"]) and torch.equal(m32["vertex_edge"], meshes[name]["vertex_edge"])
        assert m32["vertices"].dtype == torch.float32 and m32["ndc"].dtype == torch.float32


def test_sphere_volume(meshes):
    m = meshes["sphere"]
    vol, want = R.signed_volume(m["grid"].numpy(), m["faces"].numpy()), 4.0 / 3.0 * math.pi * 3.3 ** 3
    print(f"sphere: mesh volume {vol:.3f}, analytic {want:.3f}, relative {vol / want - 1:+.4f}")
    assert abs(vol / want - 1) < 0.06                               # a 9 x 11 x 13 grid; chords lie inside the sphere
    inner = R.signed_volume(meshes["nonfinite"]["grid"].numpy(), meshes["nonfinite"]["faces"].numpy())
    assert 0 < inner < vol                                          # the NaN node's pocket is counted negative


def test_non_finite_ends_sit_at_the_middle(meshes):
    m = meshes["nonfinite"]
    s = torch.from_numpy(R.nonfinite_field()).reshape(-1)
    bad = ~(torch.isfinite(s[m["node"]]) & torch.isfinite(s[m["upper"]]))
    assert int(bad.sum()) > 0 and bool((m["t"][bad] == 0.5).all()) and bool(torch.isfinite(m["vertices"]).all())


@pytest.mark.parametrize("mode", ["grid", "box", "table"])
def test_float32_restatement_is_within_its_rounding_bounds(mode):
    """One rounding per operation, u = 2^-24: |t32 - t64| <= 3u (two subtractions, one division, t <= 1); a grid coordinate i + t adds one rounding of a number
    below i + 1; an interpolated coordinate P0 + t (P1 - P0) carries t's error and the subtraction's and product's roundings times |P1 - P0| and one
    rounding of the sum."""
    worst = 0.0
    for name in ("sphere", "torus", "nonfinite"):
        f = torch.from_numpy(R.CASES[name][0]())
        D, H, W = f.shape
        kw = {"grid": {}, "box": {"box": R.BOX}, "table": {"positions": R.node_table(D, H, W)}}[mode]
        a, b = R.extract(f, R.CASES[name][1], dtype=torch.float32, **kw), R.extract(f, R.CASES[name][1], **kw)
        assert float((a["t"].double() - b["t"]).abs().max()) <= 3 * U
        ijk = torch.stack((b["node"] % W, (b["node"] // W) % H, b["node"] // (H * W)), 1).double()
        assert bool(((a["grid"].double() - b["grid"]).abs() <= U * (3 + ijk + 1)).all())
        if mode == "table":
            P = torch.from_numpy(R.node_table(D, H, W)).reshape(-1, 3).double()
            P0, P1 = P[b["node"]], P[b["upper"]]
            bound = U * (4 * (P1 - P0).abs() + 2 * torch.maximum(P0.abs(), P1.abs()))
            err = (a["vertices"].double() - b["vertices"]).abs()
            assert bool((err <= bound).all())
            worst = max(worst, float((err / bound).max()))
        elif mode == "box":
            # with dg = u (3 + i + 1) the grid coordinate's bound and n the divisor: ndc <= 1 is off by dg / n + u; size = fl(hi - lo) by u size; the
            # product by size (dg / n + u) + u size + u size; the sum adds u |lo + product| <= u (|lo| + size): size (dg / n + 4u) + u |lo| in all, first
            # order.  The bound below is that with u |lo| doubled for the second-order terms.
            lo, size = torch.from_numpy(R.BOX[0]).double(), torch.from_numpy(R.BOX[1] - R.BOX[0]).double()
            n = torch.tensor([W - 1, H - 1, D - 1]).double()
            bound = size * (U * (3 + ijk + 1) / n + 2 * U) + U * (lo.abs() + size) * 2
            assert bool(((a["vertices"].double() - b["vertices"]).abs() <= bound).all())
    if mode == "table":
        print(f"table-interpolated coordinates: worst error / bound = {worst:.3f}")


def test_a_million_random_crossing_edges_hold_the_t_bound():
    g = torch.Generator().manual_seed(1)
    s0 = torch.rand(1_000_000, generator=g) * 4 - 2
    s1 = torch.rand(1_000_000, generator=g) * 4 - 2
    lv = torch.tensor(0.25)
    cross = (s0 >= lv) != (s1 >= lv)
    s0, s1 = s0[cross], s1[cross]
    t32 = (lv - s0) / (s1 - s0)
    t64 = (lv.double() - s0.double()) / (s1.double() - s0.double())
    err = float((t32.double() - t64).abs().max())
    print(f"{int(cross.sum())} crossing edges: max |t32 - t64| = {err / U:.2f} u")
    assert err <= 3 * U and float(t32.min()) >= 0 and float(t32.max()) <= 1
