"""CPU-only checks of tests/edge_refs.py: the float64 references, the input conditions and the bounds that test_gpu_lookup_edges.py and
test_gpu_composite_f64.py hold the HIP kernels to are exercised here against torch's fp32 emulation of the same operation, so that a broken reference
or an input family that lost its property (dyadic exactness, exact-geometry projections, the <= 1 % mask-flip cap, the key collision) fails without a GPU."""
import pytest
import torch

from tests import edge_refs as E

U = E.U


@pytest.mark.parametrize("dims", E.VOLUMES)
def test_lookup_reference_against_fp32_emulation(dims):
    vol = E.make_volume(dims, seed=sum(dims))
    M = float(vol.abs().max())
    fams = [("random", E.random_pool(sum(dims)))]
    if E.is_dyadic_volume(dims):
        fams.append(("dyadic", E.dyadic_pool(sum(dims))))
    else:
        assert dims == (7, 12, 28)
    for fam, ndc in fams:
        assert float(ndc.abs().max()) <= 2.0
        ref, S = E.lookup_ref(vol, ndc)
        em = E.lookup_emul32(vol, ndc).double()
        gs = E.lookup_gs64(vol, ndc)
        assert bool(((em - ref).abs() <= E.lookup_hard_bound(S)).all()), (dims, fam)
        assert bool((em[S == 0] == 0).all())
        if fam == "dyadic":
            assert E.chain_is_exact(ndc, dims)                                   # every step of the fp32 chain is exact
            assert float((gs - ref).abs().max()) <= 1e-12 * M                    # the emulation is not checking itself
            kn = [c for c in E.corners(ndc, dims)]
            assert any(bool(((w == 0) & ok).any()) for w, ok, _ in kn)            # exact knots: weight 0 on an in-range corner
            assert bool((S > 0).all(-1).any())
            if max(dims) >= 3:                                                    # (an axis of size 1 or 2 has no ix <= -1 or >= size for k in [-32, 96])
                assert bool((S == 0).all(-1).any())                               # samples outside, ix = -1 and ix = size exactly among them
        else:
            assert bool(((em - gs).abs() <= E.lookup_hard_bound(S) + E.lookup_coord_slack(vol)).all()), (dims, fam)


def test_dyadic_pool_holds_the_edge_product():
    pool = E.dyadic_pool(3)
    e = torch.tensor(E.EDGE_VALUES, dtype=torch.float32)
    have = {tuple(r) for r in pool.tolist()}
    assert all(tuple(r) in have for r in torch.cartesian_prod(e, e, e).tolist())
    k = pool * 64
    assert torch.equal(k, k.round()) and float(k.min()) >= -32 and float(k.max()) <= 96


@pytest.mark.parametrize("V", [1, 3, 5, 6])
def test_exact_geometry_projections_agree(V):
    imgs, feats, w2cs, Ks, pts = E.exact_geometry_case(V)
    H, W = imgs.shape[2:]
    ref = E.color_ref64(imgs, w2cs, Ks, pts, feats)
    for v in range(V):
        assert torch.equal(E.project32(pts, w2cs[v], Ks[v], W, H).double(), ref["grid"][:, v]), v
    g0 = ref["grid"][:, 0]
    assert bool((g0 == 1.0).any()) and bool((g0 == -1.0).any()) and bool((g0.abs() > 1).any())      # on g = +-1 exactly, and outside
    assert bool(((g0[:, 0] == 1.0) & (ref["mask"][:, 0] == 0)).any()) and bool(((g0 == 1.0 - 2.0 ** -9).any(-1) & (ref["mask"][:, 0] == 1)).any())
    o = E.oracle_colors(imgs, w2cs, Ks, pts, feats).double()
    assert bool(((o[..., :3] - ref["col"]).abs() <= 5 * U * ref["col_S"] + 1e-30).all())
    assert bool(((o[..., 3:5] - ref["feat"]).abs() <= 5 * U * ref["feat_S"] + 1e-30).all())
    assert torch.equal(o[..., 5], ref["mask"])


def test_rig_case_conditions():
    imgs, w2cs, Ks, pts = E.rig_case()
    p = pts.reshape(-1, 3)
    ref = E.color_ref64(imgs, w2cs, Ks, p)
    assert float(ref["camz"].min()) >= 0.5
    near = E.near_mask_edge(ref["grid"])
    assert int(near.sum()) <= 0.01 * near.numel()
    assert 0.05 < float(ref["mask"].mean()) < 0.95                                  # inside and outside the images
    o = E.oracle_colors(imgs, w2cs, Ks, p).double()
    bound = 5 * U * ref["col_S"] + 2 * float(imgs.abs().max()) * ref["dpix"][..., None]
    assert bool(((o[..., :3] - ref["col"]).abs() <= bound).all())
    assert torch.equal(o[..., 3][~near], ref["mask"][~near])


def test_dir_feature_reference():
    d = E.dir_cases()
    assert float(d.norm(dim=-1).min()) > 0 and abs(float(d[9].double().norm()) / 2.0 ** -20 - 1) < 1e-6
    _, w2cs, _, _ = E.rig_case()
    for R, nrm in ((None, True), (w2cs[0], True), (None, False), (w2cs[0], False)):
        ref, b = E.dir_ref64(d, R, nrm)
        assert bool(((E.dir_emul32(d, R, nrm).double() - ref).abs() <= b).all())


@pytest.mark.parametrize("N,S", E.RAY_SHAPES)
def test_ray_ordered_samples_and_scatter_reference(N, S):
    dims = E.RAY_DIMS
    g = torch.Generator().manual_seed(N * 100 + S)
    for step in E.RAY_STEPS:
        ndc = E.ray_ordered_ndc(N, S, step)
        assert ndc.shape == (N * S, 3) and float(ndc.abs().max()) <= 2.0 and E.chain_is_exact(ndc, dims)
        fx, fy, fz = E.cell_of(ndc, dims)
        same = (fx[1:] == fx[:-1]) & (fy[1:] == fy[:-1])
        handoff = same & (fz[1:] == fz[:-1] + 1)
        if step == 1.0 and S > 1:
            assert bool(handoff.view(-1)[: S - 1].all())                          # every neighbour pair inside a ray
            if N > 1 and S < 16:
                assert bool(handoff[S - 1])                                       # ... and across the boundary of rays 0 and 1
        if step == 2.0:
            assert not bool(handoff.any())
        gf = torch.randn((N * S, 8), generator=g)
        ref, sabs, nv = E.scatter_ref(ndc, gf, dims)
        em = E.scatter_emul32(ndc, gf, dims).double()
        assert bool(((em - ref).abs() <= E.scatter_atomic_bound(sabs, nv)).all())
        assert bool((em[sabs == 0] == 0).all())
    if N * S > 1:
        assert (N * S) % 4 != 0 or N == 16                                       # the last ray ends in a partial 16-lane row


def test_collision_case_has_equal_keys():
    dims, ndc = E.collision_case()
    assert dims == (3, 3, 4100) and float(ndc.abs().max()) <= 2.0
    fx, fy, fz = E.cell_of(ndc, dims)
    assert fx.tolist() == [4097, 1] * 4 and fy.tolist() == [0, 1] * 4 and fz.tolist() == [0, 1] * 4
    key = fy * 4096 + fx
    assert len(set(key.tolist())) == 1 and len(set((key + 1).tolist())) == 1      # both x corners
    dims2, ndc2 = E.collision_case(4091, 4088)                                     # the widest volume the hand-off kernel takes: no collision
    fx, fy, fz = E.cell_of(ndc2, dims2)
    assert fx.tolist() == [4088, 1] * 4 and len(set((fy * 4096 + fx).tolist())) == 2


@pytest.mark.parametrize("S", E.S_LIST)
def test_composite_reference_against_torch_fp32(S):
    worst = {}
    for white in (False, True):
        cases = [E.composite_inputs(f, N, S) for f in E.FAMILIES for N in (1, 5, 9)] + [E.zero_ray_inputs(S), E.saturated_ray_inputs(S)]
        for raw, z in cases:
            assert bool((raw[..., 3] >= 0).all())
            ref = E.composite_ref64(raw, z, white)
            sh = E.composite_shares(E.composite_forward(raw, z, white)[:6], ref)
            for k, v in sh.items():
                worst[k] = max(worst.get(k, 0.0), v)
    assert all(v <= 1.0 for v in worst.values()), worst
    raw, z = E.composite_inputs("dense", 9, S)
    a = E.composite_ref64(raw, z)["alpha"][0]
    assert bool((a.to(torch.float32) == 1.0).any())                                # a = 1 exactly in fp32
    raw, z = E.zero_ray_inputs(S)
    assert bool(torch.isnan(E.composite_ref64(raw, z)["disp"][0]).all())           # the reference's 0/0 (the kernels return 1e10)


@pytest.mark.parametrize("S", [1, 65, 300])
def test_composite_backward_yardstick_runs(S):
    for fam in ("small", "mixed", "sparse"):
        raw, z = E.composite_inputs(fam, 9, S)
        grads = E.composite_grads(9, S)
        for combo in E.GRAD_COMBOS:
            sel = {k: grads[k] for k in combo}
            t32 = E.composite_autograd(raw, z, True, sel, torch.float32)
            r = E.composite_bwd_errors(t32, raw, z, True, sel)
            assert bool(torch.isfinite(r["e"]).all()) and bool((r["e"] == r["e_torch"]).all()) and float(r["e"].max()) < 1e-3 and r["col"] <= 1.0
