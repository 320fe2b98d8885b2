"""The one-launch Adam step (csrc/adam.hip: adam_multi_kernel behind mvsnerf_adam_step_multi) and its host class (mvsnerf_amd/optim.py) against float64, per
element.  Reference, bounds and input families live in tests/adam_refs.py (test_adam_refs.py holds them to their conditions without a GPU: the ATen-order fp32 step
sits at shares of at most 0.58 / 0.65 / 1.00 of the m / v / p bounds); u = 2^-24 and the derivation of the bounds are there.  "share" = max over elements of
|kernel - float64| / bound; every assertion on a share is share <= 1, nothing looser appears in this file.

1. float64 parity through the C entry: every scalar set, step count and input family at every size of adam_refs.SIZES, one call per tensor.
2. table edges: 1 ... 200 tensors in one call (the second and third launch of the 84-tensor job table, zero-element tensors first, last, adjacent and on both sides
   of the seam) give, bit for bit, what one call per tensor gives, and those are tied to float64.
3. fences: all four tensors of every job are carved from NaN-filled arenas with one to four NaN floats between neighbours (16-byte aligned starts for sizes that
   are multiples of four - after an aligned end the gap is then four -, starts 4, 8 and 12 bytes off alignment for the others); gaps and gradients keep their bits,
   every owned element comes out finite, two runs agree.  Parts 1 and 2 run inside the same arenas and check their gaps too.
4. one element, one answer: the quad path (1024 elements) and the scalar path (the same values as the head of 1027) give the same bits.
5. mvsnerf_amd.optim.Adam against float64 and torch.optim.Adam one step at a time (torch's state is copied into ours before every step): more than 84 and more than
   168 parameters, two groups with their own scalars and a scheduler, parameters and moments that move to other storage, zero-element parameters, misaligned
   gradients and parameters, a side stream, add_param_group."""
import ctypes

import pytest
import torch

from tests import adam_refs as A
from tests.util import record_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN_BITS = 0x7FC00001


# ------------------------------------------------------------------------------------------------------------------ arenas
class Rig:
    """Jobs of the given sizes inside four NaN-filled arenas (p, g, m, v), every NaN with a payload of its own.  Job i holds the family's pool values from index
    131 i on (cyclically), so equal sizes do not repeat values."""

    def __init__(self, sizes, scalar_set="default", family="spread", seed=0):
        self.sizes = list(sizes)
        pool = A.case_inputs(scalar_set, family, seed=seed)
        self.offs, self.cpu, self.owned, self.gaps = [], [], [], []
        for k in range(4):
            offs, e = [], 0
            for i, n in enumerate(self.sizes):
                want = 0 if n % 4 == 0 else (i + k) % 3 + 1            # in floats: 16-byte aligned, or 4, 8, 12 bytes off
                off = e + 1
                while off % 4 != want:
                    off += 1
                offs.append(off)
                e = off + n
            total = e + 3
            arena = (torch.arange(total, dtype=torch.int32) % 65521 + NAN_BITS).view(torch.float32)
            assert bool(arena.isnan().all())
            idx = [(off + torch.arange(n)) for off, n in zip(offs, self.sizes)]
            owned = torch.cat(idx) if idx else torch.zeros(0, dtype=torch.long)
            src = torch.cat([(131 * i + torch.arange(n)) % A.POOL for i, n in enumerate(self.sizes)]) if idx else owned
            arena[owned] = pool[k][src]
            gap = torch.ones(total, dtype=torch.bool)
            gap[owned] = False
            assert int(gap.sum()) == total - sum(self.sizes) and bool(gap[0]) and bool(gap[-3:].all())
            self.offs.append(offs); self.cpu.append(arena); self.owned.append(owned.to(DEV)); self.gaps.append(gap.to(DEV))
        self.x = tuple(self.cpu[k][self.owned[k].cpu()] for k in range(4))          # (p, g, m, v) of all jobs, concatenated in job order

    def device(self):
        ar = [a.to(DEV) for a in self.cpu]
        assert all(a.data_ptr() % 16 == 0 for a in ar)
        return ar

    def job(self, ar, i):
        """(p, g, m, v, numel) of job i as addresses inside the device arenas `ar` (a zero-element job points at an aligned gap float: valid, and never read)."""
        return tuple(ar[k].data_ptr() + 4 * self.offs[k][i] for k in range(4)) + (self.sizes[i],)

    def reference(self, sc):
        """-> (ref, bnd): (m', v', p') float64 and their bounds over all owned elements, on the device."""
        ref, bnd = A.step_f64(*self.x, *sc), A.bounds(*self.x, *sc)
        return tuple(t.to(DEV) for t in ref), tuple(t.to(DEV) for t in bnd)

    def shares(self, ar, ref, bnd):
        out = (ar[2][self.owned[2]], ar[3][self.owned[3]], ar[0][self.owned[0]])
        return A.shares(out, ref, bnd)

    def check_fences(self, ar, before):
        """Gaps of all four arenas and the whole gradient arena keep their bits; every owned p, m, v is finite."""
        for k in range(4):
            now, was = ar[k].view(torch.int32), before[k].view(torch.int32)
            assert torch.equal(now[self.gaps[k]], was[self.gaps[k]]), f"arena {'pgmv'[k]}: a gap was written"
            if k != 1:
                assert bool(ar[k][self.owned[k]].isfinite().all()), f"arena {'pgmv'[k]}: an owned element is not finite"
        assert torch.equal(ar[1].view(torch.int32), before[1].view(torch.int32)), "the gradients were written"


def _launch(jobs, sc, expect=0):
    """mvsnerf_adam_step_multi on jobs [(p, g, m, v, numel)] (addresses), on the current stream, with tables built here as mvsnerf_amd.optim does."""
    from mvsnerf_amd import _lib
    n = len(jobs)
    arr = ctypes.c_void_p * n
    cols = [arr(*[j[c] for j in jobs]) for c in range(4)]
    numel = (ctypes.c_int64 * n)(*[j[4] for j in jobs])
    rc = _lib.lib().mvsnerf_adam_step_multi(n, *cols, numel, *sc, torch.cuda.current_stream().cuda_stream)
    assert rc == expect, rc


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _scalars(scalar_set, step):
    lr, betas, eps = A.SCALAR_SETS[scalar_set]
    return A.step_scalars(lr, betas, eps, step)


# ------------------------------------------------------------------------------------------------------------------ 1. float64 parity
@pytest.mark.parametrize("scalar_set,family", A.cases())
def test_entry_vs_float64_every_size(scalar_set, family):
    """One call per tensor at every size of A.SIZES (both paths of the kernel, tails of 1020 ... 1028 in the second workgroup, several workgroups of the scalar
    path) and every step count: |m' - M|, |v' - V|, |p' - P| <= the bounds of adam_refs.bounds, element by element; NaN exactly where float64 has NaN (nowhere,
    on these families).  Measured on the MI355X over all 14 cases: shares m 0.600, v 0.760, p 0.997 (the last is the rounding of p' itself: half a unit in
    the last place of p' is the whole bound where the update is small); the ATen-order fp32 step on the CPU sits at 0.571, 0.644, 0.999 of the same bounds."""
    rig = Rig(A.SIZES, scalar_set, family)
    worst = [0.0, 0.0, 0.0]
    for step in A.STEPS:
        sc = _scalars(scalar_set, step)
        ref, bnd = rig.reference(sc)
        assert all(bool(r.isfinite().all()) for r in ref)
        ar = rig.device()
        before = [a.clone() for a in ar]
        for i in range(len(rig.sizes)):
            _launch([rig.job(ar, i)], sc)
        torch.cuda.synchronize()
        rig.check_fences(ar, before)
        sh = rig.shares(ar, ref, bnd)
        print(f"adam kernel vs float64, {scalar_set}/{family} step {step}: share m {sh[0]:.3f} v {sh[1]:.3f} p {sh[2]:.3f}")
        worst = [max(a, b) for a, b in zip(worst, sh)]
    for q, w in zip("mvp", worst):
        record_err(f"adam_f64_share_{q}:{scalar_set}:{family}", w, tol=1.0)
    assert max(worst) <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------ 2. table edges
CYCLE = (1, 2, 0, 3, 4, 5, 0, 0, 7, 8, 1020, 1023, 1024, 0, 1025, 1028, 2047, 2048, 4097, 3 * 1024 + 4)
assert set(CYCLE) == set(A.SIZES) | {0}


def _table_sizes(n, seam_zeros):
    sizes = [CYCLE[i % len(CYCLE)] for i in range(n)]
    if seam_zeros and n > 1:
        for i in (0, n - 1, 83, 84, 167, 168):                     # first, last, and both sides of every 84-job seam
            if i < n:
                sizes[i] = 0
    return sizes


@pytest.mark.parametrize("n,seam_zeros", [(n, True) for n in (1, 83, 84, 85, 168, 169, 200)] + [(n, False) for n in (83, 84, 85, 168, 169, 200)])
def test_job_table_edges_equal_one_call_per_tensor(n, seam_zeros):
    """n tensors in ONE call against one call per tensor, bit for bit, and the latter against float64.  The sizes cycle through A.SIZES and zero (two zero-element
    tensors side by side inside the cycle); seam_zeros puts zero-element tensors first, last and at 83 | 84 and 167 | 168 (with n = 85 and 169 the last launch then
    has no workgroup at all), the other variant keeps tensors with elements on both sides of the seams."""
    sizes = _table_sizes(n, seam_zeros)
    rig = Rig(sizes, "default", "spread", seed=1)
    sc = _scalars("default", 7)
    multi, single = rig.device(), rig.device()
    before = [a.clone() for a in multi]
    _launch([rig.job(multi, i) for i in range(n)], sc)
    for i in range(n):
        _launch([rig.job(single, i)], sc)
    torch.cuda.synchronize()
    rig.check_fences(multi, before)
    rig.check_fences(single, before)
    if not _bits_equal(multi, single):
        bad = [i for i in range(n) for k in (0, 2, 3)
               if not torch.equal(multi[k][rig.offs[k][i]:rig.offs[k][i] + sizes[i]], single[k][rig.offs[k][i]:rig.offs[k][i] + sizes[i]])]
        raise AssertionError(f"jobs {sorted(set(bad))} of {n} differ from their single-tensor call")
    ref, bnd = rig.reference(sc)
    sh = rig.shares(single, ref, bnd)
    assert max(sh) <= 1.0, sh
    if sum(sizes):
        assert not _bits_equal([multi[0]], [before[0]])           # something was updated at all


# ------------------------------------------------------------------------------------------------------------------ 3. fences
@pytest.mark.parametrize("family", A.FAMILIES)
def test_fenced_arenas_keep_their_gaps_and_gradients(family):
    sizes = [0] + list(A.SIZES) + [0, 0] + list(reversed(A.SIZES)) + [0]
    rig = Rig(sizes, "default", family, seed=2)
    for k in range(4):                                             # the layout is what the test claims
        for i, n in enumerate(sizes):
            assert (rig.offs[k][i] % 4 == 0) == (n % 4 == 0)
        assert {rig.offs[k][i] % 4 for i, n in enumerate(sizes) if n % 4} == {1, 2, 3}
        ends = [0] + [o + n for o, n in zip(rig.offs[k], sizes)]
        assert all(1 <= o - e <= 4 for o, e in zip(rig.offs[k], ends))
    sc = _scalars("default", 2)
    runs = []
    for _ in range(2):
        ar = rig.device()
        before = [a.clone() for a in ar]
        _launch([rig.job(ar, i) for i in range(len(sizes))], sc)
        torch.cuda.synchronize()
        rig.check_fences(ar, before)
        runs.append(ar)
    assert _bits_equal(runs[0], runs[1]), "two runs from the same state differ"
    assert max(rig.shares(runs[0], *rig.reference(sc))) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ 4. one element, one answer
def test_quad_path_and_scalar_path_give_the_same_bits():
    """The same 1024 (p, g, m, v) as a 1024-element tensor (16-byte path) and as the head of a 1027-element tensor (the lambda `one`): the two spellings of the
    formula were compiled separately, and an element's m', v', p' must not depend on which one served it.  They did: the quad path formed
    v' = fma(beta2, v, (omb2 g) g), the scalar path rounded beta2 v on its own, and over the sizes of A.SIZES 9821 of 114940 v' and 142 p' of the scalar path
    had other bits than the same values on the quad path (m' none).  Both paths now call adam_element, with the quad path's arithmetic."""
    differ = []
    for scalar_set, family in A.cases():
        sc = _scalars(scalar_set, 7)
        x = A.case_inputs(scalar_set, family, seed=3)
        quad = [t[:1024].to(DEV).clone() for t in x]
        scal = [t[:1027].to(DEV).clone() for t in x]
        _launch([tuple(t.data_ptr() for t in quad) + (1024,)], sc)
        _launch([tuple(t.data_ptr() for t in scal) + (1027,)], sc)
        torch.cuda.synchronize()
        for k, q in ((2, "m"), (3, "v"), (0, "p")):
            if not torch.equal(quad[k], scal[k][:1024]):
                d = (quad[k].double() - scal[k][:1024].double()).abs()
                differ.append(f"{scalar_set}/{family} {q}': {int((d > 0).sum())} of 1024 differ, by up to {float(d.max()):.3g}")
    assert not differ, "\n".join(differ)


# ------------------------------------------------------------------------------------------------------------------ 5. the host class
SHAPES = [(1,), (3,), (4,), (5,), (7,), (8,), (3, 5), (4, 6), (1023,), (1024,), (1025,), (2, 3, 4, 5), (33, 5), (16, 16), (1031,), (12,)]


def _params(shapes, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    return [torch.nn.Parameter(torch.randn(sh, generator=g).to(DEV)) for sh in shapes]


def _set_grads(pa, pb, seed, skip=()):
    """The same gradient on both sides, magnitudes over many decades with exact zeros (the spread family), a fresh tensor each."""
    for i, (a, b) in enumerate(zip(pa, pb)):
        if i in skip:
            continue
        g = A.make_inputs("spread", seed=seed * 977 + i, n=max(a.numel(), 1))[1][:a.numel()].view(a.shape).to(DEV)
        a.grad, b.grad = g.clone(), g.clone()


def _step_both(pa, pb, oa, ob, tag):
    """Copies torch's parameters and moments into ours, steps both, and holds OUR result to the float64 step of the state before: share <= 1 per group.  torch's own
    result is another fp32 evaluation of the same formula with at most one rounding more (a division written as a product with a reciprocal), so it lies within
    its bound of float64 as well and |ours - torch's| <= 2 x bound.  -> worst share."""
    with torch.no_grad():
        for a, b in zip(pa, pb):
            a.copy_(b)
            if b in ob.state and a in oa.state:
                for key in ("exp_avg", "exp_avg_sq"):
                    oa.state[a][key].copy_(ob.state[b][key])
    before = {}
    for a, b in zip(pa, pb):
        if b.grad is None:
            continue
        st = ob.state.get(b, {})
        before[b] = tuple(t.detach().clone().flatten() for t in
                          (b, b.grad, st["exp_avg"] if st else torch.zeros_like(b), st["exp_avg_sq"] if st else torch.zeros_like(b)))
    oa.step()
    ob.step()
    torch.cuda.synchronize()
    worst = 0.0
    a_of = dict(zip(pb, pa))
    for ga, gb in zip(oa.param_groups, ob.param_groups):
        assert ga["lr"] == gb["lr"] and tuple(ga["betas"]) == tuple(gb["betas"]) and ga["eps"] == gb["eps"]
        by_step = {}
        for b in gb["params"]:
            if b in before:
                assert float(oa.state[a_of[b]]["step"]) == float(ob.state[b]["step"])
                by_step.setdefault(int(ob.state[b]["step"]), []).append(b)
        for step, bs in by_step.items():
            if not sum(b.numel() for b in bs):
                continue
            sc = A.step_scalars(gb["lr"], gb["betas"], gb["eps"], step)
            x = tuple(torch.cat([before[b][k] for b in bs]) for k in range(4))
            ref, bnd = A.step_f64(*x, *sc), A.bounds(*x, *sc)
            ours = tuple(torch.cat([t.detach().flatten() for t in ts]) for ts in
                         ([oa.state[a_of[b]]["exp_avg"] for b in bs], [oa.state[a_of[b]]["exp_avg_sq"] for b in bs], [a_of[b] for b in bs]))
            theirs = tuple(torch.cat([t.detach().flatten() for t in ts]) for ts in
                           ([ob.state[b]["exp_avg"] for b in bs], [ob.state[b]["exp_avg_sq"] for b in bs], bs))
            sh = A.shares(ours, ref, bnd)
            assert max(sh) <= 1.0, (tag, step, sh)
            assert max(A.shares(ours, tuple(t.double() for t in theirs), tuple(2 * b for b in bnd))) <= 1.0, (tag, step)
            worst = max(worst, *sh)
    return worst


def test_optimizer_groups_of_100_and_169_parameters():
    """More than 84 and more than 168 tensors from Python: the second and the third launch of a call, three steps."""
    from mvsnerf_amd.optim import Adam
    s100, s169 = [SHAPES[i % len(SHAPES)] for i in range(100)], [SHAPES[(i + 5) % len(SHAPES)] for i in range(169)]
    pa, pb = _params(s100 + s169), _params(s100 + s169)
    mk = lambda ps: [{"params": ps[:100]}, {"params": ps[100:]}]
    oa, ob = Adam(mk(pa), lr=5e-4), torch.optim.Adam(mk(pb), lr=5e-4)
    worst = 0.0
    for step in range(3):
        _set_grads(pa, pb, step)
        worst = max(worst, _step_both(pa, pb, oa, ob, "100+169"))
    record_err("adam_optim_f64_share:100+169", worst, tol=1.0)
    assert all(float(oa.state[a]["step"]) == 3.0 for a in pa)


def test_optimizer_two_groups_with_their_own_scalars_and_a_scheduler():
    from mvsnerf_amd.optim import Adam
    pa, pb = _params(SHAPES, 1), _params(SHAPES, 1)
    mk = lambda ps: [{"params": ps[:9], "lr": 1e-2, "betas": (0.5, 0.9), "eps": 1e-8}, {"params": ps[9:], "lr": 1e-7, "betas": (0.9, 0.999), "eps": 1e-3}]
    oa, ob = Adam(mk(pa)), torch.optim.Adam(mk(pb))
    lam = [lambda e: 0.5 ** e, lambda e: 1.0]                      # the scheduler moves the first group only
    sa, sb = torch.optim.lr_scheduler.LambdaLR(oa, lam), torch.optim.lr_scheduler.LambdaLR(ob, lam)
    for step in range(4):
        _set_grads(pa, pb, 10 + step)
        _step_both(pa, pb, oa, ob, "two groups")
        sa.step(); sb.step()
    assert oa.param_groups[0]["lr"] == 1e-2 * 0.5 ** 4 and oa.param_groups[1]["lr"] == 1e-7


def test_optimizer_follows_a_parameter_whose_data_was_replaced():
    """p.data = fresh tensor between two steps (nn.Module._apply does this for .to(...)): id(p) stays, the address changes.  The new storage is updated as torch's
    is, the old tensor keeps its bits.  (With the tables revalidated by id alone the launch wrote the old storage and left the new one as it was.)"""
    from mvsnerf_amd.optim import Adam
    pa, pb = _params(SHAPES, 2), _params(SHAPES, 2)
    oa, ob = Adam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3)
    _set_grads(pa, pb, 20)
    _step_both(pa, pb, oa, ob, "before")
    olds = {}
    for k in (0, 7, 9, 10):
        olds[k] = pa[k].data                                       # kept: the memory stays owned by this test
        pa[k].data = pa[k].data.clone()
        pb[k].data = pb[k].data.clone()
        assert pa[k].data_ptr() != olds[k].data_ptr()
    snap = {k: t.clone() for k, t in olds.items()}
    for step in (21, 22):
        _set_grads(pa, pb, step)
        _step_both(pa, pb, oa, ob, "after p.data = ...")
    for k in olds:
        assert torch.equal(olds[k], snap[k]), f"parameter {k}: the step wrote the storage the parameter no longer has"
        assert not torch.equal(pa[k].detach(), snap[k])
    assert all(float(oa.state[a]["step"]) == 3.0 for a in pa)


def test_optimizer_follows_a_replaced_moment():
    from mvsnerf_amd.optim import Adam
    pa, pb = _params(SHAPES, 3), _params(SHAPES, 3)
    oa, ob = Adam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3)
    for step in (30, 31):
        _set_grads(pa, pb, step)
        _step_both(pa, pb, oa, ob, "before")
    olds = {}
    for k, key in ((1, "exp_avg"), (7, "exp_avg"), (9, "exp_avg_sq")):
        olds[k, key] = oa.state[pa[k]][key]
        oa.state[pa[k]][key] = olds[k, key].clone()
    snap = {k: t.clone() for k, t in olds.items()}
    _set_grads(pa, pb, 32)
    _step_both(pa, pb, oa, ob, "after a replaced moment")
    for (k, key), t in olds.items():
        assert torch.equal(t, snap[k, key]), f"{key} of parameter {k}: the step wrote the replaced tensor"
        assert not torch.equal(oa.state[pa[k]][key], snap[k, key])
    assert all(float(oa.state[a]["step"]) == 3.0 for a in pa)


def test_optimizer_steps_a_zero_element_parameter():
    """torch.optim.Adam steps nn.Parameter(torch.empty(0, 3)) with a gradient and counts the step; so does the one-launch form (its data_ptr() is null: the entry
    does not look at a tensor without elements)."""
    from mvsnerf_amd.optim import Adam
    shapes = [(5,), (0, 3), (8,), (0,), (1025,)]
    pa, pb = _params(shapes, 4), _params(shapes, 4)
    oa, ob = Adam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3)
    for step in (40, 41):
        _set_grads(pa, pb, step)
        assert pa[1].grad.shape == (0, 3) and pa[1].data_ptr() == 0
        _step_both(pa, pb, oa, ob, "zero-element")
    assert [float(oa.state[a]["step"]) for a in pa] == [float(ob.state[b]["step"]) for b in pb] == [2.0] * 5
    # ... and a group that has nothing but such parameters
    e = torch.nn.Parameter(torch.empty(0, 3, device=DEV))
    oe = Adam([e], lr=1e-3)
    e.grad = torch.empty(0, 3, device=DEV)
    oe.step()
    assert float(oe.state[e]["step"]) == 1.0


def test_optimizer_copies_a_misaligned_gradient_and_leaves_it_alone():
    """A contiguous fp32 gradient that is a view 4-byte but not 16-byte aligned, numel % 4 == 0 (a bucket view): copied for the launch, the bucket keeps its bits."""
    from mvsnerf_amd.optim import Adam
    shapes = [(4, 6), (7,), (1024,), (5, 5)]
    pa, pb = _params(shapes, 5), _params(shapes, 5)
    oa, ob = Adam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3)
    for step in (50, 51):
        _set_grads(pa, pb, step)
        flats = []
        for k in (0, 2, 3):
            n = pa[k].numel()
            flat = torch.zeros(7 + n + 5, device=DEV)
            flat[7:7 + n] = pa[k].grad.flatten()
            pa[k].grad = flat[7:7 + n].view_as(pa[k])
            assert pa[k].grad.is_contiguous() and pa[k].grad.data_ptr() % 16 == 12
            flats.append((k, flat, flat.clone()))
        _step_both(pa, pb, oa, ob, "misaligned gradient")
        for k, flat, was in flats:
            assert torch.equal(flat, was) and pa[k].grad.data_ptr() == flat.data_ptr() + 28


def test_optimizer_misaligned_parameter_views():
    """What the docstring of optim.py says: a parameter that is a view off 16-byte alignment is updated in place when its size is no multiple of four, and refused
    with a RuntimeError that names the class and the reason when it is (the update cannot land in a copy)."""
    from mvsnerf_amd.optim import Adam
    base_a, base_b = torch.randn(16, generator=torch.Generator().manual_seed(6)).to(DEV), torch.randn(16, generator=torch.Generator().manual_seed(6)).to(DEV)
    pa, pb = [torch.nn.Parameter(base_a[1:8])], [torch.nn.Parameter(base_b[1:8])]
    assert pa[0].data_ptr() % 16 == 4
    oa, ob = Adam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3)
    was = base_a.clone()
    for step in (60, 61):
        _set_grads(pa, pb, step)
        _step_both(pa, pb, oa, ob, "misaligned parameter of 7")
    assert torch.equal(base_a[:1], was[:1]) and torch.equal(base_a[8:], was[8:]) and not torch.equal(base_a[1:8], was[1:8])
    bad = torch.nn.Parameter(base_a[1:9])
    ok = torch.nn.Parameter(torch.ones(8, device=DEV))
    o2 = Adam([ok, bad], lr=1e-3)
    ok.grad, bad.grad = torch.ones(8, device=DEV), torch.ones(8, device=DEV)
    was = base_a.clone()
    with pytest.raises(RuntimeError, match=r"mvsnerf_amd\.optim\.Adam: parameter 1 of group 0 .*16-byte aligned"):
        o2.step()
    torch.cuda.synchronize()
    assert torch.equal(base_a, was) and torch.equal(ok.detach(), torch.ones(8, device=DEV))        # refused before anything was launched


def test_optimizer_step_on_a_side_stream_has_the_same_bits():
    from mvsnerf_amd.optim import Adam
    res = []
    side = torch.cuda.Stream()
    for use_side in (False, True):
        pa, pb = _params(SHAPES, 7), _params(SHAPES, 7)
        oa = Adam(pa, lr=1e-3)
        for step in (70, 71):
            _set_grads(pa, pb, step)
            n = pa[7].numel()
            flat = torch.zeros(7 + n, device=DEV)
            flat[7:] = pa[7].grad.flatten()
            pa[7].grad = flat[7:].view_as(pa[7])                   # a gradient the step has to copy: the copy is made and freed on the stream of the step
            if use_side:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    oa.step()
                torch.cuda.current_stream().wait_stream(side)
                side.synchronize()
            else:
                oa.step()
        torch.cuda.synchronize()
        res.append([a.detach().clone() for a in pa] + [oa.state[a][k].clone() for a in pa for k in ("exp_avg", "exp_avg_sq")])
    assert len(res[0]) == len(res[1]) and all(torch.equal(x, y) for x, y in zip(*res))
    assert not torch.equal(res[0][0], _params(SHAPES, 7)[0].detach())


def test_optimizer_add_param_group_after_two_steps():
    from mvsnerf_amd.optim import Adam
    pa, pb = _params(SHAPES, 8), _params(SHAPES, 8)
    oa, ob = Adam(pa[:10], lr=1e-3), torch.optim.Adam(pb[:10], lr=1e-3)
    for step in (80, 81):
        _set_grads(pa[:10], pb[:10], step)
        _step_both(pa[:10], pb[:10], oa, ob, "before add_param_group")
    oa.add_param_group({"params": pa[10:], "lr": 1e-2, "betas": (0.5, 0.9)})
    ob.add_param_group({"params": pb[10:], "lr": 1e-2, "betas": (0.5, 0.9)})
    for step in (82, 83):
        _set_grads(pa, pb, step)
        _step_both(pa, pb, oa, ob, "after add_param_group")
    assert [float(oa.state[a]["step"]) for a in pa] == [4.0] * 10 + [2.0] * 6
    assert [float(ob.state[b]["step"]) for b in pb] == [4.0] * 10 + [2.0] * 6
