"""CPU-only: tests/adam_refs.py held to its own conditions.  The ATen-order fp32 step stays inside the per-element bounds around the float64 step on
every input set (the evidence that the bounds hold for a correct fp32 evaluation); one step of CPU torch.optim.Adam has the bits of the ATen-order
restatement (so the restatement IS the optimizer); two wrong restatements break the bounds (so the bounds can fail)."""
import math

import pytest
import torch

from tests import adam_refs as A


def _scalars(scalar_set, step):
    lr, betas, eps = A.SCALAR_SETS[scalar_set]
    return A.step_scalars(lr, betas, eps, step)


def test_input_families_are_what_they_claim():
    for fam in A.FAMILIES:
        p, g, m, v = A.make_inputs(fam)
        again = A.make_inputs(fam)
        assert all(torch.equal(a, b) for a, b in zip((p, g, m, v), again)), "not deterministic"
        assert all(t.dtype == torch.float32 and t.shape == (A.POOL,) and bool(t.isfinite().all()) for t in (p, g, m, v))
        assert bool((v >= 0).all())
        if fam == "cold":
            assert bool((g == 0).all()) and bool((v == 0).all()) and bool((m != 0).any()) and bool((m == 0).any())
            continue
        nz = g[g != 0].abs()
        assert bool((g == 0).any()) and float(nz.min()) < 1e-11 and float(nz.max()) > 1e3 and float(nz.min()) >= 1e-15
        assert bool((g > 0).any()) and bool((g < 0).any())
        if fam == "spread":
            assert bool((m == 0).any()) and bool((v == 0).any()) and float(m.abs().max()) > 1e3 and float(v[v > 0].min()) < 1e-11
            assert bool(((g == 0) & (v > 0)).any()) and bool(((v == 0) & (g != 0)).any())
        else:
            k = g != 0
            assert bool(((m[k] / g[k]) > 0.49).all()) and bool(((m[k] / g[k]) < 1.51).all())
            assert bool((v[~k] == 0).all()) and bool((m[~k] == 0).all())
        p0, g0, m0, v0 = A.make_inputs(fam, g_zeros=False)
        assert bool((g0 != 0).all()) and float(g0.abs().min()) >= 1e-15
    assert ("eps0", "cold") not in A.cases() and len(A.cases()) == 14
    # every size of the list that takes another path of the kernel: scalar and quad tensors, a tail workgroup, several workgroups
    assert any(n % 4 and n > 1024 for n in A.SIZES) and any(n % 4 == 0 and n % 1024 for n in A.SIZES) and any(n % 1024 == 0 for n in A.SIZES)


def test_entry_scalars_round_one_minus_beta_from_double():
    ss, w1, b2, w2, e, bc = A.entry_scalars(*_scalars("default", 7))
    assert w2 == float(torch.tensor(0.001, dtype=torch.float32)) and b2 == float(torch.tensor(0.999, dtype=torch.float32))
    assert abs((1.0 - b2) - 0.001) > 1e-8 and abs(w2 - 0.001) < 1e-10           # 1 - (float)beta2 is another number
    assert bc == A.f32(math.sqrt(1.0 - 0.999 ** 7)) and ss == A.f32(5e-4 / (1.0 - 0.9 ** 7))


@pytest.mark.parametrize("scalar_set,family", A.cases())
def test_aten_order_fp32_step_is_inside_the_bounds(scalar_set, family):
    """share = max |ATen fp32 - float64| / bound, per quantity: <= 1 on every input set and step count."""
    worst = [0.0, 0.0, 0.0]
    for step in A.STEPS:
        sc = _scalars(scalar_set, step)
        for seed in (0, 1):
            x = A.case_inputs(scalar_set, family, seed=seed)
            ref, bnd = A.step_f64(*x, *sc), A.bounds(*x, *sc)
            assert all(bool(r.isfinite().all()) and bool(b.isfinite().all()) for r, b in zip(ref, bnd))
            sh = A.shares(A.step_aten_f32(*x, *sc), ref, bnd)
            worst = [max(a, b) for a, b in zip(worst, sh)]
    print(f"adam ATen-order fp32 vs float64, {scalar_set}/{family}: share m {worst[0]:.3f} v {worst[1]:.3f} p {worst[2]:.3f}")
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("foreach", [False, True])
@pytest.mark.parametrize("scalar_set", [s for s in A.SCALAR_SETS])
def test_cpu_torch_adam_has_the_bits_of_the_restatement(scalar_set, foreach):
    """Three steps of torch.optim.Adam on the CPU from a fresh state, every step compared bit for bit with step_aten_f32 on the state before it."""
    lr, betas, eps = A.SCALAR_SETS[scalar_set]
    for family in ("spread", "consistent"):
        p0, g0, _, _ = A.case_inputs(scalar_set, family, n=1031)
        par = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([par], lr=lr, betas=betas, eps=eps, foreach=foreach)
        m, v = torch.zeros_like(p0), torch.zeros_like(p0)
        for step in (1, 2, 3):
            g = g0 * float(step)
            want = A.step_aten_f32(par.detach(), g, m, v, *A.step_scalars(lr, betas, eps, step))
            par.grad = g.clone()
            opt.step()
            st = opt.state[par]
            assert float(st["step"]) == step
            assert torch.equal(st["exp_avg"], want[0]) and torch.equal(st["exp_avg_sq"], want[1]) and torch.equal(par.detach(), want[2]), (family, step)
            m, v = want[0], want[1]


def test_bounds_are_not_vacuous():
    for step in (1, 7):
        sc = _scalars("default", step)
        x = A.case_inputs("default", "spread")              # elements with v << g^2: there v' is (1 - beta2) g^2 and shows the weight's error in full
        ref, bnd = A.step_f64(*x, *sc), A.bounds(*x, *sc)
        sm, sv, sp = A.shares(A.step_wrong_one_minus_beta(*x, *sc), ref, bnd)
        print(f"1.0f - beta formed in fp32, step {step}: share m {sm:.3g} v {sv:.3g} p {sp:.3g}")
        assert sv > 1.0, sv
        x = A.case_inputs("default", "consistent")
        ref, bnd = A.step_f64(*x, *sc), A.bounds(*x, *sc)
        sm, sv, sp = A.shares(A.step_wrong_bias_correction(*x, *sc), ref, bnd)
        print(f"bc2_sqrt multiplied, step {step}: share m {sm:.3g} v {sv:.3g} p {sp:.3g}")
        assert sm == 0.0 and sv == 0.0 and sp > 1.0, (sm, sv, sp)
    # and the float64 step held to itself is at share 0
    assert A.shares(ref, ref, bnd) == (0.0, 0.0, 0.0)


def test_shares_treat_nan_as_equal_only_to_nan():
    r = torch.tensor([1.0, math.nan], dtype=torch.float64)
    b = torch.tensor([1.0, math.nan], dtype=torch.float64)
    assert A.shares((torch.tensor([1.5, math.nan]),), (r,), (b,)) == (0.5,)
    assert A.shares((torch.tensor([1.0, 2.0]),), (r,), (b,)) == (math.inf,)
    assert A.shares((torch.tensor([math.nan, math.nan]),), (r,), (b,)) == (math.inf,)
