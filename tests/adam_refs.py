"""Float64 reference, ATen-order fp32 restatement, per-element error bounds and input families of the one-launch Adam step (csrc/adam.hip,
mvsnerf_amd/optim.py; test_adam_refs.py holds this file to its own conditions without a GPU, test_gpu_adam.py holds the kernel to it).

The step (header of adam.hip), on fp32 p, g, m, v with the fp32 scalars the entry forms from its doubles:
    w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2), ss = (float)step_size, e = (float)eps, bc = (float)bc2_sqrt
    m' = m + w1 (g - m)        v' = b2 v + w2 g g        p' = p - ss m' / (sqrt(v') / bc + e)
with step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) formed by the caller in double.

Notation: u = 2^-24; every fp32 operation (+, -, *, /, sqrt: all correctly rounded, in ATen on the CPU and in the kernel, which is compiled without
fast-math) returns its exact result times (1 + d), |d| <= u, or is off by at most 2^-150 where the result is subnormal.  A fused multiply-add drops
one of the roundings counted below, so a count made for separately rounded operations covers a contracted evaluation as well.

Everything here is CPU-only and deterministic (seeded CPU generators)."""
import math

import torch

U = 2.0 ** -24
TINY = 4 * 2.0 ** -149            # the absolute underflow term of every bound: at most four operations per quantity can land in the subnormals
SECOND = 1.0 + 2.0 ** -20         # (1 + u)^k - 1 <= k u (1 + 2^-20) for every k <= 16: the second-order terms of the counts below

SIZES = (1, 2, 3, 4, 5, 7, 8, 1020, 1023, 1024, 1025, 1028, 2047, 2048, 4097, 3 * 1024 + 4)
POOL = 4097                       # every input family is made at this length; a tensor of n elements takes the first n (the step is element-wise)
STEPS = (1, 2, 7, 1000, 100000)
# name -> (lr, betas, eps)
SCALAR_SETS = {
    "default": (5e-4, (0.9, 0.999), 1e-8),
    "fast": (1e-2, (0.5, 0.9), 1e-8),
    "big_eps": (1e-7, (0.9, 0.999), 1e-3),
    "no_memory": (1e-3, (0.0, 0.0), 1e-8),
    "eps0": (5e-4, (0.9, 0.999), 0.0),          # only on families without g = 0 (|g| >= 1e-15): sqrt(v') > 0, nothing divides by zero
}
FAMILIES = ("spread", "consistent", "cold")


def cases():
    """(scalar set, family) pairs: every family under every scalar set, but eps = 0 never on the family that is all g = 0, v = 0."""
    return [(s, f) for s in SCALAR_SETS for f in FAMILIES if not (s == "eps0" and f == "cold")]


def step_scalars(lr, betas, eps, step):
    """-> (step_size, beta1, beta2, eps, bc2_sqrt) as doubles, formed as torch.optim.Adam forms them (bias_correction2 ** 0.5)."""
    beta1, beta2 = betas
    return lr / (1.0 - beta1 ** step), float(beta1), float(beta2), float(eps), (1.0 - beta2 ** step) ** 0.5


def f32(x):
    """The double x rounded to fp32, as a Python float."""
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def entry_scalars(step_size, beta1, beta2, eps, bc2_sqrt):
    """The six fp32 numbers the entry hands its kernel, as doubles: 1 - beta is formed in DOUBLE and rounded once."""
    return f32(step_size), f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(eps), f32(bc2_sqrt)


def _step64(p, g, m, v, ss, w1, b2, w2, e, bc):
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    m1 = m + w1 * (g - m)
    v1 = b2 * v + w2 * g * g
    den = v1.sqrt() / bc + e
    return m1, v1, p - ss * m1 / den


def step_f64(p, g, m, v, step_size, beta1, beta2, eps, bc2_sqrt):
    """-> (m', v', p') float64: the update evaluated in float64 on the fp32 inputs with the entry's fp32 scalars."""
    return _step64(p, g, m, v, *entry_scalars(step_size, beta1, beta2, eps, bc2_sqrt))


def step_aten_f32(p, g, m, v, step_size, beta1, beta2, eps, bc2_sqrt):
    """-> (m', v', p') fp32: torch.optim.Adam's single-tensor step, ATen's operations in ATen's order (inputs are not modified)."""
    p, m, v = p.clone(), m.clone(), v.clone()
    m.lerp_(g, 1.0 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    denom = (v.sqrt() / bc2_sqrt).add_(eps)
    p.addcdiv_(m, denom, value=-step_size)
    return m, v, p


def step_wrong_one_minus_beta(p, g, m, v, step_size, beta1, beta2, eps, bc2_sqrt):
    """The mistake the comment above the launch in adam.hip warns of: 1.0f - (float)beta, formed in fp32 (1.0f - 0.999f is 1.3e-5 off 0.001)."""
    ss, _, b2, _, e, bc = entry_scalars(step_size, beta1, beta2, eps, bc2_sqrt)
    one = torch.tensor(1.0, dtype=torch.float32)
    w1 = float(one - torch.tensor(beta1, dtype=torch.float32))
    w2 = float(one - torch.tensor(beta2, dtype=torch.float32))
    return _step64(p, g, m, v, ss, w1, b2, w2, e, bc)


def step_wrong_bias_correction(p, g, m, v, step_size, beta1, beta2, eps, bc2_sqrt):
    """sqrt(v') TIMES bc2_sqrt instead of divided by it."""
    ss, w1, b2, w2, e, bc = entry_scalars(step_size, beta1, beta2, eps, bc2_sqrt)
    return _step64(p, g, m, v, ss, w1, b2, w2, e, 1.0 / bc)


def bounds(p, g, m, v, step_size, beta1, beta2, eps, bc2_sqrt):
    """-> (Bm, Bv, Bp) float64: per-element bounds on |x_fp32 - x_f64| for an fp32 evaluation of the step, v >= 0.  M, V, P: the float64 results.

    m':  d = fl(g - m), t = fl(w1 d), m^ = fl(m + t).  t = w1 (g - m)(1 + d1)(1 + d2) carries 2 u of w1 |g - m|; the sum is rounded once, on
         |m + t| <= |m| + w1 |g - m| (1 + 2 u).  Together 3 u (|m| + w1 |g - m|): relative to S_m = |m| + w1 |g - m| and not to |M|, because m + t
         cancels.  ATen's other spelling for w1 >= 0.5, g - (1 - w1)(g - m) with 1 - w1 exact, has the same three roundings, (1 - w1) <= w1 there.
            Bm = 3 u S_m
    v':  fl(b2 v) carries u, fl(fl(w2 g) g) carries 2 u, and their sum, of two non-negative numbers, one more on top of the larger of the two: 3 u,
         relative to V itself as nothing cancels.
            Bv = 3 u V
    p':  s = fl(sqrt(v^)) = sqrt(V)(1 + 3 u)^(1/2)(1 + u): 2.5 u.  q = fl(s / bc): 3.5 u.  den = fl(q + e), q and e non-negative: 3.5 u Q / Den + u
         relative to Den = Q + e.  num = fl(ss m^): u.  r = fl(num / den): u.  So r = ss (M + dm) / Den (1 + theta), |theta| <= (3 + 3.5 Q / Den) u,
         |dm| <= Bm, and |r - R| <= ss Bm / Den + theta ss (|M| + Bm) / Den.  p^ = fl(p - r): u |p - r| <= u |P| + u |r - R|.
            Bp = u |P| + (1 + u)(ss Bm / Den + (3 + 3.5 Q / Den) u ss (|M| + Bm) / Den)
    Each bound is multiplied by 1 + 2^-20 for the second-order terms and gets 4 x 2^-149 for results in the subnormals.  Where Den == 0 (eps = 0 and
    v' = 0) Bp is NaN or inf: the caller compares NaN with NaN there."""
    ss, w1, b2, w2, e, bc = entry_scalars(step_size, beta1, beta2, eps, bc2_sqrt)
    M, V, P = _step64(p, g, m, v, ss, w1, b2, w2, e, bc)
    g, m = g.double(), m.double()
    Bm = 3 * U * (m.abs() + w1 * (g - m).abs())
    Bv = 3 * U * V
    Q = V.sqrt() / bc
    den = Q + e
    theta = (3.0 + 3.5 * Q / den) * U
    Bp = U * P.abs() + (1.0 + U) * (abs(ss) * Bm / den + theta * abs(ss) * (M.abs() + Bm) / den)
    return Bm * SECOND + TINY, Bv * SECOND + TINY, Bp * SECOND + TINY


def shares(out, ref, bnd):
    """max over elements of |out - ref| / bound per quantity -> (share_m, share_v, share_p) as Python floats; inf where exactly one of out / ref is NaN."""
    res = []
    for o, r, b in zip(out, ref, bnd):
        o = o.double()
        both_nan = o.isnan() & r.isnan()
        s = ((o - r).abs() / b).masked_fill(both_nan, 0.0)
        s = s.masked_fill(o.isnan() ^ r.isnan(), math.inf)
        res.append(float(s.nan_to_num(nan=math.inf, posinf=math.inf).max()) if s.numel() else 0.0)
    return tuple(res)


# ------------------------------------------------------------------------------------------------------------------ input families
def _magnitudes(n, gen, lo=-12.0, hi=4.0):
    return 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * (hi - lo) + lo)


def _signs(n, gen):
    return (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).double()


def make_inputs(family, seed=0, n=POOL, g_zeros=True):
    """-> (p, g, m, v) fp32 of n elements.
    spread:     g, m (both signs) and v (non-negative) with independent per-element magnitudes over 1e-12 ... 1e4, each exactly 0 on about one element in
                sixteen (never g when g_zeros is False: the eps = 0 runs); p standard normal.
    consistent: a state a run of Adam could have reached: m = c1 g, v = c2 g^2, c in (0.5, 1.5) per element, g as in spread.
    cold:       g = 0 and v = 0 everywhere (eps > 0 only), m as in spread: the denominator is eps alone."""
    gen = torch.Generator().manual_seed(7000 + 31 * seed + FAMILIES.index(family))
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    g = _magnitudes(n, gen) * _signs(n, gen)
    if g_zeros:
        g[torch.rand(n, generator=gen) < 1 / 16] = 0.0
    if family == "spread":
        m = _magnitudes(n, gen) * _signs(n, gen)
        m[torch.rand(n, generator=gen) < 1 / 16] = 0.0
        v = _magnitudes(n, gen)
        v[torch.rand(n, generator=gen) < 1 / 16] = 0.0
    elif family == "consistent":
        m = g * (0.5 + torch.rand(n, generator=gen, dtype=torch.float64))
        v = g * g * (0.5 + torch.rand(n, generator=gen, dtype=torch.float64))
    elif family == "cold":
        m = _magnitudes(n, gen) * _signs(n, gen)
        m[torch.rand(n, generator=gen) < 1 / 16] = 0.0
        g = torch.zeros(n, dtype=torch.float64)
        v = torch.zeros(n, dtype=torch.float64)
    else:
        raise ValueError(family)
    return tuple(t.to(torch.float32).contiguous() for t in (p, g, m, v))


def case_inputs(scalar_set, family, seed=0, n=POOL):
    return make_inputs(family, seed=seed, n=n, g_zeros=SCALAR_SETS[scalar_set][2] > 0.0)
