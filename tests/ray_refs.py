"""Float64 references, input families and error bounds of the tests for the kernels in front of the volume: raygen_kernel (csrc/sample.hip), ray_points_kernel,
sample_pdf_kernel and ray_marcher_fine_kernel (csrc/importance.hip) and posenc_kernel (test_gpu_ray_edges.py, test_gpu_importance_f64.py; test_ray_refs.py
holds every reference, family and bound here against torch's fp32 CPU arithmetic, without a GPU).

u = 2^-24 (edge_refs.U).  Every bound stands next to its reference as an operation count times u times the magnitudes involved; the GPU tests use the same
functions and never a multiple of a kernel's own error.  Everything here is CPU-only and deterministic (seeded CPU generators)."""
import math

import torch

from tests.edge_refs import U

F32 = torch.float32
F64 = torch.float64
C1E5 = torch.tensor(1e-5, dtype=F32)          # the kernels' 1e-5f
SWITCH = float(C1E5)                          # sample_pdf's `denom < 1e-5` switch as the fp32 kernels see it


# ------------------------------------------------------------------------------------------------------------------ sample_pdf
PDF_NB = (2, 3, 64, 65, 66, 127, 129, 512)
PDF_NI = (1, 63, 64, 65, 300)
PDF_N = (1, 3, 4, 5, 257)                     # N = 5 leaves three idle waves in the last workgroup
PDF_POOL_N, PDF_POOL_NI = 257, 300
PDF_FAMILIES = ("dense", "sparse", "one-hot", "zero")


def pdf_q(w):
    """The fp32 value fl32(w + 1e-5f) the kernels normalise."""
    return w.to(F32) + C1E5


def sample_pdf_ref64(bins, q, u):
    """sample_pdf (data/ray_utils.py:96-139) in float64 on the fp32 values q = fl32(w + 1e-5f): dict of z (N,NI), C (N,nb), below / above (N,NI),
    Cb, Ca, den = Ca - Cb and width = bins_a - bins_b."""
    b, q, u = bins.double(), q.double(), u.double().contiguous()
    nb = b.shape[-1]
    pdf = q / q.sum(-1, keepdim=True)
    C = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)
    inds = torch.searchsorted(C, u, right=True)
    below, above = (inds - 1).clamp(min=0), inds.clamp(max=nb - 1)
    Cb, Ca = torch.gather(C, 1, below), torch.gather(C, 1, above)
    bb, ba = torch.gather(b, 1, below), torch.gather(b, 1, above)
    den = Ca - Cb
    t = (u - Cb) / torch.where(den < SWITCH, torch.ones_like(den), den)
    return {"z": bb + t * (ba - bb), "C": C, "below": below, "above": above, "Cb": Cb, "Ca": Ca, "den": den, "width": ba - bb}


def _near_knot(C, u, rel):
    """(N,NI) bool: u within rel * C_k of a knot C_k, k >= 1 (knot 0 is exactly 0 on both sides)."""
    u = u.double().contiguous()
    knots = C[:, 1:].contiguous()
    lo = torch.searchsorted(knots, u / (1.0 + rel), right=False)
    hi = torch.searchsorted(knots, u / (1.0 - rel), right=True)
    return hi > lo


def _near_switch(den):
    return (den - SWITCH).abs() <= 1e-3 * SWITCH


def pdf_knot_uncertainty(nb):
    """g: relative uncertainty of a cdf knot.  The row sum is formed from per-lane partial sums of ceil((nb-1)/64) terms and six butterfly steps; the
    quotient, the scan's rounding of each knot and the rounding of w + 1e-5 add one u each: (ceil((nb-1)/64) + 8) u."""
    return (math.ceil((nb - 1) / 64) + 8) * U


def sample_pdf_bound(ref, bins, u, nb):
    """-> (bound (N,NI), left_out (N,NI) bool).  With knots known to g C: the interpolation parameter t = (u - C_b) / den moves by at most 2 g C_a / den
    (below the switch the kernels divide by 1 and t < 1e-5: the whole bin width covers it), the two products and sums of bins_b + t width round to
    4 u max|bins| + 4 u width.  Left out (and counted by the callers): u within g C of a knot (the kernel may choose the neighbouring bin), and bins whose den
    lies within 1e-3 relative of the switch."""
    g = pdf_knot_uncertainty(nb)
    width, den = ref["width"], ref["den"]
    amp = torch.where(den < SWITCH, torch.ones_like(den), 2 * g * ref["Ca"] / den.clamp(min=1e-300))
    bound = width * amp + 4 * U * float(bins.abs().max()) + 4 * U * width
    return bound, _near_knot(ref["C"], u, g) | _near_switch(den)


def pdf_exact_case(nb, seed=0):
    """The exact family: bins multiples of 1/256, weights w with fl32(w + 1e-5f) = d, every d a multiple of 1/16 in [1/16, 4) except the last, which makes the
    row sum a power of two; u from {0, every knot (1.0 included), the 1/2 and 1/4 points of every bin}, every candidate used by some row.  Odd rows sum to 2^13 and
    hold bins of weight 1/16, whose pdf 2^-17 lies below the `denom < 1e-5` switch: there z(u) jumps at the upper knot, so a search that takes the bin below
    a knot instead of the one above returns another value (everywhere else z is continuous across knots).  Every sum, quotient
    and cdf entry is then exact in fp32.  -> bins (257,nb), w (257,nb-1), u (257,300), d (257,nb-1), pick (257,300): the candidate
    index behind every u (0 .. nb-1 are the knots)."""
    g = torch.Generator().manual_seed(9000 + 7 * nb + seed)
    N, NI = PDF_POOL_N, PDF_POOL_NI
    bins = torch.cumsum(torch.randint(1, 9, (N, nb), generator=g), -1).to(F64) / 256.0 - 1.0
    d = torch.randint(1, 64, (N, nb - 1), generator=g).to(F64) / 16.0
    thin = torch.rand((N, nb - 1), generator=g) < 0.25
    thin[0::2] = False
    d[thin] = 1.0 / 16.0                                              # odd rows: a quarter of the bins get pdf 2^-17 < 1e-5, below the switch (see `total`)
    head = d[:, :-1].sum(-1)
    total = 2.0 ** torch.ceil(torch.log2(head + 1.0 / 16.0))          # the smallest power of two that leaves the last weight >= 1/16 ...
    total[1::2] = 8192.0                                              # ... and 2^13 on the odd rows (head < 4 * 511)
    d[:, -1] = total - head
    assert bool((d >= 1.0 / 16.0).all())
    d32 = d.to(F32)
    w = d32 - C1E5
    for _ in range(8):                                                # one-ulp steps until the fp32 sum hits d
        s = w + C1E5
        w = torch.where(s < d32, torch.nextafter(w, torch.full_like(w, math.inf)), torch.where(s > d32, torch.nextafter(w, torch.full_like(w, -math.inf)), w))
    C = torch.cat([torch.zeros((N, 1), dtype=F64), torch.cumsum(d / total[:, None], -1)], -1)
    below_switch = (d / total[:, None]) < SWITCH                      # there t = u - C_b is not a quarter: only the knots of such bins are used
    half = torch.where(below_switch, C[:, :-1], C[:, :-1] + 0.5 * (C[:, 1:] - C[:, :-1]))
    quarter = torch.where(below_switch, C[:, 1:], C[:, :-1] + 0.25 * (C[:, 1:] - C[:, :-1]))
    cand = torch.cat([C, half, quarter], -1)                          # (N, 3 nb - 2); C[:, 0] = 0 and C[:, -1] = 1
    nc = cand.shape[1]
    perm = torch.argsort(torch.rand((N, nc), generator=g), -1)
    pick = perm[:, torch.arange(NI) % nc].contiguous()                # a shuffled walk through a row's candidates (repeats where nc < NI)
    pick[0::2, 0] = 0                                                 # u = 0 / the last knot first in a row: the NI = 1 slices hold them
    pick[1::2, 0] = nb - 1
    u = torch.gather(cand, 1, pick)
    return bins.to(F32).contiguous(), w.contiguous(), u.to(F32).contiguous(), d32, pick


def pdf_conditioned_case(family, nb, seed=0):
    """bins ascending in [2, 6) (no bin so narrow that the 4 u max|bins| term passes 1 % of it), weights of the family, u uniform with u = 0 and u = 1 - 2^-24 among them.  -> bins (257,nb), w (257,nb-1), u (257,300)."""
    g = torch.Generator().manual_seed(9500 + 13 * nb + 1000 * PDF_FAMILIES.index(family) + seed)
    N, NI = PDF_POOL_N, PDF_POOL_NI
    bins = 2.0 + 4.0 * (torch.arange(nb)[None, :] + 0.8 * torch.rand((N, nb), generator=g)) / nb      # no bin narrower than 0.2 * 4 / nb
    r = torch.rand((N, nb - 1), generator=g)
    pick = torch.rand((N, nb - 1), generator=g)
    if family == "dense":
        w = r
    elif family == "sparse":
        w = torch.where(pick < 0.7, torch.zeros_like(r), r)
    elif family == "one-hot":
        w = torch.zeros_like(r)
        w[torch.arange(N), torch.randint(0, nb - 1, (N,), generator=g)] = 1.0 + 2.0 * r[:, 0]          # one weight in [1, 3)
    else:
        w = torch.zeros_like(r)
    u = torch.rand((N, NI), generator=g)
    u[0::3, 0] = 0.0
    u[1::3, 0] = 1.0 - 2.0 ** -24
    return bins.contiguous(), w.contiguous(), u.contiguous()


def kernel_order_sum32(q):
    """The row sum as wave_sample_pdf forms it in fp32: lane l adds q[l], q[l + 64], ... in turn, then six butterfly steps (xor 32, 16, ..., 1)."""
    n = q.shape[-1]
    part = torch.zeros((*q.shape[:-1], 64), dtype=F32)
    for j0 in range(0, n, 64):
        c = q[..., j0:j0 + 64]
        part[..., : c.shape[-1]] = part[..., : c.shape[-1]] + c
    lanes = torch.arange(64)
    for dlt in (32, 16, 8, 4, 2, 1):
        part = part + part[..., lanes ^ dlt]
    return part[..., 0]


# ------------------------------------------------------------------------------------------------------------------ ray_marcher_fine
FINE_S = (3, 4, 6, 34, 66, 130, 258, 512)
FINE_NI = (1, 5, 64, 65, 512)
FINE_N = (1, 5, 64)
FINE_POOL_N, FINE_POOL_NI = 64, 512
FINE_DIMS = (9, 17, 33)                      # (D, H, W): size - 1 a power of two on every axis


def fine_is_exact_S(S):
    return ((S - 2) & (S - 3)) == 0          # S - 2 a power of two (1 included)


def fine_empty_case(S, seed=0):
    """Empty rays: all-zero density, coarse depths multiples of 1/64 in [2, 6] with repeated neighbours (z[j] == z[j+1]: the bin edge equals two coarse depths),
    u multiples of 1/(4 (S - 2)) with u = 0, u = 1, knots and repeated values.  -> density (D,H,W), ndc (64,S,3), z (64,S), u (64,512)."""
    g = torch.Generator().manual_seed(9900 + S + seed)
    N, NI = FINE_POOL_N, FINE_POOL_NI
    steps = torch.randint(0, 3, (N, S), generator=g)              # 0: a repeated depth
    steps[:, 0] = 0
    scale = 2 ** max(0, math.ceil(math.log2(float(steps.sum(-1).max()) / 256.0 + 1e-9)))      # a power of two that keeps z <= 6
    z = 2.0 + torch.cumsum(steps, -1).to(F64) / (64.0 * scale)
    k = torch.randint(0, 4 * (S - 2), (N, NI), generator=g)       # u = k / (4 (S - 2)) in [0, 1)
    k[:, 0] = 0
    k[:, 1::7] = (k[:, 1::7] // 4) * 4                            # knots
    k[:, 2::5] = k[:, 1::5][:, : k[:, 2::5].shape[1]]             # repeated u
    k[0::2, 3] = 4 * (S - 2)                                      # u = 1: the last knot
    u = k.to(F64) / (4.0 * (S - 2))
    ndc = torch.rand((N, S, 3), generator=g) * 1.1 - 0.05
    return torch.zeros(FINE_DIMS), ndc.contiguous(), z.to(F32).contiguous(), u.to(F32).contiguous()


def fine_empty_ref64(z, u):
    """sort(cat(samples64, z_vals)) of empty rays in float64: pdf weights fl32(0 + 1e-5f) each, bins the interval mid points."""
    zz = z.double()
    bins = 0.5 * (zz[:, :-1] + zz[:, 1:])
    q = C1E5.expand(z.shape[0], z.shape[1] - 2)
    ref = sample_pdf_ref64(bins, q, u)
    return torch.sort(torch.cat([ref["z"], zz], -1), -1)[0], ref


def fine_binary_case(S, seed=0):
    """Binary density: a (9,17,33) volume with values in {0, 32} (alpha exactly 0 or 1), every sample on a voxel centre of the doubly transformed coordinate,
    c = (k/(size-1) + 1)/2 with integer k from one cell below the volume to one above (k < 0 gives c < 1/2: outside, reads zero); coarse depths ascending in [2, 6),
    u uniform.  (An opaque sample 0 on a long ray makes the pdf uniform at 1/(S-2), where the bound passes 1 % of a bin: such rays stop at S = 130.)  -> density, ndc (64,S,3), z (64,S), u (64,512), sigma (64,S) the density each sample reads."""
    g = torch.Generator().manual_seed(9950 + S + seed)
    N, NI = FINE_POOL_N, FINE_POOL_NI
    D, H, W = FINE_DIMS
    dens = (torch.rand(FINE_DIMS, generator=g) < 0.12).to(F32) * 32.0
    k = torch.stack([torch.randint(-2, n + 1, (N, S), generator=g) for n in (W, H, D)], -1)       # x, y, z order of ndc
    k[:, 0, 0] = -2                                                                             # sample 0 lies outside (c < 1/2): T_excl starts at 1 ...
    op = dens.nonzero()
    vox = op[torch.randint(0, op.shape[0], (N,), generator=g)].flip(-1)                         # an opaque voxel per ray, as (x, y, z)
    k[1::4, 1:7] = vox[1::4, None]                                                              # six opaque samples in a row: T runs 1, 1e-10, ..., 1e-40, 0
    if S <= 130:
        k[3::8, 0] = vox[3::8]                                                                  # ... except here: an opaque sample 0 leaves every pdf weight <= 1e-10
    size1 = torch.tensor([W - 1, H - 1, D - 1], dtype=F64)
    ndc = ((k.to(F64) / size1 + 1.0) / 2.0).to(F32)
    inside = ((k >= 0) & (k <= torch.tensor([W - 1, H - 1, D - 1]))).all(-1)
    kc = torch.minimum(k.clamp(min=0), torch.tensor([W - 1, H - 1, D - 1]))
    sigma = torch.where(inside, dens[kc[..., 2], kc[..., 1], kc[..., 0]], torch.zeros(()))
    z = 2.0 + 4.0 * (torch.arange(S)[None, :] + 0.8 * torch.rand((N, S), generator=g)) / S        # ascending, no interval below 0.2 * 4 / S
    u = torch.rand((N, NI), generator=g)
    u[0::3, 0] = 0.0
    return dens.contiguous(), ndc.contiguous(), z.contiguous(), u.contiguous(), sigma


def fine_chain_uncertainty(S):
    """dC = (2 S + 16) u: the knot uncertainty of the whole chain (S roundings of the transmittance products and S of the sums at most, sixteen for the rest)."""
    return (2 * S + 16) * U


def fine_binary_ref64(sigma, z, u):
    """The chain of ray_marcher_fine in float64 for alpha in {0, 1}: t = fl32((1 - a) + 1e-10f), exclusive transmittance, weights a T, pdf weights w[1:-1] + 1e-5f,
    bins the mid points.  -> (sample reference dict of sample_pdf_ref64, bound (N,NI), left_out (N,NI))."""
    S = z.shape[1]
    a = (sigma > 0).to(F32)
    assert bool(((sigma == 0) | (sigma == 32.0)).all())
    t = ((1.0 - a) + torch.tensor(1e-10, dtype=F32)).double()
    T = torch.cumprod(torch.cat([torch.ones_like(t[:, :1]), t], -1), -1)[:, :-1]
    w = a.double() * T
    q = w[:, 1:-1] + float(C1E5)
    zz = z.double()
    bins = 0.5 * (zz[:, :-1] + zz[:, 1:])
    ref = sample_pdf_ref64(bins, q, u)
    dC = fine_chain_uncertainty(S)
    den = ref["den"]
    amp = torch.where(den < SWITCH, torch.full_like(den, dC), (2 * dC / den.clamp(min=1e-300)).clamp(max=1.0))
    bound = ref["width"] * amp + 48 * U
    return ref, bound, _near_knot(ref["C"], u, dC) | _near_switch(den)


def order_stat_band(zs, bound, left_out, lo_all, hi_all):
    """The kernel returns its samples sorted, so sample i cannot be paired with its reference.  If every sample obeys |z_i - ref_i| <= b_i, the k-th smallest
    kernel sample lies between the k-th smallest of ref - b and the k-th smallest of ref + b.  Left-out samples get the whole range [lo_all, hi_all]."""
    lo = torch.where(left_out, torch.full_like(zs, lo_all), zs - bound)
    hi = torch.where(left_out, torch.full_like(zs, hi_all), zs + bound)
    return torch.sort(lo, -1)[0], torch.sort(hi, -1)[0]


def remove_multiset(rows, coarse):
    """rows ascending (N, S + NI), coarse ascending (N, S): remove one occurrence of every coarse value (bit for bit) from its row.
    -> (rest (N, NI), ok (N,) bool: every coarse depth of the row was found)."""
    N, S = coarse.shape
    T = rows.shape[1]
    pos = torch.searchsorted(rows.contiguous(), coarse.contiguous(), right=False)          # first occurrence; repeated coarse values take consecutive ones
    idx = torch.arange(S).expand(N, S)
    fresh = torch.cat([torch.ones((N, 1), dtype=torch.bool), coarse[:, 1:] != coarse[:, :-1]], -1)
    pos = pos + (idx - torch.cummax(torch.where(fresh, idx, torch.zeros_like(idx)), -1)[0])
    ok = (pos < T).all(-1)
    pc = pos.clamp(max=T - 1)
    ok = ok & (torch.gather(rows, 1, pc) == coarse).all(-1)
    keep = torch.ones((N, T), dtype=torch.bool)
    keep.scatter_(1, pc, False)
    ok = ok & (keep.sum(-1) == T - S)
    order = torch.argsort((~keep).long(), dim=-1, stable=True)[:, : T - S]                       # the kept positions, in their order
    return torch.gather(rows, 1, order), ok


def fine_oracle32(dens, ndc, z, u):
    from oracle import mvsnerf_oracle as O
    rays = torch.zeros((z.shape[0], 8))
    return O.ray_marcher_fine(rays, dens, z, ndc, u)[3]


# ------------------------------------------------------------------------------------------------------------------ ray points and ray generation
class Err:
    """A float64 value with a running first-order bound on the error of the same computation in fp32: every operation adds u |result| to the errors it
    inherits.  A contracted multiply-add only removes one of those roundings.  The tests double the final figure."""

    def __init__(self, v, e=None):
        v = v if torch.is_tensor(v) else torch.tensor(float(v))
        self.v = v.double()
        self.e = torch.zeros_like(self.v) if e is None else e

    def __getitem__(self, i):
        return Err(self.v[i], self.e[i])


def _E(x):
    return x if isinstance(x, Err) else Err(x)


def _rnd(v, e):
    return Err(v, e + U * v.abs())


def e_add(a, b):
    a, b = _E(a), _E(b)
    return _rnd(a.v + b.v, a.e + b.e)


def e_sub(a, b):
    a, b = _E(a), _E(b)
    return _rnd(a.v - b.v, a.e + b.e)


def e_mul(a, b):
    a, b = _E(a), _E(b)
    return _rnd(a.v * b.v, a.e * b.v.abs() + b.e * a.v.abs())


def e_div(a, b):
    a, b = _E(a), _E(b)
    v = a.v / b.v
    return _rnd(v, (a.e + v.abs() * b.e) / b.v.abs())


def e_stack(xs, dim=-1):
    return Err(torch.stack([x.v for x in xs], dim), torch.stack([x.e for x in xs], dim))


def _dot3(x, y, z, row):
    return e_add(e_add(e_mul(x, row[0]), e_mul(y, row[1])), e_mul(z, row[2]))


def points_ref64(o, d, z):
    """o + d z: o (N,3) or (1,3), d (N,3), z (N,S), tensors or Err -> Err (N,S,3)."""
    o, d, z = _E(o), _E(d), _E(z)
    return e_stack([e_add(Err(o.v[:, None, k], o.e[:, None, k]), e_mul(Err(d.v[:, None, k], d.e[:, None, k]), z)) for k in range(3)])


def ndc_ref64(pts, w2c, K, nf, W, H, pad=0, lindisp=False):
    """get_ndc_coordinate (utils.py:112-146) of pts (Err (..., 3)): R p + t, K c, the two divisions, the depth normalisation (both forms) and the pad
    re-scale.  -> Err (..., 3)."""
    M, K = w2c.double(), K.double()
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    cam = [e_add(_dot3(x, y, z, M[i, :3]), M[i, 3]) for i in range(3)]
    q = [_dot3(cam[0], cam[1], cam[2], K[i]) for i in range(3)]
    nx = e_div(e_div(q[0], q[2]), float(W - 1))
    ny = e_div(e_div(q[1], q[2]), float(H - 1))
    near, far = float(nf[0]), float(nf[1])
    if lindisp:
        inv_near = e_div(1.0, near)
        nz = e_div(e_sub(e_div(1.0, q[2]), inv_near), e_sub(e_div(1.0, far), inv_near))
    else:
        nz = e_div(e_sub(q[2], near), e_sub(far, near))
    if pad > 0:
        Wf, Hf = W / 4.0, H / 4.0                                    # exact in fp32, and so are Wf + 2 pad and Hf + 2 pad at these sizes
        ny = e_add(e_div(e_mul(ny, Hf), Hf + 2 * pad), e_div(float(pad), Hf + 2 * pad))
        nx = e_add(e_div(e_mul(nx, Wf), Wf + 2 * pad), e_div(float(pad), Wf + 2 * pad))
    return e_stack([nx, ny, nz])


def raygen_ref64(xs, ys, Kt, c2w, nf, S, lindisp=False, t_rand=None):
    """Ray generation in float64 on the fp32 inputs: dirs = [(x-cx)/fx, (y-cy)/fy, 1] R^T, z = near (1-t) + far t (or the lindisp form) with t = i/(S-1) known
    to 2 u, the stratified jitter lo + (up - lo) t_rand, pts = o + z d.  -> dict of Err: dirs (N,3), z (N,S), pts (N,S,3)."""
    Kt, M = Kt.double(), c2w.double()
    cxd = e_div(e_sub(xs, Kt[0, 2]), Kt[0, 0])
    cyd = e_div(e_sub(ys, Kt[1, 2]), Kt[1, 1])
    dirs = e_stack([e_add(e_add(e_mul(cxd, M[i, 0]), e_mul(cyd, M[i, 1])), M[i, 2]) for i in range(3)])
    N = xs.shape[0]
    tv = torch.arange(S, dtype=F64) / max(S - 1, 1)
    t = Err(tv, 2 * U * tv)
    near, far = float(nf[0]), float(nf[1])
    omt = e_sub(1.0, t)
    if lindisp:
        z = e_div(1.0, e_add(e_mul(e_div(1.0, near), omt), e_mul(e_div(1.0, far), t)))
    else:
        z = e_add(e_mul(near, omt), e_mul(far, t))
    z = Err(z.v[None].expand(N, S).contiguous(), z.e[None].expand(N, S).contiguous())
    if t_rand is not None:
        mid = e_mul(0.5, e_add(z[:, 1:], z[:, :-1]))
        lo = Err(torch.cat([z.v[:, :1], mid.v], -1), torch.cat([z.e[:, :1], mid.e], -1))
        up = Err(torch.cat([mid.v, z.v[:, -1:]], -1), torch.cat([mid.e, z.e[:, -1:]], -1))
        z = e_add(lo, e_mul(e_sub(up, lo), t_rand))
    o = c2w[:3, 3].reshape(1, 3)
    return {"dirs": dirs, "z": z, "pts": points_ref64(o, dirs, z)}


def within(out, ref, tag=""):
    """Largest |out - ref.v| / (2 ref.e): <= 1 passes.  Where the bound is exactly zero the output must equal the reference."""
    d = (out.double() - ref.v).abs()
    b = 2 * ref.e
    return float(torch.where(b > 0, d / b.clamp(min=1e-300), torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d))).max())


RAY_SHAPES = ((1, 1), (85, 3), (255, 1), (4, 64), (128, 2), (257, 1), (1021, 1), (5, 64), (7, 3))       # N * S in {1, 255, 256, 257, 1021}, 320 and 21
REF_HW = ((2, 2), (37, 50), (64, 96))         # W_ref = 50: W_ref / 4 is fractional
GEOMETRIES = ("same", "exact", "rig")


def camera_case(geometry, ref_hw):
    """-> dict: H, W of the target image, Kt, c2w (target camera), Kr, w2c (reference camera), nf (near, far of both), ref_hw.
    same:  the reference camera IS the target camera, an axis-permuting rotation with a dyadic translation (the inverse is exact); the image is ref_hw, so
           ndc.xy must give back pixel / (W-1, H-1) and ndc.z must run from 0 to 1.
    exact: the reference camera is view 0 of edge_refs.exact_geometry_case (identity pose, power-of-two focal length), the target view 1 moved by a dyadic
           translation; a 9 x 17 target image, so ref_hw differs from it.
    rig:   the last and the first view of make_rig(64, 96) (rotated cameras)."""
    Hr, Wr = ref_hw
    if geometry == "same":
        H, W = Hr, Wr
        K = torch.tensor([[1.2 * W, 0.0, 0.5 * W], [0.0, 1.2 * W, 0.5 * H], [0.0, 0.0, 1.0]], dtype=F32)
        R = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        t = torch.tensor([0.5, -0.25, 1.0])
        c2w, w2c = torch.eye(4), torch.eye(4)
        c2w[:3, :3], c2w[:3, 3] = R, t
        w2c[:3, :3], w2c[:3, 3] = R.t(), -(R.t() @ t)
        return dict(H=H, W=W, Kt=K, c2w=c2w, Kr=K.clone(), w2c=w2c, nf=torch.tensor([2.125, 4.525]), ref_hw=ref_hw)
    if geometry == "exact":
        from tests.edge_refs import exact_geometry_case
        _, _, w2cs, Ks, _ = exact_geometry_case(2)
        c2w = torch.eye(4)
        c2w[:3, 3] = torch.tensor([0.25, -0.125, 0.5])
        return dict(H=9, W=17, Kt=Ks[1].clone(), c2w=c2w, Kr=Ks[0].clone(), w2c=w2cs[0].clone(), nf=torch.tensor([1.0, 4.0]), ref_hw=ref_hw)
    from mvsnerf_amd.synth import make_rig, pose_ref_of
    rig = make_rig(64, 96, seed=7, rot_deg=2.0)
    pose = pose_ref_of(rig)
    return dict(H=64, W=96, Kt=pose["intrinsics"][-1].contiguous(), c2w=pose["c2ws"][-1].contiguous(), Kr=pose["intrinsics"][0].contiguous(),
                w2c=pose["w2cs"][0].contiguous(), nf=rig["near_fars"][0, 0].contiguous(), ref_hw=ref_hw)


def pixel_ids(cam, N, seed=0):
    """N integer pixels of the target image: the last pixel, the first, the other two corners, then random ones."""
    g = torch.Generator().manual_seed(9100 + N + seed)
    H, W = cam["H"], cam["W"]
    xs = torch.cat([torch.tensor([W - 1, 0, W - 1, 0]), torch.randint(0, W, (N,), generator=g)])[:N]
    ys = torch.cat([torch.tensor([H - 1, 0, 0, H - 1]), torch.randint(0, H, (N,), generator=g)])[:N]
    return xs.to(F32), ys.to(F32)


def ray_points_case(cam, N, S, per_ray, seed=0):
    """Inputs of ops.ray_points on the camera pair: directions of pixel_ids (formed in fp32: any fp32 direction is a valid input), depths sorted in [near, far]
    with z = near first and z = far last (S = 1: near on even rays, far on odd ones), the origin broadcast or per ray (dyadic offsets)."""
    g = torch.Generator().manual_seed(9200 + 31 * N + S + seed)
    xs, ys = pixel_ids(cam, N, seed)
    Kt, c2w = cam["Kt"], cam["c2w"]
    d = torch.stack([(xs - Kt[0, 2]) / Kt[0, 0], (ys - Kt[1, 2]) / Kt[1, 1], torch.ones(N)], -1) @ c2w[:3, :3].t()
    near, far = cam["nf"][0], cam["nf"][1]
    z = torch.sort(near + (far - near) * torch.rand((N, S), generator=g), -1)[0].clamp(float(near), float(far))
    if S == 1:
        z[0::2, 0], z[1::2, 0] = near, far
    else:
        z[:, 0], z[:, -1] = near, far
    o = c2w[:3, 3].reshape(1, 3).clone()
    if per_ray:
        o = o + torch.randint(-8, 9, (N, 3), generator=g).to(F32) / 64.0
    return o.contiguous(), d.contiguous(), z.contiguous(), xs, ys


def ndc_oracle32(cam, pts, pad, lindisp):
    from oracle import mvsnerf_oracle as O
    Hr, Wr = cam["ref_hw"]
    return O.get_ndc_coordinate(cam["w2c"], cam["Kr"], pts, torch.tensor([Wr - 1.0, Hr - 1.0]), near=cam["nf"][0], far=cam["nf"][1], pad=pad, lindisp=lindisp)


def raygen_oracle32(cam, xs, ys, S, pad, lindisp, t_rand=None):
    """The fp32 CPU oracle's ray generation (get_rays_mvs, ray_marcher / stratified_depths, get_ndc_coordinate): pts, dirs, ndc, z."""
    from oracle import mvsnerf_oracle as O
    Kt, c2w = cam["Kt"], cam["c2w"]
    N = xs.shape[0]
    d = torch.stack([(xs - Kt[0, 2]) / Kt[0, 0], (ys - Kt[1, 2]) / Kt[1, 1], torch.ones(N)], -1) @ c2w[:3, :3].t()
    rays = torch.cat([c2w[:3, 3].expand(N, 3), d, cam["nf"][0].expand(N, 1), cam["nf"][1].expand(N, 1)], -1)
    pts, _, _, z = O.ray_marcher(rays, S, lindisp=lindisp, perturb=0 if t_rand is None else 1, perturb_rand=t_rand)
    return pts, d, ndc_oracle32(cam, pts, pad, lindisp), z


def coarse_depths32(near, far, S, lindisp, t=None):
    """near (1 - t) + far t and the lindisp form with every operation rounded, as eager torch forms them (train.ray_marcher)."""
    t = torch.linspace(0, 1, S, device=near.device) if t is None else t
    return 1 / (1 / near * (1 - t) + 1 / far * t) if lindisp else near * (1 - t) + far * t


# ------------------------------------------------------------------------------------------------------------------ positional encoding
PE_D = (1, 3, 4)
PE_L = (0, 1, 10, 16)
PE_P = (1, 63, 1021)
PE_EDGES = (0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1.5, -1.5, 2.0 ** -10, -(2.0 ** -10), 0.75, 1.0 / 64, 2.0 ** -24, 1.25)


def posenc_inputs(P, d, seed=0):
    """x (P,d): the dyadic edge values first, uniform(-1.5, 1.5) for the rest."""
    g = torch.Generator().manual_seed(9300 + 17 * P + d + seed)
    x = torch.rand((P * d,), generator=g) * 3.0 - 1.5
    e = torch.tensor(PE_EDGES, dtype=F32)
    n = min(e.shape[0], P * d)
    x[:n] = e[:n]
    return x.view(P, d).contiguous()


def posenc_ref64(x, L):
    """[x | sin(x 2^f), f-major | cos(x 2^f)] in float64; the arguments x 2^f are exact fp32 numbers.  -> (ref (P, d (1 + 2L)), args (P, d L) fp32)."""
    f = 2.0 ** torch.arange(L, dtype=F64)
    a = (x.double()[:, None, :] * f[None, :, None]).reshape(x.shape[0], -1)
    assert torch.equal(a.to(F32).double(), a)
    return torch.cat([x.double(), torch.sin(a), torch.cos(a)], -1), a.to(F32)
