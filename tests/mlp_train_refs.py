"""CPU float64 references for the ray-march MLP TRAINING kernels: the fp32 and bf16 SAVE forward (csrc/mlp.hip, csrc/mlp_bf16.hip) and
mlp_dgrad_kernel / mlp_wgrad_kernel / mvsnerf_partial_sum_multi / mlp_wgrad_scatter_multi_kernel (csrc/mlp_bwd.hip).  No oracle import.

inputs(N, S, F)   tests.mlp16_refs.inputs with the features multiplied by 0.25, once, in fp32.  With the checkpoint weights the un-scaled features
                  (|x| up to 4.6) drive the pre-activations to 1e5 through the multiplicative modulation, and fp32 autograd on the CPU is then
                  1e-4 .. 3e-4 of a tensor's maximum away from float64 autograd with no ReLU flipped: a float64 bound there fails for reasons that
                  are not the kernel's.  Scaled, the pre-activations stay below about 130 and sigma > 0 holds on 40 .. 90 % of the points.
d_raw(N, S, F)    randn (N S, 4) from a seeded generator (SEEDS: a case that misses the liveness band or the dropped-share cap gets another).
network(...)      Renderer_ours (models.py:199-217) with the Embedder in a given dtype -> Net: raw, the eight ReLU arguments (pts_linears.0-5 after
                  the modulation, alpha_linear, views_linears.0), and by autograd of (raw * d_raw).sum(): d_feat (all F columns), the 22 parameter
                  gradients in ops.MLP_ORDER, and A, the abs-sums of these 22: |gp_i|^T @ |x_i| (gp_i = the gradient at linear i's output, x_i its
                  input) for a weight and sum_p |gp_i| for a bias - what a summation-order bound is relative to.
margins / keep    A point one of whose 897 ReLU arguments changes sign between fp32 and float64 has an O(1) wrong d_feat row and moves every weight
                  gradient by one point's share.  margin(point) = the smallest, over the six pts_linears stages and views_linears.0, of
                  min_units |p| / max_units |p| of that stage at that point, and |p| / (|w| . |h| + |b|) for alpha_linear.  The CPU fp32 forward is
                  off by at most 1.2e-6 (about 2^-20) in these units; keep() drops the points under tau = 2^-17, 8 x that, and masked_d_raw zeroes
                  their d_raw rows: they then contribute exactly nothing on both sides and no output element is excluded.
summation_bound   see its docstring.
case(N, S, F)     everything a test needs of one case, computed once.
"""
import collections
import functools

import torch

from tests import mlp16_refs as M
from tests.test_gpu_mlp_fold import _embed

TAU = 2.0 ** -17
U = 2.0 ** -24
FEAT_SCALE = 0.25
# (N, S, F) -> seed bump of the inputs and d_raw.  With the first draw, of 35 points: (5, 7, 12) 94 % live, (5, 7, 34) 91 % live and 26 % dropped,
# (5, 7, 32) 29 % dropped (test_mlp_train_refs.py's band is 40 .. 90 % live, at most 25 % dropped)
SEEDS = {(5, 7, 12): 1, (5, 7, 32): 1, (5, 7, 34): 1}
STAGES = [f"pts_linears.{i}" for i in range(6)] + ["alpha_linear", "views_linears.0"]

Net = collections.namedtuple("Net", "raw pre d_feat grads A margin")


def weights(F):
    return M.weights(F)


@functools.lru_cache(maxsize=None)
def inputs(N, S, F):
    """-> ndc (N, S, 3), feat (N, S, F), dirs (N, 3): fp32 CPU; the features of tests.mlp16_refs.inputs times 0.25 (an exact scaling)"""
    ndc, feat, dirs = M.inputs(N, S, F)
    bump = SEEDS.get((N, S, F), 0)
    if bump:                                             # the draws of tests/test_gpu_mlp_fold.py's _inputs from another seed
        g = torch.Generator().manual_seed(1000 * N + 10 * S + F + 100003 * bump)
        ndc = torch.rand((N, S, 3), generator=g)
        feat = torch.randn((N, S, F), generator=g)
        dirs = torch.nn.functional.normalize(torch.randn((N, 3), generator=g), dim=-1)
    return ndc.contiguous(), (feat * FEAT_SCALE).contiguous(), dirs.contiguous()


@functools.lru_cache(maxsize=None)
def d_raw(N, S, F):
    g = torch.Generator().manual_seed(910000 + 1000 * N + 10 * S + F + 100003 * SEEDS.get((N, S, F), 0))
    return torch.randn((N * S, 4), generator=g)


def network(ws, bs, ndc, feat, dirs, g_raw=None, dtype=torch.float64, with_margin=False, o_given=None):
    """Renderer_ours in `dtype` on the fp32 tensors.  g_raw None: forward only (d_feat, grads, A are None).
    o_given (N S, >= 3): never the reference - the sigmoid's derivative taken at these rgb values instead of the forward's own; in fp32 with
    the kernel's rgb it is the yardstick that carries the backward entries' documented form (tests/test_gpu_mlp_train_f64.py, _check_float64).
    grads: [w0, b0, w1, b1, ...] in ops.MLP_ORDER, A likewise; d_feat (N S, F); pre: the eight ReLU arguments, (N S, units) each."""
    lin = torch.nn.functional.linear
    N, S = ndc.shape[:2]
    P = N * S
    need = g_raw is not None
    w = [t.to(dtype).clone().requires_grad_(need) for t in ws]
    b = [t.to(dtype).clone().requires_grad_(need) for t in bs]
    x = feat.to(dtype).reshape(P, -1).clone().requires_grad_(need)
    outs, xin = [None] * 11, [None] * 11

    def L(i, h):
        xin[i] = h
        outs[i] = lin(h, w[i], b[i])
        if need:
            outs[i].retain_grad()
        return outs[i]

    pts = _embed(ndc.to(dtype)).reshape(P, -1)
    bias = L(6, x)
    h = pts
    pre = []
    for i in range(6):
        p = L(i, h) * bias
        pre.append(p)
        h = torch.relu(p)
        if i == 4:
            h = torch.cat([pts, h], -1)
    p_alpha = L(8, h)
    sigma = torch.relu(p_alpha)
    d = dirs.to(dtype)[:, None, :].expand(N, S, 3).reshape(P, 3)
    p_views = L(9, torch.cat([L(7, h), d], -1))
    rgb = torch.sigmoid(L(10, torch.relu(p_views)))
    raw = torch.cat([rgb, sigma], -1)
    pre = pre + [p_alpha, p_views]
    margin = None
    if with_margin:
        with torch.no_grad():
            ms = [(q.abs().min(-1).values / q.abs().max(-1).values) for q in pre[:6] + [p_views]]
            ms.append(p_alpha.abs()[:, 0] / (h.abs() @ w[8].abs()[0] + b[8].abs()[0]))
            margin = torch.stack(ms, -1).min(-1).values
    if not need:
        return Net(raw.detach(), [q.detach() for q in pre], None, None, None, margin)
    if o_given is None:
        (raw * g_raw.to(dtype)).sum().backward()
    else:
        # the backward entries take `raw` as an argument and form the sigmoid's derivative from it, o (1 - o) (csrc/mlp_bwd.hip:235-236), as
        # torch's sigmoid backward does from its own fp32 output: the same chain in `dtype` with that derivative taken at the GIVEN rgb
        o = o_given.to(dtype)[:, :3]
        z = outs[10]
        ((z * (g_raw.to(dtype)[:, :3] * o * (1 - o))).sum() + (sigma * g_raw.to(dtype)[:, 3:]).sum()).backward()
    grads, A = [], []
    for i in range(11):
        gp = outs[i].grad.abs()
        grads += [w[i].grad, b[i].grad]
        A += [gp.T @ xin[i].detach().abs(), gp.sum(0)]
    return Net(raw.detach(), [q.detach() for q in pre], x.grad, grads, A, margin)


def keep(margin, tau=TAU):
    """per-point mask: True = the point's ReLU pattern is safe from fp32 rounding"""
    return margin >= tau


def masked_d_raw(g_raw, kept):
    return (g_raw * kept[:, None].to(g_raw.dtype)).contiguous()


def signs_differ(pre_a, pre_b):
    """per point: some ReLU argument is > 0 in one evaluation and not in the other"""
    out = torch.zeros(pre_a[0].shape[0], dtype=torch.bool)
    for a, b in zip(pre_a, pre_b):
        out |= ((a > 0) != (b > 0)).any(-1)
    return out


def psum_depth(n_part, slices=32):
    """Additions on the longest path of one output of mvsnerf_partial_sum_multi over n_part partials (mvs_psum_walk in csrc/act.h; chunk and slices in
    mvsnerf_partial_sum_multi, csrc/wgrad3d.hip): a walk keeps eight running sums, ceil(rows / 8) additions each, folded by a three-level tree (its last line); n_part > MVS_RED_SLICES = 32 (act.h)
    walks chunks of ceil(n_part / 32) rows first and then the slices."""
    walk = lambda rows: -(-rows // 8) + 3
    if n_part <= slices:
        return walk(n_part)
    chunk = -(-n_part // slices)
    return walk(chunk) + walk(-(-n_part // chunk))


def summation_bound(per, grid, n_chunks):
    """2 * n_add * 2^-24: the largest difference, relative to the abs-sum A of an element's terms, between two fp32 summations of the same terms
    of which the longer chains n_add additions (each side is within n_add u A of the exact sum, to first order; products included: an fp32 MFMA
    step rounds like its additions).  n_add of a weight-gradient element, read from the kernels:

      one call    32 * per   a workgroup walks `per` tiles (csrc/mlp_bwd.hip:390-391); a tile is 16 v_mfma_f32_32x32x2_f32 steps onto one accumulator,
                             two products each (:443-447: 32 additions); a bias row sum is 16 additions per tile and one shuffle (:445, :468)
                + psum_depth(grid)   the `grid` partials (:588, :662)
      chunked     + 32 + psum_depth(256)   when n_chunks > 0: the other side is the float64 sum of n_chunks calls with per = 1, each at most 256
                             partials; their abs-sums add up to A, so the count of chunks does not enter - float64 adds nothing visible.
    The safe reading 32 * per + grid + n_chunks (a serial sum over the partials) is 355 at (3, 256, 3); this one is 150 there and still sees
    a lost tile (tests/test_mlp_train_refs.py::test_a_lost_tile_breaks_the_summation_bound)."""
    n_add = 32 * per + psum_depth(grid)
    if n_chunks:
        n_add += 32 + psum_depth(256)
    return 2.0 * n_add * U


Case = collections.namedtuple("Case", "N S F x g_raw kept margin ref cpu32 e_cpu live dropped flips")


@functools.lru_cache(maxsize=48)
def case(N, S, F):
    """One case, computed once: inputs x, the masked d_raw, the margin mask, the float64 Net `ref` and the CPU fp32 Net `cpu32` on the masked d_raw
    (pre-activations dropped to keep the cache small), e_cpu = the yardstick: per tensor (d_feat, then the 22 gradients) the largest difference of
    fp32 from float64 autograd over the float64 maximum; live = share of points with sigma > 0, dropped = share under tau, flips = kept points
    whose ReLU pattern differs between the fp32 and the float64 forward."""
    ws, bs = weights(F)
    x = inputs(N, S, F)
    fwd64 = network(ws, bs, *x, with_margin=True)
    kept = keep(fwd64.margin)
    g = masked_d_raw(d_raw(N, S, F), kept)
    ref = network(ws, bs, *x, g_raw=g)
    cpu = network(ws, bs, *x, g_raw=g, dtype=torch.float32)
    flips = int((signs_differ(cpu.pre, ref.pre) & kept).sum())
    e_cpu = [rel_err(c, r) for c, r in zip([cpu.d_feat] + cpu.grads, [ref.d_feat] + ref.grads)]
    live = float((ref.raw[:, 3] > 0).double().mean())
    ref, cpu = ref._replace(pre=None, margin=fwd64.margin), cpu._replace(pre=None)
    return Case(N, S, F, x, g, kept, fwd64.margin, ref, cpu, e_cpu, live, 1.0 - float(kept.double().mean()), flips)


def rel_err(got, ref):
    """largest difference over the reference's maximum, in float64 (a reference that is all zero: the largest difference itself)"""
    top = float(ref.abs().max())
    return float((got.double().reshape(ref.shape) - ref.double()).abs().max()) / (top if top > 0 else 1.0)


def tensor_names(F=None):
    return ["d_feat"] + [f"{n}.{k}" for n in M.ORDER for k in ("weight", "bias")]
