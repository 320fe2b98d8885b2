"""The ray-march MLP training kernels at their own entries: mvsnerf_mlp_fwd_train -> mvsnerf_mlp_bwd and mvsnerf_mlp_fwd_bf16_train ->
mvsnerf_mlp_bwd_bf16 (csrc/mlp.hip, csrc/mlp_bf16.hip, csrc/mlp_bwd.hip), called through _lib.lib() as ops does, on the packs of ops.mlp_pack /
mlp_pack_bf16 / mlp_pack_bwd[_bf16] and the table of ops._mlp_bwd_maps; buffer sizes from the library's size queries.  Nothing reads the layout of
`saved` / `gslots`.  References, inputs and the margin mask: tests/mlp_train_refs.py (conditions asserted by tests/test_mlp_train_refs.py).

A  float64 parity of the fp32 entries: d_feat and the 22 gradients against float64 autograd, per tensor e = largest difference / float64 maximum,
   e_kernel <= 5 e_cpu_fp32 + 8 u (the form and constants of test_fp32_abn_bwd_vs_float64_autograd: a reduction of unknown order has no derivable
   bound; e_cpu goes down to 2e-8, hence the additive term).  d_raw is zero on the points whose ReLU pattern fp32 rounding could flip.
   A tensor above that is held to CPU fp32 autograd carrying the one documented form that explains it (_check_float64: the derivative of the
   sigmoid from the fp32 `raw` the entry is handed) - same float64 reference, same 5 x / 8 u; one tensor of one case needs it.
B  multi-tile consistency, fp32 and bf16: one call (a weight-gradient workgroup walks per = 2 or 3 tiles) against calls on chunks of <= 8192
   points (per = 1, the regime A ties to float64): forward and d_feat bit-equal, gradients within summation_bound x A of the float64 sum of the
   chunks - and a chunked run that loses one tile's 32 points breaks that bound, or the test fails.
C  scratch and output contract: NaN-filled scratch and outputs give the bits of zero-filled ones; d_feat is written whole and nothing around it;
   two runs give the same bits.
D  ops.raymarch_train (mvsnerf_raymarch_bwd: the same kernels) one call against chunks of 64 rays.
E  argument contract of the four backward entries (mvsnerf_mlp_pack_bwd[_bf16] refusals: tests/test_train_wide_feat_args.py).
"""
import ctypes
import functools

import pytest
import torch

from tests import mlp_train_refs as R
from tests.test_gpu_mlp_fold import _bits, _pack_stable
from tests.util import record_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
NAN = float("nan")
A_FS = [4, 12, 20, 32, 34, 36, 40]
A_SHAPES = [(5, 7), (37, 24), (3, 300)]
B_CASES = [(65, 128, 20, 2), (129, 128, 20, 3), (517, 32, 40, 3)]          # (N, S, F, per)
C_CASES = [(5, 7, 20), (37, 24, 40), (517, 32, 40)]
CHUNK = 8192
NAMES = R.tensor_names()


def _ptrs(ts):
    return (ctypes.c_void_p * 11)(*[t.data_ptr() for t in ts])


@functools.lru_cache(maxsize=None)
def _net(F):
    from mvsnerf_amd import ops
    ws, bs = R.weights(F)
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    net = dict(wd=wd, bd=bd, f32=ops.mlp_pack(wd, bd, F), stable=_pack_stable(ws, bs, F), bf16=ops.mlp_pack_bf16(wd, F),
               bwd=ops.mlp_pack_bwd(wd, F), bwd_bf16=ops.mlp_pack_bwd_bf16(wd, F), maps=ops._mlp_bwd_maps(F, DEV))
    torch.cuda.synchronize()
    return net


def _scratch(P, bf16, fill):
    """saved, gslots, workspace: sized by the library's queries (two-byte slots under bf16), filled with `fill`"""
    from mvsnerf_amd import _lib
    l, div = _lib.lib(), 2 if bf16 else 1
    return [torch.full((n,), fill, device=DEV, dtype=torch.float32)
            for n in (l.mvsnerf_mlp_saved_floats(P) // div, l.mvsnerf_mlp_gradslot_floats(P) // div, l.mvsnerf_mlp_bwd_workspace_floats())]


def _forward(F, x, bf16, saved):
    from mvsnerf_amd import _lib, ops
    l, net = _lib.lib(), _net(F)
    ndc, feat, dirs = x
    N, S = ndc.shape[:2]
    raw = torch.full((N * S, 4), NAN, device=DEV)
    io = (F, ndc.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, N, S, raw.data_ptr(), saved.data_ptr(), ops.stream_ptr())
    if bf16:
        ops.check(l.mvsnerf_mlp_fwd_bf16_train(net["bf16"].data_ptr(), net["f32"].data_ptr(), *io), "mlp_fwd_bf16_train")
    else:
        ops.check(l.mvsnerf_mlp_fwd_train(net["f32"].data_ptr(), *io), "mlp_fwd_train")
    return raw


def _train(F, x, g_raw, n_out, bf16=False, fill=0.0, d_feat=None):
    """training forward -> backward on x = (ndc (N,S,3), feat (N,S,F), dirs (N,3)) and g_raw (N S, 4), all on the device and contiguous.
    Scratch and every output start as `fill`.  -> raw (N S, 4), d_feat (N S, n_out), [w0, b0, w1, b1, ...] gradients in ops.MLP_ORDER"""
    from mvsnerf_amd import _lib, ops
    l, net = _lib.lib(), _net(F)
    N, S = x[0].shape[:2]
    P = N * S
    saved, gslots, ws = _scratch(P, bf16, fill)
    raw = _forward(F, x, bf16, saved)
    if d_feat is None:
        d_feat = torch.full((P, n_out), fill, device=DEV)
    gw = [torch.full_like(w, fill) for w in net["wd"]]
    gb = [torch.full_like(b, fill) for b in net["bd"]]
    fn = l.mvsnerf_mlp_bwd_bf16 if bf16 else l.mvsnerf_mlp_bwd
    ops.check(fn(net["f32"].data_ptr(), net["bwd_bf16" if bf16 else "bwd"].data_ptr(), F, raw.data_ptr(), g_raw.data_ptr(), saved.data_ptr(), N, S,
                 gslots.data_ptr(), d_feat.data_ptr(), n_out, _ptrs(gw), _ptrs(gb), net["maps"].data_ptr(), ws.data_ptr(), ops.stream_ptr()),
              "mlp_bwd_bf16" if bf16 else "mlp_bwd")
    torch.cuda.synchronize()
    return raw, d_feat, [t for pair in zip(gw, gb) for t in pair]


def _dev(c):
    return tuple(t.to(DEV).contiguous() for t in c.x), c.g_raw.to(DEV).contiguous()


def _check_float64(c, n_out, raw, d_feat, grads, tag):
    """A's bound on one run; -> (failures, largest share of the bound a tensor uses).  The reference is float64 autograd throughout.

    The yardstick is CPU fp32 autograd.  ONE documented form of the kernel can exceed it, and a tensor that does is then held to the CPU fp32
    autograd that carries the same form: the backward entries are HANDED `raw` in fp32 and take the sigmoid's derivative from it,
    gz = g o (1 - o) (csrc/mlp_bwd.hip:235-236; include/mvsnerf_hip.h, mvsnerf_mlp_bwd's `raw`), as torch's sigmoid backward does from its own
    fp32 output.  Where the head saturates, o (1 - o) of a rounded o is off by u / (1 - o) of itself - 2.6e-4 at 1 - o = 2.3e-4 - per point, and the
    CPU and the kernel round to DIFFERENT o (both forwards are within 9e-7 of float64).  Measured at (3, 300, 12), the one case of A's 21 above the
    plain bound (pts_linears.0.bias: kernel 1.84e-6, CPU 1.55e-7, 1.47 of the bound): the FLOAT64 chain with nothing changed but the derivative
    taken at the kernel's rgb is 7.6e-7 .. 2.4e-6 away from float64 autograd in the 21 tensors behind the rgb head (0 in alpha_linear's), the
    kernel is within 8e-8 .. 5.3e-7 of that chain, and so is the CPU of the chain at ITS rgb (2.5e-8 .. 5.5e-7): the CPU's 1.55e-7 is a cancellation
    between its own rounding of o and the rest.  Carrying the form = the CPU fp32 chain with the derivative taken at the kernel's rgb
    (tests.mlp_train_refs.network(o_given=)).  5 x / 8 u stay; tensors that needed it are recorded (mlp_train_f64:*:carried)."""
    fails, share = [], 0.0
    refs = [c.ref.d_feat[:, :n_out]] + c.ref.grads
    cpus = [c.cpu32.d_feat[:, :n_out]] + c.cpu32.grads
    carried = None
    for name, k, r, cp in zip(NAMES, [d_feat] + grads, refs, cpus):
        k = k.cpu()
        e_k, e_c = R.rel_err(k, r), R.rel_err(cp, r)
        record_err(f"mlp_train_f64:{tag}:{name}:kernel", e_k)
        record_err(f"mlp_train_f64:{tag}:{name}:cpu_fp32", e_c)
        bound = 5 * e_c + 8 * U
        print(f"[mlp_train_f64 {tag} {name}] err / max: kernel {e_k:.3e}  CPU fp32 autograd {e_c:.3e}  share of 5 x CPU + 8 u {e_k / bound:.3f}")
        if not e_k <= bound and not name.startswith("alpha_linear"):
            if carried is None:
                net = R.network(*R.weights(c.F), *c.x, g_raw=c.g_raw, dtype=torch.float32, o_given=raw.cpu())
                carried = dict(zip(NAMES, [net.d_feat[:, :n_out]] + net.grads))
            e_c = R.rel_err(carried[name], r)
            bound = 5 * e_c + 8 * U
            record_err(f"mlp_train_f64:{tag}:{name}:carried", e_c)
            print(f"[mlp_train_f64 {tag} {name}] above the plain bound; CPU fp32 autograd with the derivative at the kernel's rgb {e_c:.3e}  share {e_k / bound:.3f}")
        share = max(share, e_k / bound)
        # Measured on an MI355X (tags mlp_train_f64:A:*), 21 cases x 23 tensors (x 2 n_feat_out): kernel 1.1e-8 .. 5.7e-6, CPU fp32 autograd
        # 1.1e-8 .. 4.5e-6.  Largest share of 5 x CPU + 8 u per case: 0.20 .. 0.60, but 0.89 at (3, 300, 20) (pts_linears.3.weight) and, at
        # (3, 300, 12), 0.91 (rgb_linear.weight) with pts_linears.0.bias at 1.47 of the plain bound = 0.18 of the carried one (docstring: CPU
        # 1.97e-6 once it takes the derivative at the kernel's rgb).  B's (129, 128, 20): 0.37.
        if not e_k <= bound:
            why = ""
            if name == "d_feat":
                row = int((k.double() - r).abs().max(-1).values.argmax())
                m = float(c.margin[row])
                why = f" worst row {row}, margin {m:.3e}: {'under 2^-15, a ReLU flip the mask missed' if m < 2.0 ** -15 else 'no flip - the kernel'}"
            fails.append(f"{tag} {name}: kernel {e_k:.3e} > 5 x {e_c:.3e} + 8 u{why}")
        # dead units: a weight-gradient row / bias entry that is exactly 0 in float64 is exactly 0 in the kernel
        if name != "d_feat":
            dead = (r == 0).reshape(r.shape[0], -1).all(-1)
            if bool(dead.any()) and bool((k.reshape(r.shape[0], -1)[dead] != 0).any()):
                fails.append(f"{tag} {name}: a row that is exactly 0 in float64 is not in the kernel")
    return fails, share


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("F", A_FS)
@pytest.mark.parametrize("N,S", A_SHAPES)
def test_fp32_training_entries_vs_float64_autograd(N, S, F):
    from mvsnerf_amd import _lib, ops
    c = R.case(N, S, F)
    x, g = _dev(c)
    fails, share = [], 0.0
    plain = torch.full((N * S, 4), NAN, device=DEV)
    ops.check(_lib.lib().mvsnerf_mlp_fwd(_net(F)["stable"].data_ptr(), F, x[0].data_ptr(), 3, x[1].data_ptr(), F, x[2].data_ptr(), 3, N, S, 0,
                                         plain.data_ptr(), ops.stream_ptr()), "mlp_fwd")
    for n_out in ([4] if F == 4 else [4, 8] if F == 34 else [8, F]):
        raw, d_feat, grads = _train(F, x, g, n_out)
        assert _bits(raw, plain), "the training forward's raw differs from mvsnerf_mlp_fwd's"
        for col in range(4):                                                # the forward itself: the fp32 bound of tests/test_mlp_train_refs.py
            top = max(1.0, float(c.ref.raw[:, col].abs().max()))
            assert float((raw[:, col].cpu().double() - c.ref.raw[:, col]).abs().max()) <= 2e-5 * top, ("raw", col)
        assert not bool(d_feat[~c.kept.to(DEV)].any()), "a dropped point (d_raw = 0) has a non-zero d_feat row"
        f, s = _check_float64(c, n_out, raw, d_feat, grads, f"A:({N},{S},{F}):n{n_out}")
        fails += f
        share = max(share, s)
    record_err(f"mlp_train_f64:A:({N},{S},{F}):share", share, tol=1.0)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ B
def _chunks(N, S):
    rays = CHUNK // S
    return [(r, min(r + rays, N)) for r in range(0, N, rays)]


def _chunked(F, x, g, S, n_out, bf16, only=None, have=None):
    """calls on consecutive chunks of whole rays; only / have: re-run chunk `only` and take the others from an earlier list (the runs are bit-stable: C)"""
    out = []
    for k, (r0, r1) in enumerate(_chunks(x[0].shape[0], S)):
        if only is not None and k != only:
            out.append(have[k])
            continue
        xs = tuple(t[r0:r1].contiguous() for t in x)
        out.append(_train(F, xs, g[r0 * S:r1 * S].contiguous(), n_out, bf16))
    return out


def _sum64(parts):
    return [sum(p[2][i].double() for p in parts) for i in range(22)]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,S,F,per", B_CASES)
def test_one_call_equals_its_chunks(N, S, F, per, bf16):
    """per: tiles per weight-gradient workgroup of the one call, ceil(4 ceil(P / 128) / 256) (csrc/mlp_bwd.hip:390-391, :588); the chunks run per = 1.
    Measured on an MI355X, the largest |one call - sum of chunks| / (summation_bound x A) over the 22 gradients: fp32 0.011 / 0.008 / 0.011,
    bf16 0.012 / 0.007 / 0.19 (views_linears.0.weight; A is the float64 network's, the bf16 kernels' operands are rounded) in the order of B_CASES -
    a worst-case bound, used to a hundredth; what it is for is the lost tile below, which breaks it in >= 8 weight gradients in all six cases."""
    c = R.case(N, S, F)
    P = N * S
    n_tiles = 4 * ((P + 127) // 128)
    assert per == -(-n_tiles // 256) and all((r1 - r0) * S <= CHUNK for r0, r1 in _chunks(N, S))
    x, g = _dev(c)
    n_chunks = len(_chunks(N, S))
    bound = R.summation_bound(per, 256, n_chunks)
    A = [a.to(DEV) for a in c.ref.A]
    kind = "bf16" if bf16 else "fp32"
    for n_out in ([8, F] if F == 40 else [8]):
        raw, d_feat, grads = _train(F, x, g, n_out, bf16)
        parts = _chunked(F, x, g, S, n_out, bf16)
        assert _bits(raw, torch.cat([p[0] for p in parts])), "forward: one call differs from its chunks"
        assert _bits(d_feat, torch.cat([p[1] for p in parts])), "d_feat: one call differs from its chunks"
        assert bool(torch.isfinite(d_feat).all())
        want = _sum64(parts)
        used = [float(((k.double() - w).abs() / (bound * a).clamp_min(1e-300)).max()) for k, w, a in zip(grads, want, A)]
        for name, u_ in zip(NAMES[1:], used):
            record_err(f"mlp_train_f64:B:{kind}:({N},{S},{F}):n{n_out}:{name}", u_, tol=1.0)
        print(f"[mlp_train_f64 B {kind} ({N},{S},{F}) n_out {n_out}] largest |one call - chunks| / (bound x A): {max(used):.3f}")
        bad = {n: u_ for n, u_ in zip(NAMES[1:], used) if not u_ <= 1.0}
        assert not bad, f"one call against the float64 sum of its chunks, in units of summation_bound({per}, 256, {n_chunks}) x A: {bad}"
    # teeth, in the test itself: the chunked side loses the 32 points of one tile (the second of its workgroup's range in the one call)
    tile = (n_tiles // 2) | 1
    assert 32 * tile + 32 <= P and bool(c.kept[32 * tile:32 * tile + 32].any())
    g_lost = g.clone()
    g_lost[32 * tile:32 * tile + 32] = 0
    k_lost = (32 * tile) // CHUNK
    lost = _sum64(_chunked(F, x, g_lost, S, n_out, bf16, only=k_lost, have=parts))
    seen = [bool(((k.double() - w).abs() > bound * a).any()) for k, w, a in zip(grads, lost, A)]
    assert sum(seen[0::2]) >= 8, f"a lost tile goes unseen: {dict(zip(NAMES[1::2], seen[0::2]))}"
    if not bf16 and (N, S, F) == (129, 128, 20):
        fails, share = _check_float64(c, n_out, raw, d_feat, grads, f"B:({N},{S},{F}):n{n_out}")
        record_err(f"mlp_train_f64:B:({N},{S},{F}):share", share, tol=1.0)
        assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,S,F", C_CASES)
def test_scratch_and_outputs_need_no_initialisation(N, S, F, bf16):
    """saved / gslots / workspace are torch.empty in ops; a tail tile's dead lanes and wholly dead tiles (n_tiles = 4 ceil(P / 128)) enter the
    weight-gradient contraction like live ones, so every slot a contraction reads must have been written, with finite values (csrc/mlp.hip:305:
    dead lanes run point P - 1).  gw / gb are OVERWRITTEN (include/mvsnerf_hip.h): every element, whatever was there."""
    c = R.case(N, S, F)
    x, g = _dev(c)
    P, n_out = N * S, (F if F == 40 else 8)
    zero = _train(F, x, g, n_out, bf16, fill=0.0)
    nan = _train(F, x, g, n_out, bf16, fill=NAN)
    for name, a, b in zip(["raw"] + NAMES, [zero[0], zero[1]] + zero[2], [nan[0], nan[1]] + nan[2]):
        assert bool(torch.isfinite(b).all()), f"{name}: not finite after a run on NaN-filled buffers (an element not written, or NaN scratch read)"
        assert _bits(a, b), f"{name}: depends on what the buffers held"
    # d_feat carved from a NaN buffer, guard rows on both sides
    big = torch.full((P + 8, n_out), NAN, device=DEV)
    again = _train(F, x, g, n_out, bf16, fill=NAN, d_feat=big[4:4 + P])
    assert bool(torch.isnan(big[:4]).all()) and bool(torch.isnan(big[4 + P:]).all()), "d_feat: written outside its rows"
    assert bool(torch.isfinite(big[4:4 + P]).all()), "d_feat: an element was not written"
    for name, a, b in zip(["raw"] + NAMES, [zero[0], zero[1]] + zero[2], [again[0], big[4:4 + P]] + again[2]):
        assert _bits(a, b), f"{name}: two runs differ"


# ------------------------------------------------------------------ D
def test_raymarch_train_one_call_equals_its_chunks():
    """ops.raymarch_train on 130 rays x 128 samples (520 tiles, per = 3), V = 3, a volume that takes no gradient, the loss of
    test_gpu_backward._setup on rgb, depth, weights, alpha: the 22 gradients of one call against the float64 sum of calls on chunks of 64 rays
    (per = 1), within summation_bound(3, 256, 3) x A'.  A' = 32 x the float64 sum of the chunks' ABSOLUTE gradients: a PROXY for the abs-sum of
    an element's terms, not a bound on it (the terms inside a chunk cancel; 32 = the points of a tile stands in for that) - the per-element
    abs-sums cannot be had through this entry.  The measured ratio is recorded (mlp_train_f64:D:*): 0.047 at the most (pts_linears.5.weight).  This ties
    mvsnerf_raymarch_bwd's use of the weight-gradient kernels to B."""
    import types
    from mvsnerf_amd import models, ops
    from tests.test_gpu_backward import _setup
    n_rays, n_samples = 130, 128
    rig, pose, vol, pts, dirs, ndc, z, ro, mlp_sd, (Rr, Q, Wt, Aa) = _setup(n_rays, n_samples, 7)
    args = types.SimpleNamespace(feat_dim=20, img_downscale=1.0, use_color_volume=False, net_type="v0", multires=10, i_embed=0,
                                 pts_dim=3, multires_views=4, dir_dim=3, netdepth=6, netwidth=128, N_importance=0, netchunk=1024,
                                 ckpt=None, perturb=1.0, N_samples=n_samples, use_viewdirs=True, white_bkgd=False, raw_noise_std=0.0)
    kw, _, _, _ = models.create_nerf_mvs(args, use_mvs=False, dir_embedder=False, pts_embedder=True)
    net = kw["network_fn"]
    net.load_state_dict(mlp_sd)
    net.to(DEV)
    V = 3
    imgs = rig["images_raw"][:, :3][0, :V].contiguous().to(DEV)
    w2cs, K = pose["w2cs"][:V].contiguous().to(DEV), pose["intrinsics"][:V].contiguous().to(DEV)
    vol_d = vol.to(DEV)
    t = [a.to(DEV) for a in (pts, ndc, z, dirs, Rr, Q, Wt, Aa)]

    def grads_of(r0, r1):
        net.zero_grad(set_to_none=True)
        p, n, zz, d, r_, q_, w_, a_ = (a[r0:r1].contiguous() for a in t)
        out = ops.raymarch_train(vol_d, imgs, w2cs, K, net, p, n, zz, d)
        ((out["rgb_map"] * r_).sum() + (out["depth"] * q_).sum() + (out["weights"] * w_).sum() + (out["alpha"] * a_).sum()).backward()
        params = [q for l in net.nerf._linears() for q in (l.weight, l.bias)]
        torch.cuda.synchronize()
        return [q.grad.detach().clone() for q in params]

    one = grads_of(0, n_rays)
    parts = [grads_of(r, min(r + 64, n_rays)) for r in range(0, n_rays, 64)]
    assert len(parts) == 3 and len(one) == 22
    bound = R.summation_bound(3, 256, 3)
    used = {}
    for i, name in enumerate(NAMES[1:]):
        want = sum(p[i].double() for p in parts)
        a_proxy = 32 * sum(p[i].double().abs() for p in parts)
        assert bool(torch.isfinite(one[i]).all()) and float(want.abs().max()) > 0, name
        used[name] = float(((one[i].double() - want).abs() / (bound * a_proxy).clamp_min(1e-300)).max())
        record_err(f"mlp_train_f64:D:{name}", used[name], tol=1.0)
    print(f"[mlp_train_f64 D] largest |one call - chunks| / (summation_bound x A'): {max(used.values()):.3f}")
    bad = {n: v for n, v in used.items() if not v <= 1.0}
    assert not bad, bad


# ------------------------------------------------------------------ E
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_backward_argument_contract(bf16):
    """MVSNERF_EUNSUPPORTED: odd F, F = 0, F = 2, F = 42, S = 0, N < 0.  MVSNERF_EINVAL: n_feat_out 0, 6, F + 4; d_feat off 16-byte alignment; a NULL
    among the pointers (seen before F).  N = 0 is OK and writes nothing.  Every refusal leaves the outputs untouched.
    F = 2: the training forward and the packs take it, the backward does not (d_feat rows are written four columns at a time, so
    4 <= n_feat_out <= F has no solution; ops only ever has F = 8 + 4V >= 12): MVSNERF_EUNSUPPORTED, as include/mvsnerf_hip.h says."""
    from mvsnerf_amd import _lib, ops
    l = _lib.lib()
    N, S, F = 5, 7, 20
    P = N * S
    c = R.case(N, S, F)
    x, g = _dev(c)
    net = _net(F)
    saved, gslots, ws = _scratch(P, bf16, 0.0)
    raw = _forward(F, x, bf16, saved)
    big = torch.full((P + 8, 8), NAN, device=DEV)
    d_feat = big[4:4 + P]
    gw, gb = [torch.full_like(w, NAN) for w in net["wd"]], [torch.full_like(b, NAN) for b in net["bd"]]
    fn = l.mvsnerf_mlp_bwd_bf16 if bf16 else l.mvsnerf_mlp_bwd
    base = dict(packed_fwd=net["f32"].data_ptr(), packed_bwd=net["bwd_bf16" if bf16 else "bwd"].data_ptr(), F=F, raw=raw.data_ptr(), d_raw=g.data_ptr(),
                saved=saved.data_ptr(), N=N, S=S, gslots=gslots.data_ptr(), d_feat=d_feat.data_ptr(), n_feat_out=8, gw=_ptrs(gw), gb=_ptrs(gb),
                maps=net["maps"].data_ptr(), workspace=ws.data_ptr())

    def call(**kw):
        a = dict(base, **kw)
        return fn(*[a[k] for k in base], ops.stream_ptr())

    refused = [("odd F", dict(F=21), EUNSUPPORTED), ("F = 0", dict(F=0), EUNSUPPORTED), ("F = 42", dict(F=42), EUNSUPPORTED),
               ("F = 2", dict(F=2), EUNSUPPORTED), ("F = 2, n_feat_out 4", dict(F=2, n_feat_out=4), EUNSUPPORTED),
               ("S = 0", dict(S=0), EUNSUPPORTED), ("N < 0", dict(N=-1), EUNSUPPORTED),
               ("n_feat_out 0", dict(n_feat_out=0), EINVAL), ("n_feat_out 6", dict(n_feat_out=6), EINVAL),
               ("n_feat_out F + 4", dict(n_feat_out=F + 4), EINVAL), ("d_feat off alignment", dict(d_feat=d_feat.data_ptr() + 4), EINVAL)]
    refused += [(f"NULL {k}", {k: None}, EINVAL) for k in base if k not in ("F", "N", "S", "n_feat_out")]
    refused += [("NULL before F", dict(F=42, maps=None), EINVAL)]
    for what, kw, want in refused:
        assert call(**kw) == want, what
    assert call(N=0) == OK, "an empty batch"
    torch.cuda.synchronize()
    assert bool(torch.isnan(big).all()) and all(bool(torch.isnan(t).all()) for t in gw + gb), "a refused call (or N = 0) wrote to an output"
    # the same arguments, put right, run - and F = 4, the smallest backward, is taken
    assert call() == OK
    torch.cuda.synchronize()
    want = _train(F, x, g, 8, bf16)
    assert _bits(d_feat, want[1]) and all(_bits(a, b) for a, b in zip([t for p in zip(gw, gb) for t in p], want[2]))
    assert bool(torch.isnan(big[:4]).all()) and bool(torch.isnan(big[4 + P:]).all())
    c4 = R.case(N, S, 4)
    x4, g4 = _dev(c4)
    out4 = _train(4, x4, g4, 4, bf16)
    assert all(bool(torch.isfinite(t).all()) for t in [out4[1]] + out4[2])
