"""feature_linear folded into views_linears.0 for the fp32 no-grad kernels (mvsnerf_mlp_pack_fold, csrc/mlp.hip, csrc/mlp_layout.h).

The reference network (models.py:209-215) has no activation between feature_linear and views_linears.0, so a no-grad forward may run them as one
affine map W' = Wv[:, :128] Wf, b' = bv + Wv[:, :128] bf.  ops.mlp_pack appends W' / b' behind the standard packed buffer and sets a flag in it;
every fp32 no-grad kernel handed such a buffer skips the feature_linear GEMM.

A  the folded kernel is the unfolded kernel on pre-folded weights, bit for bit: W', b' formed on the host in float64 (sequential chain, j
   ascending, rounded once), packed with the STABLE mvsnerf_mlp_pack as (feature_linear = (I, 0), views_linears.0 = ([W' | Wv[:, 128:]], b')).
   An identity feature_linear reproduces h5 exactly and the views chain has the same k order in both kernels.
B  sigma, the sigma-only launch and the training forward do not change; a stable re-pack into a folded buffer clears the flag.
C  accuracy against the unfolded network in float64 (CPU, same fp32 weights and inputs):
   (i)  |folded - unfolded kernel| <= 1/4 sum_n |Wr[c][n]| B_n + 4u per element of raw[..., :3], B_n = 2 (259 + 8) u S_n,
        S_n = sum_j |Wv[n][j]| (sum_k |Wf[j][k]| |h5[k]| + |bf[j]|) + sum_d |Wv[n][128+d]| |dir_d| + |bv[n]|, u = 2^-24, h5 from float64: the two
        kernels share every bit up to h5, 259 = 128 + 131 is the length of the two chains, the factor 2 and the + 8 are the per-layer
        convention of tests/test_gpu_fp32_layers.py, 1/4 is the sigmoid's Lipschitz constant;
   (ii) the mean absolute error of the folded raw[..., :3] against float64 is at most 1.25 x that of the unfolded kernel.
D  ops.raymarch (one launch, NR = 1 and NR = 2) against gather -> mvsnerf_mlp_fwd -> composite on the same folded buffer: bit identity.

Shapes: (5, 7) = one partial tile with dead lanes and dead waves; (37, 24) = six full tiles and a partial one, rays straddling tiles.
F = 12 / 20 / 36: 4 / 12 / 20 feature k-steps; F = 20 carries the checkpoint's weights.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
SHAPES = [(5, 7), (37, 24)]
FS = [12, 20, 36]
CASES = [(N, S, F) for (N, S) in SHAPES for F in FS]


# ------------------------------------------------------------------ weights, inputs, the network in torch
def _weights(F):
    """11 (weight, bias) fp32 CPU pairs in ops.MLP_ORDER: the checkpoint's at F = 20, uniform(-0.15, 0.15) otherwise."""
    from mvsnerf_amd import models
    from tests.util import load_weights
    m = models.MVSNeRF(D=6, W=128, input_ch_pts=63, input_ch_views=3, input_ch_feat=F, skips=[4], net_type="v0")
    if F == 20:
        m.load_state_dict(load_weights()[0])
    else:
        torch.manual_seed(F)
        for p in m.parameters():
            torch.nn.init.uniform_(p, -0.15, 0.15)
    lins = m.nerf._linears()
    return [l.weight.detach().clone().contiguous() for l in lins], [l.bias.detach().clone().contiguous() for l in lins]


def _inputs(N, S, F):
    g = torch.Generator().manual_seed(1000 * N + 10 * S + F)
    ndc = torch.rand((N, S, 3), generator=g)
    feat = torch.randn((N, S, F), generator=g)
    dirs = torch.nn.functional.normalize(torch.randn((N, 3), generator=g), dim=-1)
    return ndc, feat, dirs


def _embed(ndc):
    """models.py:47-51, multires 10: [xyz | sin(30) | cos(30)], the scaled input x * 2^f is exact in either precision"""
    freq = (2.0 ** torch.arange(10, dtype=ndc.dtype)).view(1, -1, 1)
    sc = (ndc.unsqueeze(-2) * freq).reshape(*ndc.shape[:-1], -1)
    return torch.cat((ndc, torch.sin(sc), torch.cos(sc)), -1)


def _trunk(ws, bs, ndc, feat):
    """-> (h5, sigma) of models.py:199-209 in the dtype of the arguments"""
    lin = torch.nn.functional.linear
    pts = _embed(ndc)
    bias = lin(feat, ws[6], bs[6])
    h = pts
    for i in range(6):
        h = torch.relu(lin(h, ws[i], bs[i]) * bias)
        if i == 4:
            h = torch.cat([pts, h], -1)
    return h, torch.relu(lin(h, ws[8], bs[8]))


def _tail(ws, bs, h5, dirs, folded=None):
    """rgb of models.py:210-217; folded = (W', b'): the one affine map in place of feature_linear -> views_linears.0"""
    lin = torch.nn.functional.linear
    d = dirs[:, None, :].expand(*h5.shape[:-1], 3)
    if folded is None:
        hv = lin(torch.cat([lin(h5, ws[7], bs[7]), d], -1), ws[9], bs[9])
    else:
        hv = lin(torch.cat([h5, d], -1), torch.cat([folded[0], ws[9][:, 128:]], 1), folded[1])
    return torch.sigmoid(lin(torch.relu(hv), ws[10], bs[10]))


def _fold_host(ws, bs):
    """W', b' in float64 with the sequential chain acc = acc + a*b, j ascending, rounded to fp32 once (the order of the pack kernel)"""
    Wv, Wf = ws[9].numpy().astype(np.float64), ws[7].numpy().astype(np.float64)
    bv, bf = bs[9].numpy().astype(np.float64), bs[7].numpy().astype(np.float64)
    accw, accb = np.zeros((64, 128)), bv.copy()
    for j in range(128):
        accw = accw + Wv[:, j:j + 1] * Wf[j:j + 1, :]
        accb = accb + Wv[:, j] * bf[j]
    return torch.from_numpy(accw.astype(np.float32)), torch.from_numpy(accb.astype(np.float32))


# ------------------------------------------------------------------ the kernels
def _pack_stable(ws, bs, F):
    """mvsnerf_mlp_pack into an exact mvsnerf_mlp_packed_floats(F) buffer"""
    from mvsnerf_amd import _lib, ops
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    packed = torch.empty(_lib.lib().mvsnerf_mlp_packed_floats(F), device=DEV, dtype=torch.float32)
    wp = (ctypes.c_void_p * 11)(*[w.data_ptr() for w in wd])
    bp = (ctypes.c_void_p * 11)(*[b.data_ptr() for b in bd])
    ops.check(_lib.lib().mvsnerf_mlp_pack(wp, bp, F, packed.data_ptr(), ops.stream_ptr()), "mlp_pack")
    torch.cuda.synchronize()
    return packed


def _fwd(packed, F, x, alpha_only=0):
    from mvsnerf_amd import ops
    ndc, feat, dirs = x
    N, S = ndc.shape[:2]
    raw = ops.mlp_forward(packed, F, ndc.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, N, S, alpha_only, ndc.device)
    torch.cuda.synchronize()
    return raw


def _fwd_train(packed, F, x):
    from mvsnerf_amd import _lib, ops
    ndc, feat, dirs = x
    N, S = ndc.shape[:2]
    raw = torch.zeros((N * S, 4), device=DEV)
    saved = torch.zeros(_lib.lib().mvsnerf_mlp_saved_floats(N * S), device=DEV)
    ops.check(_lib.lib().mvsnerf_mlp_fwd_train(packed.data_ptr(), F, ndc.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, N, S,
                                               raw.data_ptr(), saved.data_ptr(), ops.stream_ptr()), "mlp_fwd_train")
    torch.cuda.synchronize()
    return raw, saved


def _bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


@functools.lru_cache(maxsize=None)
def _net(F):
    """weights and the three packed buffers of one F, made once: folded (ops.mlp_pack), stable, and the stable pack of the pre-folded substitute"""
    from mvsnerf_amd import ops
    ws, bs = _weights(F)
    folded = ops.mlp_pack([w.to(DEV) for w in ws], [b.to(DEV) for b in bs], F)
    Wp, bp = _fold_host(ws, bs)
    ws2, bs2 = list(ws), list(bs)
    ws2[7], bs2[7] = torch.eye(128), torch.zeros(128)
    ws2[9], bs2[9] = torch.cat([Wp, ws[9][:, 128:]], 1).contiguous(), bp
    return dict(ws=ws, bs=bs, folded=folded, stable=_pack_stable(ws, bs, F), prefolded=_pack_stable(ws2, bs2, F))


@functools.lru_cache(maxsize=None)
def _case(N, S, F):
    """inputs and the kernels' outputs of one case, computed once and shared"""
    net = _net(F)
    x = tuple(t.to(DEV) for t in _inputs(N, S, F))
    return dict(net=net, x=x, raw_folded=_fwd(net["folded"], F, x), raw_stable=_fwd(net["stable"], F, x))


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("N,S,F", CASES)
def test_folded_kernel_is_the_unfolded_kernel_on_prefolded_weights(N, S, F):
    from mvsnerf_amd import _lib
    c = _case(N, S, F)
    net = c["net"]
    assert net["prefolded"].numel() == _lib.lib().mvsnerf_mlp_packed_floats(F) < net["folded"].numel() == _lib.lib().mvsnerf_mlp_packed_fold_floats(F)
    want = _fwd(net["prefolded"], F, c["x"])
    got = c["raw_folded"]
    assert got.shape == (N * S, 4)
    assert torch.equal(got, want), [float((got[:, k] - want[:, k]).abs().max()) for k in range(4)]
    # the standard part of the folded buffer is the stable pack, but for the flag
    n = net["stable"].numel()
    diff = (net["folded"][:n].view(torch.int32) != net["stable"].view(torch.int32)).nonzero().flatten().tolist()
    assert len(diff) == 1 and float(net["folded"][diff[0]]) == 1.0 and float(net["stable"][diff[0]]) == 0.0, diff


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("N,S,F", CASES)
def test_sigma_alpha_only_and_training_forward_do_not_change(N, S, F):
    c = _case(N, S, F)
    net, x = c["net"], c["x"]
    assert torch.equal(c["raw_folded"][:, 3], c["raw_stable"][:, 3])
    a_f, a_s = _fwd(net["folded"], F, x, alpha_only=1), _fwd(net["stable"], F, x, alpha_only=1)
    assert a_f.shape == (N * S, 1) and torch.equal(a_f, a_s) and torch.equal(a_f[:, 0], c["raw_stable"][:, 3])
    if F <= 32:                                        # the training forward takes F <= 32 (include/mvsnerf_hip.h)
        (r_f, s_f), (r_s, s_s) = _fwd_train(net["folded"], F, x), _fwd_train(net["stable"], F, x)
        assert _bits(r_f, r_s) and _bits(s_f, s_s)
        assert torch.equal(r_f, c["raw_stable"])        # ... which is the unfolded forward's arithmetic
    # a stable pack into memory that held a folded buffer clears the flag: the unfolded kernel's bits again
    from mvsnerf_amd import _lib, ops
    buf = net["folded"].clone()
    wd, bd = [w.to(DEV) for w in net["ws"]], [b.to(DEV) for b in net["bs"]]
    wp = (ctypes.c_void_p * 11)(*[w.data_ptr() for w in wd])
    bp = (ctypes.c_void_p * 11)(*[b.data_ptr() for b in bd])
    ops.check(_lib.lib().mvsnerf_mlp_pack(wp, bp, F, buf.data_ptr(), ops.stream_ptr()), "mlp_pack")
    torch.cuda.synchronize()
    n = net["stable"].numel()
    assert _bits(buf[:n], net["stable"])
    assert torch.equal(_fwd(buf, F, x), c["raw_stable"])


# ------------------------------------------------------------------ C
def _tail_bound(ws, bs, h5, dirs):
    """(..., 3): 1/4 sum_n |Wr[c][n]| B_n + 4u, in float64"""
    a = lambda t: t.double().abs()
    lin = torch.nn.functional.linear
    d = a(dirs)[:, None, :].expand(*h5.shape[:-1], 3)
    inner = lin(h5.abs(), a(ws[7]), a(bs[7]))                                   # sum_k |Wf[j][k]| |h5[k]| + |bf[j]|
    S_n = lin(torch.cat([inner, d], -1), a(ws[9]), a(bs[9]))
    return 0.25 * lin(2 * (259 + 8) * U * S_n, a(ws[10])) + 4 * U


@pytest.mark.parametrize("N,S,F", CASES)
def test_folded_tail_against_float64(N, S, F):
    c = _case(N, S, F)
    ws, bs = c["net"]["ws"], c["net"]["bs"]
    ndc, feat, dirs = (t.cpu() for t in c["x"])
    w64, b64 = [w.double() for w in ws], [b.double() for b in bs]
    h5, _ = _trunk(w64, b64, ndc.double(), feat.double())
    ref = _tail(w64, b64, h5, dirs.double()).reshape(N * S, 3)
    bound = _tail_bound(ws, bs, h5, dirs).reshape(N * S, 3)
    got, unf = c["raw_folded"][:, :3].cpu().double(), c["raw_stable"][:, :3].cpu().double()
    worst = float(((got - unf).abs() / bound).max())
    e_f, e_u = float((got - ref).abs().mean()), float((unf - ref).abs().mean())
    print(f"fold (N,S,F)=({N},{S},{F}): max |folded-unfolded|/bound {worst:.4f}  mean err folded {e_f:.3e} unfolded {e_u:.3e} ratio {e_f / e_u:.3f}"
          f"  max err folded {float((got - ref).abs().max()):.3e} unfolded {float((unf - ref).abs().max()):.3e}")
    assert worst <= 1.0, worst                                                  # (i)
    assert e_f <= 1.25 * e_u, (e_f, e_u)                                        # (ii)


# ------------------------------------------------------------------ D
@pytest.mark.parametrize("N,S", [(37, 16), (20, 128)])
def test_onelaunch_on_the_folded_buffer(N, S):
    from tests.test_gpu_raymarch_onelaunch import _check, _hwdc, _inputs as rm_inputs, _packed
    from mvsnerf_amd import _lib
    packed = _packed(3)
    assert packed.numel() == _lib.lib().mvsnerf_mlp_packed_fold_floats(20)          # Renderer_ours.packed() hands out folded buffers
    x = rm_inputs(N, S, seed=S)
    _check(_hwdc(x["vol"]), x, packed)
