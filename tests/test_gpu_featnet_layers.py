"""The fp32 family of FeatureNet's 2-D layers (csrc/featnet.hip, the 2-D entry of csrc/wgrad_mfma.hip and the _conv2d / _wgrad2d /
_FeatureNetFunction._backward plumbing of encoder.py; reference models.py:688-722), layer by layer against float64 on exactly the kernel's fp32
operands: forward, data gradient and weight gradient of every layer through every route the forward and the backward can take, the statistics
that leave with a launch, the InPlaceABN statistics / backward on (N, H, W, C) dims and the bias gradient of the toplayer.

route -> kernel (read against encoder._conv2d and the dispatchers mvsnerf_conv2d_fwd / _fwd_stats / _c3_nchw_fwd_stats / _dgrad_k5s2 / _wgrad):
  _conv2d want_stats=True             conv0.0 (cin_pad 4), conv0.1             conv2d_c8_lds_kernel<4|8, false> + statistics   (16x16 tiles, 18x18 halo in LDS)
  _conv2d src=_Nchw3                  conv0.0 from the (N,3,H,W) images        conv2d_c8_lds_kernel<4, true> + statistics
  _conv2d want_stats=False            conv0.0, conv0.1, dgrad of conv0.1       conv2d_kernel<4|8, 8, 3, 1, 8>                  (VALU, 16x16 tiles)
  _conv2d want_stats=True | False     conv1.0, conv1.1, conv2.0, conv2.1       conv2d_mfma_kernel<8,16,5,2> <16,16,3,1> <16,32,5,2> <32,32,3,1>
                                                                               (+ statistics | none; M-tiles of 16 / 32 linear pixels, 4 per workgroup)
  _conv2d mode="dgrad"                conv1.1, conv2.1                         conv2d_mfma_kernel<16,16,3,1> / <32,32,3,1> on mirrored, role-swapped weights
  _conv2d bias=... and mode="dgrad"   toplayer                                 conv2d_kernel<32, 16, 1, 1, 32>                 (VALU, 16x16 tiles, two channel groups)
  mvsnerf_conv2d_dgrad_k5s2           conv1.0 (16 -> 8), conv2.0 (32 -> 16)    conv2d_dgrad_k5s2_kernel<16, 8> / <32, 16>      (16x16 tiles per parity class)
  _wgrad2d sums=None | _PartialSums   the six k3 / k5 shapes                   conv_wgrad_mfma4_kernel (images as z) + mvs_partial_sum | mvsnerf_partial_sum_multi
                                      toplayer (k = 1)                         conv2d_wgrad_kernel<1, 1, 1> (VALU) + the same reductions
  mvsnerf_channel_sum                 toplayer bias gradient                   channel_sum_partial_kernel + mvs_partial_sum
  _abn_stats / _abn_bwd               as in test_gpu_fp32_layers, here on (N, H, W, C) dims and on the 2-D kernels' partial layouts
A route is asserted to be the route through what it leaves: statistics (and how many slots: 16x16 tiles or M-tiles) or none, what
mvsnerf_conv2d_mfma_tiles reports for the shape, the key of the packed weights in the layer's cache, the number of partial rows of a weight gradient.

Bound, per output ELEMENT (a border pixel cannot hide behind the interior maximum): with K products in the element, u = 2^-24 and S the same
operation on |operands| in float64,  |out - ref| <= 2 (K + 8) u S + 1e-30.  Any fp32 summation order gives (K + 2) u S with round-to-nearest
operations; + 6 for the fma of a pending activation; the factor 2 for a matrix-core accumulator that truncates.  K: forward k^2 cin_pad (+ 1 with a
bias); stride-1 data gradient k^2 Cout; dgrad_k5s2 25 Cin_g (at most 9 taps contribute); weight gradient and channel sum N Ho Wo.
Yardstick beside it: the largest err / S of torch's own fp32 operation on the same operands on the same GPU; the kernel's must stay within 5 x that + 4 u.

Bit identities (torch.equal; each is a claim csrc/featnet.hip makes): the NCHW first layer == the LDS kernel on the zero-padded channel-last copy (output
and every partial sum); the LDS kernel == the VALU kernel for (4, 8, 3, 1) and (8, 8, 3, 1); conv2d_mfma_kernel with == without statistics.  The two
reductions of a weight gradient (mvs_partial_sum: two running sums; mvsnerf_partial_sum_multi: eight) are NOT documented as the same order: both are held
to the bounds."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.test_gpu_fp32_layers import U, _abn_autograd, _act32, _act64, _check_abn_stats, _check_partials, _lazy_pair, _stats_ref
from tests.util import record_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

# name: (Cin, Cout, k, stride)
LAYERS = {"conv0.0": (3, 8, 3, 1), "conv0.1": (8, 8, 3, 1), "conv1.0": (8, 16, 5, 2), "conv1.1": (16, 16, 3, 1), "conv2.0": (16, 32, 5, 2),
          "conv2.1": (32, 32, 3, 1), "toplayer": (32, 32, 1, 1)}
# Sizes (N, H, W) of the layer's INPUT, per kernel from its tiling.
# 16x16-tile kernels (conv0.x, toplayer, the VALU data gradients): a single partial tile; an exact tile; one pixel over a tile edge in both axes; ragged
# multi-tile; several images.  Tiles N ceil(H / 16) ceil(W / 16) = 1, 2, 6, 27, 40 (and 3840 at the training size): xcd_contiguous_tile renumbers grids
# below 8, not a multiple of 8 and multiples of 8.
T16 = [(1, 3, 5), (2, 16, 16), (1, 17, 33), (3, 37, 45), (2, 50, 70)]
# Linear M-tile kernels, stride 1 (conv1.1: MT = 16, conv2.1: MT = 32; also their data gradients), npix = N H W:
#   (1, 3, 5)     npix    15: below one M-tile                              tiles % 4: 1 | 1
#   (2, 16, 16)   npix   512: % 16 = 0, % 32 = 0 (exact)                    tiles 32 | 16, % 4: 0 | 0
#   (3, 37, 45)   npix  4995: % 16 = 3, % 32 = 3, W divides neither         tiles 313 | 157, % 4: 1 | 1
#   (2, 25, 35)   npix  1750: % 16 = 6, % 32 = 22                           tiles 110 | 55, % 4: 2 | 3
#   (3, 128, 160) npix 61440: exact                                         tiles 3840 | 1920, % 4: 0 | 0
MS1 = [(1, 3, 5), (2, 16, 16), (3, 37, 45), (2, 25, 35), (3, 128, 160)]
# Stride-2 layers (conv1.0: MT = 16, conv2.0: MT = 32) and mvsnerf_conv2d_dgrad_k5s2: both parities in both axes; Ho = (H - 1) // 2 + 1, npix = N Ho Wo:
#   (1, 3, 5)     2 x 3,   npix     6: below one M-tile
#   (2, 33, 17)   17 x 9,  npix   306: % 16 = 2, % 32 = 18                  tiles 20 | 10, % 4: 0 | 2
#   (3, 37, 45)   19 x 23, npix  1311: % 16 = 15, % 32 = 31                 tiles 82 | 41, % 4: 2 | 1
#   (2, 50, 70)   25 x 35, npix  1750: % 16 = 6, % 32 = 22                  tiles 110 | 55, % 4: 2 | 3
#   (1, 2, 2)     1 x 1,   npix     1: every parity class of the data gradient has one pixel
#   (3, 128, 160) 64 x 80, npix 15360: exact                                tiles 960 | 480, % 4: 0 | 0
MS2 = [(1, 3, 5), (2, 33, 17), (3, 37, 45), (2, 50, 70), (1, 2, 2), (3, 128, 160)]
SIZES = {"conv0.0": T16 + [(3, 512, 640)], "conv0.1": T16 + [(3, 512, 640)], "conv1.0": MS2, "conv1.1": MS1, "conv2.0": MS2, "conv2.1": MS1,
         "toplayer": T16}
CASES = [(name, dims) for name in LAYERS for dims in SIZES[name]]
DGRAD_CASES = [c for c in CASES if c[0] != "conv0.0"]           # the data gradient towards the images is never needed
_ids = lambda cases: [f"{n}-{'x'.join(map(str, d))}" for n, d in cases]


def _cdiv(a, b):
    return (a + b - 1) // b


def _layer(name):
    from mvsnerf_amd import encoder as E
    cin, cout, k, stride = LAYERS[name]
    torch.manual_seed(cin * 1000 + cout * 10 + k)
    conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=name == "toplayer").to(DEV)
    return conv, E._PackedConv2d(conv)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


def _poison(*numels):
    """The allocator hands a launch's torch.empty the block of the same size freed last: fill such blocks with NaN first, so that an element or a
    partial-sum slot the launch skips cannot inherit a right value from recycled memory."""
    for n in numels:
        t = torch.full((int(n),), NAN, device=DEV)
        del t


def _check(tag, out, ref, S, y32, K, fails, yardstick=True):
    """out (fp32) against the float64 ref elementwise: the hard bound 2 (K + 8) u S and the 5 x torch-fp32 + 4 u yardstick (module docstring).
    Failures are collected so that one case reports every route.  -> (kernel err / S, torch err / S)"""
    if tuple(out.shape) != tuple(ref.shape):
        fails.append(f"{tag}: shape {tuple(out.shape)} != {tuple(ref.shape)}")
        return None
    if not bool(torch.isfinite(out).all()):
        fails.append(f"{tag}: {int((~torch.isfinite(out)).sum())} of {out.numel()} elements are not finite (never written, or a sum over unwritten partials)")
        return None
    err = (out.double() - ref).abs()
    bound = 2 * (K + 8) * U * S + 1e-30
    over = err > bound
    Sp = S.clamp_min(1e-300)
    r_k, r_t = float((err / Sp).max()), float(((y32.double() - ref).abs() / Sp).max())
    record_err(f"featnet_layer:{tag}:kernel_err_over_S", r_k, scale=float(S.max()), tol=2 * (K + 8) * U)
    record_err(f"featnet_layer:{tag}:torch_err_over_S", r_t, scale=float(S.max()))
    print(f"[{tag}] err / S: kernel {r_k:.3e}  torch fp32 {r_t:.3e}  share of 5 x torch + 4 u {r_k / (5 * r_t + 4 * U):.2f}  of the hard bound "
          f"{r_k / (2 * (K + 8) * U):.4f}")
    if bool(over.any()):
        i = int((err - bound).argmax())
        fails.append(f"{tag}: {int(over.sum())} of {over.numel()} elements over 2 (K + 8) u S; worst at flat index {i}: err {float(err.flatten()[i]):.3e}, "
                     f"bound {float(bound.flatten()[i]):.3e}")
    if yardstick and r_k > 5 * r_t + 4 * U:
        fails.append(f"{tag}: err / S {r_k:.3e} > 5 x torch fp32 ({r_t:.3e}) + 4 u")
    return r_k, r_t


def _conv_refs(op, x64, x32, w, bias=None):
    """op(x, w, bias) on NCHW operands -> channel-last (float64 value, float64 magnitude S, torch's own fp32 result)."""
    b64 = None if bias is None else bias.double()
    ref, S = op(x64, w.double(), b64), op(x64.abs(), w.double().abs(), None if b64 is None else b64.abs())
    with torch.backends.cudnn.flags(enabled=False):      # torch's native fp32 convolution: no per-shape kernel search
        y32 = op(x32, w, bias)
    return _nhwc(ref), _nhwc(S), _nhwc(y32)


def _route_kind(name):
    return "lds" if name.startswith("conv0") else ("top" if name == "toplayer" else "mfma")


def _slots(name, N, Ho, Wo):
    """(what mvsnerf_conv2d_mfma_tiles must report for the layer on this grid, i.e. the partial-sum slots of its statistics launch)"""
    kind, cout = _route_kind(name), LAYERS[name][1]
    if kind == "top":
        return 0
    if kind == "lds":
        return N * _cdiv(Ho, 16) * _cdiv(Wo, 16)
    return _cdiv(N * Ho * Wo, 32 if cout == 32 else 16)


# ------------------------------------------------------------------ 1. forward of every layer, every route
@pytest.mark.parametrize("name,dims", CASES, ids=_ids(CASES))
def test_featnet_layer_forward_every_route_vs_float64(name, dims):
    from mvsnerf_amd import encoder as E, _lib
    L = _lib.lib()
    cin, cout, k, stride = LAYERS[name]
    N, H, W = dims
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    conv, pk = _layer(name)
    w = conv.weight.detach()
    bias = None if conv.bias is None else conv.bias.detach()
    cp = pk.cin_pad
    K = k * k * cp + (0 if bias is None else 1)
    kind, nslots = _route_kind(name), _slots(name, N, Ho, Wo)
    g = torch.Generator(DEV).manual_seed(H * 131 + W * 7 + cin)
    tag0 = f"{name}:{N}x{H}x{W}"
    fails = []
    assert not E._LAYER_BF16[0] and E.FUSED_ABN_STATS              # outside every precision context: the fp32 kernels, statistics from the launch
    assert L.mvsnerf_conv2d_mfma_tiles(cp, cout, N, H, W, k, stride) == nslots, "the library reports another kernel for this layer than the table above"
    op = lambda xx, ww, bb: F.conv2d(xx, ww, bb, stride=stride, padding=k // 2)
    with torch.no_grad():
        if name == "conv0.0":
            imgs = torch.randn((N, 3, H, W), device=DEV, generator=g)
            cl4, ld = E._images_channel_last(imgs, 4)                  # what a training step's first layer reads: ld = 4, a zero fourth channel
            assert ld == 4 and torch.equal(cl4[..., :3], _nhwc(imgs)) and bool((cl4[..., 3] == 0).all())
            forms = [("plain", cl4, imgs.double(), imgs), ("nchw", E._Nchw3(imgs), imgs.double(), imgs)]
        else:
            ld = cin
            x = torch.randn((N, H, W, cin), device=DEV, generator=g)
            lz, a64, a32 = _lazy_pair(E, (N, H, W, cin), g)
            forms = [("plain", x, _nchw(x.double()), _nchw(x)), ("lazy", lz, _nchw(a64), _nchw(a32))]
        kept = {}
        for form, src, x64, x32 in forms:
            ref, S, y32 = _conv_refs(op, x64, x32, w, bias)
            tag = f"{tag0}:{form}"
            n_out = N * Ho * Wo * cout
            _poison(n_out, 2 * cout * max(nslots, 1))
            out_s, partials = E._conv2d(src, (N, H, W, ld), ld, pk.get, cp, cout, k, stride, bias=bias, want_stats=True, packed=pk)
            _check(f"{tag}:stats", out_s, ref, S, y32, K, fails)
            if kind == "top":                                          # a biased layer has no InPlaceABN behind it: the VALU kernel, nothing left
                if partials is not None:
                    fails.append(f"{tag}: statistics from the biased toplayer")
            else:
                if partials is None or partials[1] != nslots:
                    fails.append(f"{tag}: {'no statistics' if partials is None else f'{partials[1]} statistics slots'} where the route leaves {nslots}")
                _check_partials(f"{tag}:stats", partials, out_s, cout, fails)
                if partials is not None:
                    # (1, 2, 2) through a stride-2 layer is ONE value per channel: train-mode batch normalisation is not defined there (torch's own
                    # raises "Expected more than 1 value per channel"), and var = 0 against eps = 1e-5 turns the rounding of the fp32 sum of squares
                    # (<= u v^2) into up to 0.5 u v^2 / eps ~ 1e-3 of invstd, whatever the kernel.  The sums themselves are checked above.
                    if N * Ho * Wo > 1:
                        _check_abn_stats(f"2d:{tag}", E, out_s, partials, H * 7 + cin, fails)
                    kept[form] = (out_s, partials[0])
            if form != "nchw" and kind != "top":
                _poison(n_out)
                out_p = E._conv2d(src, (N, H, W, ld), ld, pk.get, cp, cout, k, stride, packed=pk)          # conv0.x: the VALU kernel; else the same kernel
                assert torch.is_tensor(out_p)
                _check(f"{tag}:no_stats", out_p, ref, S, y32, K, fails)
                if not torch.equal(out_p, out_s):
                    what = "the LDS kernel's bits are not the VALU kernel's" if kind == "lds" else "the launch without statistics differs from the one with"
                    fails.append(f"{tag}: {what}: {int((out_p != out_s).sum())} of {out_p.numel()} elements differ")
                out_p.fill_(NAN)
            if form not in kept:
                out_s.fill_(NAN)
        if name == "conv0.0" and len(kept) == 2:                       # the first layer straight from the images == on the padded channel-last copy
            (o_cl, p_cl), (o_nc, p_nc) = kept["plain"], kept["nchw"]
            if not torch.equal(o_cl, o_nc):
                fails.append(f"{tag0}: the NCHW first layer differs from the channel-last one in {int((o_cl != o_nc).sum())} elements")
            if not torch.equal(p_cl, p_nc):
                fails.append(f"{tag0}: the NCHW first layer leaves other partial sums than the channel-last one")
        for o, p in kept.values():
            o.fill_(NAN); p.fill_(NAN)
    assert set(pk.cache) == {"fwd"}
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 2. data gradients, as _FeatureNetFunction._backward issues them
@pytest.mark.parametrize("name,dims", DGRAD_CASES, ids=_ids(DGRAD_CASES))
def test_featnet_layer_dgrad_vs_float64(name, dims):
    from mvsnerf_amd import encoder as E, _lib
    from mvsnerf_amd.ops import stream_ptr
    L = _lib.lib()
    cin, cout, k, stride = LAYERS[name]
    N, H, W = dims
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    conv, pk = _layer(name)
    w = conv.weight.detach()
    g = torch.Generator(DEV).manual_seed(H * 37 + W * 3 + cout)
    go = torch.randn((N, Ho, Wo, cout), device=DEV, generator=g)
    tag = f"dgrad:{name}:{N}x{H}x{W}"
    fails = []
    assert not E._LAYER_BF16[0]
    with torch.no_grad():
        _poison(N * H * W * cin)
        if stride == 1:
            # the convolution that computes it: Cout -> Cin channels on the (Ho, Wo) = (H, W) grid, taps mirrored
            assert L.mvsnerf_conv2d_mfma_tiles(cout, cin, N, H, W, k, 1) == _slots(name, N, H, W), "another kernel than the table above"
            gx = E._conv2d(go, (N, Ho, Wo, cout), cout, lambda: pk.get("dgrad"), cout, pk.cin, k, 1, packed=pk, mode="dgrad")
            op = lambda gg, ww, bb: F.conv_transpose2d(gg, ww, stride=1, padding=k // 2)
            K = k * k * cout
        else:
            gx = torch.full((N, H, W, cin), NAN, device=DEV)
            rc = L.mvsnerf_conv2d_dgrad_k5s2(go.data_ptr(), cout, N, Ho, Wo, pk.get("dgrad").data_ptr(), cin, H, W, gx.data_ptr(), stream_ptr())
            assert rc == 0, f"mvsnerf_conv2d_dgrad_k5s2 -> {rc}"
            op = lambda gg, ww, bb: F.conv_transpose2d(gg, ww, stride=2, padding=2, output_padding=1)[:, :, :H, :W]
            K = 25 * cout
        assert set(pk.cache) == {"dgrad"}                              # the mirrored (stride 1) / role-swapped weights, not the layer's own
        ref, S, y32 = _conv_refs(op, _nchw(go.double()), _nchw(go), w)
        _check(tag, gx, ref, S, y32, K, fails)
        gx.fill_(NAN)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 3. weight gradients, both reductions
def _wgrad_parts_model(A, B, N, Ho, Wo, k):
    """Rows of partial results mvsnerf_conv2d_wgrad leaves (featnet.hip wgrad2d_nwg for the VALU kernel: one workgroup per 64 pixels, at most
    4096 / (A / 8); wgrad_mfma.hip balanced_nx for the matrix-core kernel: 8 x TOY tiles dealt evenly to at most 512 workgroups over all channel
    groups, times the work shares of a workgroup).  The two differ, so the count tells which kernel the library chose."""
    cap = 4096 // (A // 8)
    if k == 1:
        return max(1, min(N * Ho * Wo // 64, cap))
    ncg, toy = (1 if B <= 4 else (2 if B == 8 else 4)), (16 if k == 3 else 8)
    ntiles, gy, nq = _cdiv(Wo, 8) * _cdiv(Ho, toy) * N, _cdiv(_cdiv(B, 4), ncg), 4 // ncg
    nmax = min(512 // gy, cap // nq)
    return _cdiv(ntiles, _cdiv(ntiles, nmax)) * nq


@pytest.mark.parametrize("name,dims", CASES, ids=_ids(CASES))
def test_featnet_layer_wgrad_both_reductions_vs_float64(name, dims):
    """_wgrad2d as the backward calls it (sums = a _PartialSums, flushed once: gw = NULL, mvsnerf_conv2d_wgrad_parts rows, mvsnerf_partial_sum_multi)
    and on its own (sums = None: mvs_partial_sum inside the entry).  The two reductions add in different orders (two / eight running sums), so both are
    held to the bounds and not to each other.  A third, direct launch on a NaN-filled workspace shows that exactly mvsnerf_conv2d_wgrad_parts rows are written."""
    from mvsnerf_amd import encoder as E, _lib
    from mvsnerf_amd.ops import stream_ptr
    L = _lib.lib()
    B, A, k, stride = LAYERS[name]
    N, H, W = dims
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    ldx = (B + 3) // 4 * 4
    shape = (A, B, k, k)
    n_out = A * B * k * k
    K = N * Ho * Wo
    gen = torch.Generator(DEV).manual_seed(H * 53 + W * 11 + A)
    G = torch.randn((N, Ho, Wo, A), device=DEV, generator=gen)
    fails = []
    assert not E._LAYER_BF16[0]
    parts = L.mvsnerf_conv2d_wgrad_parts(A, B, N, Ho, Wo, k, stride)
    assert parts == _wgrad_parts_model(A, B, N, Ho, Wo, k), "the library's partial-row count is not that of the kernel the table above names"
    if name == "conv0.0":
        x = torch.randn((N, H, W, 4), device=DEV, generator=gen)
        x[..., 3] = 0
        forms = [("plain", x, x[..., :3].double(), x[..., :3])]
    else:
        x = torch.randn((N, H, W, B), device=DEV, generator=gen)
        lz, a64, a32 = _lazy_pair(E, (N, H, W, B), gen)
        forms = [("plain", x, x.double(), x), ("lazy", lz, a64, a32)]
    g64, g32 = _nchw(G.double()), _nchw(G)
    wg = lambda xx, gg: torch.nn.grad.conv2d_weight(xx, shape, gg, stride=stride, padding=k // 2)
    with torch.no_grad():
        for form, X, x64, x32 in forms:
            tag = f"wgrad:{name}:{N}x{H}x{W}:{form}"
            ref, S = wg(_nchw(x64), g64), wg(_nchw(x64.abs()), g64.abs())
            with torch.backends.cudnn.flags(enabled=False):
                y32 = wg(_nchw(x32).contiguous(), g32.contiguous())
            _poison(n_out)
            gw1 = E._wgrad2d(G, A, X, B, ldx, (N, Ho, Wo), (N, H, W, ldx), k, stride, shape)
            _check(f"{tag}:own_sum", gw1, ref, S, y32, K, fails)
            gw1.fill_(NAN)
            sums = E._PartialSums()
            _poison(n_out)
            gw2 = E._wgrad2d(G, A, X, B, ldx, (N, Ho, Wo), (N, H, W, ldx), k, stride, shape, sums)
            assert len(sums.jobs) == 1 and sums.jobs[0][1] == parts
            sums.flush()
            _check(f"{tag}:multi_sum", gw2, ref, S, y32, K, fails)
            gw2.fill_(NAN)
            # the partial rows themselves: gw = NULL leaves `parts` rows at the start of the workspace and touches nothing behind them
            ws = torch.full((L.mvsnerf_conv2d_wgrad_workspace_floats(A, B, k),), NAN, device=DEV)
            rc = L.mvsnerf_conv2d_wgrad(G.data_ptr(), A, *E._ptrs(X), B, ldx, N, Ho, Wo, H, W, k, stride, 0, ws.data_ptr(), stream_ptr())
            assert rc == 0, f"mvsnerf_conv2d_wgrad -> {rc}"
            rows = ws.view(-1, n_out)
            if not bool(torch.isfinite(rows[:parts]).all()):
                fails.append(f"{tag}: some of the {parts} partial rows mvsnerf_conv2d_wgrad_parts promises were not written")
            elif bool(torch.isfinite(rows[parts:]).any()):
                fails.append(f"{tag}: the launch wrote behind the {parts} partial rows mvsnerf_conv2d_wgrad_parts reports")
            else:
                _check(f"{tag}:rows", rows[:parts].double().sum(0).float().view(shape), ref, S, y32, K, fails, yardstick=False)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 4. the toplayer's bias gradient
# C = 32: 256 / C = 8 rows per workgroup pass, at most 256 workgroups (2048 rows per grid pass)
SUM_CASES = [(32, 1), (32, 7), (32, 8), (32, 9), (32, 2047), (32, 2049), (32, 3 * 128 * 160), (8, 8197), (64, 1027)]


@pytest.mark.parametrize("C,n", SUM_CASES, ids=[f"C{c}-n{n}" for c, n in SUM_CASES])
def test_channel_sum_vs_float64(C, n):
    from mvsnerf_amd import _lib
    from mvsnerf_amd.ops import stream_ptr
    L = _lib.lib()
    gen = torch.Generator(DEV).manual_seed(C * 100000 + n)
    g = torch.randn((n, C), device=DEV, generator=gen)
    out = torch.full((C,), NAN, device=DEV)
    ws = torch.full((L.mvsnerf_channel_sum_workspace_floats(C),), NAN, device=DEV)
    assert L.mvsnerf_channel_sum(g.data_ptr(), n, C, out.data_ptr(), ws.data_ptr(), stream_ptr()) == 0
    fails = []
    _check(f"channel_sum:C{C}:n{n}", out, g.double().sum(0), g.double().abs().sum(0), g.sum(0), n, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 5. InPlaceABN statistics and backward on (N, H, W, C) dims
ABN_DIMS = [(1, 3, 5), (3, 37, 45), (2, 50, 70), (3, 128, 160)]


@pytest.mark.parametrize("C", [8, 16, 32])
@pytest.mark.parametrize("dims", ABN_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_abn_stats_2d_from_the_tensor_vs_float64(C, dims):
    from mvsnerf_amd import encoder as E
    N, H, W = dims
    g = torch.Generator(DEV).manual_seed(C + N * H * W)
    x = torch.randn((N, H, W, C), device=DEV, generator=g) * 2 + 0.7
    fails = []
    _check_abn_stats(f"2d:tensor:C{C}:{N}x{H}x{W}", E, x, None, C + W, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("C", [8, 16, 32])
@pytest.mark.parametrize("dims", [(1, 3, 5), (3, 37, 45), (2, 50, 70)], ids=lambda d: "x".join(map(str, d)))
def test_abn_bwd_2d_vs_float64_autograd(C, dims):
    """mvsnerf_abn_bwd on (N, H, W, C) dims as _FeatureNetFunction._backward calls it (one upstream gradient), with the reference and the yardstick of
    test_gpu_fp32_layers.test_fp32_abn_bwd_vs_float64_autograd unchanged: per output tensor, the kernel's largest difference from float64 autograd
    relative to the tensor's float64 maximum within 5 x that of the same autograd in float32 on the CPU + 8 u; no pre-activation within 1e-4 of the kink."""
    from mvsnerf_amd import encoder as E
    N, H, W = dims
    n = N * H * W
    g = torch.Generator(DEV).manual_seed(C * 1000 + n)
    x = torch.randn((N, H, W, C), device=DEV, generator=g) * 1.5 + 0.3
    bn = E.InPlaceABN(C).to(DEV)
    with torch.no_grad():
        wv = torch.rand(C, device=DEV, generator=g) + 0.5
        wv[1::3] *= -1
        bn.weight.copy_(wv); bn.bias.copy_(torch.randn(C, device=DEV, generator=g) * 0.5)

        def pre64(xx):
            sc, shf, _, _, _ = _stats_ref(xx, bn.weight, bn.bias, bn.eps)
            return xx.double() * sc + shf, sc
        p, sc = pre64(x)
        near = p.abs() < 4e-3
        x = torch.where(near, ((torch.where(p >= 0, 8e-3, -8e-3) - p) / sc + x.double()).float(), x)
        p, _ = pre64(x)
        assert float(p.abs().min()) >= 1e-4, "a pre-activation lies within 1e-4 of the kink"
        g1 = torch.randn((N, H, W, C), device=DEV, generator=g)
        scale, shift, mean, invstd = E._abn_stats(x, n, bn, update_running=False)
        lz = E._Lazy(x, scale, shift, (N, H, W, C), mean, invstd)
        gx, gw, gb = E._abn_bwd(lz, bn, g1)
        assert bool(((torch.addcmul(shift, x, scale) > 0) == (p > 0)).all())
    ref = _abn_autograd(x.double(), bn.weight.double(), bn.bias.double(), g1.double(), bn.eps)
    cpu = _abn_autograd(x.cpu(), bn.weight.cpu(), bn.bias.cpu(), g1.cpu(), bn.eps)
    fails = []
    for nm, kk, r, c in zip(("gx", "g_weight", "g_bias"), (gx, gw, gb), ref, cpu):
        top = float(r.abs().max())
        e_k = float((kk.double().reshape(r.shape) - r).abs().max()) / top
        e_c = float((c.double().to(DEV) - r).abs().max()) / top
        record_err(f"featnet_abn_bwd:C{C}:{N}x{H}x{W}:{nm}:kernel", e_k, scale=top)
        record_err(f"featnet_abn_bwd:C{C}:{N}x{H}x{W}:{nm}:cpu_fp32", e_c, scale=top)
        print(f"[abn_bwd 2d C={C} {N}x{H}x{W} {nm}] err / max: kernel {e_k:.3e}  CPU fp32 autograd {e_c:.3e}")
        if not e_k <= 5 * e_c + 8 * U:
            fails.append(f"{nm}: kernel {e_k:.3e} > 5 x CPU fp32 {e_c:.3e} + 8 u")
    assert not fails, "\n".join(fails)
