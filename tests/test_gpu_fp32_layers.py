"""The fp32 family of CostRegNet's 3-D layers (csrc/conv_mfma.hip and the convolution / transposed-convolution / InPlaceABN kernels of
csrc/conv3d.hip and csrc/abn.hip; reference models.py:674-685, 725-769), layer by layer against float64 on exactly the kernel's fp32 operands: forward and
data gradient of every layer through every route encoder._conv / encoder._conv_t can take, the statistics that leave with a launch, the
InPlaceABN statistics / backward / apply-and-add kernels and the depth-fastest output sum.  Sizes have ragged last tiles in every dimension,
odd sizes for the strided layers, one single partial tile and one with more than one full tile plus a remainder per tile dimension.

route -> kernel (read against encoder._conv / _conv_t and the dispatchers in conv3d.hip / conv_mfma.hip):
  _conv   packed=pk, one source (plain | _Lazy)   conv1, dgrad of conv11            conv3d_k3_mfma16_kernel<8, 2>          (32 voxels / wave, 4 waves)
                                                  conv3 .. conv6, their s1 dgrads,
                                                  dgrad of conv7 / conv9            conv3d_k3_mfma32_kernel                (32 voxels / workgroup)
                                                  conv2 with want_stats             conv3d_k3s1_tiled_kernel<16,16,16> + statistics (mvsnerf_conv3d_fwd_stats; 8x8x4 tiles)
  _conv   packed=None | two sources               stride 1 (and dgrad 8 -> Cin_pad) conv3d_k3s1_tiled_kernel               (mvsnerf_conv3d_fwd; 8x8x4 tiles)
                                                  stride 2                          conv3d_k3_kernel                       (mvsnerf_conv3d_fwd; 256 voxels / workgroup)
  mvsnerf_conv3d_fwd, Cout = 8, stride 1, one source, Cin in 32 .. 56               conv3d_k3s1_c8_mfma_kernel             (16x16x4 tiles)
  _conv_t packed=pk, 16 -> 8 (conv11, dgrad of conv1), any sources                  convT3d_k3s2_c16to8_mfma4_kernel       (16x8x2 input tiles)
  _conv_t packed=pk, plain tensor                 conv7, conv9, dgrad of conv3 / 5  convT3d_k3s2_mfma32_kernel             (32 input positions / M-tile)
  _conv_t packed=None | _Lazy source(s)           conv7, conv9, (conv11)            convT3d_k3s2_kernel                    (mvsnerf_conv_transpose3d_fwd; 256 voxels / workgroup)
  _abn_stats                                      abn_partial_kernel + abn_finalize_kernel; partials=...: abn_finalize_kernel alone
  _abn_bwd                                        abn_bwd_partial_kernel, abn_bwd_finalize_kernel, abn_bwd_apply_kernel
  _apply_add / _neural_volume                     abn_apply_add_kernel / abn_apply_add_hwdc_kernel (32 depth planes x 16 columns through LDS)

Bound of a convolution, per output ELEMENT (a border voxel cannot hide behind the interior maximum): with K = 27 Cin products, u = 2^-24 and
S = conv(|x|, |w|) in float64,  |out - ref| <= 2 (K + 8) u S + 1e-30.  Any fp32 summation order gives (K + 2) u S with round-to-nearest
operations; + 6 for the fma of a pending activation and the sum of two sources; the factor 2 for a matrix-core accumulator that truncates.
Yardstick beside it: the largest err / S of torch's own fp32 convolution of the same operands on the same GPU; the kernel's must stay within
5 x that + 4 u."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.util import record_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24

# name: (Cin, Cout, stride, transposed)
LAYERS = {"conv1": (8, 16, 2, False), "conv2": (16, 16, 1, False), "conv3": (16, 32, 2, False), "conv4": (32, 32, 1, False),
          "conv5": (32, 64, 2, False), "conv6": (64, 64, 1, False), "conv7": (64, 32, 2, True), "conv9": (32, 16, 2, True),
          "conv11": (16, 8, 2, True)}
# input sizes (D, H, W): a single partial tile of every kernel on the route; ragged (odd for the strided layers); the even sizes of
# test_gpu_bf16_layers.LAYERS; and one size with more than one full tile plus a remainder in every tile dimension of the tiled kernels
# (forward and data gradient: 8x8x4 VALU tiles, 16x8x2 input tiles of the 16 -> 8 transposed kernel) and several M-tiles plus a remainder
# of the flat ones (32 / 128 voxels); the three full-resolution layers also at the large ragged sizes of that table
SIZES = {
    "conv1": [(3, 4, 5), (11, 21, 37), (12, 20, 36), (25, 39, 41), (96, 130, 172)],
    "conv2": [(3, 5, 7), (9, 13, 21), (9, 19, 21), (5, 19, 35), (50, 70, 78)],
    "conv3": [(3, 4, 5), (11, 15, 19), (10, 14, 18)],
    "conv4": [(2, 3, 5), (6, 10, 14), (9, 17, 19)],
    "conv5": [(3, 4, 5), (9, 13, 11), (8, 12, 12)],
    "conv6": [(2, 3, 5), (4, 6, 10), (9, 17, 18)],
    "conv7": [(1, 2, 3), (4, 5, 7), (3, 6, 8)],
    "conv9": [(1, 2, 3), (6, 7, 9), (5, 8, 10)],
    "conv11": [(1, 3, 5), (8, 12, 20), (5, 19, 35), (24, 40, 48), (48, 65, 86)],
}
CASES = [(name, dims) for name in LAYERS for dims in SIZES[name]]


def _layer(cin, cout, stride, transposed, seed):
    torch.manual_seed(seed)
    conv = (nn.ConvTranspose3d(cin, cout, 3, padding=1, output_padding=1, stride=2, bias=False) if transposed
            else nn.Conv3d(cin, cout, 3, stride=stride, padding=1, bias=False))
    return conv.to(DEV)


def _nc(x):
    """channel-last (D, H, W, C) -> (1, C, D, H, W)"""
    return x.permute(3, 0, 1, 2)[None]


def _cl(y):
    return y[0].permute(1, 2, 3, 0)


def _layer_op(x, w, stride, transposed):
    """The layer itself on NCDHW operands of any dtype."""
    if transposed:
        return F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1)
    return F.conv3d(x, w, stride=stride, padding=1)


def _adjoint_op(g, w, stride, transposed, in_dims):
    """The layer's data gradient (test_gpu_bf16_layers.py:76-92), cropped where an odd input has one row fewer than twice the output."""
    if transposed:
        return F.conv3d(g, w, stride=2, padding=1)
    if stride == 1:
        return F.conv_transpose3d(g, w, stride=1, padding=1)
    D, H, W = in_dims
    return F.conv_transpose3d(g, w, stride=2, padding=1, output_padding=1)[:, :, :D, :H, :W]


def _act64(x, sc, sh):
    return F.leaky_relu(x.double() * sc.double() + sh.double(), 0.01)


def _act32(x, sc, sh):
    return F.leaky_relu(torch.addcmul(sh, x, sc), 0.01)


def _lazy_pair(E, shape, g):
    """A raw tensor with a pending InPlaceABN, as CostRegNet._run hands a layer its input -> (_Lazy, its float64 value, its fp32 torch value)."""
    C = shape[-1]
    x = torch.randn(shape, device=DEV, generator=g)
    sc, sh = torch.rand(C, device=DEV, generator=g) + 0.5, torch.randn(C, device=DEV, generator=g) * 0.3
    return E._Lazy(x, sc, sh, shape), _act64(x, sc, sh), _act32(x, sc, sh)


def _check_conv(tag, out, op, x64, x32, w, K, fails, crop=None):
    """out (channel-last, fp32) against op(x64, w64): the hard per-element bound and the 5 x torch-fp32 yardstick (module docstring).
    Failures are collected so that one case reports every route."""
    w64 = w.double()
    ref, S = _cl(op(x64, w64)), _cl(op(x64.abs(), w64.abs()))
    with torch.backends.cudnn.flags(enabled=False):      # torch's native fp32 convolution (vol2col + sgemm): no per-shape kernel search
        y32 = _cl(op(x32, w))
    if crop is not None:
        out = out[:crop[0], :crop[1], :crop[2]]
    if tuple(out.shape) != tuple(ref.shape):
        fails.append(f"{tag}: shape {tuple(out.shape)} != {tuple(ref.shape)}")
        return
    if not bool(torch.isfinite(out).all()):
        fails.append(f"{tag}: non-finite output")
        return
    err = (out.double() - ref).abs()
    bound = 2 * (K + 8) * U * S + 1e-30
    over = err > bound
    Sp = S.clamp_min(1e-300)
    r_k, r_t = float((err / Sp).max()), float(((y32.double() - ref).abs() / Sp).max())
    record_err(f"fp32_layer:{tag}:kernel_err_over_S", r_k, scale=float(S.max()), tol=2 * (K + 8) * U)
    record_err(f"fp32_layer:{tag}:torch_err_over_S", r_t, scale=float(S.max()))
    print(f"[{tag}] err / S: kernel {r_k:.3e}  torch fp32 {r_t:.3e}  ratio {r_k / max(r_t, 1e-300):.2f}  hard bound {2 * (K + 8) * U:.3e}")
    if bool(over.any()):
        i = int((err - bound).argmax())
        fails.append(f"{tag}: {int(over.sum())} of {over.numel()} elements over 2 (K + 8) u S; worst at flat index {i}: err {float(err.flatten()[i]):.3e}, "
                     f"bound {float(bound.flatten()[i]):.3e}")
    # Measured on an MI355X (the records tests.util.record_err appends, tags fp32_layer:*), largest err / S over the 271 launches this module checks:
    # kernel 5.3e-7 (9 u), torch fp32 4.7e-7.  Kernel / torch per launch: 0.3 .. 1.5 for the 32x32x2 matrix-core kernels on a plain input
    # (conv3 .. conv9 and their data gradients), up to 3.4 for conv1 / conv11 / the Cout = 8 kernel, up to 4.3 for the VALU kernels, 5.4 once
    # (data gradient of conv2 on 3x5x7, where torch's maximum over 1680 elements is 0.7 u).  The largest share of 5 x torch + 4 u any launch
    # uses is 0.55 (conv6, lazy input, VALU kernel); of the hard bound 0.02 (conv1, lazy input).  Every route meets the yardstick.
    if r_k > 5 * r_t + 4 * U:
        fails.append(f"{tag}: err / S {r_k:.3e} > 5 x torch fp32 ({r_t:.3e}) + 4 u")


def _check_partials(tag, partials, out, cout, fails):
    """The InPlaceABN partial sums of a launch: relative 1e-6 against float64 sums of the output it wrote (test_gpu_bf16_layers.py:70-75)."""
    if partials is None:
        fails.append(f"{tag}: the route left no statistics (fell through to another kernel)")
        return
    part, nblk = partials
    s = part.view(2, cout, nblk).double().sum(2)
    o64 = out.double()
    e0 = float((s[0] - o64.sum((0, 1, 2))).abs().max()) / float(o64.abs().sum((0, 1, 2)).max())
    e1 = float((s[1] - (o64 ** 2).sum((0, 1, 2))).abs().max()) / float((o64 ** 2).sum((0, 1, 2)).max())
    if not (e0 < 1e-6 and e1 < 1e-6):
        fails.append(f"{tag}: partial sums off by {e0:.2e} (sum), {e1:.2e} (sum of squares) relative")


def _stats_ref(raw, bn_weight, bn_bias, eps):
    xf = raw.reshape(-1, raw.shape[-1]).double()
    mean, var = xf.mean(0), xf.var(0, unbiased=False)
    invstd = 1 / torch.sqrt(var + eps)
    scale = (bn_weight.double().abs() + eps) * invstd
    return scale, bn_bias.double() - mean * scale, mean, invstd, var * (xf.shape[0] / max(xf.shape[0] - 1, 1))


def _check_abn_stats(tag, E, raw, partials, seed, fails):
    """encoder._abn_stats (from the tensor: partials None; or stage 2 alone on a producer's partial sums) against float64: the bounds of
    test_abn_stats_and_conv_vs_torch_full_size (1e-6 on scale, mean, invstd, running mean; 1e-5 on shift), relative to the value where it
    exceeds 1 (a conv output's invstd and scale do); the running variance like the running mean."""
    C = raw.shape[-1]
    g = torch.Generator().manual_seed(seed)
    bn = E.InPlaceABN(C).to(DEV)
    with torch.no_grad():
        w = torch.rand(C, generator=g) + 0.5
        w[::3] *= -1                                     # InPlaceABN takes |weight| + eps
        bn.weight.copy_(w); bn.bias.copy_(torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g)); bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        rm0, rv0 = bn.running_mean.double().clone(), bn.running_var.double().clone()
        n = raw.numel() // C
        got = E._abn_stats(raw, n, bn, update_running=True, partials=partials)
        E._flush_nbt()
        sc, shf, mean, invstd, unb = _stats_ref(raw, bn.weight, bn.bias, bn.eps)
        m = bn.momentum
        pairs = (("scale", got[0], sc, 1e-6), ("shift", got[1], shf, 1e-5), ("mean", got[2], mean, 1e-6), ("invstd", got[3], invstd, 1e-6),
                 ("running_mean", bn.running_mean, (1 - m) * rm0 + m * mean, 1e-6), ("running_var", bn.running_var, (1 - m) * rv0 + m * unb, 1e-6))
        for name, a, b, tol in pairs:
            e, mag = float((a.double() - b).abs().max()), max(1.0, float(b.abs().max()))
            record_err(f"fp32_abn_stats:{tag}:{name}", e, scale=mag, tol=tol * mag)
            if not e < tol * mag:
                fails.append(f"{tag}: _abn_stats {name} off by {e:.3e} (bound {tol * mag:.1e})")
        if int(bn.num_batches_tracked) != 1:
            fails.append(f"{tag}: num_batches_tracked = {int(bn.num_batches_tracked)}")


def _supported(E, cin, cout, stride):
    from mvsnerf_amd import _lib
    return _lib.lib().mvsnerf_conv3d_mfma_supported(cin, cout, stride) == 1


# ------------------------------------------------------------------ 1. forward of every layer, every route
@pytest.mark.parametrize("name,dims", CASES, ids=[f"{n}-{'x'.join(map(str, d))}" for n, d in CASES])
def test_fp32_layer_forward_every_route_vs_float64(name, dims):
    from mvsnerf_amd import encoder as E, _lib
    L = _lib.lib()
    cin, cout, stride, transposed = LAYERS[name]
    D, H, W = dims
    shape = (D, H, W, cin)
    conv = _layer(cin, cout, stride, transposed, cin * 100 + cout)
    pk = E._PackedConv(conv, transposed)
    w = conv.weight.detach()
    g = torch.Generator(DEV).manual_seed(D * 31 + W)
    x = torch.randn(shape, device=DEV, generator=g)
    l1, a1_64, a1_32 = _lazy_pair(E, shape, g)
    l2, a2_64, a2_32 = _lazy_pair(E, shape, g)
    op = lambda xx, ww: _layer_op(xx, ww, stride, transposed)
    K = 27 * cin
    tag0 = f"{name}:{D}x{H}x{W}"
    fails = []
    assert not E._LAYER_BF16[0] and E._LAYER_F16X3[0] is None          # outside every precision context: the fp32 kernels
    operands = {"plain": (x, None, _nc(x.double()), _nc(x)),
                "lazy": (l1, None, _nc(a1_64), _nc(a1_32)),
                "two_lazy": (l1, l2, _nc(a1_64 + a2_64), _nc(a1_32 + a2_32))}
    with torch.no_grad():
        assert L.mvsnerf_conv3d_mfma_supported(8, 16, 2) == 1, "the matrix-core kernels are switched off"
        for kind, (s1, s2, x64, x32) in operands.items():
            for packed in (pk, None):
                tag = f"{tag0}:{kind}:{'packed' if packed is not None else 'stable'}"
                if transposed:
                    # which kernel _conv_t picks (asserted through what it leaves: only the matrix-core kernels leave statistics)
                    c8 = packed is not None and L.mvsnerf_conv_transpose3d_c8_supported(cin, cout) == 1
                    m32 = packed is not None and not c8 and kind == "plain" and L.mvsnerf_conv_transpose3d_mfma_supported(cin, cout) == 1
                    if packed is not None and kind == "plain":
                        assert c8 or m32, "no matrix-core kernel for a transposed layer"
                    out, partials = E._conv_t(s1, s2, shape, pk.get, cin, cout, packed=packed, want_stats=True)
                    if m32:              # conv7 / conv9 also have an entry without statistics (mvsnerf_conv_transpose3d_mfma_fwd)
                        plain = E._conv_t(s1, s2, shape, pk.get, cin, cout, packed=packed)
                        if not torch.equal(plain, out):
                            fails.append(f"{tag}: the launch without statistics differs from the one with")
                    want_partials = c8 or m32
                else:
                    m = packed is not None and s2 is None and _supported(E, cin, cout, stride)
                    if packed is not None and s2 is None and name != "conv2":
                        assert m, "no matrix-core kernel for this layer"
                    out, partials = E._conv(s1, s2, shape, cin, pk.get, cin, cout, stride, packed=packed, want_stats=True)
                    want_partials = m or (s2 is None and (cin, cout, stride) == (16, 16, 1))       # conv2: mvsnerf_conv3d_fwd_stats, packed or not
                _check_conv(tag, out, op, x64, x32, w, K, fails)
                if want_partials:
                    _check_partials(tag, partials, out, cout, fails)
                    if partials is not None and kind != "two_lazy":
                        _check_abn_stats(tag, E, out, partials, D * 7 + cin, fails)
                elif partials is not None:
                    fails.append(f"{tag}: statistics from a route that should have none: the dispatch is not the one this test describes")
                out.fill_(float("nan"))          # the allocator hands the next route this memory again: a voxel it skips must not inherit a right value
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ conv0's stable-tier kernel: Cout = 8, stride 1 through mvsnerf_conv3d_fwd
C8_CASES = [(0, (3, 5, 7)), (0, (9, 35, 37)), (1, (5, 17, 19)), (2, (5, 17, 19)), (3, (9, 35, 37)), (3, (4, 16, 16)), (5, (5, 17, 19)),
            (6, (5, 17, 19)), (7, (3, 5, 7)), (7, (9, 35, 37))]


def _conv0_layer(V):
    torch.manual_seed(900 + V)
    return nn.Conv3d(32 + 3 * V, 8, 3, padding=1, bias=False).to(DEV)


@pytest.mark.parametrize("V,dims", C8_CASES, ids=[f"cin{(32 + 3 * v + 3) // 4 * 4}-{'x'.join(map(str, d))}" for v, d in C8_CASES])
def test_fp32_c8_stride1_forward_through_the_stable_entry(V, dims):
    """mvsnerf_conv3d_fwd with Cout = 8, stride 1, cin_ld == Cin in {32, 36, 40, 44, 48, 52, 56}: conv3d_k3s1_c8_mfma_kernel (16x16x4 tiles), which
    the product itself never launches (it hands conv0 a channel-blocked volume).  Weights packed by mvsnerf_conv3d_pack_weights from a layer with
    32 + 3 V real channels, zero padding; the input's padding channels hold values (their weights are zero)."""
    from mvsnerf_amd import _lib
    from mvsnerf_amd import encoder as E
    from mvsnerf_amd.ops import stream_ptr
    L = _lib.lib()
    conv = _conv0_layer(V)
    w = conv.weight.detach().contiguous()
    cr = 32 + 3 * V
    cp = (cr + 3) // 4 * 4
    D, H, W = dims
    g = torch.Generator(DEV).manual_seed(V * 131 + W)
    wp = torch.full((27 * cp * 8,), float("nan"), device=DEV)
    assert L.mvsnerf_conv3d_pack_weights(w.data_ptr(), cr, 8, cp, 8, 27, cr * 27, 0, wp.data_ptr(), stream_ptr()) == 0
    assert L.mvsnerf_conv3d_mfma_supported(8, 16, 2) == 1, "the matrix-core kernels are switched off: mvsnerf_conv3d_fwd would take the VALU kernel"
    x = torch.randn((D, H, W, cp), device=DEV, generator=g)
    lz, a64, a32 = _lazy_pair(E, (D, H, W, cp), g)
    op = lambda xx, ww: F.conv3d(xx, ww, padding=1)
    fails = []
    with torch.no_grad():
        for kind, ptrs, x64, x32 in (("plain", (x.data_ptr(), 0, 0), x.double(), x),
                                     ("lazy", (lz.x.data_ptr(), lz.scale.data_ptr(), lz.shift.data_ptr()), a64, a32)):
            out = torch.full((D, H, W, 8), float("nan"), device=DEV)
            assert L.mvsnerf_conv3d_fwd(*ptrs, 0, 0, 0, cp, cp, D, H, W, wp.data_ptr(), 8, 1, out.data_ptr(), stream_ptr()) == 0
            _check_conv(f"c8s1:{cp}->8:{D}x{H}x{W}:{kind}", out, op, _nc(x64[..., :cr]), _nc(x32[..., :cr].contiguous()), w, 27 * cr, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 2. data gradients, as _costreg_backward issues them
@pytest.mark.parametrize("name,dims", CASES, ids=[f"{n}-{'x'.join(map(str, d))}" for n, d in CASES])
def test_fp32_layer_dgrad_vs_float64(name, dims):
    from mvsnerf_amd import encoder as E
    cin, cout, stride, transposed = LAYERS[name]
    D, H, W = dims
    conv = _layer(cin, cout, stride, transposed, cin * 100 + cout)
    pk = E._PackedConv(conv, transposed)
    w = conv.weight.detach()
    Do, Ho, Wo = (2 * D, 2 * H, 2 * W) if transposed else ((D - 1) // stride + 1, (H - 1) // stride + 1, (W - 1) // stride + 1)
    g = torch.Generator(DEV).manual_seed(D * 37 + W)
    go = torch.randn((Do, Ho, Wo, cout), device=DEV, generator=g)
    op = lambda gg, ww: _adjoint_op(gg, ww, stride, transposed, dims)
    fails = []
    assert not E._LAYER_BF16[0]
    with torch.no_grad():
        if transposed:
            assert _supported(E, cout, cin, 2)
            gx = E._conv(go, None, (Do, Ho, Wo, cout), cout, lambda: pk.get("dgrad"), cout, pk.cin, 2, packed=pk, mode="dgrad")
        elif stride == 1:
            assert name == "conv2" or _supported(E, cout, pk.cin_pad, 1)
            gx = E._conv(go, None, (Do, Ho, Wo, cout), cout, lambda: pk.get("dgrad"), cout, pk.cin_pad, 1, packed=pk, mode="dgrad")
        else:
            gx = E._conv_t(go, None, (Do, Ho, Wo, cout), lambda: pk.get("dgrad"), cout, pk.cin_pad, packed=pk, mode="dgrad")
        _check_conv(f"dgrad:{name}:{D}x{H}x{W}", gx, op, _nc(go.double()), _nc(go), w, 27 * cout, fails, crop=dims)
        gx.fill_(float("nan"))               # (as in the forward test: nothing stale for a later launch of the same size)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("V,dims", C8_CASES, ids=[f"cin{(32 + 3 * v + 3) // 4 * 4}-{'x'.join(map(str, d))}" for v, d in C8_CASES])
def test_fp32_conv0_dgrad_and_variance_slice_vs_float64(V, dims):
    """conv0's data gradient 8 -> Cin_pad (_CostRegFunction.backward) and the variance-channel slice 8 -> 32 of _SweepRegFunction.backward
    (pk.get_dgrad_slice(3 V, 32)): conv3d_k3s1_tiled_kernel<8, Cin_pad, Cin_pad> / <8, 32, 32>."""
    from mvsnerf_amd import encoder as E
    conv = _conv0_layer(V)
    pk = E._PackedConv(conv, False)
    w = conv.weight.detach()
    D, H, W = dims
    g = torch.Generator(DEV).manual_seed(V * 17 + H)
    go = torch.randn((D, H, W, 8), device=DEV, generator=g)
    fails = []
    with torch.no_grad():
        gx = E._conv(go, None, (D, H, W, 8), 8, lambda: pk.get("dgrad"), 8, pk.cin_pad, 1, packed=pk, mode="dgrad")
        assert tuple(gx.shape) == (D, H, W, pk.cin_pad)
        if pk.cin_pad > pk.cin and not bool((gx[..., pk.cin:] == 0).all()):
            fails.append("the padding channels of the data gradient are not zero")
        op = lambda gg, ww: F.conv_transpose3d(gg, ww, stride=1, padding=1)
        _check_conv(f"dgrad:conv0:8->{pk.cin_pad}:{D}x{H}x{W}", gx[..., :pk.cin], op, _nc(go.double()), _nc(go), w, 27 * 8, fails)
        gs = E._conv(go, None, (D, H, W, 8), 8, pk.get_dgrad_slice(3 * V, 32), 8, 32, 1)
        ws = w[:, 3 * V:3 * V + 32].contiguous()          # the slice is channels 3V .. 3V + 31 of the full float64 data gradient
        _check_conv(f"dgrad_slice:conv0:{pk.cin_pad}[{3 * V}:{3 * V + 32}]:{D}x{H}x{W}", gs, op, _nc(go.double()), _nc(go), ws, 27 * 8, fails)
        gx.fill_(float("nan")); gs.fill_(float("nan"))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 3. InPlaceABN pieces and the output sum
# voxel counts: below one workgroup (256 threads), not a multiple of the grid-stride (blocks x 256 / (C / 4) voxels), beyond the 1024-block cap
ABN_DIMS = [(1, 1, 37), (3, 5, 17), (1, 61, 67), (23, 31, 211)]


@pytest.mark.parametrize("C", [8, 16, 32, 64])
@pytest.mark.parametrize("dims", ABN_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_fp32_abn_stats_from_the_tensor_vs_float64(C, dims):
    from mvsnerf_amd import encoder as E
    D, H, W = dims
    g = torch.Generator(DEV).manual_seed(C + D * H * W)
    x = torch.randn((D, H, W, C), device=DEV, generator=g) * 2 + 0.7
    fails = []
    _check_abn_stats(f"tensor:C{C}:n{D * H * W}", E, x, None, C + W, fails)
    assert not fails, "\n".join(fails)


def _abn_autograd(x, w, b, gy, eps):
    """leaky_relu(batch_norm(x; |w| + eps, b), 0.01) with batch statistics (biased variance) -> (d x, d w, d b) for the upstream gradient gy."""
    x, w, b = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    C = x.shape[-1]
    y = F.leaky_relu(F.batch_norm(x.reshape(-1, C), None, None, w.abs() + eps, b, True, 0.0, eps), 0.01)
    (y * gy.reshape(-1, C)).sum().backward()
    return x.grad, w.grad, b.grad


@pytest.mark.parametrize("two", [False, True], ids=["one_grad", "two_grads"])
@pytest.mark.parametrize("C", [8, 16, 32, 64])
@pytest.mark.parametrize("dims", [(3, 5, 7), (7, 9, 13), (23, 31, 37)], ids=lambda d: "x".join(map(str, d)))
def test_fp32_abn_bwd_vs_float64_autograd(C, dims, two):
    """mvsnerf_abn_bwd against float64 autograd.  Yardstick (no bound can be derived for reductions of unknown order): the same autograd in
    float32 on the CPU; per output tensor, the kernel's largest difference from float64 relative to the tensor's float64 maximum must be
    within 5 x the CPU's + 8 u.  No pre-activation lies within 1e-4 of the kink of the leaky ReLU (asserted), so every element counts."""
    from mvsnerf_amd import encoder as E
    D, H, W = dims
    n = D * H * W
    g = torch.Generator(DEV).manual_seed(C * 1000 + n + int(two))
    x = torch.randn((D, H, W, C), device=DEV, generator=g) * 1.5 + 0.3
    bn = E.InPlaceABN(C).to(DEV)
    with torch.no_grad():
        wv = torch.rand(C, device=DEV, generator=g) + 0.5
        wv[1::3] *= -1
        bn.weight.copy_(wv); bn.bias.copy_(torch.randn(C, device=DEV, generator=g) * 0.5)

        def pre64(xx):
            sc, shf, _, _, _ = _stats_ref(xx, bn.weight, bn.bias, bn.eps)
            return xx.double() * sc + shf, sc
        # move the elements whose pre-activation is near zero away from it (one pass; the statistics move by far less than the margin)
        p, sc = pre64(x)
        near = p.abs() < 4e-3
        x = torch.where(near, ((torch.where(p >= 0, 8e-3, -8e-3) - p) / sc + x.double()).float(), x)
        p, _ = pre64(x)
        assert float(p.abs().min()) >= 1e-4, "a pre-activation lies within 1e-4 of the kink"
        g1 = torch.randn((D, H, W, C), device=DEV, generator=g)
        g2 = torch.randn((D, H, W, C), device=DEV, generator=g) if two else None
        scale, shift, mean, invstd = E._abn_stats(x, n, bn, update_running=False)
        lz = E._Lazy(x, scale, shift, (D, H, W, C), mean, invstd)
        gx, gw, gb = E._abn_bwd(lz, bn, g1, g2)
        # the kernel's own pre-activation (fp32 scale / shift) has the sign of the float64 one
        assert bool(((torch.addcmul(shift, x, scale) > 0) == (p > 0)).all())
    gy64 = g1.double() + (g2.double() if two else 0)
    ref = _abn_autograd(x.double(), bn.weight.double(), bn.bias.double(), gy64, bn.eps)
    gy32 = (g1 + g2 if two else g1).cpu()
    cpu = _abn_autograd(x.cpu(), bn.weight.cpu(), bn.bias.cpu(), gy32, bn.eps)
    fails = []
    for nm, k, r, c in zip(("gx", "g_weight", "g_bias"), (gx, gw, gb), ref, cpu):
        top = float(r.abs().max())
        e_k = float((k.double().reshape(r.shape) - r).abs().max()) / top
        e_c = float((c.double().to(DEV) - r).abs().max()) / top
        record_err(f"fp32_abn_bwd:C{C}:n{n}:{'2' if two else '1'}:{nm}:kernel", e_k, scale=top)
        record_err(f"fp32_abn_bwd:C{C}:n{n}:{'2' if two else '1'}:{nm}:cpu_fp32", e_c, scale=top)
        print(f"[abn_bwd C={C} n={n} grads={1 + int(two)} {nm}] err / max: kernel {e_k:.3e}  CPU fp32 autograd {e_c:.3e}")
        # Measured on an MI355X (tags fp32_abn_bwd:*), largest over the 24 cases, kernel | CPU fp32 autograd: gx 2.1e-7 | 3.0e-7,
        # g_weight 2.6e-7 | 9.5e-7, g_bias 6.4e-7 | 1.3e-6 (smallest CPU figure 0.4e-7); the largest share of 5 x CPU + 8 u a case uses is 0.45 (g_bias)
        if not e_k <= 5 * e_c + 8 * U:
            fails.append(f"{nm}: kernel {e_k:.3e} > 5 x CPU fp32 {e_c:.3e} + 8 u")
    assert not fails, "\n".join(fails)


APPLY_DIMS = [(37, 1, 19), (5, 3, 50), (70, 2, 33), (32, 24, 32)]       # D not a multiple of 32, W not of 16, H = 1; a network-like size


@pytest.mark.parametrize("dims", APPLY_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_fp32_apply_add_and_neural_volume_vs_float64(dims):
    """out = leaky(a * s + t) [+ leaky(b * s' + t')]: one fma, one select (times 0.01) and one add per element -> 4 u (|a| + |b|) on the activated
    values; the depth-fastest neural volume equals the channel-last one bit for bit (same fp32 arithmetic per element)."""
    from mvsnerf_amd import encoder as E
    D, H, W = dims
    g = torch.Generator(DEV).manual_seed(D * 100 + W)
    fails = []
    with torch.no_grad():
        for C in (8, 16, 32, 64):
            la, a64, _ = _lazy_pair(E, (D, H, W, C), g)
            lb, b64, _ = _lazy_pair(E, (D, H, W, C), g)
            for two in (False, True):
                out = E._apply_add(la, lb if two else None)
                ref = a64 + (b64 if two else 0)
                bound = 4 * U * (a64.abs() + (b64.abs() if two else 0))
                err = (out.double() - ref).abs()
                record_err(f"fp32_apply_add:C{C}:{D}x{H}x{W}:{1 + int(two)}", float((err / bound.clamp_min(1e-300)).max()) * 4 * U)
                if not bool((err <= bound).all()):
                    fails.append(f"_apply_add C={C} sources={1 + int(two)}: {int((err > bound).sum())} elements over 4 u (|a| + |b|)")
            if C == 8:
                assert E.VOLUME_LAYOUT == "hwdc"
                vol = E._neural_volume(la, lb)
                assert tuple(vol.shape) == (1, 8, D, H, W) and vol.stride(2) == 8 and vol.stride(4) == D * 8, "not the depth-fastest layout"
                dhwc = E._cl_view_to_ncdhw(E._apply_add(la, lb))
                if not torch.equal(vol, dhwc):
                    fails.append(f"the depth-fastest volume differs from the channel-last one in {int((vol != dhwc).sum())} elements")
                err = (vol.double() - _nc(a64 + b64)).abs()
                if not bool((err <= _nc(4 * U * (a64.abs() + b64.abs()))).all()):
                    fails.append("_neural_volume over 4 u (|a| + |b|)")
    assert not fails, "\n".join(fails)
