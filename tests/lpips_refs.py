"""The yardstick of the LPIPS tests: LPIPS-VGG restated on torch CPU ops (F.conv2d, F.max_pool2d, the channel normalisation with its 1e-10, the 1x1 heads),
parametrised by dtype and run in float64, plus the seeded weight recipe the tests draw their networks from.  NCHW inside, channel-last at the borders
(the library's convention).  It follows the published definition (Zhang et al. 2018; lpips 0.1 `LPIPS(net='vgg')`: scaling layer, taps after relu1_2,
relu2_2, relu3_3, relu4_3, relu5_3, normalize_tensor, spatial mean, sum over layers); the lpips package is not in this image, so nothing here is pinned
against it."""
import functools

import torch
import torch.nn.functional as F

VGG_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
TAPS = (1, 3, 6, 9, 12)              # positions in VGG_CONVS after whose ReLU a feature map is tapped
POOL_BEFORE = (2, 4, 7, 10)          # positions in VGG_CONVS preceded by a 2x2 max-pool
SLICE_OF = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def seeded_conv(cin, cout, seed):
    """weight N(0, 2 / (9 cin)), bias U(-0.1, 0.1), fp32."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.rand((cout,), generator=g) * 0.2 - 0.1
    return w, b


def seeded_lin(C, seed):
    """lin_c = U(0, 1) / C, fp32."""
    return torch.rand((C,), generator=torch.Generator().manual_seed(seed)) / C


@functools.lru_cache(maxsize=None)
def seeded_network(seed=0):
    """([(weight, bias)] * 13, [lin] * 5) of the recipe; computed once per seed and shared - do not modify."""
    convs, cin = [], 3
    for i, cout in enumerate(VGG_WIDTHS):
        convs.append(seeded_conv(cin, cout, 1000 * seed + i))
        cin = cout
    lins = [seeded_lin(VGG_WIDTHS[t], 1000 * seed + 100 + i) for i, t in enumerate(TAPS)]
    return convs, lins


def state_dicts(convs, lins, form="torchvision"):
    """The weights under the key names of the published packages: form 'torchvision' -> (features state dict, lin state dict), 'features' -> the same with a
    'features.' prefix, 'lpips' -> (one lpips.LPIPS(net='vgg') state dict, None)."""
    lin = {f"lin{i}.model.1.weight": v.reshape(1, -1, 1, 1) for i, v in enumerate(lins)}
    if form == "lpips":
        sd = {"scaling_layer.shift": torch.tensor(SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(SCALE).view(1, 3, 1, 1)}
        for idx, (w, b) in zip(VGG_CONVS, convs):
            sd[f"net.slice{SLICE_OF[idx]}.{idx}.weight"], sd[f"net.slice{SLICE_OF[idx]}.{idx}.bias"] = w, b
        sd.update(lin)
        return sd, None
    pre = "features." if form == "features" else ""
    sd = {}
    for idx, (w, b) in zip(VGG_CONVS, convs):
        sd[f"{pre}{idx}.weight"], sd[f"{pre}{idx}.bias"] = w, b
    return sd, lin


def images(K, H, W, seed):
    """(K,H,W,3) fp32, U[0,1)."""
    return torch.rand((K, H, W, 3), generator=torch.Generator().manual_seed(seed))


def scale_input(x_nchw, dtype):
    """LPIPS's scaling layer on a [0,1] image: ((2x - 1) - shift) / scale."""
    x = x_nchw.to(dtype)
    shift, scale = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1), torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    return ((2 * x - 1) - shift) / scale


def conv_relu(x_nhwc, w, b, dtype=torch.float64, scaled_input=False):
    """conv3x3 + bias + ReLU, zero padding 1, on a channel-last tensor; scaled_input: x is a [0,1] image and goes through the scaling layer first (the zero
    padding happens after the scaling)."""
    x = x_nhwc.permute(0, 3, 1, 2)
    x = scale_input(x, dtype) if scaled_input else x.to(dtype)
    return F.relu(F.conv2d(x, w.to(dtype), b.to(dtype), padding=1)).permute(0, 2, 3, 1).contiguous()


def conv1_shift_folded(x_nhwc, w, b, dtype=torch.float64):
    """The WRONG conv1_1 the issue warns of: the shift folded into the bias (b - sum w shift / scale), the image only scaled by 2 / scale and offset by -1 / scale.
    Equal to conv_relu(..., scaled_input=True) wherever no tap is padding, different on the one-pixel border."""
    x = x_nhwc.permute(0, 3, 1, 2).to(dtype)
    shift, scale = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1), torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    wd = w.to(dtype)
    b_f = b.to(dtype) - (wd * (shift / scale)).sum(dim=(1, 2, 3))
    return F.relu(F.conv2d((2 * x - 1) / scale, wd, b_f, padding=1)).permute(0, 2, 3, 1).contiguous()


def pool(x_nhwc):
    return F.max_pool2d(x_nhwc.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()


def features(x_nhwc, convs, dtype=torch.float64):
    """The five tap maps, channel-last, of (K,H,W,3) images in [0,1]."""
    x, taps = x_nhwc, []
    for i, (w, b) in enumerate(convs):
        if i in POOL_BEFORE:
            x = pool(x)
        x = conv_relu(x, w, b, dtype, scaled_input=i == 0)
        if i in TAPS:
            taps.append(x)
    return taps


def head(f0, f1, lin, dtype=torch.float64):
    """(K,h,w,C) x 2, (C,) -> (K,): mean over pixels of sum_c lin_c (f0_c / n0 - f1_c / n1)^2, n = sqrt(sum_c f_c^2) + 1e-10."""
    f0, f1, lin = f0.to(dtype), f1.to(dtype), lin.to(dtype)
    n0 = torch.sqrt((f0 ** 2).sum(-1, keepdim=True)) + 1e-10
    n1 = torch.sqrt((f1 ** 2).sum(-1, keepdim=True)) + 1e-10
    d = ((f0 / n0 - f1 / n1) ** 2 * lin).sum(-1)
    return d.mean(dim=(1, 2))


def lpips(x0, x1, convs, lins, dtype=torch.float64):
    """(K,H,W,3) x 2 in [0,1] -> (total (K,), layers (K,5)) in dtype."""
    t0, t1 = features(x0, convs, dtype), features(x1, convs, dtype)
    layers = torch.stack([head(a, b, l, dtype) for a, b, l in zip(t0, t1, lins)], dim=1)
    return layers.sum(1), layers
