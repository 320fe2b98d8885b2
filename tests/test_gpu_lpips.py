"""LPIPS-VGG on the GPU (csrc/lpips.hip through ops.lpips_* and evaluate.LPIPS) against tests/lpips_refs.py in float64, at the real channel widths (the
kernels are specialised for them) and the smallest pixel counts that cross every tile boundary.  Weights: the seeded recipe of lpips_refs, drawn at test time.

Bounds (none comes from what the kernels return):
* a conv layer:   mean|hip - f64| <= 4 mean|torch fp32 on the CPU - f64|: the margin tests/test_gpu_metrics.py gives a differently ordered fp32 summation over
                  the same yardstick (which alone measures 1.2e-7 to 8.8e-7 per layer, so no floor is needed).  conv1_1: its border ring and interior apart.
* the pool:       equal to F.max_pool2d.
* a head:         mean|hip - f64| <= 4 mean|torch fp32 - f64| over the frames.
* the metric:     per layer value and total, |hip - f64| <= max(4 |torch fp32 - f64|, 2^-20 |f64|); the floor because the CPU's fp32 scalar lands within
                  2e-8 to 1.6e-7 of float64 by cancellation in the mean, and 2^-20 is twice the largest relative error of the features under the yardstick.
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools

import pytest
import torch

from tests import lpips_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

PAIRS = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512)]
# N, H, W: smaller than any tile; partial tiles on both axes of the 4 x 32 pixel tile; (64 -> 64 only) several tiles and two images
CONV_CASES = [(ci, co, 2, 5, 7) for ci, co in PAIRS] + [(ci, co, 1, 37, 50) for ci, co in PAIRS] + [(64, 64, 2, 70, 133)]
SIZES = [(16, 16), (37, 50), (70, 133)]


@functools.lru_cache(maxsize=None)
def _conv_case(cin, cout, N, H, W):
    """input (channel-last fp32: an image in [0,1] for conv1_1, else half-zero non-negative activations as a ReLU leaves them), weights, the float64
    result and the CPU fp32 result."""
    g = torch.Generator().manual_seed(cin * 7919 + cout * 31 + H * W + N)
    x = torch.rand((N, H, W, 3), generator=g) if cin == 3 else torch.randn((N, H, W, cin), generator=g).clamp_(min=0)
    w, b = R.seeded_conv(cin, cout, seed=cin + cout)
    ref64 = R.conv_relu(x, w, b, torch.float64, scaled_input=cin == 3)
    ref32 = R.conv_relu(x, w, b, torch.float32, scaled_input=cin == 3)
    return x, w, b, ref64, ref32


@functools.lru_cache(maxsize=None)
def _metric_case(H, W):
    """two frames and their target, the float64 (total, layers) and the CPU fp32 ones"""
    convs, lins = R.seeded_network(0)
    x0, x1 = R.images(2, H, W, seed=H * W), R.images(2, H, W, seed=H * W + 1)
    return x0, x1, R.lpips(x0, x1, convs, lins, torch.float64), R.lpips(x0, x1, convs, lins, torch.float32)


@pytest.fixture(scope="module")
def lp():
    from mvsnerf_amd import evaluate
    convs, lins = R.seeded_network(0)
    return evaluate.LPIPS(*R.state_dicts(convs, lins, "torchvision"), device=DEV)


@pytest.mark.parametrize("cin,cout,N,H,W", CONV_CASES)
def test_conv_layer_against_float64(cin, cout, N, H, W):
    from mvsnerf_amd import ops
    x, w, b, ref64, ref32 = _conv_case(cin, cout, N, H, W)
    packed = ops.lpips_conv_pack(w.to(DEV), b.to(DEV))
    assert packed.numel() == ops.lpips_conv_packed_floats(cin, cout)
    out = ops.lpips_conv(x.to(DEV), packed, cout)
    assert tuple(out.shape) == (N, H, W, cout) and out.dtype == torch.float32
    got = out.cpu().double()
    assert torch.isfinite(got).all() and float(got.min()) >= 0.0
    err, yard = (got - ref64).abs(), (ref32.double() - ref64).abs()
    print(f"conv {cin}->{cout} N={N} {H}x{W}: mean|hip-f64| = {float(err.mean()):.3e}, mean|torch32-f64| = {float(yard.mean()):.3e}, "
          f"ratio {float(err.mean() / yard.mean()):.2f}, max|hip-f64| = {float(err.max()):.3e}")
    assert float(err.mean()) <= 4 * float(yard.mean())
    if cin == 3:                                   # the trap: zero padding after the scaling layer - the one-pixel ring on its own
        ring = torch.ones((H, W), dtype=torch.bool)
        ring[1:-1, 1:-1] = False
        print(f"   ring {float(err[:, ring].mean()):.3e} (yardstick {float(yard[:, ring].mean()):.3e}), "
              f"interior {float(err[:, ~ring].mean()):.3e} (yardstick {float(yard[:, ~ring].mean()):.3e})")
        assert float(err[:, ring].mean()) <= 4 * float(yard[:, ring].mean())
        assert float(err[:, ~ring].mean()) <= 4 * float(yard[:, ~ring].mean())
    # image n of the batch has the bits of the image alone
    if N > 1:
        alone = ops.lpips_conv(x[1:2].to(DEV), packed, cout)
        assert torch.equal(alone[0], out[1])


@pytest.mark.parametrize("H,W", [(37, 50), (16, 16)])
def test_pool_equals_max_pool2d(H, W):
    from mvsnerf_amd import ops
    x = torch.randn((2, H, W, 64), generator=torch.Generator().manual_seed(H))
    out = ops.lpips_pool(x.to(DEV))
    assert tuple(out.shape) == (2, H // 2, W // 2, 64)
    assert torch.equal(out.cpu(), R.pool(x))


def _check_head(f0, f1, lin, what):
    from mvsnerf_amd import ops
    ref64, ref32 = R.head(f0, f1, lin, torch.float64), R.head(f0, f1, lin, torch.float32)
    total = torch.full((f0.shape[0],), 7.0, device=DEV, dtype=torch.float64)
    got = ops.lpips_head(f0.to(DEV), f1.to(DEV), lin.to(DEV), total=total, accumulate=True)
    assert got.dtype == torch.float64 and torch.isfinite(got).all()
    assert torch.equal(total, got + 7.0)
    err, yard = float((got.cpu() - ref64).abs().mean()), float((ref32.double() - ref64).abs().mean())
    print(f"head {what}: f64 {ref64.tolist()}, mean|hip-f64| = {err:.3e}, mean|torch32-f64| = {yard:.3e}")
    assert err <= 4 * yard
    return got


def test_head_layer_against_float64():
    g = torch.Generator().manual_seed(5)
    f0, f1 = torch.randn((2, 4, 6, 512), generator=g).clamp_(min=0), torch.randn((2, 4, 6, 512), generator=g).clamp_(min=0)
    lin = R.seeded_lin(512, 9)
    _check_head(f0, f1, lin, "C=512 K=2 4x6")
    f1z = f1.clone()
    f1z[0, 1, 2] = 0
    f1z[1, 3, 5] = 0                               # all-zero feature vectors in one image ...
    _check_head(f0, f1z, lin, "zero vectors in one image")
    f0z = f0.clone()
    f0z[0, 1, 2] = 0                               # ... then in both (that pixel contributes exactly 0)
    _check_head(f0z, f1z, lin, "zero vectors in both images")


@pytest.mark.parametrize("H,W", SIZES)
def test_whole_metric_against_float64(lp, H, W):
    x0, x1, (t64, l64), (t32, l32) = _metric_case(H, W)
    total, layers = lp(x0.to(DEV), x1.to(DEV), per_layer=True)
    assert tuple(total.shape) == (2,) and tuple(layers.shape) == (2, 5) and total.dtype == layers.dtype == torch.float64
    total, layers = total.cpu(), layers.cpu()
    for name, got, r64, r32 in (("layers", layers, l64, l32), ("total", total, t64, t32)):
        err, yard = (got - r64).abs(), (r32.double() - r64).abs()
        bound = torch.maximum(4 * yard, 2.0 ** -20 * r64.abs())
        print(f"lpips {H}x{W} {name}: f64 {r64.flatten().tolist()}\n   |hip-f64| {err.flatten().tolist()}\n   |torch32-f64| {yard.flatten().tolist()}\n"
              f"   worst |hip-f64| / bound = {float((err / bound).max()):.3f}, worst |hip-f64| / |f64| = {float((err / r64.abs()).max()):.3e}")
        assert (err <= bound).all()
    assert torch.equal(layers.sum(1), total) or float((layers.sum(1) - total).abs().max()) <= 2.0 ** -50      # total = the five layer values, added in order


def test_properties(lp):
    from mvsnerf_amd import evaluate
    x0, x1, _, _ = _metric_case(37, 50)
    a, b = x0.to(DEV), x1.to(DEV)
    d, layers = lp(a, b, per_layer=True)
    # identical inputs: exactly 0
    z, zl = lp(a, a.clone(), per_layer=True)
    assert (z == 0).all() and (zl == 0).all()
    # two calls: equal bits
    d2, layers2 = lp(a, b, per_layer=True)
    assert torch.equal(d, d2) and torch.equal(layers, layers2)
    # frame k of a batch = the frame alone ((H,W,3) inputs), bit for bit
    for k in range(2):
        dk, lk = lp(a[k], b[k], per_layer=True)
        assert tuple(dk.shape) == (1,) and torch.equal(dk[0], d[k]) and torch.equal(lk[0], layers[k])
    # chunked batches (one pair per trunk launch) give the same bits as one launch
    small = evaluate.LPIPS.__new__(evaluate.LPIPS)
    small.__dict__.update(lp.__dict__)
    small.chunk_bytes = 1
    assert torch.equal(small(a, b), d)
    # target features computed once and reused
    feats = lp.features(b)
    assert [tuple(f.shape) for f in feats] == [(2, 37, 50, 64), (2, 18, 25, 128), (2, 9, 12, 256), (2, 4, 6, 512), (2, 2, 3, 512)]
    assert torch.equal(lp(a, feats), d)
    # crop=True = the call on the sliced tensors (37 // 10 = 3 rows, 50 // 10 = 5 columns from every side)
    assert torch.equal(lp(a, b, crop=True), lp(a[:, 3:-3, 5:-5].contiguous(), b[:, 3:-3, 5:-5].contiguous()))
    assert torch.equal(lp(a, lp.features(b, crop=True), crop=True), lp(a, b, crop=True))
    # the lpips key of frame_metrics
    out = evaluate.frame_metrics(a, b, lpips=lp)
    assert torch.equal(out["lpips"], d)
    assert sorted(set(out) - set(evaluate.frame_metrics(a, b))) == ["lpips"]
    # refusals
    with pytest.raises(ValueError, match="H, W >= 16"):
        lp(a[:, :15], b[:, :15])
    with pytest.raises(NotImplementedError, match="no backward kernel"):
        lp(a.clone().requires_grad_(True), b)


def test_dead_last_layer_contributes_zero():
    """conv5_3 with its bias at -10: relu5_3 is all zero in both images, every pixel's feature vector is 0 / 1e-10 = 0, the layer adds 0 and the total is finite"""
    from mvsnerf_amd import evaluate
    convs, lins = R.seeded_network(0)
    convs = list(convs[:-1]) + [(convs[-1][0], torch.full_like(convs[-1][1], -10.0))]
    dead = evaluate.LPIPS(*R.state_dicts(convs, lins, "lpips"), device=DEV)
    x0, x1, (t64, l64), _ = _metric_case(37, 50)
    total, layers = dead(x0.to(DEV), x1.to(DEV), per_layer=True)
    assert float(dead.features(x0.to(DEV))[4].abs().max()) == 0.0
    assert (layers[:, 4] == 0).all() and torch.isfinite(total).all() and (total > 0).all()
    assert torch.equal(total, layers[:, :4].sum(1) + 0.0) or float((total - layers[:, :4].sum(1)).abs().max()) <= 2.0 ** -50
    # the four live layers are those of the unmodified network
    assert float((layers[:, :4].cpu() - l64[:, :4]).abs().max()) <= 2.0 ** -18 * float(l64[:, :4].abs().max())
