"""CPU-only: properties of tests/lpips_refs.py, the float64 yardstick of tests/test_gpu_lpips.py - so that a mistake in the restatement does not pass as a
kernel's error bound."""
import torch

from tests import lpips_refs as R


def test_identical_images_give_exactly_zero():
    convs, lins = R.seeded_network(0)
    x = R.images(2, 19, 23, seed=1)
    for dtype in (torch.float64, torch.float32):
        total, layers = R.lpips(x, x.clone(), convs, lins, dtype)
        assert total.dtype == dtype and tuple(layers.shape) == (2, 5)
        assert (total == 0).all() and (layers == 0).all()


def test_symmetry_and_positivity():
    convs, lins = R.seeded_network(0)
    x, y = R.images(2, 19, 23, seed=1), R.images(2, 19, 23, seed=2)
    a, la = R.lpips(x, y, convs, lins)
    b, lb = R.lpips(y, x, convs, lins)
    assert torch.equal(a, b) and torch.equal(la, lb)              # (u - v)^2 == (v - u)^2 term by term
    assert (la > 0).all() and torch.isfinite(a).all()
    # the features stay alive through all five taps (the recipe's point): no tap map is all zero, none blows up
    # (at 19 x 23 relu5_3 is one pixel whose taps are mostly padding: 0.04 there, 0.4 to 1.1 above; 0.75 to 1.5 on all five at 70 x 133)
    for t in R.features(x, convs):
        m = float(t.abs().mean())
        assert 0.01 < m < 10.0, m
        assert int(((t ** 2).sum(-1) == 0).sum()) == 0


def test_shift_folded_into_the_bias_is_wrong_on_the_border_only():
    """The trap of conv1_1: zero padding happens AFTER the scaling layer.  Folding the shift into the bias moves relu1_2 on the one-pixel border (by more than
    1e-3, so a kernel that does it is seen) and nowhere else."""
    convs, _ = R.seeded_network(0)
    x = R.images(1, 12, 15, seed=3)
    (w0, b0), (w1, b1) = convs[0], convs[1]
    good = R.conv_relu(R.conv_relu(x, w0, b0, scaled_input=True), w1, b1)
    bad1 = R.conv1_shift_folded(x, w0, b0)
    d1 = (bad1 - R.conv_relu(x, w0, b0, scaled_input=True)).abs().amax(-1)[0]          # relu1_1: wrong on the outer ring only
    assert float(d1[1:-1, 1:-1].max()) < 1e-12
    assert float(d1[0].min()) > 0 and float(d1[-1].min()) > 0 and float(d1[:, 0].min()) > 0 and float(d1[:, -1].min()) > 0
    d2 = (R.conv_relu(bad1, w1, b1) - good).abs().amax(-1)[0]                          # relu1_2: the ring spreads one pixel inwards, no further
    assert float(d2[2:-2, 2:-2].max()) < 1e-12
    ring = torch.cat([d2[0], d2[-1], d2[1:-1, 0], d2[1:-1, -1]])
    assert float(ring.min()) > 1e-3, float(ring.min())


def test_pool_floors_odd_sizes():
    x = torch.arange(2 * 5 * 7 * 3, dtype=torch.float32).reshape(2, 5, 7, 3)
    p = R.pool(x)
    assert tuple(p.shape) == (2, 2, 3, 3)
    assert torch.equal(p, x[:, 1:4:2, 1:6:2])                     # increasing data: the window's last element; row 4 and column 6 never read
    y = x.clone()
    y[:, 4], y[:, :, 6] = 1e9, 1e9
    assert torch.equal(R.pool(y), p)
    taps = R.features(R.images(1, 37, 50, seed=4), R.seeded_network(0)[0])
    assert [tuple(t.shape[1:3]) for t in taps] == [(37, 50), (18, 25), (9, 12), (4, 6), (2, 3)]


def test_all_zero_feature_vectors_give_zero_not_nan():
    lin = R.seeded_lin(64, 5)
    f0 = torch.rand((1, 3, 4, 64), generator=torch.Generator().manual_seed(6))
    f1 = f0.clone()
    f1[0, 1, 2] = 0
    d = R.head(f0, f1, lin)
    assert torch.isfinite(d).all() and float(d) > 0
    f0[0, 1, 2] = 0
    assert float(R.head(f0, f1, lin)) == 0.0
