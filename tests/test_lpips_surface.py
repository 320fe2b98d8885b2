"""CPU-only: the host side of evaluate.LPIPS - the three state-dict forms, the refusals, the size queries of the C ABI (no GPU needed) and that
evaluate.frame_metrics without lpips= is what it was."""
import pytest
import torch

from mvsnerf_amd import _lib, evaluate, ops
from tests import lpips_refs as R


def _tiny_forms():
    convs, lins = R.seeded_network(0)
    return convs, lins, {form: R.state_dicts(convs, lins, form) for form in ("torchvision", "features", "lpips")}


def test_three_state_dict_forms_parse_to_the_same_tensors():
    convs, lins, forms = _tiny_forms()
    for form, (vgg, lin) in forms.items():
        c, l = evaluate.parse_lpips_weights(vgg, lin)
        assert len(c) == 13 and len(l) == 5, form
        for (w, b), (w0, b0) in zip(c, convs):
            assert torch.equal(w, w0) and torch.equal(b, b0) and w.dtype == torch.float32, form
        for v, v0 in zip(l, lins):
            assert tuple(v.shape) == tuple(v0.shape) and torch.equal(v, v0), form
    assert evaluate.VGG_CONVS == R.VGG_CONVS and evaluate.VGG_WIDTHS == R.VGG_WIDTHS and evaluate.LPIPS_TAPS == R.TAPS


def test_missing_and_misshapen_entries_are_named():
    convs, lins, forms = _tiny_forms()
    vgg, lin = forms["torchvision"]
    with pytest.raises(KeyError, match="convolution 12"):
        evaluate.parse_lpips_weights({k: v for k, v in vgg.items() if k != "12.weight"}, lin)
    with pytest.raises(KeyError, match="17.bias"):
        evaluate.parse_lpips_weights({k: v for k, v in vgg.items() if k != "17.bias"}, lin)
    with pytest.raises(KeyError, match="lin3.model.1.weight"):
        evaluate.parse_lpips_weights(vgg, {k: v for k, v in lin.items() if not k.startswith("lin3")})
    with pytest.raises(KeyError, match="lin0"):
        evaluate.parse_lpips_weights(vgg, None)                     # a torchvision dict alone has no heads
    bad = dict(vgg)
    bad["5.weight"] = torch.zeros((128, 64, 5, 5))
    with pytest.raises(RuntimeError, match="5.weight"):
        evaluate.parse_lpips_weights(bad, lin)
    bad = dict(vgg)
    bad["28.bias"] = torch.zeros((256,))
    with pytest.raises(RuntimeError, match="28.bias"):
        evaluate.parse_lpips_weights(bad, lin)
    bad = dict(lin)
    bad["lin4.model.1.weight"] = torch.zeros((1, 256, 1, 1))
    with pytest.raises(RuntimeError, match="lin4"):
        evaluate.parse_lpips_weights(vgg, bad)
    # the constructor parses before it packs: the same errors without a GPU
    with pytest.raises(KeyError, match="convolution 0"):
        evaluate.LPIPS({}, lin)


def test_frames_are_refused_before_any_launch():
    with pytest.raises(ValueError, match="H, W >= 16"):
        evaluate._lpips_frames(torch.zeros((15, 40, 3)), "rgb", False)
    with pytest.raises(ValueError, match="after the crop"):
        evaluate._lpips_frames(torch.zeros((2, 17, 40, 3)), "rgb", True)        # 17 - 2 * 1 = 15 rows stay
    x = evaluate._lpips_frames(torch.zeros((20, 40, 3)), "rgb", True)
    assert tuple(x.shape) == (1, 16, 32, 3) and x.is_contiguous()
    with pytest.raises(RuntimeError, match=r"\(H,W,3\)"):
        evaluate._lpips_frames(torch.zeros((3, 20, 40)), "rgb", False)
    with pytest.raises(NotImplementedError, match="no backward kernel"):
        evaluate._lpips_frames(torch.zeros((20, 40, 3), requires_grad=True), "rgb", False)


def test_size_queries_run_without_a_gpu():
    l = _lib.lib()
    assert l.mvsnerf_lpips_conv_packed_floats(3, 64) == 27 * 64 + 64
    cin = 64
    for cout in (64, 128, 256, 512):
        assert l.mvsnerf_lpips_conv_packed_floats(cin, cout) == 9 * cin * cout + cout
        assert ops.lpips_conv_packed_floats(cout, cout) == 9 * cout * cout + cout
        cin = cout
    for cin, cout in ((3, 128), (32, 64), (64, 96), (0, 64), (64, 0), (1024, 512)):
        assert l.mvsnerf_lpips_conv_packed_floats(cin, cout) == 0
    assert l.mvsnerf_lpips_head_workspace_bytes(2, 4, 6, 512) == 2 * 1 * 8
    assert l.mvsnerf_lpips_head_workspace_bytes(3, 37, 50, 64) == 3 * ((37 * 50 + 63) // 64) * 8
    for args in ((0, 4, 6, 64), (1, 0, 6, 64), (1, 4, 0, 64), (1, 4, 6, 96), (1, 4, 6, 3)):
        assert l.mvsnerf_lpips_head_workspace_bytes(*args) == 0
    # the entries refuse their arguments before touching the device
    assert l.mvsnerf_lpips_conv_fwd(0, 0, 1, 8, 8, 64, 64, 0, 0) == -1
    assert l.mvsnerf_lpips_conv_fwd(256, 256, 1, 8, 8, 64, 96, 256, 0) == -2
    assert l.mvsnerf_lpips_conv_fwd(256, 256, 1, 8, 8, 64, 64, 260, 0) == -3
    assert l.mvsnerf_lpips_pool_fwd(256, 1, 1, 8, 64, 256, 0) == -2
    assert l.mvsnerf_lpips_head_fwd(256, 256, 256, 1, 4, 4, 64, 0, 0, 0, 256, 0) == -1        # neither layer_out nor total


def test_frame_metrics_without_lpips_is_unchanged(monkeypatch):
    calls = []

    def fake_rows(pred, gt, depth_pred=None, depth_gt=None, **kw):
        calls.append(sorted(kw))
        return torch.ones((1 if pred.dim() == 3 else pred.shape[0], ops.METRICS_ROW), dtype=torch.float64)
    monkeypatch.setattr(ops, "frame_metrics", fake_rows)
    rgb = torch.zeros((2, 20, 24, 3))
    out = evaluate.frame_metrics(rgb, rgb)
    assert list(out) == ["psnr", "psnr_center_crop", "psnr_masked", "ssim", "abs_err", "acc_l_0.01", "acc_l_0.05", "acc_l_0.1"]
    assert calls == [["K1", "K2", "data_range", "gt_scale", "thresholds", "win_size"]]

    class Stub:
        def __call__(self, a, b):
            assert a is rgb and b is rgb
            return torch.full((2,), 0.25, dtype=torch.float64)
    out2 = evaluate.frame_metrics(rgb, rgb, lpips=Stub())
    assert list(out2) == list(out) + ["lpips"] and float(out2["lpips"][1]) == 0.25
    assert all(torch.equal(out[k], out2[k]) for k in out)
