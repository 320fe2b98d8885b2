"""Evaluation protocol of the reference's notebooks (renderer.ipynb) - host-side arithmetic on finished frames.

* `abs_error`, `acc_threshold`            utils.py:71-82
* `psnr_center_crop`                      renderer.ipynb cell 8, l.95-100 (Blender / LLFF: centre crop to 0.8 of each side)
* `psnr_masked`                           renderer.ipynb cell 16, l.120-124 (DTU: pixels whose GT depth is 0 are background)
* `depth_metrics`                         renderer.ipynb cell 16, l.99-106 (abs error and the 0.01/0.05/0.1 accuracy thresholds)

* `ssim`                                  renderer.ipynb cell 8 l.111 / cell 16: `skimage.metrics.structural_similarity(rgb, img, multichannel=True)` restated on
                                          numpy + scipy (skimage is not in this image, so this restatement is NOT pinned against the library here: it follows the
                                          published algorithm of skimage 0.19, the version the notebook's deprecation warning identifies)

* `LPIPS`                                 renderer.ipynb cells 8 / 16: `lpips.LPIPS(net='vgg')(rgb*2-1, img*2-1)` on the GPU (csrc/lpips.hip), from the two
                                          weight files a user of the reference has (neither package is in this image: the arithmetic follows the published
                                          definition and is NOT pinned against the lpips package here)
"""
import numpy as np
import torch

from .utils import mse2psnr


def abs_error(depth_pred, depth_gt, mask):
    """utils.py:71-74."""
    return (depth_pred[mask] - depth_gt[mask]).abs()


def acc_threshold(depth_pred, depth_gt, mask, threshold):
    """utils.py:76-82: per-pixel indicator |err| < threshold over the masked pixels."""
    return (abs_error(depth_pred, depth_gt, mask) < threshold).float()


def _psnr(mse):
    return float(mse2psnr(torch.as_tensor(mse, dtype=torch.float32)))


def psnr_center_crop(rgb, img):
    """rgb, img: (H,W,3) in [0,1].  Crop H//10 rows and W//10 columns from every side, then PSNR of the mean squared error."""
    rgb, img = torch.as_tensor(rgb, dtype=torch.float32), torch.as_tensor(img, dtype=torch.float32)
    hc, wc = rgb.shape[0] // 10, rgb.shape[1] // 10
    if hc == 0 or wc == 0:
        raise ValueError("psnr_center_crop: the reference's [H_crop:-H_crop] slicing is empty for images smaller than 10 pixels")
    a, b = rgb[hc:-hc, wc:-wc], img[hc:-hc, wc:-wc]
    return _psnr(((a - b) ** 2).mean())


def psnr_masked(rgb, img, depth_gt):
    """DTU protocol: mask = (depth_gt == 0) is background; PSNR over the remaining pixels."""
    rgb, img = torch.as_tensor(rgb, dtype=torch.float32), torch.as_tensor(img, dtype=torch.float32)
    keep = torch.as_tensor(depth_gt) != 0
    return _psnr(((rgb[keep] - img[keep]) ** 2).mean())


def depth_metrics(depth_pred, depth_gt, thresholds=(0.01, 0.05, 0.1), gt_scale=1.0 / 200.0):
    """cell 16 l.99-106: mask = depth_gt > 0; GT is in mm/200 units there (depth_gt/200)."""
    depth_pred = torch.as_tensor(depth_pred, dtype=torch.float32)
    depth_gt = torch.as_tensor(depth_gt, dtype=torch.float32)
    mask = depth_gt > 0
    gt = depth_gt * gt_scale
    err = abs_error(depth_pred, gt, mask)
    out = {"abs_err": float(err.mean())}
    for t in thresholds:
        out[f"acc_l_{t}"] = float((err < t).float().mean())
    return out


def ssim(rgb, img, win_size=7, data_range=None, K1=0.01, K2=0.03):
    """Mean structural similarity of two (H,W,3) float images as the reference's notebooks compute it:
    `structural_similarity(rgb, img, multichannel=True)` of skimage 0.19 with its defaults - 7x7 UNIFORM window (no gaussian weights), sample
    covariance (normalised by N-1), K1 = 0.01, K2 = 0.03, the SSIM map cropped by (win_size-1)/2 at every border, mean over pixels and then over
    channels.  data_range=None reproduces the library's default for float images at that version: the width of the dtype's nominal range [-1, 1],
    i.e. 2 - NOT the 1.0 the images actually span (the numbers in the reference's tables were produced that way); pass data_range=1.0 for the
    conventional value."""
    from scipy.ndimage import uniform_filter
    a = np.asarray(torch.as_tensor(rgb, dtype=torch.float32).cpu().numpy())
    b = np.asarray(torch.as_tensor(img, dtype=torch.float32).cpu().numpy())
    if a.shape != b.shape or a.ndim != 3:
        raise ValueError("ssim: two (H,W,C) images of the same shape")
    if min(a.shape[:2]) < win_size or win_size % 2 == 0:
        raise ValueError("ssim: win_size must be odd and not exceed the image sides")
    R = 2.0 if data_range is None else float(data_range)
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    n_p = win_size ** 2
    cov_norm = n_p / (n_p - 1.0)
    pad = (win_size - 1) // 2
    vals = []
    for c in range(a.shape[2]):
        x, y = a[..., c], b[..., c]
        ux, uy = uniform_filter(x, size=win_size), uniform_filter(y, size=win_size)
        uxx, uyy, uxy = uniform_filter(x * x, size=win_size), uniform_filter(y * y, size=win_size), uniform_filter(x * y, size=win_size)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        vals.append(S[pad:-pad, pad:-pad].astype(np.float64).mean())
    return float(np.mean(vals))


# ---- the same protocol on the GPU (csrc/metrics.hip through ops.frame_metrics): frames stay on the device, nothing synchronises the host

def _psnr_of_sums(sse, n):
    """mse2psnr's formula on a sum of squared errors over n pixels of 3 channels, per frame, in float64; n == 0 gives NaN."""
    return -10.0 * torch.log(sse / (3.0 * n)) / float(np.log(10.0))


def frame_metrics(rgb, img, depth_pred=None, depth_gt=None, win_size=7, data_range=None, K1=0.01, K2=0.03, thresholds=(0.01, 0.05, 0.1),
                  gt_scale=1.0 / 200.0, lpips=None):
    """psnr, psnr_center_crop, psnr_masked, ssim, abs_err and acc_l_<t> of K frames in one library call.  rgb, img: (H,W,3) or (K,H,W,3) fp32
    tensors on the GPU, depth_pred / depth_gt (H,W) or (K,H,W) or both None.  Returns a dict of (K,) float64 tensors on the GPU and does not
    synchronise the host: collect the dicts of a validation loop and copy once.  data_range=None is 2.0, as in `ssim`.  A key whose pixel
    count is zero (psnr_masked / abs_err / acc_l_* without depth or under an all-zero depth_gt) is NaN for that frame.  lpips: an `LPIPS`
    instance adds the key "lpips" = lpips(rgb, img) (the full frame; the notebook's cropped protocol is lpips(rgb, img, crop=True))."""
    from . import ops
    if torch.is_tensor(rgb) and rgb.dim() in (3, 4) and (rgb.shape[-3] // 10 == 0 or rgb.shape[-2] // 10 == 0):
        raise ValueError("psnr_center_crop: the reference's [H_crop:-H_crop] slicing is empty for images smaller than 10 pixels")
    row = ops.frame_metrics(rgb, img, depth_pred, depth_gt, win_size=win_size, data_range=2.0 if data_range is None else float(data_range),
                            K1=K1, K2=K2, gt_scale=gt_scale, thresholds=thresholds)
    out = {"psnr": _psnr_of_sums(row[:, ops.M_SSE], row[:, ops.M_N]),
           "psnr_center_crop": _psnr_of_sums(row[:, ops.M_SSE_CROP], row[:, ops.M_N_CROP]),
           "psnr_masked": _psnr_of_sums(row[:, ops.M_SSE_MASK], row[:, ops.M_N_MASK]),
           "ssim": row[:, ops.M_SSIM0:ops.M_SSIM2 + 1].sum(1) / (3.0 * row[:, ops.M_N_SSIM]),
           "abs_err": row[:, ops.M_ABS_ERR] / row[:, ops.M_N_DEPTH]}
    for i, t in enumerate(thresholds):
        out[f"acc_l_{t}"] = row[:, ops.M_ACC0 + i] / row[:, ops.M_N_DEPTH]
    if lpips is not None:
        out["lpips"] = lpips(rgb, img)
    return out


def ssim_hip(rgb, img, win_size=7, data_range=None, K1=0.01, K2=0.03):
    """`ssim` of K frames on the GPU: (H,W,3) or (K,H,W,3) fp32 tensors -> (K,) float64 tensor on the GPU, no host synchronisation."""
    from . import ops
    row = ops.frame_metrics(rgb, img, win_size=win_size, data_range=2.0 if data_range is None else float(data_range), K1=K1, K2=K2)
    return row[:, ops.M_SSIM0:ops.M_SSIM2 + 1].sum(1) / (3.0 * row[:, ops.M_N_SSIM])


# ---- geometry: DTU's accuracy / completeness and the Tanks-and-Temples precision / recall / F-score of clouds and meshes (csrc/cloud_metrics.hip)

def _cloud_of(x, name):
    """x as ((n,3) fp32 tensor | None, mesh | None): a tensor, a TriangleMesh (sampled later), or anything with .points."""
    from . import geometry
    if isinstance(x, geometry.TriangleMesh):
        geometry._cloud_tensor(x.vertices, f"{name}.vertices", "cloud_metrics")
        return None, x
    if not torch.is_tensor(x) and hasattr(x, "points"):
        x = x.points
    return geometry._cloud_tensor(x, name, "cloud_metrics"), None


def cloud_metrics(pred, gt, max_dist, taus=(0.5, 1.0, 2.0), grids=None, spacing=None):
    """How far a reconstruction is from a scan, on the device.  pred, gt: (n,3) fp32 tensors on the GPU, a geometry.PointCloud (its .points) or anything
    with .points, or a geometry.TriangleMesh, which is sampled with geometry.sample_mesh(mesh, spacing=spacing) first (spacing= is then required).
    One exact nearest-neighbour query within max_dist per direction (geometry.PointGrid), then a two-launch float64 reduction per direction.  Returns a
    dict of float64 tensors on the device; nothing is read back (a grid that has to find its own box reads six floats, see PointGrid):
        accuracy        the mean of the finite distances from pred to gt - DTU's mean(D(D < MaxDist)); NaN when there is none
        completeness    the same from gt to pred;   overall = (accuracy + completeness) / 2
        n_accuracy, n_completeness      how many distances were finite
        precision       (n_tau,) the share of ALL pred points with dist < tau (tau rounded to fp32, an fp32 compare); 0 for an empty pred
        recall          (n_tau,) the same over all gt points;   fscore = 2 P R / (P + R), 0 where P + R == 0
        dist_pred, index_pred (fp32, int32; +inf and -1 where nothing is within max_dist), dist_gt, index_gt: for a caller's own observation mask
    taus: 1 to 8 numbers (the default is DTU-style millimetres).  grids: (PointGrid over gt, PointGrid over pred) of an earlier call with the same clouds
    and max_dist, reused as they are.  A PointCloud fused with a capacity carries unwritten rows past its count: pass cloud.points[:n]."""
    from . import geometry, ops
    who = "cloud_metrics"
    r = geometry._radius(max_dist, who)
    try:
        taus = [float(t) for t in taus]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: taus must be 1..{ops.CLOUD_METRICS_MAX_TAUS} numbers, got {taus!r}") from None
    if not 1 <= len(taus) <= ops.CLOUD_METRICS_MAX_TAUS or any(np.isnan(t) for t in taus):
        raise ValueError(f"{who}: taus must be 1..{ops.CLOUD_METRICS_MAX_TAUS} numbers, none of them NaN, got {taus!r}")
    clouds = [_cloud_of(pred, "pred"), _cloud_of(gt, "gt")]
    if any(m is not None for _, m in clouds) and spacing is None:
        raise ValueError(f"{who}: a TriangleMesh is scored through its surface samples: pass spacing= (geometry.sample_mesh)")
    if grids is not None:
        if not (isinstance(grids, (tuple, list)) and len(grids) == 2 and all(isinstance(g, geometry.PointGrid) for g in grids)):
            raise ValueError(f"{who}: grids must be a pair (PointGrid over gt, PointGrid over pred)")
        if any(g.max_dist != r for g in grids):
            raise ValueError(f"{who}: grids were built for max_dist {[g.max_dist for g in grids]}, not {r}")
    P, G = (t if m is None else geometry.sample_mesh(m, spacing).points for t, m in clouds)
    if P.device != G.device:
        raise ValueError(f"{who}: pred and gt must be on one device, got {P.device} and {G.device}")
    if grids is None:
        grids = (geometry.PointGrid(G, r), geometry.PointGrid(P, r))
    elif grids[0].n != G.shape[0] or grids[1].n != P.shape[0]:
        raise ValueError(f"{who}: grids hold {grids[0].n} gt and {grids[1].n} pred points, the clouds {G.shape[0]} and {P.shape[0]}")
    out = {}
    rows = []
    for cloud, grid, side in ((P, grids[0], "pred"), (G, grids[1], "gt")):
        dist, index = grid.nearest(cloud)
        with torch.cuda.device(cloud.device):
            rows.append(ops.cloud_metrics_row(dist, taus))
        out[f"dist_{side}"], out[f"index_{side}"] = dist, index
    k = len(taus)
    (rp, rg), (n_p, n_g) = rows, (int(P.shape[0]), int(G.shape[0]))
    out["accuracy"], out["completeness"] = rp[0] / rp[1], rg[0] / rg[1]                   # 0 / 0 = NaN: nothing within max_dist
    out["overall"] = (out["accuracy"] + out["completeness"]) / 2.0
    out["n_accuracy"], out["n_completeness"] = rp[1], rg[1]
    # (a tensor divisor: torch divides a GPU tensor by a Python number as a product with its reciprocal, which is not the correctly rounded share)
    out["precision"] = rp[2:2 + k] / torch.full_like(rp[2:2 + k], n_p) if n_p else torch.zeros_like(rp[2:2 + k])
    out["recall"] = rg[2:2 + k] / torch.full_like(rg[2:2 + k], n_g) if n_g else torch.zeros_like(rg[2:2 + k])
    s = out["precision"] + out["recall"]
    out["fscore"] = torch.where(s > 0, 2.0 * out["precision"] * out["recall"] / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(s))
    return out


# ---- LPIPS-VGG on the GPU (csrc/lpips.hip through ops.lpips_*)

VGG_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)           # indices of the 13 convolutions in torchvision's vgg16().features
VGG_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
LPIPS_TAPS = (1, 3, 6, 9, 12)                                           # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (position in VGG_CONVS)
_LPIPS_SLICE = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}


def parse_lpips_weights(vgg_state, lin_state=None):
    """The 26 + 5 tensors of LPIPS-VGG out of the state dicts a user of the reference has -> ([(weight, bias)] * 13, [lin] * 5), fp32 on the CPU.
    vgg_state: torchvision's `vgg16().features.state_dict()` ("0.weight", "0.bias", "2.weight", ...), the same under a "features." prefix (the whole
    `vgg16().state_dict()`), or - with lin_state None - one `lpips.LPIPS(net='vgg').state_dict()` ("net.slice{1..5}.{idx}.weight|bias" and the lin keys).
    lin_state: "lin{0..4}.model.1.weight" of shape (1,C,1,1), the lpips package's weights/v0.1/vgg.pth.  The key names are written from the published
    packages; neither is in this image, so they are not pinned against the libraries here.  A missing entry raises KeyError and a misshapen one
    RuntimeError, each naming it, before anything is packed."""
    if lin_state is None:
        lin_state = vgg_state
    convs, cin = [], 3
    for idx, cout in zip(VGG_CONVS, VGG_WIDTHS):
        forms = (f"{idx}", f"features.{idx}", f"net.slice{_LPIPS_SLICE[idx]}.{idx}")
        stem = next((f for f in forms if f + ".weight" in vgg_state), None)
        if stem is None:
            raise KeyError(f"LPIPS: no convolution {idx} in the VGG state dict (looked for {', '.join(f + '.weight' for f in forms)})")
        if stem + ".bias" not in vgg_state:
            raise KeyError(f"LPIPS: {stem}.bias is missing from the VGG state dict")
        w, b = torch.as_tensor(vgg_state[stem + ".weight"]), torch.as_tensor(vgg_state[stem + ".bias"])
        if tuple(w.shape) != (cout, cin, 3, 3):
            raise RuntimeError(f"LPIPS: {stem}.weight is {tuple(w.shape)}, VGG-16 has {(cout, cin, 3, 3)} there")
        if tuple(b.shape) != (cout,):
            raise RuntimeError(f"LPIPS: {stem}.bias is {tuple(b.shape)}, VGG-16 has {(cout,)} there")
        convs.append((w.detach().to("cpu", torch.float32), b.detach().to("cpu", torch.float32)))
        cin = cout
    lins = []
    for i, t in enumerate(LPIPS_TAPS):
        key = f"lin{i}.model.1.weight"
        if key not in lin_state:
            raise KeyError(f"LPIPS: {key} is missing from the head state dict")
        v = torch.as_tensor(lin_state[key])
        if tuple(v.shape) != (1, VGG_WIDTHS[t], 1, 1):
            raise RuntimeError(f"LPIPS: {key} is {tuple(v.shape)}, the VGG heads have {(1, VGG_WIDTHS[t], 1, 1)} there")
        lins.append(v.detach().to("cpu", torch.float32).reshape(-1))
    return convs, lins


def _lpips_frames(t, name, crop):
    """(H,W,3) | (K,H,W,3) -> contiguous fp32 (K,H',W',3), centre-cropped if asked; the refusals of LPIPS's inputs."""
    from . import ops
    ops._need_no_grad(t, op="LPIPS")
    if not (torch.is_tensor(t) and t.dim() in (3, 4) and t.shape[-1] == 3):
        raise RuntimeError(f"LPIPS: {name} must be (H,W,3) or (K,H,W,3), got {tuple(getattr(t, 'shape', ()))}")
    if t.dim() == 3:
        t = t[None]
    if crop:
        hc, wc = t.shape[1] // 10, t.shape[2] // 10
        t = t[:, hc:t.shape[1] - hc, wc:t.shape[2] - wc]
    if t.shape[1] < 16 or t.shape[2] < 16:
        raise ValueError(f"LPIPS: frames of {t.shape[1]} x {t.shape[2]} pixels{' after the crop' if crop else ''}: relu5_3 needs H, W >= 16")
    return t.detach().to(torch.float32).contiguous()


class LPIPS:
    """LPIPS-VGG of rendered frames on the GPU: `lpips.LPIPS(net='vgg')(rgb * 2 - 1, img * 2 - 1)` as the reference's renderer.ipynb calls it per held-out
    view, on the library's own kernels (13 conv3x3 + bias + ReLU as exact-fp32 MFMA implicit GEMMs, 4 max-pools, 5 heads; csrc/lpips.hip).

        lp = LPIPS(vgg_state, lin_state)            # or LPIPS.from_files(vgg16_path, lpips_vgg_path) / LPIPS.from_state_dict(lpips_state)
        d = lp(rgb, img)                            # (H,W,3) | (K,H,W,3) fp32 in [0,1] on the GPU -> (K,) float64 on the GPU, no host synchronisation
        d = lp(rgb, img, crop=True)                 # the notebook's Blender / LLFF protocol (cell 8): centre crop by H//10, W//10 first; DTU's is the full frame
        d, layers = lp(rgb, img, per_layer=True)    # layers (K,5): the five tap values whose sum is d
        f = lp.features(img); d = lp(rgb, f)        # the target's five feature maps, computed once per held-out view; the same bits as lp(rgb, img)

    The weights are parsed (`parse_lpips_weights`), packed once and kept on the device.  Inputs are not clamped; H, W >= 16 (relu5_3 needs a pixel).  No
    gradients.  Memory: frames go through the trunk in chunks of `chunk_bytes` (default 512 MiB) of activations, at least one (prediction, target)
    pair at a time - the peak is a pair's relu1_1 and relu1_2 maps, 4 x 256 H W bytes = 336 MB at 512 x 640 - and `features` keeps 488 H W bytes per frame
    (five taps, 160 MB at 512 x 640).  The key names of the state dicts follow the published torchvision and lpips packages; neither is in this image, so the
    result is NOT pinned against the lpips package here - tests/lpips_refs.py restates the definition in float64."""

    def __init__(self, vgg_state, lin_state=None, device="cuda", chunk_bytes=512 << 20):
        from . import ops
        convs, lins = parse_lpips_weights(vgg_state, lin_state)
        self.device = torch.device(device)
        self.chunk_bytes = int(chunk_bytes)
        with torch.no_grad():
            self.packed = [ops.lpips_conv_pack(w.to(self.device), b.to(self.device)) for w, b in convs]
            self.lins = [v.to(self.device).contiguous() for v in lins]

    @classmethod
    def from_state_dict(cls, state, device="cuda", **kw):
        """One `lpips.LPIPS(net='vgg').state_dict()`: the trunk under net.slice{1..5} and the heads under lin{0..4}."""
        return cls(state, None, device=device, **kw)

    @classmethod
    def from_files(cls, vgg16_path, lpips_vgg_path, device="cuda", **kw):
        """torch.load of torchvision's vgg16 checkpoint (vgg16-397923af.pth) and the lpips package's weights/v0.1/vgg.pth."""
        return cls(torch.load(vgg16_path, map_location="cpu"), torch.load(lpips_vgg_path, map_location="cpu"), device=device, **kw)

    # -- the trunk on a (N,H,W,3) batch: the five tap maps
    def _taps(self, x):
        from . import ops
        taps = []
        for i, cout in enumerate(VGG_WIDTHS):
            if i in (2, 4, 7, 10):
                x = ops.lpips_pool(x)
            x = ops.lpips_conv(x, self.packed[i], cout)
            if i in LPIPS_TAPS:
                taps.append(x)
        return taps

    def _chunk(self, H, W):
        return max(1, self.chunk_bytes // (512 * H * W))          # relu1_1 + relu1_2 of one frame: 2 x 64 channels x 4 bytes per pixel

    def features(self, img, crop=False):
        """The five tap maps of K frames, a list of (K,h,w,C) fp32 tensors: what `__call__` accepts in place of the target frames."""
        x = _lpips_frames(img, "img", crop)
        step = self._chunk(x.shape[1], x.shape[2])
        parts = [self._taps(x[k:k + step]) for k in range(0, x.shape[0], step)]
        return [torch.cat([p[i] for p in parts]) if len(parts) > 1 else parts[0][i] for i in range(5)]

    def __call__(self, rgb, img, crop=False, per_layer=False):
        from . import ops
        x = _lpips_frames(rgb, "rgb", crop)
        K, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        feats = None
        if isinstance(img, (list, tuple)):
            feats = list(img)
            want = [(K, H >> s, W >> s, VGG_WIDTHS[t]) for s, t in enumerate(LPIPS_TAPS)]
            if len(feats) != 5 or any(not torch.is_tensor(f) or tuple(f.shape) != w for f, w in zip(feats, want)):
                raise RuntimeError(f"LPIPS: target features must be the five maps of LPIPS.features for these frames, {want}")
            ops._need_no_grad(*feats, op="LPIPS")
        else:
            y = _lpips_frames(img, "img", crop)
            if y.shape != x.shape:
                raise RuntimeError(f"LPIPS: rgb and img must have one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
        total = torch.empty((K,), device=x.device, dtype=torch.float64)
        layers = torch.empty((5, K), device=x.device, dtype=torch.float64)
        step = self._chunk(H, W)
        if feats is None:
            step = max(1, step // 2)
        for k in range(0, K, step):
            n = min(step, K - k)
            if feats is None:
                taps = self._taps(torch.cat([x[k:k + n], y[k:k + n]]))       # prediction and target as one launch per layer
                pairs = [(t[:n], t[n:]) for t in taps]
            else:
                pairs = [(t, f[k:k + n].contiguous()) for t, f in zip(self._taps(x[k:k + n]), feats)]
            for i, (f0, f1) in enumerate(pairs):
                ops.lpips_head(f0, f1, self.lins[i], layer_out=layers[i, k:k + n], total=total[k:k + n], accumulate=i > 0)
        return (total, layers.t().contiguous()) if per_layer else total
