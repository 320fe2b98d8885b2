"""Geometry from rendered depth: the depth maps of a scene's views fused into a coloured point cloud.

`render_view` and the systems' `render_rays` return a depth map per view and `SceneRays` holds every camera and every 8-bit image of the scene on the
device.  `fuse_depths` runs the cross-view geometric-consistency filter of the MVSNet line of work over the M depth maps (reproject each pixel into its
source views and back, keep it where enough views agree, average the agreeing depths) and compacts the kept pixels into points, colours and view counts,
all on the device (csrc/depth_fusion.hip).  The reference has no counterpart; the result is not pinned against any external fusion tool.
"""
import math

import numpy as np
import torch

from . import ops
from .utils import get_nearest_pose_ids

MAX_SOURCES = 32        # one bit per source view in `seen`


class PointCloud:
    """What fuse_depths returns.
        points (N,3) fp32 world, colors (N,3) uint8, n_views (N,) uint8, index (N,) int64 flat ray indices (view-major, then row-major), ascending
        count   (1,) int64 on the device: the true number of kept pixels (N = min(count, capacity) rows are meaningful when a capacity was given)
        depth (M,H,W) fp32 fused depth maps, mask (M,H,W) bool, seen (M,H,W) int32 bit masks (bit j: source j of src_ids agrees)
        src_ids (M,n_src) int32: the source views used, -1 where there is none"""

    def __init__(self, points, colors, n_views, index, count, depth, mask, seen, src_ids):
        self.points, self.colors, self.n_views, self.index, self.count = points, colors, n_views, index, count
        self.depth, self.mask, self.seen, self.src_ids = depth, mask, seen, src_ids


def nearest_source_ids(scene, n_src):
    """(M, n_src) int32: per view the n_src nearest OTHER views, nearest first (utils.get_nearest_pose_ids over the bank's float64 cameras), padded with -1
    when the scene has fewer than n_src other views."""
    c2w = scene._c2w64.numpy()
    M = c2w.shape[0]
    ids = np.full((M, n_src), -1, dtype=np.int32)
    for r in range(M):
        others = np.array([m for m in range(M) if m != r], dtype=np.int64)
        if len(others):
            near = get_nearest_pose_ids(c2w[r:r + 1], c2w[others], n_src)[0]
            ids[r, :len(near)] = others[near]
    return ids


def _source_ids(scene, src_ids, n_src):
    M = scene.n_views
    if src_ids is None:
        n_src = int(n_src)
        if not 1 <= n_src <= MAX_SOURCES:
            raise ValueError(f"fuse_depths: n_src must be in 1..{MAX_SOURCES} (one bit of `seen` per source view), got {n_src}")
        return nearest_source_ids(scene, n_src)
    ids = src_ids.cpu().numpy() if torch.is_tensor(src_ids) else np.asarray(src_ids)
    if ids.ndim != 2 or ids.shape[0] != M or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f"fuse_depths: src_ids must be an integer array of shape ({M}, n_src), got {ids.shape} {ids.dtype}")
    if not 1 <= ids.shape[1] <= MAX_SOURCES:
        raise ValueError(f"fuse_depths: src_ids must name 1..{MAX_SOURCES} source views per view (n_src > {MAX_SOURCES} has no bit in `seen`), "
                         f"got {ids.shape[1]}")
    if ids.min() < -1 or ids.max() >= M:
        raise ValueError(f"fuse_depths: src_ids must hold view ids in [0, {M}) or -1 for no view, got values in [{ids.min()}, {ids.max()}]")
    own = np.nonzero((ids == np.arange(M)[:, None]).any(1))[0]
    if len(own):
        raise ValueError(f"fuse_depths: src_ids names view {int(own[0])} as a source of itself; a view's sources are other views")
    return np.ascontiguousarray(ids, dtype=np.int32)


@torch.no_grad()
def render_depths(system, scene, **render_rays_kw):
    """(M,H,W) fp32 on the device: system.render_rays(scene.view(m)[0], **render_rays_kw)[1] for every view m of the bank, for any system with render_rays
    (MVSSystemFinetune, FusedScene)."""
    H, W = scene.hw
    out = []
    for m in range(scene.n_views):
        depth = system.render_rays(scene.view(m)[0], **render_rays_kw)[1]
        out.append(depth.reshape(H, W).to(scene.device, torch.float32))
    return torch.stack(out).contiguous()


@torch.no_grad()
def fuse_depths(scene, depths, src_ids=None, n_src=4, pix_thr=1.0, rel_thr=0.01, min_views=3, valid=None, capacity=None):
    """The M depth maps of `scene` (a SceneRays) -> a PointCloud.
        depths      (M,H,W) fp32 on the bank's device: camera-space z per pixel, as the systems render it.  A depth that is not finite or <= 0, a pixel
                    with valid == 0 and a pixel whose image has alpha 0 are holes: never kept and never a usable tap.
        src_ids     None: per view its n_src nearest other views (nearest_source_ids); or an (M,n_src) integer array, -1 for no view, n_src <= 32
        pix_thr, rel_thr    a source agrees when the pixel comes back within pix_thr pixels and its depth within rel_thr relative
        min_views   a pixel is kept when at least min_views sources agree
        valid       (M,H,W) bool | uint8 on the bank's device, or None
        capacity    None: the count is read from the device once and the outputs have exactly that many rows.  An integer: the outputs have `capacity`
                    rows, nothing is read from the device, and cloud.count says on the device how many pixels were kept (rows past it are not written;
                    a count above capacity means the cloud was cut and the call wants repeating)."""
    M, (H, W) = scene.n_views, scene.hw
    dev = scene.device
    if not torch.is_tensor(depths) or depths.dtype != torch.float32:
        raise TypeError(f"fuse_depths: depths must be a float32 tensor of shape ({M},{H},{W}), got {getattr(depths, 'dtype', type(depths).__name__)}")
    if tuple(depths.shape) != (M, H, W):
        raise ValueError(f"fuse_depths: depths must be ({M},{H},{W}), one map per view of the bank, got {tuple(depths.shape)}")
    if depths.device != scene.images.device:
        raise ValueError(f"fuse_depths: depths must be on the bank's device {scene.images.device}, got {depths.device}")
    if valid is not None:
        if not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"fuse_depths: valid must be a bool or uint8 tensor of shape ({M},{H},{W}), got {getattr(valid, 'dtype', type(valid).__name__)}")
        if tuple(valid.shape) != (M, H, W):
            raise ValueError(f"fuse_depths: valid must be ({M},{H},{W}), like depths, got {tuple(valid.shape)}")
        if valid.device != scene.images.device:
            raise ValueError(f"fuse_depths: valid must be on the bank's device {scene.images.device}, got {valid.device}")
    if H < 2 or W < 2:
        raise ValueError(f"fuse_depths: views of at least 2 x 2 pixels (a bilinear cell), got {H} x {W}")
    ids = _source_ids(scene, src_ids, n_src)
    pix_thr, rel_thr, min_views = float(pix_thr), float(rel_thr), int(min_views)
    if not (math.isfinite(pix_thr) and pix_thr > 0 and math.isfinite(rel_thr) and rel_thr > 0):
        raise ValueError(f"fuse_depths: pix_thr (pixels) and rel_thr (relative depth) must be finite and > 0, got {pix_thr}, {rel_thr}")
    if min_views < 0:
        raise ValueError(f"fuse_depths: min_views must be >= 0, got {min_views}")
    if capacity is not None and int(capacity) < 0:
        raise ValueError(f"fuse_depths: capacity must be None or >= 0, got {capacity}")

    w2c = np.linalg.inv(scene._c2w64.numpy())[:, :3, :4]                                 # float64 on the host, rounded once
    w2cs = torch.from_numpy(np.ascontiguousarray(w2c, dtype=np.float32)).to(dev)
    with torch.cuda.device(dev):
        src = torch.from_numpy(ids).to(dev)
        v8 = None if valid is None else (valid.view(torch.uint8) if valid.dtype == torch.bool else valid).contiguous()
        seen, fused, mask = ops.depth_consistency(scene.images, scene.c2ws, w2cs, scene.intrinsics, depths.contiguous(), src, pix_thr, rel_thr, min_views,
                                                  valid=v8, alpha=scene.has_alpha)
        bank = (scene.images, scene.c2ws, scene.intrinsics, fused, seen, mask)
        if capacity is None:
            count = ops.point_cloud(*bank, 0)[4]
            capacity = int(count.item())                                                # the one host read
        points, colors, n_views, index, count = ops.point_cloud(*bank, int(capacity))
    return PointCloud(points, colors, n_views, index, count, fused, mask.view(torch.bool), seen, src)


def save_ply(path, cloud):
    """A binary little-endian PLY of the cloud's points and colours: x y z float, red green blue uchar, 15 bytes per vertex.  Host side (numpy), next to
    utils.save_frames; takes a PointCloud or a (points, colors) pair.  Of a PointCloud with a caller-given capacity the first min(count, capacity) rows are
    written.  Returns the number of vertices."""
    if isinstance(cloud, PointCloud):
        n = min(int(cloud.count.item()), int(cloud.points.shape[0]))
        points, colors = cloud.points[:n], cloud.colors[:n]
    else:
        points, colors = cloud
    xyz = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    rgb = colors.detach().cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape or rgb.dtype != np.uint8:
        raise ValueError(f"save_ply: points (N,3) float and colors (N,3) uint8, got {xyz.shape} {xyz.dtype} and {rgb.shape} {rgb.dtype}")
    rec = np.empty(xyz.shape[0], dtype=PLY_VERTEX)
    for k, name in enumerate(("x", "y", "z")):
        rec[name] = xyz[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        rec[name] = rgb[:, k]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(rec)
    header += "".join(f"property {'float' if PLY_VERTEX[name] == np.dtype('<f4') else 'uchar'} {name}\n" for name in PLY_VERTEX.names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
    return len(rec)


PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
