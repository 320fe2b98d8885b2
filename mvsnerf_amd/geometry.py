"""Geometry from rendered depth: the depth maps of a scene's views fused into a coloured point cloud.

`render_view` and the systems' `render_rays` return a depth map per view and `SceneRays` holds every camera and every 8-bit image of the scene on the
device.  `fuse_depths` runs the cross-view geometric-consistency filter of the MVSNet line of work over the M depth maps (reproject each pixel into its
source views and back, keep it where enough views agree, average the agreeing depths) and compacts the kept pixels into points, colours and view counts,
all on the device (csrc/depth_fusion.hip).  The reference has no counterpart; the result is not pinned against any external fusion tool.

Geometry from density: `extract_mesh` turns a (D,H,W) field - a scene's node density, ops.node_density - into the triangle mesh of its level set by marching
tetrahedra over the Kuhn split of every cell (csrc/mesh.hip), `vertex_colors` asks the radiance network for a colour per vertex and `scene_mesh`
does both for a fine-tuned scene.  Not pinned against any external mesher either.

Geometry from depth, as a surface: `fuse_tsdf` integrates the depth maps into a truncated signed distance volume over a world box (csrc/tsdf.hip, DESIGN.md
4o) and `tsdf_mesh` meshes its zero level, unobserved space masked, with colours from the volume.

Geometry, measured: `PointGrid` answers exact nearest-neighbour queries within a radius between clouds of millions of points and `sample_mesh` puts points on a
mesh (csrc/cloud_metrics.hip); `evaluate.cloud_metrics` builds DTU's accuracy / completeness and the Tanks-and-Temples F-score on them.

Geometry, looked at: `render_mesh` rasterises a mesh into the scene's cameras (depth, face and colour maps; csrc/raster.hip), `face_views` counts
the views a face is seen in, `filter_mesh` cuts a mesh down to a subset of its faces, `cull_unseen` composes the three and `mesh_frames` makes the
`rgb | depth` turntable.  Not pinned against any external rasteriser.
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


def _depth_args(scene, depths, valid, who):
    """The refusals of a bank's depth maps and their valid mask, shared by fuse_depths and fuse_tsdf."""
    M, (H, W) = scene.n_views, scene.hw
    if not torch.is_tensor(depths) or depths.dtype != torch.float32:
        raise TypeError(f"{who}: depths must be a float32 tensor of shape ({M},{H},{W}), got {getattr(depths, 'dtype', type(depths).__name__)}")
    if tuple(depths.shape) != (M, H, W):
        raise ValueError(f"{who}: depths must be ({M},{H},{W}), one map per view of the bank, got {tuple(depths.shape)}")
    if depths.device != scene.images.device:
        raise ValueError(f"{who}: depths must be on the bank's device {scene.images.device}, got {depths.device}")
    if valid is not None:
        if not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"{who}: valid must be a bool or uint8 tensor of shape ({M},{H},{W}), got {getattr(valid, 'dtype', type(valid).__name__)}")
        if tuple(valid.shape) != (M, H, W):
            raise ValueError(f"{who}: valid must be ({M},{H},{W}), like depths, got {tuple(valid.shape)}")
        if valid.device != scene.images.device:
            raise ValueError(f"{who}: valid must be on the bank's device {scene.images.device}, got {valid.device}")


def _u8(mask):
    return (mask.view(torch.uint8) if mask.dtype == torch.bool else mask).contiguous()


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
    _depth_args(scene, depths, valid, "fuse_depths")
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
        v8 = None if valid is None else _u8(valid)
        seen, fused, mask = ops.depth_consistency(scene.images, scene.c2ws, w2cs, scene.intrinsics, depths.contiguous(), src, pix_thr, rel_thr, min_views,
                                                  valid=v8, alpha=scene.has_alpha)
        bank = (scene.images, scene.c2ws, scene.intrinsics, fused, seen, mask)
        if capacity is None:
            count = ops.point_cloud(*bank, 0)[4]
            capacity = int(count.item())                                                # the one host read
        points, colors, n_views, index, count = ops.point_cloud(*bank, int(capacity))
    return PointCloud(points, colors, n_views, index, count, fused, mask.view(torch.bool), seen, src)


class TriangleMesh:
    """What extract_mesh and scene_mesh return.
        vertices (V,3) fp32 world (box= or positions=; grid coordinates without either), ndc (V,3) fp32: the coordinates ops.volume_sample resolves
        faces (T,3) int32 vertex numbers, counter-clockwise seen from the side where the field is below the level
        vertex_edge (V,) int64, ascending: node * 8 + e, the grid edge a vertex lies on (node = (k H + j) W + i, e = 0..6 the owned edge)
        colors (V,3) uint8 or None
        count   (2,) int64 on the device: the true numbers of vertices and faces (the first min(count, rows) rows of each array are meaningful when a
                capacity was given; a count above it means the mesh was cut and the call wants repeating)"""

    def __init__(self, vertices, ndc, faces, vertex_edge, count, colors=None):
        self.vertices, self.ndc, self.faces, self.vertex_edge, self.count, self.colors = vertices, ndc, faces, vertex_edge, count, colors


def _mesh_args(field, level, positions, box, capacity, who, valid=None):
    """The refusals of extract_mesh, before the library is touched -> (level, box as a (2,3) fp32 host tensor | None, capacity pair | None)."""
    if not torch.is_tensor(field) or field.dtype != torch.float32:
        raise TypeError(f"{who}: field must be a float32 tensor of shape (D,H,W), got {getattr(field, 'dtype', type(field).__name__)}")
    if field.dim() != 3 or min(field.shape) < 2:
        raise ValueError(f"{who}: field must be (D,H,W) with every dimension >= 2 (a cell), got {tuple(field.shape)}")
    D, H, W = (int(v) for v in field.shape)
    if D * H * W > ops.MESH_MAX_NODES:
        raise ValueError(f"{who}: at most 2^27 nodes (vertex and face numbers are int32), got {D} x {H} x {W}")
    level = float(level)
    if not math.isfinite(level):
        raise ValueError(f"{who}: level must be finite, got {level}")
    if positions is not None and box is not None:
        raise ValueError(f"{who}: positions (a table of node positions) and box (lo, hi) exclude each other")
    if positions is not None:
        if not torch.is_tensor(positions) or positions.dtype != torch.float32:
            raise TypeError(f"{who}: positions must be a float32 tensor of shape ({D},{H},{W},3), got {getattr(positions, 'dtype', type(positions).__name__)}")
        if tuple(positions.shape) != (D, H, W, 3):
            raise ValueError(f"{who}: positions must be ({D},{H},{W},3), one position per node, got {tuple(positions.shape)}")
        if positions.device != field.device:
            raise ValueError(f"{who}: positions must be on the field's device {field.device}, got {positions.device}")
    if box is not None:
        box = torch.as_tensor(box).detach().to("cpu", torch.float32)
        if box.numel() != 6 or not bool(torch.isfinite(box).all()):
            raise ValueError(f"{who}: box must be (lo, hi), 2 x 3 finite numbers, got {tuple(box.shape)}")
        box = box.reshape(2, 3)
    if valid is not None:
        if not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"{who}: valid must be a bool or uint8 tensor of shape ({D},{H},{W}), got {getattr(valid, 'dtype', type(valid).__name__)}")
        if tuple(valid.shape) != (D, H, W):
            raise ValueError(f"{who}: valid must be ({D},{H},{W}), a byte per node, got {tuple(valid.shape)}")
        if valid.device != field.device:
            raise ValueError(f"{who}: valid must be on the field's device {field.device}, got {valid.device}")
    if capacity is not None:
        try:
            cap = (int(capacity[0]), int(capacity[1]))
            ok = len(capacity) == 2 and min(cap) >= 0
        except (TypeError, ValueError, IndexError):
            ok = False
        if not ok:
            raise ValueError(f"{who}: capacity must be None or a pair (max_vertices, max_faces) of numbers >= 0, got {capacity!r}")
        capacity = cap
    return level, box, capacity


@torch.no_grad()
def extract_mesh(field, level, positions=None, box=None, capacity=None, valid=None):
    """The level set of a scalar field on a grid as a TriangleMesh: marching tetrahedra over the Kuhn split of every cell (csrc/mesh.hip).
        field       (D,H,W) fp32 on the GPU, e.g. a scene's node density; a node is inside iff field >= level (NaN: outside; write -inf into nodes to mask)
        level       finite
        positions   (D,H,W,3) fp32 node positions on the field's device (ops.voxel_points(...)[1] of a frustum volume): vertices interpolate them
        box         (lo, hi), 2 x 3 numbers: vertices = lo + ndc * (hi - lo) (a box volume's bbox_3d).  Neither: vertices are grid coordinates.
        capacity    None: the counts are read from the device once and the arrays have exactly V and T rows.  A pair (max_vertices, max_faces): nothing
                    is read from the device, mesh.count holds the true totals and rows past them are not written.
        valid       (D,H,W) bool | uint8 on the field's device, non-zero = valid, or None: an edge carries a vertex only if both its ends are valid and a
                    tetrahedron emits faces only if its four corners are valid - the unmasked mesh with every vertex on an edge with an invalid end and
                    every face using such a vertex dropped.  Vertices no surviving face uses are kept; the surface is open along invalid nodes.
    The surface is closed and consistently oriented wherever it does not touch the grid border; a positions table with a mirrored mapping flips the
    winding."""
    level, box, capacity = _mesh_args(field, level, positions, box, capacity, "extract_mesh", valid)
    with torch.cuda.device(field.device):
        vertices, ndc, vertex_edge, faces, count = ops.mesh_extract(field.contiguous(), level, None if positions is None else positions.contiguous(),
                                                                    box, capacity, valid=None if valid is None else _u8(valid))
    return TriangleMesh(vertices, ndc, faces, vertex_edge, count)


class TSDFVolume:
    """What fuse_tsdf returns.
        tsdf (D,H,W) fp32: the mean truncated signed distance in units of trunc, positive in front of the surface, at most 1; +1 where nothing was seen
        weight (D,H,W) int32: the number of views that contributed; colors (D,H,W,4) uint8: the mean RGB of the views within trunc of the surface and
        alpha 255, or four zero bytes where there is none
        box (2,3) fp32 on the host: (lo, hi), the world positions of nodes (0,0,0) and (W-1,H-1,D-1); trunc: the truncation distance in world units"""

    def __init__(self, tsdf, weight, colors, box, trunc):
        self.tsdf, self.weight, self.colors, self.box, self.trunc = tsdf, weight, colors, box, trunc


@torch.no_grad()
def fuse_tsdf(scene, depths, box, dims, trunc=None, valid=None, views=None, z_min=0.0):
    """The M depth maps of `scene` (a SceneRays) -> a TSDFVolume: every node of a dims = (D,H,W) grid over the world box is projected into every view and
    takes the truncated difference between the depth of its NEAREST pixel and its own (csrc/tsdf.hip).
        depths, valid   as fuse_depths takes them: holes are depths that are not finite or <= 0, pixels with valid == 0 and pixels of alpha 0
        box         (lo, hi), 2 x 3 finite numbers with hi > lo: node (i,j,k) sits at lo + (i/(W-1), j/(H-1), k/(D-1)) * (hi - lo)
        dims        (D,H,W), each >= 2, at most 2^27 nodes
        trunc       the truncation distance in world units; None: 3 x the longest voxel edge
        views       a list of distinct view ids (integrated in ascending order), default every view
        z_min       a node nearer to a camera than this (camera-space z) takes nothing from it
    Not pinned against any external fusion tool."""
    who = "fuse_tsdf"
    M = scene.n_views
    _depth_args(scene, depths, valid, who)
    box = torch.as_tensor(box).detach().to("cpu", torch.float32)
    if box.numel() != 6 or not bool(torch.isfinite(box).all()):
        raise ValueError(f"{who}: box must be (lo, hi), 2 x 3 finite numbers, got {tuple(box.shape)}")
    box = box.reshape(2, 3)
    if not bool((box[1] > box[0]).all()):
        raise ValueError(f"{who}: box must have hi > lo on every axis, got lo {box[0].tolist()}, hi {box[1].tolist()}")
    try:
        D, H, W = (int(v) for v in dims)
        ok = len(dims) == 3 and all(int(v) == v for v in dims) and min(D, H, W) >= 2
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{who}: dims must be three integers (D,H,W), each >= 2, got {dims!r}")
    if D * H * W > ops.MESH_MAX_NODES:
        raise ValueError(f"{who}: at most 2^27 nodes (the mesher's vertex and face numbers are int32), got {D} x {H} x {W}")
    if trunc is None:
        trunc = 3.0 * max(float(box[1, 0] - box[0, 0]) / (W - 1), float(box[1, 1] - box[0, 1]) / (H - 1), float(box[1, 2] - box[0, 2]) / (D - 1))
    trunc, z_min = float(trunc), float(z_min)
    if not (math.isfinite(trunc) and trunc > 0):
        raise ValueError(f"{who}: trunc (world units) must be finite and > 0, got {trunc}")
    if not (math.isfinite(z_min) and z_min >= 0):
        raise ValueError(f"{who}: z_min must be finite and >= 0, got {z_min}")
    ids = None
    if views is not None:
        ids = views.cpu().numpy() if torch.is_tensor(views) else np.asarray(views)
        if ids.ndim != 1 or ids.size < 1 or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError(f"{who}: views must be a 1-D list of at least one integer view id, got shape {ids.shape} {ids.dtype}")
        if ids.min() < 0 or ids.max() >= M or len(np.unique(ids)) != ids.size:
            raise ValueError(f"{who}: views must hold distinct view ids in [0, {M}), got {ids.tolist()}")
        ids = np.sort(ids).astype(np.int32)

    dev = scene.device
    w2c = np.linalg.inv(scene._c2w64.numpy())[:, :3, :4]                                 # float64 on the host, rounded once
    w2cs = torch.from_numpy(np.ascontiguousarray(w2c, dtype=np.float32)).to(dev)
    with torch.cuda.device(dev):
        tsdf, weight, colors = ops.tsdf_integrate(scene.images, w2cs, scene.intrinsics, depths.contiguous(), box, (D, H, W), trunc,
                                                  valid=None if valid is None else _u8(valid), alpha=scene.has_alpha,
                                                  views=None if ids is None else torch.from_numpy(ids).to(dev), z_min=z_min)
    return TSDFVolume(tsdf, weight, colors, box, trunc)


@torch.no_grad()
def tsdf_mesh(vol, min_weight=1, colors=True, capacity=None):
    """The zero level of a TSDFVolume as a TriangleMesh in the volume's world box: extract_mesh(-vol.tsdf, 0.0, box=vol.box, valid=vol.weight >= min_weight),
    so only space that at least min_weight views observed carries surface and the faces are counter-clockwise seen from the observed side.
    colors: mesh.colors = the end nodes' colours interpolated at each vertex (ops.tsdf_vertex_colors); rows past the count stay 0."""
    if not isinstance(vol, TSDFVolume):
        raise TypeError(f"tsdf_mesh: a TSDFVolume (fuse_tsdf's result) expected, got {type(vol).__name__}")
    if int(min_weight) != min_weight or int(min_weight) < 1:
        raise ValueError(f"tsdf_mesh: min_weight must be an integer >= 1 (a node nobody observed has no distance), got {min_weight}")
    level, box, capacity = _mesh_args(vol.tsdf, 0.0, None, vol.box, capacity, "tsdf_mesh")
    with torch.cuda.device(vol.tsdf.device):
        mesh = extract_mesh(-vol.tsdf, level, box=box, valid=vol.weight >= int(min_weight), capacity=capacity)
        if colors:
            mesh.colors = ops.tsdf_vertex_colors(vol.tsdf, vol.colors, mesh.vertex_edge, mesh.count)
    return mesh


def _scene_sources(system):
    """(the keywords of ops.node_density but dilate, the system's reference pose) - train._density_sources, as the systems' own density methods call it."""
    from . import train
    if isinstance(system, train.MVSSystemFusion):
        system._need_volume()
        F = system.args.feat_dim
        pose = system.pose_source_ref
        return train._density_sources(system.network_fn, F, system.volume.feat_volume.detach(), pose, (F - 8) // 4), pose
    if isinstance(system, train.MVSSystemFinetune):
        V = system.imgs.shape[1]
        vol = system.volume.feat_volume.detach()
        H, W = system.imgs.shape[-2:]
        src = train._density_sources(system.network_fn, system.args.feat_dim, vol, system.pose_source, V, system.imgs[0] if vol.shape[1] == 8 else None,
                                     near_far=system.near_far_source, ref_hw=(int(H), int(W)), pad=system.args.pad,
                                     lindisp=bool(getattr(system.args, "use_disp", False)))
        return src, system.pose_source
    raise TypeError(f"a fine-tuned scene (MVSSystemFinetune or MVSSystemFusion) expected, got {type(system).__name__}")


@torch.no_grad()
def vertex_colors(system, mesh, origin=None, chunk=262144):
    """(rows,3) uint8: the radiance network's colour at each vertex of `mesh`, seen from `origin` - a world point (3 numbers), default the centre of
    the system's reference camera.  Per chunk of rows: ops.gather (8-channel volume and source images, at mesh.vertices / mesh.ndc) or
    ops.gather_colorvol (colour volume, at mesh.ndc) on rows shaped (n,1,3) -> ops.dir_feature(vertices - origin, w2c_ref, normalize=True) ->
    ops.mlp_forward(alpha_only=False) with N = n, S = 1 (the way ops.node_density queries nodes) -> trunc(clamp(rgb, 0, 1) * 255).  The sources are
    train._density_sources', so any network mlp_forward runs works.  The count is read from the device once: rows past min(count, rows) - a mesh
    with a caller-given capacity has such - are left 0."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"vertex_colors: chunk must be >= 1, got {chunk}")
    src, pose = _scene_sources(system)
    vol_cl, F = src["vol_cl"], int(system.args.feat_dim)
    dev = vol_cl.device
    alt = {k: v for k, v in src.items() if k not in ("vol_cl", "packed", "w2cs", "imgs", "intrinsics", "camera")}
    with torch.cuda.device(dev):
        rows = min(int(mesh.count[0].item()), int(mesh.vertices.shape[0]))
        colors = torch.zeros((int(mesh.vertices.shape[0]), 3), device=dev, dtype=torch.uint8)
        o = pose["c2ws"][0][:3, 3] if origin is None else torch.as_tensor(origin, dtype=torch.float32).reshape(3)
        o = o.to(dev, torch.float32).contiguous()
        w2c_ref = pose["w2cs"][0].contiguous()
        for a in range(0, rows, chunk):
            n = min(chunk, rows - a)
            v, ndc = mesh.vertices[a:a + n], mesh.ndc[a:a + n].view(n, 1, 3)
            if "imgs" in src:
                feat, _ = ops.gather(vol_cl, src["imgs"], src["w2cs"], src["intrinsics"], v.view(n, 1, 3), ndc)
            else:
                feat, _ = ops.gather_colorvol(vol_cl, ndc)
            dirs = ops.dir_feature(ops.mesh_dirs(v, o), w2c_ref, normalize=True)
            raw = ops.mlp_forward(src["packed"], F, ndc.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, n, 1, 0, dev, **alt)
            colors[a:a + n] = ops.mesh_rgb_u8(raw)
    return colors


@torch.no_grad()
def scene_mesh(system, level, colors=True, origin=None, dilate=0, capacity=None):
    """The surface sigma = level of a fine-tuned scene as a TriangleMesh in world coordinates.  MVSSystemFusion: the field is the box volume's node
    density (ops.node_density) and box = bbox_3d.  MVSSystemFinetune: the field is the render-space node density and positions are the world positions
    of the frustum's nodes (ops.voxel_points with the reference camera).  dilate: ops.node_density's.  colors: vertex_colors(system, mesh, origin).
    No attribute of the system is assigned: system.density_volume stays what it was."""
    from . import train
    src, pose = _scene_sources(system)
    with torch.cuda.device(src["vol_cl"].device):
        field = ops.node_density(dilate=dilate, **src)
        if isinstance(system, train.MVSSystemFusion):
            mesh = extract_mesh(field, level, box=system.bbox_3d, capacity=capacity)
        else:
            D, H, W = field.shape
            Hi, Wi = system.imgs.shape[-2:]      # the reference view, as _density_sources hands it to ops.node_density (a colour volume's sources hold none)
            positions = ops.voxel_points(D, H, W, K_ref=pose["intrinsics"][0], c2w_ref=pose["c2ws"][0], near_far=system.near_far_source,
                                         ref_hw=(int(Hi), int(Wi)), pad=system.args.pad, lindisp=bool(getattr(system.args, "use_disp", False)),
                                         device=field.device)[1]
            mesh = extract_mesh(field, level, positions=positions.view(D, H, W, 3), capacity=capacity)
    if colors:
        mesh.colors = vertex_colors(system, mesh, origin)
    return mesh


# ---- how far two products are from each other: a point grid, the exact nearest neighbour within a radius, points on a mesh (csrc/cloud_metrics.hip,
#      DESIGN.md 4p; evaluate.cloud_metrics puts the DTU / Tanks-and-Temples scores on top)
GRID_CELL_FACTOR = 0.5      # cell=None: the edge is max_dist * this (DESIGN.md 4p holds the measurement behind the choice)
GRID_CELL_CAP = 1 << 22     # ... grown by a quarter at a time until the table has at most this many cells (16 MiB of cell starts); ops.GRID_MAX_CELLS is the kernels' limit


def _cloud_tensor(t, name, who):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{who}: {name} must be a float32 tensor of shape (n,3), got {type(t).__name__} {getattr(t, 'dtype', '')} "
                         f"{tuple(getattr(t, 'shape', ()))}")
    if t.shape[0] >= 1 << 31:
        raise ValueError(f"{who}: {name} must hold fewer than 2^31 rows, got {t.shape[0]}")
    return t


def _radius(max_dist, who):
    """max_dist as the fp32 number the kernels use; its square must be a finite, positive fp32 number too."""
    try:
        r = float(max_dist)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: max_dist must be a finite number > 0, got {max_dist!r}") from None
    with np.errstate(over="ignore"):
        r32 = np.float32(r) if math.isfinite(r) else np.float32("nan")
        sq = r32 * r32
    if not (r > 0 and math.isfinite(float(r32)) and math.isfinite(float(sq)) and float(sq) > 0):
        raise ValueError(f"{who}: max_dist must be finite and > 0 (and so must its fp32 square), got {max_dist!r}")
    return float(r32)


class PointGrid:
    """A uniform grid over a target cloud for exact nearest-neighbour queries within max_dist.
        points      (n,3) fp32 on the GPU, 0 <= n < 2^31; rows with a non-finite coordinate are left out and are never anyone's neighbour
        max_dist    finite, > 0: the search radius of `nearest`
        cell        None: max_dist * GRID_CELL_FACTOR; or the edge of a cell.  Either is grown until the table has at most GRID_CELL_CAP cells.
        box         None: the bounds of the finite rows, from a min / max reduction on the device and ONE host read of six floats (the host sizes the
                    cell table); or (lo, hi), 2 x 3 finite numbers: nothing is read from the device.  Points outside the box land in its border cells.
    No result of `nearest` depends on cell or box.  Attributes: lo (3 floats), cell, dims (dx, dy, dz), cell_start (cells + 1,) int32, records (n,4) fp32
    (x, y, z, the bits of the original row; grouped by cell, the first cell_start[-1] rows are written)."""

    def __init__(self, points, max_dist, cell=None, box=None):
        who = "PointGrid"
        _cloud_tensor(points, "points", who)
        self.max_dist = _radius(max_dist, who)
        if cell is not None:
            cell = float(cell)
            with np.errstate(over="ignore", divide="ignore"):
                ok = math.isfinite(cell) and cell > 0 and math.isfinite(float(np.float32(cell))) and math.isfinite(float(np.float32(1) / np.float32(cell)))
            if not ok:
                raise ValueError(f"{who}: cell must be None or a finite edge > 0 with a finite fp32 reciprocal, got {cell}")
        if box is not None:
            if not torch.is_tensor(box) and all(isinstance(b, np.ndarray) for b in box):
                box = np.stack([np.asarray(b, dtype=np.float32).reshape(-1) for b in box])       # (a list of arrays is the slow path of torch.as_tensor)
            box = torch.as_tensor(box).detach().to("cpu", torch.float32)
            if box.numel() != 6 or not bool(torch.isfinite(box).all()) or bool((box.reshape(2, 3)[1] < box.reshape(2, 3)[0]).any()):
                raise ValueError(f"{who}: box must be (lo, hi), 2 x 3 finite numbers with lo <= hi, got {tuple(box.shape)}")
            box = box.reshape(2, 3).tolist()
        self.n = int(points.shape[0])
        self.device = points.device
        with torch.cuda.device(self.device):
            points = points.contiguous()
            if box is None:
                box = [[0.0] * 3, [0.0] * 3]
                if self.n:
                    b = ops.grid_bounds(points).tolist()                               # the one host read
                    if all(math.isfinite(v) for v in b):                              # (no finite row: the grid is empty, any box does)
                        box = [b[:3], b[3:]]
            self.lo, self.cell, self.dims = _grid_layout(box[0], box[1], self.max_dist * GRID_CELL_FACTOR if cell is None else cell, GRID_CELL_CAP)
            self.cell_start, self.records = ops.grid_build(points, self.lo, self.cell, self.dims)

    @torch.no_grad()
    def nearest(self, query):
        """query (N,3) fp32 on the grid's device -> (dist (N,) fp32, index (N,) int32): the grid point with the smallest d2 = (dx dx + dy dy) + dz dz (fp32,
        every operation rounded on its own) among those with d2 <= max_dist max_dist, the lowest original index among equals, dist = sqrt(d2); +inf and -1
        when there is none or the query row is not finite.  Exact: the grid only decides which points are looked at."""
        _cloud_tensor(query, "query", "PointGrid.nearest")
        if query.device != self.device:
            raise ValueError(f"PointGrid.nearest: query must be on the grid's device {self.device}, got {query.device}")
        with torch.cuda.device(self.device):
            return ops.grid_nearest(self.lo, self.cell, self.dims, self.cell_start, self.records, query.contiguous(), self.max_dist)


def _grid_layout(lo, hi, cell, cap):
    """(lo, cell as the fp32 number, (dx, dy, dz)): dim = floor((hi - lo) / cell) + 1 per axis, the edge grown by a quarter until dx dy dz <= cap."""
    lo = [float(np.float32(v)) for v in lo]
    ext = [max(float(h) - l, 0.0) for l, h in zip(lo, hi)]
    cell = float(np.float32(cell))
    while True:
        dims = tuple(int(e // cell) + 1 for e in ext)
        if dims[0] * dims[1] * dims[2] <= cap:
            return lo, cell, dims
        cell = float(np.float32(cell * 1.25))


class MeshSamples(tuple):
    """What sample_mesh returns: the pair (points (P,3) fp32, face (P,) int32), with .points, .face and .count - (2,) int64 on the device: the true number
    of points (above the rows when a capacity was given and was too small) and the largest subdivision n of any face."""

    def __new__(cls, points, face, count):
        self = super().__new__(cls, (points, face))
        self.points, self.face, self.count = points, face, count
        return self


@torch.no_grad()
def sample_mesh(mesh, spacing, capacity=None):
    """Points on the surface of a TriangleMesh about `spacing` apart, the same bytes every run (csrc/cloud_metrics.hip).
    Per face n = max(1, ceil(L / spacing)) with L its longest edge; the face emits the centroids of the n n congruent sub-triangles of its barycentric
    lattice (rows j = 0..n-1 from the edge AB towards C, in a row i = 0..n-1-j from A towards B: the upward triangle, then the downward one).  A face with
    a non-finite vertex emits nothing; a zero-area face emits its n n points like any other.  Ordered by face, then by lattice order.
        capacity    None: the count is read from the device once, the outputs have exactly P rows, and a face that needs n > 1024 raises RuntimeError.
                    An integer: nothing is read from the device; .count[0] is the true P (rows past it are not written), a face with n > 1024 emits
                    nothing and .count[1] > 1024 says so.
    Of a mesh extracted with a capacity only the first min(mesh.count, rows) vertices and faces are read."""
    who = "sample_mesh"
    if not (hasattr(mesh, "vertices") and hasattr(mesh, "faces")):
        raise ValueError(f"{who}: a TriangleMesh (vertices, faces) expected, got {type(mesh).__name__}")
    _cloud_tensor(mesh.vertices, "mesh.vertices", who)
    if not torch.is_tensor(mesh.faces) or mesh.faces.dtype != torch.int32 or mesh.faces.dim() != 2 or mesh.faces.shape[1] != 3:
        raise ValueError(f"{who}: mesh.faces must be an int32 tensor of shape (T,3), got {getattr(mesh.faces, 'dtype', '')} {tuple(getattr(mesh.faces, 'shape', ()))}")
    try:
        spacing = float(spacing)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: spacing must be a finite number > 0, got {spacing!r}") from None
    if not (math.isfinite(spacing) and spacing > 0 and math.isfinite(float(np.float32(spacing))) and float(np.float32(spacing)) > 0):
        raise ValueError(f"{who}: spacing must be finite and > 0, got {spacing}")
    if capacity is not None and not 0 <= int(capacity) < 1 << 31:
        raise ValueError(f"{who}: capacity must be None or in [0, 2^31), got {capacity}")
    with torch.cuda.device(mesh.vertices.device):
        points, face, count = ops.mesh_sample(mesh.vertices.contiguous(), mesh.faces.contiguous(), spacing, None if capacity is None else int(capacity),
                                              mesh_count=getattr(mesh, "count", None))
    return MeshSamples(points, face, count)


# ---- a mesh back in the scene's cameras: the z-buffer rasteriser, the views a face is seen in, a mesh cut down to a subset of its faces (csrc/raster.hip,
#      DESIGN.md 4r).  Not pinned against any external rasteriser.
RASTER_MAX_FACES = (1 << 31) - 1


class MeshImage:
    """What render_mesh returns: depth (M,H,W) fp32 camera-space z, 0 where nothing was hit (the bank's hole); face (M,H,W) int32, -1 for nothing;
    colors (M,H,W,3) uint8 or None (a mesh without vertex colours); views: the view ids shown, in order (None: every view of the bank); mask = face >= 0."""

    def __init__(self, depth, face, colors, views=None):
        self.depth, self.face, self.colors, self.views = depth, face, colors, views

    @property
    def mask(self):
        return self.face >= 0


def _raster_mesh(mesh, who):
    """The refusals of a mesh handed to the rasteriser or the filter, before the library is touched."""
    if not (hasattr(mesh, "vertices") and hasattr(mesh, "faces")):
        raise TypeError(f"{who}: a TriangleMesh (vertices, faces) expected, got {type(mesh).__name__}")
    v, f = mesh.vertices, mesh.faces
    if not torch.is_tensor(v) or v.dtype != torch.float32:
        raise TypeError(f"{who}: mesh.vertices must be a float32 tensor of shape (V,3), got {getattr(v, 'dtype', type(v).__name__)}")
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"{who}: mesh.vertices must be (V,3), got {tuple(v.shape)}")
    if not torch.is_tensor(f) or f.dtype != torch.int32:
        raise TypeError(f"{who}: mesh.faces must be an int32 tensor of shape (T,3), got {getattr(f, 'dtype', type(f).__name__)}")
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"{who}: mesh.faces must be (T,3), got {tuple(f.shape)}")
    if f.shape[0] > RASTER_MAX_FACES or v.shape[0] > RASTER_MAX_FACES:
        raise ValueError(f"{who}: at most 2^31 - 1 vertices and faces (a face number is an int32), got {v.shape[0]} and {f.shape[0]}")
    if f.device != v.device:
        raise ValueError(f"{who}: mesh.faces must be on the vertices' device {v.device}, got {f.device}")
    c = getattr(mesh, "colors", None)
    if c is not None:
        if not torch.is_tensor(c) or c.dtype != torch.uint8:
            raise TypeError(f"{who}: mesh.colors must be None or a uint8 tensor of shape ({v.shape[0]},3), got {getattr(c, 'dtype', type(c).__name__)}")
        if tuple(c.shape) != (v.shape[0], 3):
            raise ValueError(f"{who}: mesh.colors must be ({v.shape[0]},3), a row per vertex, got {tuple(c.shape)}")
        if c.device != v.device:
            raise ValueError(f"{who}: mesh.colors must be on the vertices' device {v.device}, got {c.device}")
    n = getattr(mesh, "count", None)
    if n is not None and not (torch.is_tensor(n) and n.dtype == torch.int64 and tuple(n.shape) == (2,) and n.device == v.device):
        raise ValueError(f"{who}: mesh.count must be None or a (2,) int64 tensor on the vertices' device {v.device}")
    return v.device


def _raster_cameras(scene, cameras, dev, who):
    """(w2c (M,3,4) float64 -> fp32 rounded once, K (M,3,3) fp32, (H, W)) on the host, from a SceneRays or cameras=(c2ws, intrinsics, (H, W))."""
    if cameras is not None:
        if scene is not None:
            raise ValueError(f"{who}: scene (a SceneRays) and cameras=(c2ws, intrinsics, (H, W)) exclude each other")
        try:
            c2ws, K, hw = cameras
            H, W = (int(v) for v in hw)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: cameras must be (c2ws (M,4,4), intrinsics (M,3,3) | (3,3), (H, W)), got {type(cameras).__name__}") from None
        c2w = torch.as_tensor(c2ws).detach().to("cpu", torch.float64)
        if c2w.dim() != 3 or c2w.shape[0] < 1 or tuple(c2w.shape[1:]) not in ((4, 4), (3, 4)):
            raise ValueError(f"{who}: cameras[0] must be (M,4,4) or (M,3,4) poses, got {tuple(c2w.shape)}")
        M = int(c2w.shape[0])
        if c2w.shape[1] == 3:
            c2w = torch.cat((c2w, torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(M, 1, 4)), 1)
        K64 = torch.as_tensor(K).detach().to("cpu", torch.float64)
        if tuple(K64.shape) == (3, 3):
            K64 = K64.expand(M, 3, 3)
        if tuple(K64.shape) != (M, 3, 3):
            raise ValueError(f"{who}: cameras[1] must be ({M},3,3) or (3,3) intrinsics, got {tuple(K64.shape)}")
    else:
        if not (hasattr(scene, "_c2w64") and hasattr(scene, "_K64") and hasattr(scene, "hw")):
            raise TypeError(f"{who}: a SceneRays expected (or cameras=(c2ws, intrinsics, (H, W))), got {type(scene).__name__}")
        bank = scene.images.device if hasattr(scene, "images") else torch.device(scene.device)     # (SceneRays.device may lack the index)
        if bank != dev:
            raise ValueError(f"{who}: the mesh must be on the bank's device {bank}, got {dev}")
        c2w, K64, (H, W) = scene._c2w64, scene._K64, scene.hw
    if not (1 <= H <= ops.RASTER_MAX_IMAGE and 1 <= W <= ops.RASTER_MAX_IMAGE):
        raise ValueError(f"{who}: views of 1 x 1 to {ops.RASTER_MAX_IMAGE} x {ops.RASTER_MAX_IMAGE} pixels, got {H} x {W}")
    w2c = np.linalg.inv(c2w.numpy())[:, :3, :4]                                          # float64 on the host, rounded once
    return (torch.from_numpy(np.ascontiguousarray(w2c, dtype=np.float32)), K64.to(torch.float32).contiguous(), (int(H), int(W)))


def _render_args(views, M, cull, z_min, background, who):
    ids = None
    if views is not None:
        ids = views.cpu().numpy() if torch.is_tensor(views) else np.asarray(views)
        if ids.ndim != 1 or ids.size < 1 or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError(f"{who}: views must be a 1-D list of at least one integer view id, got shape {ids.shape} {ids.dtype}")
        if ids.min() < 0 or ids.max() >= M:
            raise ValueError(f"{who}: views must hold view ids in [0, {M}), got {ids.tolist()}")
        ids = np.ascontiguousarray(ids, dtype=np.int32)
    if (ids.size if ids is not None else M) > ops.RASTER_MAX_VIEWS:
        raise ValueError(f"{who}: at most {ops.RASTER_MAX_VIEWS} views a call, got {ids.size if ids is not None else M}")
    if isinstance(cull, bool) or cull not in (-1, 0, 1):
        raise ValueError(f"{who}: cull must be 0 (both windings), +1 (drop A > 0: back faces of the library's own meshes) or -1, got {cull!r}")
    try:
        z_min = float(z_min)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: z_min must be finite and >= 0, got {z_min!r}") from None
    if not (math.isfinite(z_min) and z_min >= 0):
        raise ValueError(f"{who}: z_min must be finite and >= 0, got {z_min}")
    try:
        bg = tuple(int(b) for b in background)
        ok = len(bg) == 3 and all(int(b) == b for b in background) and min(bg) >= 0 and max(bg) <= 255
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{who}: background must be three bytes (R, G, B) in 0..255, got {background!r}")
    return ids, int(cull), z_min, bg


@torch.no_grad()
def render_mesh(mesh, scene=None, views=None, cull=0, z_min=0.0, background=(255, 255, 255), cameras=None):
    """A TriangleMesh rasterised into the scene's pinhole cameras -> a MeshImage (csrc/raster.hip, DESIGN.md 4r, where the definition is written out).
        scene       a SceneRays: its cameras and image size.  For novel poses cameras=(c2ws (M,4,4), intrinsics (M,3,3) | (3,3), (H, W)) replaces it.
        views       a list of view ids, shown in the list's order; default every view
        cull        0 keeps both windings; +1 drops faces whose snapped screen area A is > 0, -1 those with A < 0.  The front faces of the library's own
                    meshes (extract_mesh, tsdf_mesh) seen from outside have A < 0, so cull=+1 is back-face culling for them.
        z_min       a vertex or a fragment nearer than this (camera-space z) is not drawn; a face with such a vertex is dropped whole (no clipping)
        background  the bytes of a pixel nothing covers in `colors`
    Vertices are snapped to 1/256 pixel and coverage follows the top-left fill rule in integers: shared edges are watertight and no pixel is hit twice.
    The nearest fragment wins, the lowest face number among equal depths, whatever the order of arrival: the same bytes every run.  Of a mesh extracted with
    a capacity only the first min(mesh.count, rows) vertices and faces are read.  Not pinned against any external rasteriser."""
    who = "render_mesh"
    dev = _raster_mesh(mesh, who)
    w2c, K, hw = _raster_cameras(scene, cameras, dev, who)
    ids, cull, z_min, bg = _render_args(views, int(w2c.shape[0]), cull, z_min, background, who)
    with torch.cuda.device(dev):
        depth, face, colors = ops.mesh_raster(mesh.vertices.contiguous(), mesh.faces.contiguous(), w2c.to(dev), K.to(dev), hw,
                                              colors=None if mesh.colors is None else mesh.colors.contiguous(),
                                              views=None if ids is None else torch.from_numpy(ids).to(dev), cull=cull, z_min=z_min, background=bg,
                                              mesh_count=getattr(mesh, "count", None))
    return MeshImage(depth, face, colors, None if ids is None else ids.tolist())


@torch.no_grad()
def face_views(face, n_faces):
    """face (M,H,W) int32 on the GPU (MeshImage.face) -> (n_faces,) int32: the number of views in which a face owns at least one pixel."""
    who = "face_views"
    if not torch.is_tensor(face) or face.dtype != torch.int32:
        raise TypeError(f"{who}: face must be an int32 tensor of shape (M,H,W), got {getattr(face, 'dtype', type(face).__name__)}")
    if face.dim() != 3 or face.numel() < 1:
        raise ValueError(f"{who}: face must be a non-empty (M,H,W), got {tuple(face.shape)}")
    if face.shape[0] > ops.RASTER_MAX_VIEWS:
        raise ValueError(f"{who}: at most {ops.RASTER_MAX_VIEWS} views a call, got {face.shape[0]}")
    if isinstance(n_faces, bool) or int(n_faces) != n_faces or not 0 <= int(n_faces) <= RASTER_MAX_FACES:
        raise ValueError(f"{who}: n_faces must be an integer in [0, 2^31), got {n_faces!r}")
    with torch.cuda.device(face.device):
        return ops.mesh_face_views(face.contiguous(), int(n_faces))[0]


@torch.no_grad()
def filter_mesh(mesh, keep):
    """The TriangleMesh of the faces with keep != 0, in order, and the vertices they use, in order.
        keep        (T,) bool | uint8 on the mesh's device
    vertices / ndc / vertex_edge / colors are carried over; sub.vertex_index (V',) and sub.face_index (T',) int64 hold the original numbers.  A kept face
    with a vertex number outside the mesh is dropped.  The two totals are read from the device once; sub.count holds them.  Stable: the same bytes every run."""
    who = "filter_mesh"
    dev = _raster_mesh(mesh, who)
    T = int(mesh.faces.shape[0])
    if not torch.is_tensor(keep) or keep.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{who}: keep must be a bool or uint8 tensor of shape ({T},), got {getattr(keep, 'dtype', type(keep).__name__)}")
    if tuple(keep.shape) != (T,):
        raise ValueError(f"{who}: keep must be ({T},), a flag per face, got {tuple(keep.shape)}")
    if keep.device != dev:
        raise ValueError(f"{who}: keep must be on the mesh's device {dev}, got {keep.device}")
    V = int(mesh.vertices.shape[0])
    ndc, edge = getattr(mesh, "ndc", None), getattr(mesh, "vertex_edge", None)
    for name, t, dtype, shape in (("ndc", ndc, torch.float32, (V, 3)), ("vertex_edge", edge, torch.int64, (V,))):
        if t is not None and not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == shape and t.device == dev):
            raise ValueError(f"{who}: mesh.{name} must be None or a {shape} {dtype} tensor on {dev}")
    with torch.cuda.device(dev):
        v, n, e, c, vi, f, fi, count = ops.mesh_filter(mesh.vertices.contiguous(), mesh.faces.contiguous(), _u8(keep),
                                                       ndc=None if ndc is None else ndc.contiguous(), vertex_edge=None if edge is None else edge.contiguous(),
                                                       colors=None if mesh.colors is None else mesh.colors.contiguous(), mesh_count=getattr(mesh, "count", None))
    sub = TriangleMesh(v, n, f, e, count, c)
    sub.vertex_index, sub.face_index = vi, fi
    return sub


@torch.no_grad()
def cull_unseen(mesh, scene=None, min_views=1, **render_kw):
    """`mesh` without the faces that fewer than min_views cameras see: render_mesh(mesh, scene, **render_kw) -> face_views -> filter_mesh.  A face is seen by
    a view when it owns at least one pixel of that view's face map.  Removes the inner shells and back sides of a density mesh, which no scan could contain."""
    if isinstance(min_views, bool) or int(min_views) != min_views or int(min_views) < 0:
        raise ValueError(f"cull_unseen: min_views must be an integer >= 0, got {min_views!r}")
    img = render_mesh(mesh, scene, **render_kw)
    with torch.cuda.device(img.face.device):
        n = ops.mesh_face_views(img.face, int(mesh.faces.shape[0]), mesh_count=getattr(mesh, "count", None))[0]
        return filter_mesh(mesh, n >= int(min_views))


@torch.no_grad()
def mesh_frames(mesh, poses, hw, focal, crop=False, **render_kw):
    """uint8 (K, H', 2 W', 3) `rgb | depth` frames of the mesh seen from poses (K,4,4) | (K,3,4), the turntable render_path makes for a radiance field:
    the cameras of train.get_ray_directions (fx, fy = focal, centre (W / 2, H / 2)) -> render_mesh -> ops.frame_u8 per pose, with ONE depth range over the
    whole path (ops.depth_range of the K depth maps; holes are 0 and do not count towards the minimum), so utils.save_frames works on the result.
    A mesh without colours is drawn grey (128).  crop: True removes H // 20 rows and W // 20 columns from every side of each panel, or a pair."""
    H, W = int(hw[0]), int(hw[1])
    f = [float(v) for v in np.asarray(focal, dtype=np.float64).reshape(-1)]
    fx, fy = (f[0], f[0]) if len(f) == 1 else (f[0], f[1])
    K = torch.tensor([[fx, 0.0, W / 2], [0.0, fy, H / 2], [0.0, 0.0, 1.0]], dtype=torch.float64)
    if getattr(mesh, "colors", None) is None and hasattr(mesh, "vertices"):
        grey = TriangleMesh(mesh.vertices, getattr(mesh, "ndc", None), mesh.faces, getattr(mesh, "vertex_edge", None), getattr(mesh, "count", None),
                            torch.full((int(mesh.vertices.shape[0]), 3), 128, dtype=torch.uint8, device=mesh.vertices.device))
        mesh = grey
    crop = (H // 20, W // 20) if crop is True else ((0, 0) if not crop else (int(crop[0]), int(crop[1])))
    if crop[0] < 0 or crop[1] < 0 or 2 * crop[0] >= H or 2 * crop[1] >= W:
        raise ValueError(f"mesh_frames: crop {crop} leaves nothing of a {H} x {W} frame")
    img = render_mesh(mesh, None, cameras=(poses, K, (H, W)), **render_kw)
    n = int(img.depth.shape[0])
    with torch.cuda.device(img.depth.device):
        frames = torch.empty((n, H - 2 * crop[0], (W - 2 * crop[1]) * 2, 3), device=img.depth.device, dtype=torch.uint8)
        mm = ops.depth_range(img.depth)
        for k in range(n):
            ops.frame_u8(mesh_rgb(img.colors[k]), img.depth[k], minmax=mm, crop=crop, out=frames[k])
    return frames


def mesh_rgb(colors):
    """uint8 colours as the fp32 rgb ops.frame_u8 takes: (c + 0.5) / 255, which frame_u8's trunc(clamp(rgb, 0, 1) * 255) maps back to c for every byte."""
    return (colors.to(torch.float32) + 0.5) / 255.0


def _mesh_ply(path, mesh):
    nv = min(int(mesh.count[0].item()), int(mesh.vertices.shape[0]))
    nf = min(int(mesh.count[1].item()), int(mesh.faces.shape[0]))
    xyz = mesh.vertices[:nv].detach().cpu().numpy()
    rgb = np.full((nv, 3), 128, np.uint8) if mesh.colors is None else mesh.colors[:nv].detach().cpu().numpy()
    tri = mesh.faces[:nf].detach().cpu().numpy()
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape or rgb.dtype != np.uint8 or tri.ndim != 2 or tri.shape[1] != 3:
        raise ValueError(f"save_ply: vertices (V,3) float, colors (V,3) uint8 and faces (T,3) int, got {xyz.shape}, {rgb.shape} {rgb.dtype}, {tri.shape}")
    rec = np.empty(nv, dtype=PLY_VERTEX)
    for k, name in enumerate(("x", "y", "z")):
        rec[name] = xyz[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        rec[name] = rgb[:, k]
    frec = np.empty(nf, dtype=PLY_FACE)
    frec["n"], frec["v"] = 3, tri
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % nv
    header += "".join(f"property {'float' if PLY_VERTEX[name] == np.dtype('<f4') else 'uchar'} {name}\n" for name in PLY_VERTEX.names)
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % nf
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
        f.write(frec.tobytes())
    return nv, nf


def save_ply(path, cloud):
    """A binary little-endian PLY of the cloud's points and colours: x y z float, red green blue uchar, 15 bytes per vertex.  Host side (numpy), next to
    utils.save_frames; takes a PointCloud or a (points, colors) pair.  Of a PointCloud with a caller-given capacity the first min(count, capacity) rows are
    written.  Returns the number of vertices.
    A TriangleMesh: the same vertex records (colours (128,128,128) when mesh.colors is None), then `element face T` with `property list uchar int
    vertex_indices`, 13 bytes per face; the first min(count, rows) rows of each array are written.  Returns (V, T)."""
    if isinstance(cloud, TriangleMesh):
        return _mesh_ply(path, cloud)
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
PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", 3)])
