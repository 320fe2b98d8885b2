"""Python faces of the C-ABI entry points (include/mvsnerf_hip.h).  Tensors in, tensors out;
all arithmetic happens in libmvsnerf_hip.so.  No fallbacks."""
import collections
import ctypes
import weakref

import torch

from . import _lib
from ._lib import check, dev_f32, stream_ptr


def _need_no_grad(*tensors, op):
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError(
            f"{op}: this stand-alone op has no backward kernel (gradients are provided for the fused paths: "
            "renderer.rendering / RefVolume -> ops.RayMarchFunction, MVSNet.build_volume_costvar* and CostRegNet); "
            "call it under torch.no_grad() or go through those entry points")


# ------------------------------------------------------------------ volume layout
_cl_cache = {}
FUSED_GATHER = True      # ops.raymarch: one gather launch (False: the three stand-alone lookups; same bits)


class _Keep:
    """Pointer helper for one C-ABI call: makes a tensor contiguous fp32 if needed and keeps that (possibly temporary) tensor
    alive until the call has been issued - a temporary's block may otherwise be handed to the next temporary by the caching
    allocator before the kernel is even enqueued."""

    def __init__(self):
        self.alive = []

    def __call__(self, t, name):
        t = t.to(torch.float32).contiguous()
        self.alive.append(t)
        return dev_f32(t, name)


VOL_DHWC, VOL_HWDC = 0, 1      # MVSNERF_VOL_* of include/mvsnerf_hip.h


def vol_ptr_layout(vol_cl, cur=None):
    """(device pointer, MVSNERF_VOL_* layout) of a (D,H,W,C)-shaped volume view as channels_last_volume returns it: contiguous memory is
    vol[d][y][x][c]; a view whose (H,W,D,C) permutation is contiguous is the depth-fastest vol[y][x][d][c] the encoder emits."""
    if vol_cl.is_contiguous():
        return dev_f32(vol_cl, "volume", cur), VOL_DHWC
    m = vol_cl.permute(1, 2, 0, 3)
    if m.is_contiguous():
        return dev_f32(m, "volume", cur), VOL_HWDC
    raise RuntimeError("volume: expected vol[d][y][x][c] or vol[y][x][d][c] memory (ops.channels_last_volume makes one of them)")


def channels_last_volume(volume_feature):
    """(1,C,D,H,W) reference-layout volume -> (D,H,W,C)-shaped tensor the kernels read: a zero-copy VIEW when the memory already is
    channel-last in one of the two orders of include/mvsnerf_hip.h - vol[d][y][x][c] (RefVolume, channels_last_3d tensors) or the
    depth-fastest vol[y][x][d][c] our MVSNet emits; otherwise one HIP transpose to vol[d][y][x][c], cached on (storage, version)."""
    v = volume_feature
    hit = _cl_cache.get("last")          # the same tensor object, unmodified, as in the previous call (a render loop): ~0.3 us instead of ~6
    if hit is not None and hit[0]() is v and hit[1] == (v._version, _lib.weights_epoch()):
        return hit[2]
    out = _channels_last_volume(v)
    # a WEAK reference to the tensor object: an encoder output still carries its grad_fn, and a module-level strong reference would keep the whole
    # encoder graph (its saved activations, GB-scale at config 2/3) alive until the next call.  `out` (a no-grad view or a transposed copy) keeps
    # only the volume's own storage; RayMarchFunction.backward drops the entry.
    # The DETACHED view is what is cached AND returned (a miss used to return the view with its grad_fn, a hit the detached one - whether a stand-alone
    # op saw a gradient-requiring volume depended on the cache).  The differentiable paths take the volume tensor itself (RayMarchFunction), never this view.
    out = out.detach()
    _cl_cache["last"] = (weakref.ref(v), (v._version, _lib.weights_epoch()), out)
    return out


def _channels_last_volume(volume_feature):
    v = volume_feature
    if v.dim() == 5:
        if v.shape[0] != 1:
            raise RuntimeError("volume batch must be 1 (the reference assumes it too, models.py:916)")
        v = v[0]
    if v.dim() != 4:
        raise RuntimeError(f"volume must be (1,C,D,H,W) or (C,D,H,W), got {tuple(volume_feature.shape)}")
    cl = v.permute(1, 2, 3, 0)
    if cl.is_contiguous() or cl.permute(1, 2, 0, 3).is_contiguous():
        vol_ptr_layout(cl)
        return cl
    # cache key: storage identity + version.  The entry keeps the source storage alive, so the caching
    # allocator cannot hand the same address to a different tensor while the entry exists.
    st = v.untyped_storage()
    key = (st.data_ptr(), v.storage_offset(), v._version, _lib.weights_epoch(), tuple(v.shape), tuple(v.stride()))
    hit = _cl_cache.get("k")
    if hit is not None and hit[0] == key:
        return hit[2]
    src = v.detach().contiguous()
    C, D, H, W = src.shape
    dst = torch.empty((D, H, W, C), device=src.device, dtype=torch.float32)
    check(_lib.lib().mvsnerf_ncdhw_to_ndhwc(dev_f32(src, "volume"), dst.data_ptr(), C, D, H, W, stream_ptr()), "ncdhw_to_ndhwc")
    _cl_cache["k"] = (key, st, dst)
    return dst


def channels_last_images(imgs):
    """(V,3,H,W) un-normalised source images -> (V,H,W,4) copy (rgb + pad) for the fused gather; one HIP transpose per
    scene, cached on (storage, version) like the volume."""
    if imgs.dim() != 4 or imgs.shape[1] != 3:
        raise RuntimeError(f"imgs must be (V,3,H,W), got {tuple(imgs.shape)}")
    st = imgs.untyped_storage()
    key = (st.data_ptr(), imgs.storage_offset(), imgs._version, tuple(imgs.shape), tuple(imgs.stride()))
    hit = _cl_cache.get("imgs")
    if hit is not None and hit[0] == key:
        return hit[2]
    src = imgs.detach().contiguous()
    V, _, H, W = src.shape
    dst = torch.empty((V, H, W, 4), device=src.device, dtype=torch.float32)
    check(_lib.lib().mvsnerf_nchw_to_nhwc(dev_f32(src, "imgs"), dst.data_ptr(), V, 3, H, W, 4, stream_ptr()), "nchw_to_nhwc")
    _cl_cache["imgs"] = (key, st, dst)
    return dst


def _count_ptr(count, S, op):
    """count= of a counted launch after its refusals, made before the library is touched: the one-element int32 device tensor of
    ops.live_samples / live_samples_range, on rows with S == 1.  Returns its address."""
    if not (torch.is_tensor(count) and count.is_cuda and count.dtype == torch.int32 and count.numel() == 1):
        raise RuntimeError(f"{op}: count must be the one-element int32 device tensor of ops.live_samples")
    if S != 1:
        raise RuntimeError(f"{op}: count= takes the rows form only (S == 1: every row is its own ray), got S = {S}")
    return count.data_ptr()


def _gather_out(out, N, S, F, with_dirs, dev, op):
    """(feat (N,S,F), dirs (N,3) | None) of a gather: fresh, or the caller's pair `out` (what a counted launch leaves untouched stays visible)."""
    if out is None:
        return (torch.empty((N, S, F), device=dev, dtype=torch.float32), torch.empty((N, 3), device=dev, dtype=torch.float32) if with_dirs else None)
    feat, dirs = out
    if tuple(feat.shape) != (N, S, F) or (with_dirs and (dirs is None or tuple(dirs.shape) != (N, 3))):
        raise RuntimeError(f"{op}: out must be (feat ({N},{S},{F}), dirs ({N},3))")
    dev_f32(feat, f"{op}: out[0]")
    if with_dirs:
        dev_f32(dirs, f"{op}: out[1]")
    return feat, dirs if with_dirs else None


def gather(vol_cl, imgs, w2cs, intrinsics, rays_pts, rays_ndc, rays_dir=None, count=None, out=None):
    """Fused gen_pts_feats (+ gen_dir_feature when rays_dir is given): -> (input_feat (N,S,8+4V), dirs (N,3) | None).
    count: the (1,) int32 device tensor of ops.live_samples - the counted launch of DESIGN.md 4i on rows (S == 1): N is then the capacity, rows
    [0, min(max(count, 0), N)) get the bits of the call on that many rows and no other row is written.  out: a caller-owned (feat, dirs) pair."""
    _need_no_grad(vol_cl, imgs, rays_pts, rays_ndc, op="gather")
    N, S = rays_ndc.shape[:2]
    cptr = None if count is None else _count_ptr(count, S, "gather")
    V = imgs.shape[0]
    F = 8 + 4 * V
    D, H, W, C = vol_cl.shape
    if C != 8:
        raise RuntimeError("gather: the neural volume must have 8 channels")
    feat, dirs = _gather_out(out, N, S, F, rays_dir is not None, rays_ndc.device, "gather")
    icl = channels_last_images(imgs)
    vp, vl = vol_ptr_layout(vol_cl)
    head = (vp, D, H, W, icl.data_ptr(), V, imgs.shape[2], imgs.shape[3], dev_f32(w2cs, "w2cs"), dev_f32(intrinsics, "intrinsics"),
            dev_f32(rays_pts, "rays_pts"), dev_f32(rays_ndc, "rays_ndc"))
    tail = (0 if rays_dir is None else dev_f32(rays_dir, "rays_dir"), feat.data_ptr(), F, 0 if dirs is None else dirs.data_ptr(), vl, stream_ptr())
    if cptr is None:
        check(_lib.lib().mvsnerf_gather_fwd(*head, N, S, *tail), "gather_fwd")
    else:
        check(_lib.lib().mvsnerf_gather_fwd_counted(*head, N, cptr, *tail), "gather_fwd_counted")
    return feat, dirs


def gather_colorvol(vol_cl, rays_ndc, rays_dir=None, w2c_ref=None, force_offsets64=False, count=None, out=None):
    """gen_pts_feats of --use_color_volume (+ gen_dir_feature when rays_dir is given) in one launch: vol_cl (D,H,W,C) with C % 4 == 0,
    8 < C <= 40; rays_ndc (N,S,3) -> (input_feat (N,S,C), dirs (N,3) | None).  The bits of volume_sample / dir_feature(normalize=True).
    force_offsets64: run the kernel's 64-bit-offset form whatever the sizes (tests).  count / out: as ops.gather."""
    _need_no_grad(vol_cl, rays_ndc, rays_dir, op="gather_colorvol")
    if rays_ndc.dim() != 3 or rays_ndc.shape[-1] != 3:
        raise RuntimeError(f"gather_colorvol: rays_ndc must be (N,S,3), got {tuple(rays_ndc.shape)}")
    N, S = rays_ndc.shape[:2]
    cptr = None if count is None else _count_ptr(count, S, "gather_colorvol")
    D, H, W, C = vol_cl.shape
    if rays_dir is not None and tuple(rays_dir.shape) != (N, 3):
        raise RuntimeError(f"gather_colorvol: rays_dir must be ({N},3), got {tuple(rays_dir.shape)}")
    feat, dirs = _gather_out(out, N, S, C, rays_dir is not None, rays_ndc.device, "gather_colorvol")
    vp, vl = vol_ptr_layout(vol_cl)
    head = (vp, D, H, W, C, dev_f32(rays_ndc, "rays_ndc"))
    tail = (0 if rays_dir is None else dev_f32(rays_dir, "rays_dir"), 0 if w2c_ref is None else dev_f32(w2c_ref, "w2c_ref"), feat.data_ptr(), C,
            0 if dirs is None else dirs.data_ptr(), vl, int(bool(force_offsets64)), stream_ptr())
    if cptr is None:
        check(_lib.lib().mvsnerf_gather_colorvol_fwd(*head, N, S, *tail), "gather_colorvol_fwd")
    else:
        check(_lib.lib().mvsnerf_gather_colorvol_fwd_counted(*head, N, cptr, *tail), "gather_colorvol_fwd_counted")
    return feat, dirs


def ndhwc_to_ncdhw(vol_cl):
    """vol[d][y][x][c] memory -> a contiguous (C,D,H,W) tensor (boundary helper for callers that want the reference's layout)."""
    D, H, W, C = vol_cl.shape
    if not vol_cl.is_contiguous():
        raise RuntimeError("ndhwc_to_ncdhw: vol[d][y][x][c] memory expected (a depth-fastest volume converts with tensor.contiguous())")
    dst = torch.empty((C, D, H, W), device=vol_cl.device, dtype=torch.float32)
    check(_lib.lib().mvsnerf_ndhwc_to_ncdhw(dev_f32(vol_cl, "volume"), dst.data_ptr(), C, D, H, W, stream_ptr()), "ndhwc_to_ncdhw")
    return dst


# ------------------------------------------------------------------ gathers
def volume_sample(vol_cl, ndc, out=None, out_stride=None):
    """vol_cl (D,H,W,C) ; ndc (...,3) -> (..., C) (or written into `out` rows of stride out_stride)."""
    _need_no_grad(vol_cl, ndc, op="volume_sample")
    D, H, W, C = vol_cl.shape
    P = ndc.numel() // 3
    if out is None:
        out = torch.empty((*ndc.shape[:-1], C), device=ndc.device, dtype=torch.float32)
        out_stride = C
    vp, vl = vol_ptr_layout(vol_cl)
    check(_lib.lib().mvsnerf_volume_sample_fwd(vp, D, H, W, C, dev_f32(ndc, "ndc"), P,
                                               out.data_ptr(), out_stride, vl, stream_ptr()), "volume_sample_fwd")
    return out


def color_sample(imgs, w2cs, intrinsics, pts, with_mask=True, out=None, out_ptr=None, out_stride=None):
    """imgs (V,3,H,W) ; w2cs (V,4,4) ; intrinsics (V,3,3) ; pts (...,3) -> (..., V*(3+mask))."""
    _need_no_grad(imgs, pts, op="color_sample")
    V, _, H, W = imgs.shape
    Cv = 3 + int(bool(with_mask))
    P = pts.numel() // 3
    if out is None:
        out = torch.empty((*pts.shape[:-1], V * Cv), device=pts.device, dtype=torch.float32)
        out_ptr, out_stride = out.data_ptr(), V * Cv
    check(_lib.lib().mvsnerf_color_sample_fwd(dev_f32(imgs, "imgs"), V, H, W, dev_f32(w2cs, "w2cs"), dev_f32(intrinsics, "intrinsics"),
                                              dev_f32(pts, "pts"), P, int(bool(with_mask)), out_ptr, out_stride, stream_ptr()),
          "color_sample_fwd")
    return out


def color_feat_sample(imgs, img_feat, w2cs, intrinsics, pts, with_mask=True, out=None, out_ptr=None, out_stride=None):
    """build_color_volume's img_feat branch: imgs (V,3,H,W), img_feat (V,Cf,Hf,Wf) -> (..., V*(3+Cf+mask))."""
    _need_no_grad(imgs, img_feat, pts, op="color_feat_sample")
    V, _, H, W = imgs.shape
    if img_feat.dim() != 4 or img_feat.shape[0] != V:
        raise RuntimeError(f"img_feat must be (V={V},Cf,Hf,Wf), got {tuple(img_feat.shape)}")
    Cf, Hf, Wf = img_feat.shape[1:]
    Cv = 3 + Cf + int(bool(with_mask))
    P = pts.numel() // 3
    if out is None:
        out = torch.empty((*pts.shape[:-1], V * Cv), device=pts.device, dtype=torch.float32)
        out_ptr, out_stride = out.data_ptr(), V * Cv
    check(_lib.lib().mvsnerf_color_feat_sample_fwd(dev_f32(imgs, "imgs"), V, H, W, dev_f32(img_feat, "img_feat"), Cf, Hf, Wf,
                                                   dev_f32(w2cs, "w2cs"), dev_f32(intrinsics, "intrinsics"), dev_f32(pts, "pts"), P,
                                                   int(bool(with_mask)), out_ptr, out_stride, stream_ptr()), "color_feat_sample_fwd")
    return out


def dir_feature(rays_dir, w2c_ref=None, normalize=True):
    _need_no_grad(rays_dir, op="dir_feature")
    out = torch.empty_like(rays_dir)
    check(_lib.lib().mvsnerf_dir_feature_fwd(dev_f32(rays_dir, "rays_dir"), 0 if w2c_ref is None else dev_f32(w2c_ref, "w2c_ref"),
                                             rays_dir.shape[0], int(bool(normalize)), out.data_ptr(), stream_ptr()), "dir_feature_fwd")
    return out


def posenc(x, num_freqs):
    """Embedder.embed (models.py:47-51) as a stand-alone op: (...,d) -> (..., d*(1+2L))."""
    _need_no_grad(x, op="posenc")
    d = x.shape[-1]
    out = torch.empty((*x.shape[:-1], d * (1 + 2 * num_freqs)), device=x.device, dtype=torch.float32)
    check(_lib.lib().mvsnerf_posenc_fwd(dev_f32(x, "x"), x.numel() // d, d, num_freqs, out.data_ptr(), stream_ptr()), "posenc_fwd")
    return out


def raygen(H, W, K_tgt, c2w_tgt, K_ref, w2c_ref, nf_tgt, nf_ref, N_samples, pad=0, lindisp=False,
           xs=None, ys=None, first_pixel=0, n_rays=None, t_rand=None, ref_hw=None):
    """Ray generation kernel (utils.build_rays / build_rays_test downstream of the RNG draws).
    Either xs/ys (float pixel ids, (N,)) or first_pixel + n_rays (row-major ids).  All camera tensors stay on the device.
    Returns rays_pts (N,S,3), rays_dir (N,3), rays_ndc (N,S,3), z_vals (N,S), pix (2,N)."""
    dev = c2w_tgt.device
    N = int(xs.shape[0]) if xs is not None else int(n_rays)
    f32 = dict(device=dev, dtype=torch.float32)
    pts = torch.empty((N, N_samples, 3), **f32)
    ndc = torch.empty((N, N_samples, 3), **f32)
    dirs = torch.empty((N, 3), **f32)
    z = torch.empty((N, N_samples), **f32)
    pix = torch.empty((2, N), **f32)
    c = _Keep()
    check(_lib.lib().mvsnerf_raygen_fwd(0 if xs is None else c(xs, "xs"), 0 if ys is None else c(ys, "ys"), int(first_pixel), W, H,
                                        0 if ref_hw is None else int(ref_hw[1]), 0 if ref_hw is None else int(ref_hw[0]),
                                        c(K_tgt, "K_tgt"), c(c2w_tgt, "c2w_tgt"), c(K_ref, "K_ref"), c(w2c_ref, "w2c_ref"),
                                        c(nf_tgt, "near_far_tgt"), c(nf_ref, "near_far_ref"), int(pad), int(bool(lindisp)),
                                        0 if t_rand is None else c(t_rand, "t_rand"), N, N_samples,
                                        pts.data_ptr(), dirs.data_ptr(), ndc.data_ptr(), z.data_ptr(), pix.data_ptr(), stream_ptr()), "raygen_fwd")
    return pts, dirs, ndc, z, pix


def raygen_train(H, W, K_tgt, c2w_tgt, K_ref, w2c_ref, nf_tgt, nf_ref, N_samples, xs, ys, t_rand, tgt_img, depth_map=None, z_map=None,
                 depth_mode=0, pad=0, lindisp=False):
    """build_rays of a training step in one launch (mvsnerf_raygen_train_fwd): ray generation + target-colour gather (+ ground-truth depth
    gather, + the per-pixel depth ranges of importanceSampling (depth_mode 1) / with_depth (depth_mode 2, one candidate per ray)).
    Returns rays_pts (N,S,3), rays_dir (N,3), rays_ndc (N,S,3), z_vals (N,S), pix (2,N), colors (N,3), rays_depth (N,) | None."""
    dev = c2w_tgt.device
    N = int(xs.shape[0])
    S = 1 if depth_mode == 2 else int(N_samples)
    f32 = dict(device=dev, dtype=torch.float32)
    pts, ndc, dirs = torch.empty((N, S, 3), **f32), torch.empty((N, S, 3), **f32), torch.empty((N, 3), **f32)
    z, pix, colors = torch.empty((N, S), **f32), torch.empty((2, N), **f32), torch.empty((N, 3), **f32)
    rd = None if depth_map is None else torch.empty((N,), **f32)
    c = _Keep()
    if tuple(tgt_img.shape) != (3, H, W) or (depth_map is not None and tuple(depth_map.shape) != (H, W)) or (z_map is not None and tuple(z_map.shape) != (H, W)):
        raise RuntimeError("raygen_train: tgt_img must be (3,H,W), depth_map / z_map (H,W)")
    check(_lib.lib().mvsnerf_raygen_train_fwd(c(xs, "xs"), c(ys, "ys"), W, H, 0, 0, c(K_tgt, "K_tgt"), c(c2w_tgt, "c2w_tgt"), c(K_ref, "K_ref"),
                                              c(w2c_ref, "w2c_ref"), c(nf_tgt, "near_far_tgt"), c(nf_ref, "near_far_ref"), int(pad), int(bool(lindisp)),
                                              0 if t_rand is None else c(t_rand, "t_rand"), N, S, c(tgt_img, "tgt_img"),
                                              0 if depth_map is None else c(depth_map, "depth_map"), 0 if z_map is None else c(z_map, "z_map"),
                                              int(depth_mode), pts.data_ptr(), dirs.data_ptr(), ndc.data_ptr(), z.data_ptr(), pix.data_ptr(),
                                              colors.data_ptr(), 0 if rd is None else rd.data_ptr(), stream_ptr()), "raygen_train_fwd")
    return pts, dirs, ndc, z, pix, colors, rd


def ray_points(rays_o, rays_d, z_vals, w2c_ref=None, K_ref=None, near_far_ref=None, ref_hw=None, pad=0, lindisp=False):
    """pts = o + d*z (N,S,3) and, when the reference camera is given, their NDC coordinates (get_ndc_coordinate)."""
    _need_no_grad(rays_o, rays_d, z_vals, op="ray_points")
    N, S = z_vals.shape
    dev = z_vals.device
    c = _Keep()
    per_ray = int(rays_o.dim() == 2 and rays_o.shape[0] == N and N > 1)
    pts = torch.empty((N, S, 3), device=dev, dtype=torch.float32)
    ndc = None if w2c_ref is None else torch.empty((N, S, 3), device=dev, dtype=torch.float32)
    check(_lib.lib().mvsnerf_ray_points_fwd(c(rays_o.reshape(-1, 3), "rays_o"), per_ray, c(rays_d, "rays_d"), c(z_vals, "z_vals"),
                                            0 if ndc is None else c(w2c_ref, "w2c_ref"), 0 if ndc is None else c(K_ref, "K_ref"),
                                            0 if ndc is None else c(near_far_ref.reshape(-1)[:2], "near_far_ref"),
                                            0 if ndc is None else int(ref_hw[1]), 0 if ndc is None else int(ref_hw[0]), int(pad), int(bool(lindisp)),
                                            N, S, pts.data_ptr(), 0 if ndc is None else ndc.data_ptr(), stream_ptr()), "ray_points_fwd")
    return pts, ndc


def ray_march_bbox(rays, bbox_3d, N_samples, lindisp=False, perturb=0.0, jitter=None, t=None):
    """ray_marcher(rays, N_samples, lindisp, perturb, bbox_3D) (data/ray_utils.py:143-197) and the box coordinates of the fusion script
    (train_mvs_nerf_fusion_finetuning_pl.py:263) in one launch: rays (N,8), bbox_3d (2,3) -> (pts (N,S,3), ndc (N,S,3), z (N,S)).
    jitter: the (N,S) uniform draw of :190, required when perturb > 0; t: linspace(0, 1, N_samples) when the caller keeps one."""
    _need_no_grad(rays, bbox_3d, op="ray_march_bbox")
    if rays.dim() != 2 or rays.shape[1] != 8 or tuple(bbox_3d.shape) != (2, 3):
        raise RuntimeError(f"ray_march_bbox: rays (N,8) and bbox_3d (2,3), got {tuple(rays.shape)} and {tuple(bbox_3d.shape)}")
    N, S = rays.shape[0], int(N_samples)
    dev = rays.device
    if perturb > 0 and (jitter is None or tuple(jitter.shape) != (N, S)):
        raise RuntimeError(f"ray_march_bbox: perturb > 0 needs the ({N}, {S}) uniform draw as jitter=")
    if t is None:
        t = torch.linspace(0, 1, S, device=dev)
    if t.numel() != S:
        raise RuntimeError(f"ray_march_bbox: t must hold {S} values")
    c = _Keep()
    z = torch.empty((N, S), device=dev, dtype=torch.float32)
    pts, ndc = torch.empty((N, S, 3), device=dev, dtype=torch.float32), torch.empty((N, S, 3), device=dev, dtype=torch.float32)
    check(_lib.lib().mvsnerf_ray_march_bbox_fwd(c(rays, "rays"), c(bbox_3d, "bbox_3d"), c(t, "t"), c(jitter, "jitter") if perturb > 0 else 0,
                                                float(perturb), int(bool(lindisp)), N, S, z.data_ptr(), pts.data_ptr(), ndc.data_ptr(),
                                                stream_ptr()), "ray_march_bbox_fwd")
    return pts, ndc, z


def _bank_images(images, op):
    """(M, H, W) of an image bank (SceneRays.images): a contiguous (M,H,W,4) uint8 tensor on the current device."""
    if not (torch.is_tensor(images) and images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4 and images.shape[-1] == 4
            and images.is_contiguous()):
        raise RuntimeError(f"{op}: images must be a contiguous (M,H,W,4) uint8 tensor on the GPU (SceneRays.images), got "
                           f"{tuple(getattr(images, 'shape', ()))} {getattr(images, 'dtype', None)} {getattr(images, 'device', None)}")
    if images.device.index != torch.cuda.current_device():
        raise RuntimeError(f"{op}: the bank is on {images.device} but the current device is cuda:{torch.cuda.current_device()}")
    return tuple(int(v) for v in images.shape[:3])


def _scene_bank(images, c2ws, intrinsics, near_far, depths, idx, op):
    """The bank and index pointers of the scene_rays entries (mvsnerf_amd.rays.SceneRays holds the tensors in this form): images (M,H,W,4) uint8,
    c2ws (M,3,4), intrinsics (M,3,3), near_far (M,2) fp32, depths (M,H,W) fp32 | None, idx (B,) int64; all contiguous on the current device."""
    M, H, W = _bank_images(images, op)
    if tuple(c2ws.shape) != (M, 3, 4) or tuple(intrinsics.shape) != (M, 3, 3) or tuple(near_far.shape) != (M, 2):
        raise RuntimeError(f"{op}: c2ws ({M},3,4), intrinsics ({M},3,3) and near_far ({M},2) expected, got {tuple(c2ws.shape)}, "
                           f"{tuple(intrinsics.shape)}, {tuple(near_far.shape)}")
    if depths is not None and tuple(depths.shape) != (M, H, W):
        raise RuntimeError(f"{op}: depths must be ({M},{H},{W}), got {tuple(depths.shape)}")
    if idx.dim() != 1 or idx.dtype != torch.int64 or idx.device != images.device or not idx.is_contiguous():
        raise RuntimeError(f"{op}: idx must be a contiguous (B,) int64 tensor on {images.device}, got {tuple(idx.shape)} {idx.dtype} {idx.device}")
    return M, H, W


def scene_rays_gather(images, c2ws, intrinsics, near_far, depths, idx, want_depth=False, want_mask=False):
    """all_rays[idx], all_rgbs[idx] of the all-rays buffer the reference's datasets build (data/dtu_ft.py:143-188, data/blender.py:49-85), formed from the
    8-bit images and the cameras in one launch: -> (rays (B,8), rgbs (B,3), depth (B,) | None, mask (B,) bool | None).  idx: flat int64 indices into M*H*W,
    view-major then row-major; an index outside the bank gives zero rows."""
    _need_no_grad(c2ws, intrinsics, near_far, op="scene_rays_gather")
    M, H, W = _scene_bank(images, c2ws, intrinsics, near_far, depths, idx, "scene_rays_gather")
    if want_depth and depths is None:
        raise RuntimeError("scene_rays_gather: want_depth needs a bank with depths")
    B, dev = int(idx.shape[0]), images.device
    c = _Keep()
    rays, rgb = torch.empty((B, 8), device=dev, dtype=torch.float32), torch.empty((B, 3), device=dev, dtype=torch.float32)
    depth = torch.empty((B,), device=dev, dtype=torch.float32) if want_depth else None
    mask = torch.empty((B,), device=dev, dtype=torch.uint8) if want_mask else None
    if B == 0:                                       # (an empty tensor has no address to hand over)
        return rays, rgb, depth, None if mask is None else mask.view(torch.bool)
    check(_lib.lib().mvsnerf_scene_rays_gather_fwd(images.data_ptr(), c(c2ws, "c2ws"), c(intrinsics, "intrinsics"), c(near_far, "near_far"),
                                                   0 if depths is None else c(depths, "depths"), M, H, W, idx.data_ptr(), B, rays.data_ptr(), rgb.data_ptr(),
                                                   0 if depth is None else depth.data_ptr(), 0 if mask is None else mask.data_ptr(), stream_ptr()),
          "scene_rays_gather_fwd")
    return rays, rgb, depth, None if mask is None else mask.view(torch.bool)


def scene_rays_march(images, c2ws, intrinsics, near_far, idx, N_samples, t=None, jitter=None, perturb=0.0, lindisp=False, ref=None):
    """The front end of a fine-tuning step in one launch: the rows of scene_rays_gather, ray_marcher's depths (data/ray_utils.py:152-197), o + d*z and,
    with ref = (w2c_ref, K_ref, near_far_ref, (H_ref, W_ref), pad), get_ndc_coordinate -> (rays (B,8), rgbs (B,3), z (B,S), pts (B,S,3), ndc (B,S,3) | None).
    jitter: the (B,S) uniform draw of :190, required when perturb > 0; t: linspace(0, 1, N_samples) when the caller keeps one."""
    _need_no_grad(c2ws, intrinsics, near_far, op="scene_rays_march")
    M, H, W = _scene_bank(images, c2ws, intrinsics, near_far, None, idx, "scene_rays_march")
    B, S, dev = int(idx.shape[0]), int(N_samples), images.device
    if perturb > 0 and (jitter is None or tuple(jitter.shape) != (B, S)):
        raise RuntimeError(f"scene_rays_march: perturb > 0 needs the ({B}, {S}) uniform draw as jitter=")
    if t is None:
        t = torch.linspace(0, 1, S, device=dev)
    if t.numel() != S:
        raise RuntimeError(f"scene_rays_march: t must hold {S} values")
    c = _Keep()
    f32 = dict(device=dev, dtype=torch.float32)
    rays, rgb, z = torch.empty((B, 8), **f32), torch.empty((B, 3), **f32), torch.empty((B, S), **f32)
    pts = torch.empty((B, S, 3), **f32)
    ndc = None if ref is None else torch.empty((B, S, 3), **f32)
    if B == 0:                                       # (an empty tensor has no address to hand over)
        return rays, rgb, z, pts, ndc
    if ref is None:
        cam = (0, 0, 0, 0, 0, 0)
    else:
        w2c_ref, K_ref, nf_ref, ref_hw, pad = ref
        cam = (c(w2c_ref, "w2c_ref"), c(K_ref, "K_ref"), c(nf_ref.reshape(-1)[:2], "near_far_ref"), int(ref_hw[1]), int(ref_hw[0]), int(pad))
    check(_lib.lib().mvsnerf_scene_rays_march_fwd(images.data_ptr(), c(c2ws, "c2ws"), c(intrinsics, "intrinsics"), c(near_far, "near_far"), M, H, W,
                                                  idx.data_ptr(), B, c(t, "t"), S, c(jitter, "jitter") if perturb > 0 else 0, float(perturb),
                                                  int(bool(lindisp)), *cam, rays.data_ptr(), rgb.data_ptr(), z.data_ptr(), pts.data_ptr(),
                                                  0 if ndc is None else ndc.data_ptr(), stream_ptr()), "scene_rays_march_fwd")
    return rays, rgb, z, pts, ndc


def source_images(images, ids, mean, std):
    """The `imgs` of read_source_views (data/dtu_ft.py:72-119) from the bank in one launch: images (M,H,W,4) uint8, ids (V,) int64 on the bank's device ->
    (V,3,H,W) fp32 = T.Normalize(mean, std)(ToTensor, blended onto white); an id outside [0, M) gives zeros."""
    M, H, W = _bank_images(images, "source_images")
    if ids.dim() != 1 or ids.dtype != torch.int64 or ids.device != images.device or not ids.is_contiguous() or ids.shape[0] < 1:
        raise RuntimeError(f"source_images: ids must be a contiguous (V,) int64 tensor on {images.device}, V >= 1, got {tuple(ids.shape)} {ids.dtype} {ids.device}")
    V = int(ids.shape[0])
    f3 = ctypes.c_float * 3
    out = torch.empty((V, 3, H, W), device=images.device, dtype=torch.float32)
    check(_lib.lib().mvsnerf_source_images_fwd(images.data_ptr(), ids.data_ptr(), V, M, H, W, f3(*[float(v) for v in mean]), f3(*[float(v) for v in std]),
                                               out.data_ptr(), stream_ptr()), "source_images_fwd")
    return out


RESAMPLE_SUPPORT = {"lanczos": 3.0, "bilinear": 1.0}
_resample_cache = {}


def _resample_filter(name, x):
    import math
    if name == "lanczos":                              # Pillow's lanczos_filter: a truncated sinc, sinc(x) sinc(x / 3) on [-3, 3)
        if -3.0 <= x < 3.0:
            a, b = x * math.pi, x / 3 * math.pi
            return (1.0 if a == 0.0 else math.sin(a) / a) * (1.0 if b == 0.0 else math.sin(b) / b)
        return 0.0
    x = abs(x)                                         # bilinear_filter
    return 1.0 - x if x < 1.0 else 0.0


def _resample_tables(n_in, n_out, resample):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c) for one axis, in float64 on the host:
    -> (win (n_out,2) int32 = (xmin, n), kk (n_out,ksize) int32, ksize) as numpy arrays; cached per (n_in, n_out, resample)."""
    key = (int(n_in), int(n_out), resample)
    if key in _resample_cache:
        return _resample_cache[key]
    import math
    import numpy as np
    n_in, n_out = key[:2]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = RESAMPLE_SUPPORT[resample] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    win, kk = np.zeros((n_out, 2), dtype=np.int32), np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [_resample_filter(resample, (x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:                                    # left to right, as Pillow sums
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        win[xx] = xmin, n
        kk[xx, :n] = [int(v * 4194304.0 - 0.5) if v < 0 else int(v * 4194304.0 + 0.5) for v in w]       # 2^22, truncation towards zero
    if len(_resample_cache) >= 64:
        _resample_cache.clear()
    _resample_cache[key] = (win, kk, ksize)
    return _resample_cache[key]


_resample_dev_cache = {}


def _resample_tables_dev(n_in, n_out, resample, device):
    """The tables of _resample_tables as int32 device tensors, cached per (n_in, n_out, resample, device): the pattern of _mlp_bwd_maps."""
    key = (int(n_in), int(n_out), resample, str(device))
    if key not in _resample_dev_cache:
        win, kk, ksize = _resample_tables(n_in, n_out, resample)
        if len(_resample_dev_cache) >= 64:
            _resample_dev_cache.clear()
        _resample_dev_cache[key] = (torch.from_numpy(win).to(device), torch.from_numpy(kk).to(device), ksize)
    return _resample_dev_cache[key]


def resample_u8(src, size_hw, resample="lanczos", premultiply=False, out=None):
    """`Image.resize((W', H'), LANCZOS | BILINEAR)` of Pillow on 8-bit images in the bank's layout, byte for byte (csrc/resample.hip):
    src (M,H,W,4) uint8 on the GPU -> (M,H',W',4).  premultiply=False: an RGB image; three channels are resampled and the alpha byte of the result is 255.
    premultiply=True: an image with alpha; resampled premultiplied and divided by the new alpha again, as Pillow resizes mode RGBA.  out: a contiguous
    (M,H',W',4) uint8 tensor to write into (a view's slot of a bank)."""
    if resample not in RESAMPLE_SUPPORT:
        raise ValueError(f"resample_u8: resample must be one of {sorted(RESAMPLE_SUPPORT)}, got {resample!r}")
    if not torch.is_tensor(src) or src.dim() != 4 or src.shape[-1] != 4 or src.dtype != torch.uint8 or not src.is_cuda or not src.is_contiguous():
        raise RuntimeError(f"resample_u8: src must be a contiguous (M,H,W,4) uint8 tensor on the GPU, got {tuple(getattr(src, 'shape', ()))} "
                           f"{getattr(src, 'dtype', None)} {getattr(src, 'device', None)}")
    M, H, W = (int(v) for v in src.shape[:3])
    Ho, Wo = (int(v) for v in size_hw)
    if min(M, H, W) < 1 or min(Ho, Wo) < 1:
        raise ValueError(f"resample_u8: empty images or target, {tuple(src.shape)} -> {(Ho, Wo)}")
    if src.device.index != torch.cuda.current_device():
        raise RuntimeError(f"resample_u8: src is on {src.device} but the current device is cuda:{torch.cuda.current_device()}")
    if out is None:
        out = torch.empty((M, Ho, Wo, 4), device=src.device, dtype=torch.uint8)
    elif tuple(out.shape) != (M, Ho, Wo, 4) or out.dtype != torch.uint8 or out.device != src.device or not out.is_contiguous():
        raise RuntimeError(f"resample_u8: out must be a contiguous ({M},{Ho},{Wo},4) uint8 tensor on {src.device}, got {tuple(out.shape)} {out.dtype} {out.device}")
    xw, xk, xks = _resample_tables_dev(W, Wo, resample, src.device) if Wo != W else (None, None, 0)
    yw, yk, yks = _resample_tables_dev(H, Ho, resample, src.device) if Ho != H else (None, None, 0)
    lib = _lib.lib()
    nbytes = lib.mvsnerf_resample_u8_workspace_bytes(M, H, W, Ho, Wo)
    work = torch.empty((nbytes,), device=src.device, dtype=torch.uint8) if nbytes else None
    p = lambda t: 0 if t is None else t.data_ptr()
    check(lib.mvsnerf_resample_u8_fwd(src.data_ptr(), M, H, W, out.data_ptr(), Ho, Wo, p(xw), p(xk), xks, p(yw), p(yk), yks, int(bool(premultiply)),
                                      p(work), stream_ptr()), "resample_u8_fwd")
    return out


def sample_pdf(bins, weights, u):
    """data/ray_utils.py:96-139 with the uniform draws supplied: bins (N,nb), weights (N,nb-1), u (N,NI) -> (N,NI)."""
    _need_no_grad(bins, weights, u, op="sample_pdf")
    N, nb = bins.shape
    out = torch.empty(tuple(u.shape), device=u.device, dtype=torch.float32)
    c = _Keep()
    check(_lib.lib().mvsnerf_sample_pdf_fwd(c(bins, "bins"), c(weights, "weights"), c(u, "u"),
                                            N, nb, u.shape[1], out.data_ptr(), stream_ptr()), "sample_pdf_fwd")
    return out


def ray_marcher_fine_z(density_volume, rays_ndc, z_vals, u):
    """data/ray_utils.py:207-219: density (D,H,W), ndc (N,S,3), z (N,S), u (N,NI) -> sorted depths (N,S+NI)."""
    _need_no_grad(density_volume, rays_ndc, z_vals, u, op="ray_marcher_fine")
    N, S = z_vals.shape
    D, H, W = density_volume.shape
    out = torch.empty((N, S + u.shape[1]), device=z_vals.device, dtype=torch.float32)
    c = _Keep()
    check(_lib.lib().mvsnerf_ray_marcher_fine_fwd(c(density_volume, "density_volume"), D, H, W, c(rays_ndc, "rays_ndc"),
                                                  c(z_vals, "z_vals"), c(u, "u"), N, S, u.shape[1],
                                                  out.data_ptr(), stream_ptr()), "ray_marcher_fine_fwd")
    return out


# ------------------------------------------------------------------ MLP
MLP_ORDER = [f"pts_linears.{i}" for i in range(6)] + ["pts_bias", "feature_linear", "alpha_linear", "views_linears.0", "rgb_linear"]
_Ptr11 = ctypes.c_void_p * 11       # the C entries' `const float* const w[11]`: one pointer per linear, in MLP_ORDER


def mlp_pack(weights, biases, F, variant=0):
    """weights/biases: 11 contiguous fp32 GPU tensors in MLP_ORDER -> packed fragment-ordered buffer: the standard layout plus the fold tail
    (feature_linear folded into views_linears.0 for the fp32 no-grad kernels; include/mvsnerf_hip_internal.h).
    variant: 0 = Renderer_ours (h = relu(p * bias)), 1 = Renderer_linear (h = relu(p + bias), un-clamped sigma-only output); the buffer carries
    it and every fp32 kernel handed the buffer follows it - the 16-bit kernels do not (models.Renderer_linear keeps v2 off them)."""
    if variant not in (0, 1):
        raise ValueError(f"mlp_pack: variant must be 0 (Renderer_ours) or 1 (Renderer_linear), got {variant!r}")
    n = _lib.lib().mvsnerf_mlp_packed_fold_floats(F)
    if n == 0:
        raise RuntimeError(f"mlp_pack: feat_dim {F} unsupported (must be even, <= 40)")
    expect = [(128, 63)] + [(128, 128)] * 4 + [(128, 191), (128, F), (128, 128), (1, 128), (64, 131), (3, 64)]
    for name, w, e in zip(MLP_ORDER, weights, expect):
        if tuple(w.shape) != e:
            raise RuntimeError(f"mlp_pack: {name}.weight has shape {tuple(w.shape)}, kernel is specialised for {e} "
                               "(netdepth 6, netwidth 128, skips [4], multires 10, raw 3-d view dirs)")
    packed = torch.empty(n, device=weights[0].device, dtype=torch.float32)
    wp = _Ptr11(*[dev_f32(w, "weight") for w in weights])
    bp = _Ptr11(*[dev_f32(b, "bias") for b in biases])
    if variant:
        check(_lib.lib().mvsnerf_mlp_pack_fold_variant(wp, bp, F, int(variant), packed.data_ptr(), stream_ptr()), "mlp_pack")
    else:
        check(_lib.lib().mvsnerf_mlp_pack_fold(wp, bp, F, packed.data_ptr(), stream_ptr()), "mlp_pack")
    return packed


WIDE_WIDTH = 256            # the one width of csrc/mlp_wide.hip


class WidePacked:
    """The packed weights of a netwidth-256 network (mlp_pack_wide): the buffer of csrc/mlp_wide_layout.h with the width, feat_dim and variant it
    was packed for.  Deliberately not a tensor: only ops.mlp_forward takes it; every other entry that takes a packed MLP buffer hands its
    pointer to a 128-wide kernel, which would read the buffer with its own offsets, and refuses it instead (_need_narrow)."""
    __slots__ = ("buffer", "width", "F", "variant")

    def __init__(self, buffer, width, F, variant):
        self.buffer, self.width, self.F, self.variant = buffer, int(width), int(F), int(variant)

    @property
    def device(self):
        return self.buffer.device

    def __repr__(self):
        return f"WidePacked(width={self.width}, F={self.F}, variant={self.variant}, device={self.buffer.device})"


def _wide_refusal(op):
    return NotImplementedError(
        f"{op}: netwidth {WIDE_WIDTH} runs on the no-grad fp32 network query only (ops.mlp_forward: MVSNeRF.query / forward / forward_alpha, "
        "renderer.rendering's piecewise path); the fused ray march, the whole-frame entries, training and the 16-bit kernels are built for "
        "netwidth 128")


def _need_narrow(packed, op):
    """Refuse a netwidth-256 buffer - or the 11 weights of such a network - before anything is launched."""
    if isinstance(packed, WidePacked):
        raise _wide_refusal(op)
    if isinstance(packed, (list, tuple)) and len(packed) and torch.is_tensor(packed[0]) and packed[0].shape[0] != 128:
        raise _wide_refusal(op)


def mlp_pack_wide(weights, biases, F, width=WIDE_WIDTH, variant=0):
    """mlp_pack for a netwidth-256 network (mvsnerf_mlp_pack_wide): 11 contiguous fp32 GPU tensors each in MLP_ORDER -> WidePacked."""
    if variant not in (0, 1):
        raise ValueError(f"mlp_pack_wide: variant must be 0 (Renderer_ours) or 1 (Renderer_linear), got {variant!r}")
    W = int(width)
    if W != WIDE_WIDTH:
        raise NotImplementedError(f"mlp_pack_wide: netwidth {W}: the wide kernel is built for netwidth {WIDE_WIDTH} (and mlp_pack for 128)")
    expect = [(W, 63)] + [(W, W)] * 4 + [(W, W + 63), (W, F), (W, W), (1, W), (W // 2, W + 3), (3, W // 2)]
    if len(weights) != 11 or len(biases) != 11:
        raise RuntimeError("mlp_pack_wide: 11 weights and 11 biases in ops.MLP_ORDER")
    for name, w, b, e in zip(MLP_ORDER, weights, biases, expect):
        if tuple(w.shape) != e or tuple(b.shape) != (e[0],):
            raise RuntimeError(f"mlp_pack_wide: {name} has weight {tuple(w.shape)}, bias {tuple(b.shape)}; netwidth {W} needs {e}, {(e[0],)} "
                               "(netdepth 6, skips [4], multires 10, raw 3-d view dirs)")
    n = _lib.lib().mvsnerf_mlp_wide_packed_floats(F, W)
    if n == 0:
        raise RuntimeError(f"mlp_pack_wide: feat_dim {F} unsupported (must be even, 4 <= F <= 40)")
    packed = torch.empty(n, device=weights[0].device, dtype=torch.float32)
    wp = _Ptr11(*[dev_f32(w, "weight") for w in weights])
    bp = _Ptr11(*[dev_f32(b, "bias") for b in biases])
    check(_lib.lib().mvsnerf_mlp_pack_wide(wp, bp, F, W, int(variant), packed.data_ptr(), stream_ptr()), "mlp_pack_wide")
    return WidePacked(packed, W, F, variant)


MLP_PRECISION = "auto"      # "auto" (default) | "fp32" | "bf16" | "bf16x3" | "bf16x6" | "fp16x3"; see set_mlp_precision
N_SPLIT = {"bf16x3": 2, "bf16x6": 3, "fp16x3": 18}      # n_split of mvsnerf_mlp_*_split; 18 = MVSNERF_SPLIT_FP16 (include/mvsnerf_hip.h)
_MODES = ("auto", "fp32", "bf16", "bf16x3", "bf16x6", "fp16x3")


def set_mlp_precision(mode):
    """Select the matrix-core arithmetic of the MLP:
      "auto"    (default) a step that needs gradients runs "fp32"; a no-grad rendering / network query runs the GUARDED fp16x3 sequence:
                the two-piece fp16 kernel (fp32-grade results, 2.5x the fp32-MFMA rate; operands and weights carry exact power-of-two
                scales, so fp16's exponent range is not a limit) reports what it cannot represent - a non-finite weight or value -
                through a device-side guard word, and the fp32-MFMA kernel enqueued right behind it - predicated on that word -
                recomputes the batch when it is set.  No host synchronisation (include/mvsnerf_hip.h, "guarded 16-bit sequences");
                ops.guard_fallbacks() tells how often the fp32 kernel had to step in.
      "fp32"    v_mfma_f32_32x32x2_f32 everywhere (the arithmetic of bench.py's headline and of the parity tests that pin the fp32 kernel)
      "bf16"    v_mfma_f32_32x32x16_bf16, operands rounded to bf16 (BASELINE configs 3/4; ~1e-2 errors); in training this is the
                reference's AMP switch (train_mvs_nerf_pl.py:317-318): forward, data- and weight-gradient GEMMs on bf16 operands
                with fp32 accumulation, fp32 master weights and fp32 gradients
      (the split modes below are inference-only)
      "bf16x6"  split-bf16 fp32 emulation: operands as 3 bf16 pieces, 6 bf16 MFMAs per product (fp32-grade results, fp32's range)
      "bf16x3"  2 bf16 pieces, 3 MFMAs (~1e-5 relative)
      "fp16x3"  the UNGUARDED two-piece fp16 kernel alone (csrc/mlp_f16x3.hip)"""
    global MLP_PRECISION
    if mode not in _MODES:
        raise ValueError(f"mlp precision must be one of {_MODES}")
    MLP_PRECISION = mode


def inference_mlp_mode():
    """What a no-grad query runs under the current MLP_PRECISION ("guarded" for "auto")."""
    return "guarded" if MLP_PRECISION == "auto" else MLP_PRECISION


def training_mlp_mode():
    return "fp32" if MLP_PRECISION == "auto" else MLP_PRECISION


class mlp_precision:
    """`with ops.mlp_precision("bf16"): ...` - set_mlp_precision for the duration of a block (the previous mode is restored)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = MLP_PRECISION
        set_mlp_precision(self.mode)

    def __exit__(self, *exc):
        set_mlp_precision(self.prev)


_guards = {}


def guard_words(device=None):
    """The guard words of the guarded 16-bit sequences enqueued on (this device, the CURRENT stream): int32[4] = {tripped (re-armed by every
    sequence), sequences that fell back to the fp32 kernels so far, 0, 0}.  One buffer per (device, stream), allocated once and owned here (the
    library allocates nothing): a sequence arms, reads and re-arms word 0 in STREAM order only, so two streams (or two host threads on their own
    streams) must never share a buffer - stream B's consume kernel could re-arm the word between stream A's fp16 kernel tripping it and A's
    predicated fp32 kernel reading it (include/mvsnerf_hip.h, "guarded 16-bit sequences": one guard buffer per stream)."""
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    key = (idx, torch.cuda.current_stream(idx).cuda_stream)
    g = _guards.get(key)
    if g is None:
        with torch.cuda.device(idx):
            g = _guards[key] = torch.zeros(4, device=torch.device("cuda", idx), dtype=torch.int32)
    return g


def guard_fallbacks(device=None):
    """Number of guarded sequences (ray-march batches, network queries, scene encodes) on this device - all streams - whose fp32 kernels had to
    take over because a value left fp16's range.  Reading it synchronises - it is for tests and reports, the hot path never looks at it."""
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    torch.cuda.synchronize(idx)
    return sum(int(g[1].item()) for (d, _), g in list(_guards.items()) if d == idx)


def mlp_pack_split(weights, F, n_split):
    n = _lib.lib().mvsnerf_mlp_packed_split_elems(F, n_split)
    if n == 0:
        raise RuntimeError(f"mlp_pack_split: feat_dim {F} / n_split {n_split} unsupported")
    packed = torch.empty(n, device=weights[0].device, dtype=torch.bfloat16)
    wp = _Ptr11(*[dev_f32(w, "weight") for w in weights])
    check(_lib.lib().mvsnerf_mlp_pack_split(wp, F, n_split, packed.data_ptr(), stream_ptr()), "mlp_pack_split")
    return packed


def mlp_pack_bf16(weights, F):
    n = _lib.lib().mvsnerf_mlp_packed_bf16_elems(F)
    packed = torch.empty(n, device=weights[0].device, dtype=torch.bfloat16)
    wp = _Ptr11(*[dev_f32(w, "weight") for w in weights])
    check(_lib.lib().mvsnerf_mlp_pack_bf16(wp, F, packed.data_ptr(), stream_ptr()), "mlp_pack_bf16")
    return packed


def mlp_forward(packed, F, ndc_ptr, ndc_stride, feat_ptr, feat_stride, dirs_ptr, dirs_stride, N, S, alpha_only, device, *,
                packed_bf16=None, packed_split=None, guard=None, count=None, out=None):
    """Network query (run_network_mvs, renderer.py:42-63) -> raw (N*S, 1 if alpha_only else 4).  The keywords choose the kernel as the ray march
    does (Renderer_ours.packed_alt returns them): guard + packed_split = (fp16x3 planes, 18) -> the guarded sequence, packed_split = (planes,
    n_split) -> the split kernel, packed_bf16 -> bf16, none -> fp32.  A WidePacked (netwidth 256) runs the wide fp32 kernel and takes no keyword.
    count: the (1,) int32 device tensor of ops.live_samples - the counted launch of DESIGN.md 4i on dense rows (S == 1, strides 3 / F / 3): N is
    then the capacity, rows [0, min(max(count, 0), N)) of raw get the bits of the call with that N and no other row is written; the bf16 family has
    no counted kernel.  out: a caller-owned contiguous fp32 (N*S, 1 | 4) tensor to write into."""
    cptr = None
    if count is not None:           # the refusals of a counted launch, before the library is touched
        cptr = _count_ptr(count, S, "mlp_forward")
        _device_count_mode(packed_bf16, packed_split, "mlp_forward(count=)")
        if (ndc_stride, feat_stride, dirs_stride) != (3, F, 3):
            raise RuntimeError(f"mlp_forward: count= takes dense rows (strides 3 / {F} / 3), got {ndc_stride} / {feat_stride} / {dirs_stride}")
    wide = isinstance(packed, WidePacked)
    if wide:
        if packed_bf16 is not None or packed_split is not None or guard is not None:
            raise ValueError("mlp_forward: netwidth 256 runs on the fp32 wide kernel only; packed_bf16 / packed_split / guard select 128-wide kernels")
        if packed.F != F:
            raise RuntimeError(f"mlp_forward: the buffer was packed for feat_dim {packed.F}, the call says {F}")
    l = _lib.lib()
    raw = torch.empty((N * S, 1 if alpha_only else 4), device=device, dtype=torch.float32) if out is None else out
    if out is not None:
        if tuple(raw.shape) != (N * S, 1 if alpha_only else 4):
            raise RuntimeError(f"mlp_forward: out must be ({N * S},{1 if alpha_only else 4}), got {tuple(raw.shape)}")
        dev_f32(raw, "mlp_forward: out")
    # (wide | guarded | split | bf16 | fp32) x (plain | counted): the entry is mvsnerf_mlp_fwd[_<kernel>][_counted](*head, *io[, guard], stream);
    # a counted call has been refused above for the kernels without a counted entry
    if wide:
        kernel, head = "_wide", (dev_f32(packed.buffer, "packed"), F, packed.width)
    elif guard is not None:
        if packed_split is None or packed_split[1] != N_SPLIT["fp16x3"]:
            raise ValueError("mlp_forward: a guard needs the fp16x3 split planes (the guarded sequence)")
        kernel, head = "_guarded", (packed_split[0].data_ptr(), packed.data_ptr(), F)
    elif packed_split is not None:
        kernel, head = "_split", (packed_split[0].data_ptr(), packed.data_ptr(), F, packed_split[1])
    elif packed_bf16 is not None:
        kernel, head = "_bf16", (packed_bf16.data_ptr(), packed.data_ptr(), F)
    else:
        kernel, head = "", (packed.data_ptr(), F)
    if cptr is None:
        name, io = f"mlp_fwd{kernel}", (ndc_ptr, ndc_stride, feat_ptr, feat_stride, dirs_ptr, dirs_stride, N, S)
    else:
        name, io = f"mlp_fwd{kernel}_counted", (ndc_ptr, feat_ptr, dirs_ptr, N, cptr)
    check(getattr(l, "mvsnerf_" + name)(*head, *io, int(alpha_only), raw.data_ptr(), *(() if guard is None else (guard.data_ptr(),)), stream_ptr()), name)
    return raw


def _device_count_mode(packed_bf16, packed_split, op):
    """The bf16 family has no counted forward kernel: a kernel choice (MVSNeRF.packed_alt's keywords) that names one is refused
    by its mode's name."""
    mode = "bf16" if packed_bf16 is not None else None
    if packed_split is not None and packed_split[1] != N_SPLIT["fp16x3"]:
        mode = {v: k for k, v in N_SPLIT.items()}.get(packed_split[1], f"n_split {packed_split[1]}")
    if mode is not None:
        raise NotImplementedError(f"{op}: the {mode!r} MLP kernels take their row count from the host only; device counts run under "
                                  "'auto', 'fp32' and 'fp16x3' (and netwidth 256)")


def _mlp_fields(packed_bf16, packed_split, guard):
    """The MLP-choice fields of mvsnerf_raymarch_args and mvsnerf_render_args."""
    return dict(packed_mlp_bf16=0 if packed_bf16 is None else packed_bf16.data_ptr(),
                packed_mlp_split=0 if packed_split is None else packed_split[0].data_ptr(),
                n_split=0 if packed_split is None else int(packed_split[1]), guard=0 if guard is None else guard.data_ptr())


# ------------------------------------------------------------------ compositing
def composite(raw, z_vals, white_bkgd=False):
    """raw (N,S,4), z (N,S) -> rgb_map, disp, acc, weights, depth, alpha  (renderer.py:65-92).
    One deviation from the reference: a ray whose densities are all zero has depth / acc = 0/0; renderer.py:87 (torch.max) returns disp = NaN there, the kernels'
    fmaxf(1e-10f, NaN) is 1e-10 and they return the finite disp = 1e10 (rgb = 0, or 1 with white_bkgd; acc = depth = weights = alpha = 0 exactly).  The compositing
    epilogue of ops.raymarch does the same."""
    _need_no_grad(raw, z_vals, op="composite")
    N, S = z_vals.shape
    dev = raw.device
    rgb = torch.empty((N, 3), device=dev, dtype=torch.float32)
    disp = torch.empty((N,), device=dev, dtype=torch.float32)
    acc = torch.empty((N,), device=dev, dtype=torch.float32)
    depth = torch.empty((N,), device=dev, dtype=torch.float32)
    weights = torch.empty((N, S), device=dev, dtype=torch.float32)
    alpha = torch.empty((N, S), device=dev, dtype=torch.float32)
    check(_lib.lib().mvsnerf_composite_fwd(dev_f32(raw, "raw"), dev_f32(z_vals, "z_vals"), N, S, int(bool(white_bkgd)),
                                           rgb.data_ptr(), disp.data_ptr(), acc.data_ptr(), weights.data_ptr(),
                                           depth.data_ptr(), alpha.data_ptr(), stream_ptr()), "composite_fwd")
    return rgb, disp, acc, weights, depth, alpha


# ------------------------------------------------------------------ fused ray march
def _raymarch_block(vol_cl, imgs, w2cs, intrinsics, packed, rays_pts, rays_ndc, z_vals, rays_dir, white_bkgd, packed_bf16, packed_split, guard, want, imgs_cl, cur):
    """Output tensors + the filled mvsnerf_raymarch_args (_lib.RaymarchArgs) of one batch.  imgs None: a batch on an (8 + 4V)-channel colour volume
    (V from w2cs; the caller has checked the channel count) - the image, intrinsics and point fields stay 0."""
    N, S = z_vals.shape
    D, H, W, C = vol_cl.shape
    V = w2cs.shape[0] if imgs is None else imgs.shape[0]
    if imgs is not None and C != 8:
        raise RuntimeError("raymarch: the neural volume must have 8 channels")
    shapes = {"input_feat": (N, S, C if imgs is None else 8 + 4 * V), "raw": (N, S, 4), "rgb_map": (N, 3), "weights": (N, S), "depth": (N,),
              "alpha": (N, S), **{k: (N,) for k in want}, "_dirs_tmp": (N, 3)}
    out = {k: torch.empty(sh, device=rays_ndc.device, dtype=torch.float32) for k, sh in shapes.items()}
    if imgs is not None and imgs_cl is None and FUSED_GATHER:
        imgs_cl = channels_last_images(imgs)
    vp, vl = vol_ptr_layout(vol_cl, cur)
    ptrs = {k: out[k].data_ptr() if k in out else 0 for k in ("input_feat", "raw", "rgb_map", "disp", "acc", "weights", "depth", "alpha")}
    if imgs is not None:
        ptrs.update(imgs=dev_f32(imgs, "imgs", cur), IH=imgs.shape[2], IW=imgs.shape[3],
                    imgs_nhwc4=imgs_cl.data_ptr() if (FUSED_GATHER and imgs_cl is not None) else 0,
                    K=dev_f32(intrinsics, "intrinsics", cur), rays_pts=dev_f32(rays_pts, "rays_pts", cur))
    return out, _lib.RaymarchArgs(
        vol=vp, D=D, H=H, W=W, vol_layout=vl, V=V, w2c=dev_f32(w2cs, "w2cs", cur), packed_mlp=dev_f32(packed, "packed", cur),
        rays_ndc=dev_f32(rays_ndc, "rays_ndc", cur), z_vals=dev_f32(z_vals, "z_vals", cur),
        rays_dir=dev_f32(rays_dir, "rays_dir", cur), N=N, S=S, white_bkgd=int(bool(white_bkgd)), dirs_tmp=out["_dirs_tmp"].data_ptr(), **ptrs,
        **_mlp_fields(packed_bf16, packed_split, guard))


def raymarch(vol_cl, imgs, w2cs, intrinsics, packed, rays_pts, rays_ndc, z_vals, rays_dir, white_bkgd=False, packed_bf16=None, packed_split=None,
             guard=None, want=("disp", "acc"), imgs_cl=None):
    """One FFI call for rendering() (renderer.py:138-165).  Returns dict of outputs.
    want: which of the optional per-ray maps `disp` / `acc` to produce (rendering() returns neither: it passes ()).
    imgs_cl: the channel-last copy of `imgs` when the caller already holds it (renderer's per-scene cache)."""
    _need_narrow(packed, "raymarch")
    _need_no_grad(vol_cl, imgs, rays_pts, rays_ndc, z_vals, rays_dir, op="raymarch")
    out, blk = _raymarch_block(vol_cl, imgs, w2cs, intrinsics, packed, rays_pts, rays_ndc, z_vals, rays_dir, white_bkgd, packed_bf16, packed_split,
                               guard, want, imgs_cl, torch.cuda.current_device())
    check(_lib.lib().mvsnerf_raymarch_fwd(ctypes.byref(blk), stream_ptr()), "raymarch_fwd")
    return out


def raymarch_batched(vol_cl, imgs, w2cs, intrinsics, packed, ray_batches, white_bkgd=False, packed_bf16=None, packed_split=None, guard=None, want=(),
                     imgs_cl=None):
    """K ray batches of one scene in ONE FFI call (mvsnerf_raymarch_fwd_batched): ray_batches = [(rays_pts, rays_ndc, z_vals, rays_dir), ...].
    Returns the list of per-batch output dicts of raymarch().  One batch is ~0.1 ms of GPU work; issued one call at a time, a render loop is
    paced by the host."""
    _need_narrow(packed, "raymarch_batched")
    cur = torch.cuda.current_device()
    outs, blocks = [], (_lib.RaymarchArgs * len(ray_batches))()
    for k, (pts, ndc, z, rdir) in enumerate(ray_batches):
        _need_no_grad(vol_cl, imgs, pts, ndc, z, rdir, op="raymarch_batched")
        out, blocks[k] = _raymarch_block(vol_cl, imgs, w2cs, intrinsics, packed, pts, ndc, z, rdir, white_bkgd, packed_bf16, packed_split, guard, want,
                                         imgs_cl, cur)
        outs.append(out)
    check(_lib.lib().mvsnerf_raymarch_fwd_batched(blocks, len(ray_batches), stream_ptr()), "raymarch_fwd_batched")
    return outs


def raymarch_colorvol_batched(vol_cl, w2cs, packed, ray_batches, white_bkgd=False, packed_bf16=None, packed_split=None, guard=None, want=()):
    """raymarch_batched on an (8 + 4V)-channel colour volume (mvsnerf_raymarch_colorvol_fwd_batched): ray_batches = [(rays_ndc, z_vals, rays_dir), ...];
    w2cs (V,4,4), view 0 the reference view.  No images, intrinsics or points are needed: the feature row is one lookup of the volume."""
    _need_narrow(packed, "raymarch_colorvol_batched")
    cur = torch.cuda.current_device()
    C, V = vol_cl.shape[-1], w2cs.shape[0]
    if C != 8 + 4 * V:
        raise RuntimeError(f"raymarch_colorvol_batched: the volume has {C} channels, 8 + 4V is {8 + 4 * V}")
    if not ray_batches:
        vol_ptr_layout(vol_cl, cur)                 # (a volume no batch would have met is refused all the same)
    outs, blocks = [], (_lib.RaymarchArgs * len(ray_batches))()
    for k, (ndc, z, rdir) in enumerate(ray_batches):
        _need_no_grad(vol_cl, ndc, z, rdir, op="raymarch_colorvol_batched")
        out, blocks[k] = _raymarch_block(vol_cl, None, w2cs, None, packed, None, ndc, z, rdir, white_bkgd, packed_bf16, packed_split, guard, want, None, cur)
        outs.append(out)
    check(_lib.lib().mvsnerf_raymarch_colorvol_fwd_batched(blocks, len(ray_batches), C, stream_ptr()), "raymarch_colorvol_fwd_batched")
    return outs


def render_rays(vol_cl, rays, t, packed, K_ref, w2c_ref, nf_ref, ref_hw, n_views, imgs=None, w2cs=None, intrinsics=None, first_ray=0, n_rays=None,
                density=None, u=None, pad=0, lindisp=False, white_bkgd=False, batch_rays=16384, want=("depth",), packed_bf16=None, packed_split=None,
                guard=None):
    """Rays [first_ray, first_ray + n_rays) of `rays` (N,8) = [o | d | near | far] of a fine-tuned scene in ONE FFI call (mvsnerf_render_rays_fwd: the
    chunk loop of the fine-tuning script's validation_step).  vol_cl (D,H,W,C): C == 8 renders from the volume and the source images (imgs (V,3,IH,IW)
    un-normalised, w2cs (V,4,4), intrinsics (V,3,3)); C == 8 + 4*n_views is a colour volume and needs none of them.  t (S,) = linspace(0,1,S);
    density (DD,DH,DW) + u (N,NI): importance sampling (ray_marcher_fine).  Returns dict with rgb (n,3) and the requested extras among depth/acc/disp (n,)."""
    _need_narrow(packed, "render_rays")
    _need_no_grad(vol_cl, rays, imgs, density, op="render_rays")
    lib = _lib.lib()
    if rays.dim() != 2 or rays.shape[1] != 8:
        raise RuntimeError(f"render_rays: rays must be (N,8), got {tuple(rays.shape)}")
    n = rays.shape[0] - first_ray if n_rays is None else int(n_rays)
    if first_ray < 0 or n < 0 or first_ray + n > rays.shape[0]:
        raise RuntimeError(f"render_rays: rays [{first_ray}, {first_ray + n}) outside the {rays.shape[0]} given")
    V = int(n_views)
    D, Hv, Wv, C = vol_cl.shape
    F, S = 8 + 4 * V, int(t.shape[0])
    fine = density is not None and u is not None and u.shape[-1] > 0
    NI = int(u.shape[1]) if fine else 0
    if fine and u.shape[0] != rays.shape[0]:
        raise RuntimeError(f"render_rays: u must hold one row per ray ({rays.shape[0]}), got {tuple(u.shape)}")
    if C == 8 and (imgs is None or w2cs is None or intrinsics is None or imgs.shape[0] != V):
        raise RuntimeError("render_rays: an 8-channel volume needs imgs (n_views,3,H,W), w2cs and intrinsics")
    dev = vol_cl.device
    B = int(min(batch_rays, max(n, 1)))
    ws_n = lib.mvsnerf_render_rays_workspace_floats(B, S, NI, F)
    if ws_n == 0:
        raise RuntimeError(f"render_rays: unsupported sizes (batch_rays {B}, S {S}, n_importance {NI}, F {F})")
    ws = _render_workspace(ws_n, dev, "rays")
    out, ptrs = _render_outputs(n, want, dev)
    if n == 0:
        return out
    c = _Keep()
    vp, vl = vol_ptr_layout(vol_cl)
    src = {}
    if C == 8:
        src = dict(imgs_nhwc4=channels_last_images(imgs).data_ptr(), IH=imgs.shape[2], IW=imgs.shape[3], w2c=c(w2cs, "w2cs"), K=c(intrinsics, "intrinsics"))
    if fine:
        src.update(density=c(density, "density_volume"), DD=density.shape[0], DH=density.shape[1], DW=density.shape[2], u=c(u, "u"), n_importance=NI)
    a = _lib.RenderRaysArgs(
        vol=vp, D=D, H=Hv, W=Wv, C=C, vol_layout=vl, V=V, K_ref=c(K_ref, "K_ref"), w2c_ref=c(w2c_ref, "w2c_ref"),
        near_far_ref=c(nf_ref.reshape(-1)[:2], "near_far_ref"), W_ref=int(ref_hw[1]), H_ref=int(ref_hw[0]), pad=int(pad), lindisp=int(bool(lindisp)),
        packed_mlp=packed.data_ptr(), rays=c(rays, "rays"), first_ray=int(first_ray), n_rays=n, t=c(t, "t"), S=S,
        white_bkgd=int(bool(white_bkgd)), batch_rays=B, workspace=ws.data_ptr(), workspace_floats=ws_n, **ptrs, **src,
        **_mlp_fields(packed_bf16, packed_split, guard))
    check(lib.mvsnerf_render_rays_fwd(ctypes.byref(a), stream_ptr()), "render_rays_fwd")
    return out


def render_pixels(vol_cl, imgs, w2cs, intrinsics, packed, H, W, K_tgt, c2w_tgt, K_ref, w2c_ref, nf_tgt, nf_ref, N_samples,
                  first_pixel=0, n_pixels=None, pad=0, lindisp=False, white_bkgd=False, packed_bf16=None, batch_rays=4096,
                  want=("depth",), ref_hw=None, packed_split=None, guard=None):
    """Pixel range of one target view in ONE FFI call (the chunk loop of validation_step, train_mvs_nerf_pl.py:198-208).
    Returns dict with rgb (n,3) and the requested extras among depth/acc/disp (n,)."""
    _need_no_grad(vol_cl, imgs, op="render_pixels")
    _need_narrow(packed, "render_pixels")
    lib = _lib.lib()
    n = H * W - first_pixel if n_pixels is None else int(n_pixels)
    V = imgs.shape[0]
    D, Hv, Wv, C = vol_cl.shape
    if C != 8:
        raise RuntimeError("render_pixels: the neural volume must have 8 channels")
    dev = vol_cl.device
    B = int(min(batch_rays, max(n, 1)))
    ws_n = lib.mvsnerf_render_workspace_floats(B, N_samples, V)
    ws = _render_workspace(ws_n, dev, "pixels")
    out, ptrs = _render_outputs(n, want, dev)
    if n == 0:
        return out
    c = _Keep()
    vp, vl = vol_ptr_layout(vol_cl)
    a = _lib.RenderArgs(
        vol=vp, D=D, H=Hv, W=Wv, vol_layout=vl, imgs_nhwc4=channels_last_images(imgs).data_ptr(), V=V, IH=imgs.shape[2], IW=imgs.shape[3],
        w2c=c(w2cs, "w2cs"), K=c(intrinsics, "intrinsics"), packed_mlp=packed.data_ptr(), K_tgt=c(K_tgt, "K_tgt"), c2w_tgt=c(c2w_tgt, "c2w_tgt"),
        K_ref=c(K_ref, "K_ref"), w2c_ref=c(w2c_ref, "w2c_ref"), near_far_tgt=c(nf_tgt, "near_far_tgt"), near_far_ref=c(nf_ref, "near_far_ref"),
        W_img=W, H_img=H, pad=int(pad), lindisp=int(bool(lindisp)), W_ref=0 if ref_hw is None else int(ref_hw[1]), H_ref=0 if ref_hw is None else int(ref_hw[0]),
        first_pixel=int(first_pixel), n_pixels=n, S=int(N_samples), white_bkgd=int(bool(white_bkgd)), batch_rays=B, workspace=ws.data_ptr(),
        workspace_floats=ws_n, **ptrs, **_mlp_fields(packed_bf16, packed_split, guard))
    check(lib.mvsnerf_render_pixels_fwd(ctypes.byref(a), stream_ptr()), "render_pixels_fwd")
    return out


_render_ws = {}


def _render_workspace(ws_n, dev, kind):
    """The workspace of a whole-frame render, one per (size, device, STREAM, kind): two streams rendering on one device must not share intermediates
    (same reason as guard_words).  At most four are kept; the oldest goes first."""
    key = (ws_n, dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream, kind)
    ws = _render_ws.get(key)
    if ws is None:
        while len(_render_ws) >= 4:
            _render_ws.pop(next(iter(_render_ws)))
        ws = _render_ws[key] = torch.empty(ws_n, device=dev, dtype=torch.float32)
    return ws


def _render_outputs(n, want, dev):
    """(the dict a whole-frame render returns: rgb (n,3) and those of depth / acc / disp (n,) that are in `want`; the four output fields of its
    argument block, 0 for a map that is not wanted)"""
    out = {"rgb": torch.empty((n, 3), device=dev, dtype=torch.float32)}
    out.update({k: torch.empty((n,), device=dev, dtype=torch.float32) for k in ("depth", "acc", "disp") if k in want})
    return out, {k: out[k].data_ptr() if k in out else 0 for k in ("rgb", "depth", "acc", "disp")}


# ------------------------------------------------------------------ empty-space skipping (csrc/sparse.hip)
def _thr_f32(thr, op):
    thr = float(thr)
    if thr != thr:
        raise ValueError(f"{op}: the density threshold is NaN")
    return thr


def _ray_batch(rays_ndc, rays_pts, rays_dir, ray_T, op):
    """(N, S) of a ray batch after the shape checks: rays_ndc (N,S,3), rays_pts (N,S,3) | None, rays_dir (N,3) | None, ray_T (N,) | None, S >= 1 and
    N * S below 2^31."""
    if rays_ndc.dim() != 3 or rays_ndc.shape[-1] != 3:
        raise RuntimeError(f"{op}: rays_ndc must be (N,S,3), got {tuple(rays_ndc.shape)}")
    N, S = int(rays_ndc.shape[0]), int(rays_ndc.shape[1])
    for t, name, shape in ((rays_pts, "rays_pts", (N, S, 3)), (rays_dir, "rays_dir", (N, 3)), (ray_T, "ray_T", (N,))):
        if t is not None and tuple(t.shape) != shape:
            raise RuntimeError(f"{op}: {name} must be ({','.join(map(str, shape))}{',' if len(shape) == 1 else ''}), got {tuple(t.shape)}")
    if S < 1 or N * S >= 2 ** 31:
        raise RuntimeError(f"{op}: {N} x {S} samples: S >= 1 and fewer than 2^31 samples (idx is int32)")
    return N, S


def live_samples(density, rays_ndc, thr, rays_pts=None, rays_dir=None):
    """Which samples of a ray batch can contribute, and their stable compaction (mvsnerf_live_samples_fwd): density (D,H,W), rays_ndc (N,S,3) ->
    (count, idx, ndc_c, pts_c, dir_c).  A sample is live iff a coordinate is non-finite or some in-grid corner of its trilinear cell in `density`
    holds a value v with not (v <= thr) (thr is rounded to fp32; a NaN voxel is live).  count: int32 (1,) on the device; idx: int32 (P,), its first
    count entries the flat indices n*S + s of the live samples, ascending (torch.nonzero's order); ndc_c / pts_c / dir_c: (P,3), their first count rows
    the live samples' NDC rows, rays_pts rows and the rays_dir row of their ray (None for an input that is None).  Buffers have the worst-case size;
    what lies behind count is not written.  Three launches on the current stream, no host synchronisation, no atomics: two runs give the same bytes."""
    _need_no_grad(density, rays_ndc, rays_pts, rays_dir, op="live_samples")
    thr = _thr_f32(thr, "live_samples")
    if density.dim() != 3:
        raise RuntimeError(f"live_samples: density must be (D,H,W), got {tuple(density.shape)}")
    N, S = _ray_batch(rays_ndc, rays_pts, rays_dir, None, "live_samples")
    P = N * S
    lib = _lib.lib()
    dev = rays_ndc.device
    D, H, W = density.shape
    c = _Keep()
    count = torch.empty((1,), device=dev, dtype=torch.int32)
    idx = torch.empty((P,), device=dev, dtype=torch.int32)
    rows = [torch.empty((P, 3), device=dev, dtype=torch.float32) if t is not None else None for t in (rays_ndc, rays_pts, rays_dir)]
    ws = torch.empty((max(int(lib.mvsnerf_live_samples_workspace_bytes(P)), 8) // 8,), device=dev, dtype=torch.int64)
    check(lib.mvsnerf_live_samples_fwd(c(density, "density"), D, H, W, thr, c(rays_ndc, "rays_ndc"),
                                       0 if rays_pts is None else c(rays_pts, "rays_pts"), 0 if rays_dir is None else c(rays_dir, "rays_dir"),
                                       N, S, count.data_ptr(), idx.data_ptr(), *[0 if r is None else r.data_ptr() for r in rows],
                                       ws.data_ptr(), stream_ptr()), "live_samples_fwd")
    return (count, idx, *rows)


def _need_row_index(idx, count, op):
    if not (idx.dtype == torch.int32 and idx.is_cuda and idx.is_contiguous() and count.dtype == torch.int32 and count.is_cuda and count.numel() == 1):
        raise RuntimeError(f"{op}: idx and count are the int32 device tensors of ops.live_samples / ops.live_samples_range")


def expand_rows(src, idx, count, P, out=None):
    """dst (P,C) with dst[idx[j]] = src[j] for j < count and every other row zero (mvsnerf_expand_rows_fwd): src (n,C) fp32, idx / count as
    ops.live_samples returns them (count is read on the device and clamped to n).  Every element of dst is written, whatever it held
    (out: a caller-owned contiguous fp32 (P,C) tensor to write into)."""
    _need_no_grad(src, op="expand_rows")
    if src.dim() != 2:
        raise RuntimeError(f"expand_rows: src must be (n,C), got {tuple(src.shape)}")
    n, C = int(src.shape[0]), int(src.shape[1])
    P = int(P)
    _need_row_index(idx, count, "expand_rows")
    if n > P or idx.numel() < n:
        raise RuntimeError(f"expand_rows: {n} source rows, {idx.numel()} indices, {P} destination rows")
    c = _Keep()
    dst = torch.empty((P, C), device=src.device, dtype=torch.float32) if out is None else out
    if tuple(dst.shape) != (P, C):
        raise RuntimeError(f"expand_rows: out must be ({P},{C}), got {tuple(dst.shape)}")
    dev_f32(dst, "expand_rows: out")
    check(_lib.lib().mvsnerf_expand_rows_fwd(c(src, "src") if n else 0, idx.data_ptr() if n else 0, count.data_ptr(), n, P, C, dst.data_ptr(), stream_ptr()),
          "expand_rows_fwd")
    return dst


def compact_rows(src, idx, count, n_rows, out=None):
    """dst (n_rows,C) with dst[j] = src[idx[j]] for j < count and every other row zero (mvsnerf_compact_rows_fwd), the inverse of expand_rows:
    src (P,C) fp32, idx / count as ops.live_samples returns them (count is read on the device and clamped to n_rows; an idx entry outside [0, P)
    gives a zero row).  Every element of dst is written, whatever it held (out: a caller-owned contiguous fp32 (n_rows,C) tensor to write into)."""
    _need_no_grad(src, op="compact_rows")
    if src.dim() != 2:
        raise RuntimeError(f"compact_rows: src must be (P,C), got {tuple(src.shape)}")
    P, C = int(src.shape[0]), int(src.shape[1])
    n = int(n_rows)
    _need_row_index(idx, count, "compact_rows")
    if n < 0 or n > P or idx.numel() < n:
        raise RuntimeError(f"compact_rows: {P} source rows, {idx.numel()} indices, {n} destination rows")
    c = _Keep()
    dst = torch.empty((n, C), device=src.device, dtype=torch.float32) if out is None else out
    if tuple(dst.shape) != (n, C):
        raise RuntimeError(f"compact_rows: out must be ({n},{C}), got {tuple(dst.shape)}")
    if n:               # an empty destination has no row to write (and an empty tensor no address to hand over)
        dev_f32(dst, "compact_rows: out")
        check(_lib.lib().mvsnerf_compact_rows_fwd(c(src, "src"), idx.data_ptr(), count.data_ptr(), P, n, C, dst.data_ptr(), stream_ptr()), "compact_rows_fwd")
    return dst


def _sparse_march(vol_cl, imgs, w2cs, intrinsics, rays_pts, rays_ndc, z_vals, rays_dir, density, thr, white_bkgd, mlp, device_count=False):
    """The sparse ray march both faces run (ops.raymarch_sparse, SparseRayMarchFunction.forward): live_samples of `density` at `thr` -> ONE host read
    of the count (the only synchronisation; at 0 neither a gather nor an MLP launch is enqueued and raw_c is empty) -> ops.gather (ops.gather_colorvol
    for an (8+4V)-channel colour volume, which needs no imgs / intrinsics / rays_pts) on the compact rows as (n_live,1,3) -> the MLP stage with
    N = n_live, S = 1: mlp(ndc_l (n_live,3), feat (n_live,1,F), dirs (n_live,3), n_live) -> raw_c (n_live,4) -> expand_rows into raw (N,S,4) ->
    ops.composite (mvsnerf_composite_fwd).  Dead samples have raw = (0,0,0,0), so alpha = weight = 0; live ones the bits of the dense sequence (a
    sample's MLP column does not depend on its neighbours in the tile).
    device_count=True: no host read - the count goes to _compact_rows_mlp as the device tensor, the rows are the worst-case N*S, mlp
    is called with count= and n_live is the int32 device scalar.
    Returns (idx, count, ndc_l, raw_c, raw, n_live) - what a backward has to keep - and ops.composite's (rgb_map, disp, acc, weights, depth, alpha)."""
    N, S = z_vals.shape
    color_vol = vol_cl.shape[-1] != 8
    count, idx, ndc_c, pts_c, dir_c = live_samples(density, rays_ndc, thr, None if color_vol else rays_pts, rays_dir)
    n_live = count.reshape(()) if device_count else int(count.item())
    ndc_l, raw_c = _compact_rows_mlp(vol_cl, imgs, w2cs, intrinsics, ndc_c, pts_c, dir_c, count if device_count else n_live, mlp)
    raw = expand_rows(raw_c, idx, count, N * S).view(N, S, 4)
    return (idx, count, ndc_l, raw_c, raw, n_live), composite(raw, z_vals, white_bkgd)


def _compact_rows_mlp(vol_cl, imgs, w2cs, intrinsics, ndc_c, pts_c, dir_c, n, mlp):
    """The gather-and-MLP stage of the compacted marches (_sparse_march, raymarch_early_stop) on the compact rows of ops.live_samples /
    ops.live_samples_range: ops.gather (ops.gather_colorvol for a colour volume) on the rows as (rows,1,3) -> mlp(ndc_l, feat, dirs, rows).
    n a host integer: the first n rows, and n == 0 enqueues nothing.  n the (1,) int32 device count: the worst-case buffers whole, the
    counted gather and mlp(..., count=n), both enqueued whatever the count holds - rows [0, count) of raw_c are written; a capacity of 0 rows enqueues
    nothing.  Returns (ndc_l (rows,3), raw_c (rows,4))."""
    if torch.is_tensor(n):
        rows, take, kw = ndc_c.shape[0], (lambda t: t), {"count": n}
    else:
        rows, take, kw = n, (lambda t: t[:n]), {}
    ndc_l = take(ndc_c)
    if not rows:
        return ndc_l, torch.empty((0, 4), device=ndc_c.device, dtype=torch.float32)
    ndc_g, dir_l = ndc_l.view(rows, 1, 3), take(dir_c)
    if vol_cl.shape[-1] != 8:
        feat, dirs = gather_colorvol(vol_cl, ndc_g, dir_l, w2cs[0].contiguous(), **kw)
    else:
        feat, dirs = gather(vol_cl, imgs, w2cs, intrinsics, take(pts_c).view(rows, 1, 3), ndc_g, dir_l, **kw)
    return ndc_l, mlp(ndc_l, feat, dirs, rows, **kw)


def _rows_mlp(packed, F, dev, **packed_alt):
    """ops.mlp_forward as the MLP stage of _compact_rows_mlp: (ndc_l (n,3), feat (n,1,F), dirs (n,3), n[, count=]) -> raw_c (n,4), N = n, S = 1."""
    return lambda ndc_l, feat, dirs, n, count=None: mlp_forward(packed, F, ndc_l.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, n, 1, 0, dev,
                                                                count=count, **packed_alt)


def _march_outputs(raw, composited, want, **extras):
    """The dict a compacted march returns: raw, ops.composite's maps (disp / acc when in `want`), then the counts."""
    rgb, disp, acc, weights, depth, alpha = composited
    out = {"raw": raw, "rgb_map": rgb, "weights": weights, "depth": depth, "alpha": alpha}
    out.update({k: v for k, v in (("disp", disp), ("acc", acc)) if k in want})
    out.update(extras)
    return out


def raymarch_sparse(vol_cl, imgs, w2cs, intrinsics, packed, rays_pts, rays_ndc, z_vals, rays_dir, density, thr, white_bkgd=False, want=(),
                    device_count=False, **packed_alt):
    """ops.raymarch's outputs with the radiance MLP run on the live samples only (ops.live_samples of `density` at `thr`): the sequence of
    _sparse_march with ops.mlp_forward as its MLP stage.  packed: mlp_pack's buffer or a WidePacked; **packed_alt: the kernel choice of
    ops.mlp_forward (MVSNeRF.packed_alt).  Returns raw, rgb_map, weights, depth, alpha, disp / acc when in `want`, and n_live (int).
    device_count=True: the same sequence without the host read - the gather and the MLP are counted launches on the worst-case (N*S)-row
    buffers, enqueued whatever the count is; the outputs have the same bits, n_live is an int32 device scalar, and the call can be enqueued ahead or
    captured into a graph.  Not under the bf16-family modes (NotImplementedError)."""
    if device_count:
        _device_count_mode(packed_alt.get("packed_bf16"), packed_alt.get("packed_split"), "raymarch_sparse(device_count=True)")
    _need_no_grad(vol_cl, imgs, rays_pts, rays_ndc, z_vals, rays_dir, density, op="raymarch_sparse")
    thr = _thr_f32(thr, "raymarch_sparse")
    C = vol_cl.shape[-1]
    F = C if C != 8 else 8 + 4 * imgs.shape[0]
    if C != 8 and C != 8 + 4 * w2cs.shape[0]:
        raise RuntimeError(f"raymarch_sparse: the volume has {C} channels, 8 + 4V is {8 + 4 * w2cs.shape[0]}")
    (_, _, _, _, raw, n_live), composited = _sparse_march(vol_cl, imgs, w2cs, intrinsics, rays_pts, rays_ndc, z_vals, rays_dir, density, thr, white_bkgd,
                                                          _rows_mlp(packed, F, rays_ndc.device, **packed_alt), device_count)
    return _march_outputs(raw, composited, want, n_live=n_live)


# ------------------------------------------------------------------ early ray termination (csrc/sparse.hip)
def _early_stop_args(eps, stop_every, op):
    """(eps, stop_every) of an early_stop call as (float, int) after the refusals: eps in [0, 1) (NaN refused), stop_every an integer >= 1."""
    eps = float(eps)
    if not (0.0 <= eps < 1.0):                      # NaN fails both compares
        raise ValueError(f"{op}: early_stop (eps) must be a transmittance in [0, 1), got {eps}")
    if isinstance(stop_every, bool) or int(stop_every) != stop_every or int(stop_every) < 1:
        raise ValueError(f"{op}: stop_every must be an integer >= 1, got {stop_every}")
    return eps, int(stop_every)


def _window(S, s0, s1, op):
    s0, s1 = int(s0), int(s1)
    if not (0 <= s0 < s1 <= S):
        raise RuntimeError(f"{op}: the window [{s0}, {s1}) is not inside the {S} samples of a ray")
    return s0, s1


def ray_transmittance(raw, s0, s1, ray_T):
    """ray_T[n] *= prod_{s0 <= s < s1} ((1 - alpha) + 1e-10), alpha = 1 - exp(-raw[n,s,3]), in place (mvsnerf_ray_transmittance_fwd): raw (N,S,4) and
    ray_T (N,) contiguous fp32 device tensors, ray_T set to 1 by the caller before the first window.  Ascending s, every product rounded - compositing's
    running transmittance, whatever the windows are.  Returns ray_T."""
    _need_no_grad(raw, ray_T, op="ray_transmittance")
    if raw.dim() != 3 or raw.shape[-1] != 4 or tuple(ray_T.shape) != (raw.shape[0],) or not (raw.is_contiguous() and ray_T.is_contiguous()):
        raise RuntimeError(f"ray_transmittance: raw must be a contiguous (N,S,4) and ray_T (N,), got {tuple(raw.shape)} and {tuple(ray_T.shape)}")
    N, S = int(raw.shape[0]), int(raw.shape[1])
    s0, s1 = _window(S, s0, s1, "ray_transmittance")
    if N:
        check(_lib.lib().mvsnerf_ray_transmittance_fwd(dev_f32(raw, "raw"), N, S, s0, s1, dev_f32(ray_T, "ray_T"), stream_ptr()), "ray_transmittance_fwd")
    return ray_T


def live_samples_range(density, rays_ndc, thr, s0, s1, ray_T=None, eps=0.0, rays_pts=None, rays_dir=None):
    """ops.live_samples over the window s0 <= s < s1 of every ray (mvsnerf_live_samples_range_fwd): a sample is selected iff not (ray_T[n] < eps) when
    ray_T (N,) is given, and its cell is live in `density` at `thr` when density is given (density None: thr is not read).  Returns (count, idx, ndc_c,
    pts_c, dir_c) as ops.live_samples, idx holding the flat indices n*S + s, ascending; the buffers have N * (s1 - s0) entries."""
    _need_no_grad(density, rays_ndc, rays_pts, rays_dir, ray_T, op="live_samples_range")
    thr = 0.0 if density is None else _thr_f32(thr, "live_samples_range")
    eps = float(eps)
    if eps != eps:
        raise ValueError("live_samples_range: eps is NaN")
    if density is not None and density.dim() != 3:
        raise RuntimeError(f"live_samples_range: density must be (D,H,W), got {tuple(density.shape)}")
    N, S = _ray_batch(rays_ndc, rays_pts, rays_dir, ray_T, "live_samples_range")
    s0, s1 = _window(S, s0, s1, "live_samples_range")
    lib = _lib.lib()
    dev = rays_ndc.device
    D, H, W = (0, 0, 0) if density is None else density.shape
    P = N * (s1 - s0)
    c = _Keep()
    opt = lambda t, name: 0 if t is None else c(t, name)
    count = torch.empty((1,), device=dev, dtype=torch.int32)
    idx = torch.empty((P,), device=dev, dtype=torch.int32)
    rows = [torch.empty((P, 3), device=dev, dtype=torch.float32) if t is not None else None for t in (rays_ndc, rays_pts, rays_dir)]
    ws = torch.empty((max(int(lib.mvsnerf_live_samples_range_workspace_bytes(N, s1 - s0)), 8) // 8,), device=dev, dtype=torch.int64)
    check(lib.mvsnerf_live_samples_range_fwd(opt(density, "density"), D, H, W, thr, c(rays_ndc, "rays_ndc"), opt(rays_pts, "rays_pts"),
                                             opt(rays_dir, "rays_dir"), N, S, s0, s1, opt(ray_T, "ray_T"), eps, count.data_ptr(), idx.data_ptr(),
                                             *[0 if r is None else r.data_ptr() for r in rows], ws.data_ptr(), stream_ptr()), "live_samples_range_fwd")
    return (count, idx, *rows)


def scatter_rows(src, idx, count, dst):
    """dst[idx[j]] = src[j] for j < count, every other row of dst (P,C) untouched (mvsnerf_scatter_rows_fwd): src (n,C) fp32, idx / count as
    ops.live_samples_range returns them (count is read on the device and clamped to n; an idx entry outside [0, P) writes nothing).  Returns dst."""
    _need_no_grad(src, dst, op="scatter_rows")
    if src.dim() != 2 or dst.dim() != 2 or src.shape[1] != dst.shape[1] or not dst.is_contiguous():
        raise RuntimeError(f"scatter_rows: src must be (n,C) and dst a contiguous (P,C), got {tuple(src.shape)} and {tuple(dst.shape)}")
    n, C, P = int(src.shape[0]), int(src.shape[1]), int(dst.shape[0])
    _need_row_index(idx, count, "scatter_rows")
    if n > P or idx.numel() < n:
        raise RuntimeError(f"scatter_rows: {n} source rows, {idx.numel()} indices, {P} destination rows")
    if n:
        c = _Keep()
        check(_lib.lib().mvsnerf_scatter_rows_fwd(c(src, "src"), idx.data_ptr(), count.data_ptr(), n, P, C, dev_f32(dst, "scatter_rows: dst"), stream_ptr()),
              "scatter_rows_fwd")
    return dst


def raymarch_early_stop(vol_cl, imgs, w2cs, intrinsics, packed, rays_pts, rays_ndc, z_vals, rays_dir, eps, stop_every=32, density=None, thr=None,
                        white_bkgd=False, want=(), **packed_alt):
    """ops.raymarch's outputs with rays stopped once they are opaque: the S samples are marched in segments of stop_every; a ray whose
    transmittance in front of a segment, T = prod ((1 - alpha) + 1e-10) over the samples before it (fp32, compositing's expression and order), is
    < eps is stopped there - its remaining samples do not reach the gather or the MLP and have raw = (0,0,0,0).  Every other sample has the bits of
    the dense sequence.  With density / thr (together or not at all) a sample also has to be live by ops.live_samples' predicate: then "dense" is
    ops.raymarch_sparse.  Per segment, in stream order: live_samples_range (with ray_T from the second segment on) -> ONE host read of the count (at 0
    nothing more is enqueued for the segment) -> the gather-and-MLP stage of _sparse_march on the compact rows -> scatter_rows into the zero-filled
    raw -> ray_transmittance over the segment (not after the last one); then ops.composite.  eps = 0 stops no ray: every output equals the dense call's.
    The dropped weights of a ray sum to less than eps (1 + S 1e-10): rgb_map and acc move by at most eps, depth by eps max|z|.
    Returns raymarch_sparse's dict plus n_live (samples that went through the MLP) and n_stopped (rays stopped at some boundary).
    device_count (keyword, default False; it travels among **packed_alt because this function's named parameters are pinned): True is
    the march without a host read - every segment is enqueued with counted gather and MLP launches on its worst-case buffers, the per-segment counts
    are summed on the device and n_live / n_stopped are int32 device scalars; the other outputs have the same bits.  Not under the bf16-family modes
    (NotImplementedError)."""
    device_count = bool(packed_alt.pop("device_count", False))
    if device_count:
        _device_count_mode(packed_alt.get("packed_bf16"), packed_alt.get("packed_split"), "raymarch_early_stop(device_count=True)")
    eps, G = _early_stop_args(eps, stop_every, "raymarch_early_stop")
    if (density is None) != (thr is None):
        raise ValueError("raymarch_early_stop: density and thr are given together or not at all")
    _need_no_grad(vol_cl, imgs, rays_pts, rays_ndc, z_vals, rays_dir, density, op="raymarch_early_stop")
    if thr is not None:
        thr = _thr_f32(thr, "raymarch_early_stop")
    C = vol_cl.shape[-1]
    color_vol = C != 8
    F = C if color_vol else 8 + 4 * imgs.shape[0]
    if color_vol and C != 8 + 4 * w2cs.shape[0]:
        raise RuntimeError(f"raymarch_early_stop: the volume has {C} channels, 8 + 4V is {8 + 4 * w2cs.shape[0]}")
    N, S = z_vals.shape
    dev = rays_ndc.device
    mlp = _rows_mlp(packed, F, dev, **packed_alt)
    raw = torch.zeros((N, S, 4), device=dev, dtype=torch.float32)
    bounds = list(range(0, S, G)) + [S]
    ray_T = torch.ones((N,), device=dev, dtype=torch.float32) if len(bounds) > 2 else None
    # the two modes differ in how a segment's count reaches the stage and in how the counts are summed: Python ints read from the device, or int32
    # device scalars
    n_live, n_stopped = (torch.zeros((), device=dev, dtype=torch.int32) if device_count else 0), 0
    for k, (s0, s1) in enumerate(zip(bounds[:-1], bounds[1:])):
        count, idx, ndc_c, pts_c, dir_c = live_samples_range(density, rays_ndc, thr, s0, s1, ray_T if k else None, eps,
                                                             None if color_vol else rays_pts, rays_dir)
        if device_count:
            n, n_live = count, n_live + count[0]
        else:
            if s1 == S and ray_T is not None:       # the last segment: the stopped rays travel with its count, one host read
                n, n_stopped = torch.stack((count[0], (ray_T < eps).sum(dtype=torch.int32))).tolist()
            else:
                n = int(count.item())
            n_live += n
        _, raw_c = _compact_rows_mlp(vol_cl, imgs, w2cs, intrinsics, ndc_c, pts_c, dir_c, n, mlp)
        scatter_rows(raw_c, idx, count, raw.view(N * S, 4))
        if s1 < S:
            ray_transmittance(raw, s0, s1, ray_T)
    if device_count:
        n_stopped = torch.zeros((), device=dev, dtype=torch.int32) if ray_T is None else (ray_T < eps).sum(dtype=torch.int32)
    return _march_outputs(raw, composite(raw, z_vals, white_bkgd), want, n_live=n_live, n_stopped=n_stopped)


# ------------------------------------------------------------------ a density volume in the renderer's frame (csrc/occupancy.hip)
def _host_f32(t, n, name):
    """A camera tensor as a contiguous fp32 HOST tensor of at least n values (the C entry reads it during the call; a device tensor is copied once)."""
    h = torch.as_tensor(t).detach().to("cpu", torch.float32).contiguous()
    if h.numel() < n:
        raise RuntimeError(f"voxel_points: {name} must hold at least {n} values, got {tuple(h.shape)}")
    return h


def voxel_points(D, H, W, K_ref=None, c2w_ref=None, near_far=None, ref_hw=None, pad=0, lindisp=False, planes=None, device=None, out=None):
    """The nodes of planes [d0, d1) (planes=; default all) of a (D,H,W) volume, rows in [k][j][i] order (mvsnerf_voxel_points_fwd) -> (ndc (n,3), pts (n,3) |
    None): ndc = (i/(W-1), j/(H-1), k/(D-1)), the coordinates ops.volume_sample / ops.live_samples resolve to the node itself; pts, when the reference
    camera is given (K_ref (3,3), c2w_ref (4,4) | (3,4), near_far (2,), ref_hw = the reference view's (H_img, W_img), pad, lindisp as ops.ray_points takes
    them), the world positions ops.ray_points maps to those coordinates.  A box volume (MVSSystemFusion) has no camera: leave K_ref None.
    Camera tensors on the device are read back once per call (pass host tensors to a loop).  device: where the rows go (default: the camera's device, or the
    current GPU).  out: (ndc_all, pts_all | None) caller-owned (D*H*W,3) fp32 tensors; rows [d0*H*W, d1*H*W) of them are written, no other, and views
    of those rows are returned."""
    D, H, W = int(D), int(H), int(W)
    d0, d1 = (0, D) if planes is None else (int(planes[0]), int(planes[1]))
    with_pts = K_ref is not None
    if with_pts and (c2w_ref is None or near_far is None or ref_hw is None):
        raise RuntimeError("voxel_points: world positions need K_ref, c2w_ref, near_far and ref_hw together")
    if D < 1 or H < 1 or W < 1 or not 0 <= d0 <= d1 <= D:
        raise RuntimeError(f"voxel_points: planes [{d0}, {d1}) of a ({D},{H},{W}) volume")
    if device is None:
        device = K_ref.device if (torch.is_tensor(K_ref) and K_ref.is_cuda) else torch.device("cuda", torch.cuda.current_device())
    n, lo = (d1 - d0) * H * W, d0 * H * W
    if out is None:
        ndc = torch.empty((n, 3), device=device, dtype=torch.float32)
        pts = torch.empty((n, 3), device=device, dtype=torch.float32) if with_pts else None
    else:
        if tuple(out[0].shape) != (D * H * W, 3) or (with_pts and (out[1] is None or tuple(out[1].shape) != (D * H * W, 3))):
            raise RuntimeError(f"voxel_points: out must hold ({D * H * W},3) tensors")
        dev_f32(out[0], "voxel_points: out[0]")
        ndc = out[0][lo:lo + n]
        pts = None
        if with_pts:
            dev_f32(out[1], "voxel_points: out[1]")
            pts = out[1][lo:lo + n]
    cam = (0, 0, 0, 0, 0)
    if with_pts:
        hK, hc, hn = _host_f32(K_ref, 9, "K_ref"), _host_f32(c2w_ref, 12, "c2w_ref"), _host_f32(torch.as_tensor(near_far).reshape(-1), 2, "near_far")
        cam = (hK.data_ptr(), hc.data_ptr(), hn.data_ptr(), int(ref_hw[1]), int(ref_hw[0]))
    if n:               # an empty plane range has no row to write (and an empty tensor no address to hand over)
        check(_lib.lib().mvsnerf_voxel_points_fwd(D, H, W, d0, d1, *cam, int(pad), int(bool(lindisp)), ndc.data_ptr(), 0 if pts is None else pts.data_ptr(),
                                                  stream_ptr()), "voxel_points_fwd")
    return ndc, pts


def max_dilate3d(density, r):
    """(D,H,W) fp32 -> the maximum over the (2r+1)^3 window clipped to the grid, r in {0, 1, 2} (mvsnerf_max_dilate3d_fwd); a NaN in the window gives NaN,
    r = 0 is a copy.  A new tensor: the input is never written."""
    _need_no_grad(density, op="max_dilate3d")
    r = int(r)
    if density.dim() != 3:
        raise RuntimeError(f"max_dilate3d: density must be (D,H,W), got {tuple(density.shape)}")
    if r not in (0, 1, 2):
        raise ValueError(f"max_dilate3d: r must be 0, 1 or 2, got {r}")
    D, H, W = density.shape
    c = _Keep()
    src = c(density, "density")
    out = torch.empty((D, H, W), device=density.device, dtype=torch.float32)
    ws = torch.empty((D, H, W), device=density.device, dtype=torch.float32) if r else None
    check(_lib.lib().mvsnerf_max_dilate3d_fwd(src, D, H, W, r, out.data_ptr(), 0 if ws is None else ws.data_ptr(), stream_ptr()), "max_dilate3d_fwd")
    return out


def node_density(vol_cl, packed, w2cs, imgs=None, intrinsics=None, camera=None, dilate=0, planes_per_call=8, **packed_alt):
    """The sigma the renderer's kernels give AT the nodes of the volume they render from -> (D,H,W) fp32: per slab of planes_per_call planes
    voxel_points -> ops.gather (8-channel volume + source images: imgs (V,3,IH,IW) un-normalised, w2cs (V,4,4), intrinsics (V,3,3), and camera =
    dict(K_ref, c2w_ref, near_far, ref_hw, pad[, lindisp]) of the reference view, for the world positions the colour lookup projects) or
    ops.gather_colorvol ((8+4V)-channel volume: no images, no camera, the coordinates may be a box's) on the node rows as (n,1,3) without a view
    direction -> ops.mlp_forward(alpha_only=True) into the slab of the result; then max_dilate3d(dilate) when dilate > 0.  The lookups and the MLP entry
    are the ray march's (ops.raymarch_sparse runs the same two on its live rows), so density[k,j,i] is the sigma-only output a sample ON node (k,j,i)
    gets; net_type v2 has no ReLU on it, as forward_alpha has none.  packed / **packed_alt: MVSNeRF.packed / packed_alt (the kernel choice).
    The slab loop bounds the workspace (8 planes of a 128 x 176 x 208 volume are 293 k rows of 8+4V features); the result does not depend on it."""
    _need_no_grad(vol_cl, imgs, w2cs, intrinsics, op="node_density")
    dilate, step = int(dilate), int(planes_per_call)
    if dilate not in (0, 1, 2):
        raise ValueError(f"node_density: dilate must be 0, 1 or 2, got {dilate}")
    if step < 1:
        raise ValueError(f"node_density: planes_per_call must be >= 1, got {planes_per_call}")
    if vol_cl.dim() != 4:
        raise RuntimeError(f"node_density: vol_cl must be (D,H,W,C) (ops.channels_last_volume), got {tuple(vol_cl.shape)}")
    D, H, W, C = vol_cl.shape
    color_vol = C != 8
    if color_vol:
        if C != 8 + 4 * w2cs.shape[0]:
            raise RuntimeError(f"node_density: the volume has {C} channels, 8 + 4V is {8 + 4 * w2cs.shape[0]}")
        F, cam = C, {}
    else:
        if imgs is None or intrinsics is None or camera is None:
            raise RuntimeError("node_density: an 8-channel volume needs imgs, intrinsics and camera= (the reference view) for the colour lookup")
        F = 8 + 4 * imgs.shape[0]
        cam = dict(K_ref=_host_f32(camera["K_ref"], 9, "K_ref"), c2w_ref=_host_f32(camera["c2w_ref"], 12, "c2w_ref"),
                   near_far=_host_f32(torch.as_tensor(camera["near_far"]).reshape(-1), 2, "near_far"), ref_hw=camera["ref_hw"],
                   pad=int(camera.get("pad", 0)), lindisp=bool(camera.get("lindisp", False)))
    dev = vol_cl.device
    density = torch.empty((D, H, W), device=dev, dtype=torch.float32)
    for d0 in range(0, D, step):
        d1 = min(d0 + step, D)
        n = (d1 - d0) * H * W
        ndc, pts = voxel_points(D, H, W, planes=(d0, d1), device=dev, **cam)
        ndc = ndc.view(n, 1, 3)
        if color_vol:
            feat, _ = gather_colorvol(vol_cl, ndc)
        else:
            feat, _ = gather(vol_cl, imgs, w2cs, intrinsics, pts.view(n, 1, 3), ndc)
        raw = mlp_forward(packed, F, ndc.data_ptr(), 3, feat.data_ptr(), F, 0, 3, n, 1, 1, dev, **packed_alt)
        density[d0:d1].copy_(raw.view(d1 - d0, H, W))
    return max_dilate3d(density, dilate) if dilate else density


# ------------------------------------------------------------------ training path (autograd)
def _act_n(q, h):
    return (q >> 4) * 32 + (q & 3) + 8 * ((q & 15) >> 2) + 4 * h


_maps_cache = {}


def _mlp_bwd_maps(F, device):
    """int32 table: fragment row -> nn.Linear row/column (layout documented at mvsnerf_mlp_bwd in csrc/mlp_bwd.hip)."""
    key = (F, str(device))
    if key in _maps_cache:
        return _maps_cache[key]
    import numpy as np
    t = -np.ones(1376, dtype=np.int32)
    act128 = np.array([_act_n(r >> 1, r & 1) for r in range(128)], dtype=np.int32)
    act64 = act128[:64].copy()
    pe = np.array([(r & 1) if (r >> 1) == 0 else ((2 if (r & 1) == 0 else -1) if (r >> 1) == 1 else 3 + ((r >> 1) - 2) + 30 * (r & 1))
                   for r in range(64)], dtype=np.int32)
    feat = np.array([((r & 1) * (F // 2) + (r >> 1)) if (r >> 1) < F // 2 else -1 for r in range(32)], dtype=np.int32)
    t[0:128], t[128:192], t[192:256], t[320:352] = act128, act64, pe, feat
    t[512:515] = [0, 1, 2]
    t[547] = 0
    t[576:640], t[640:768] = pe, 63 + act128
    t[768:896] = act128
    t[896:899] = [128, 129, 130]
    t[928:992] = act64
    t[1184:1312] = act128
    # F > 32: the pts_bias weight gradient contracts over [S_FV (16 slots) | the S_DR block, whose slots 2..5 hold feature operands 16..19]
    t[1312:1344] = feat
    t[1344:1376] = [((r & 1) * (F // 2) + 14 + (r >> 1)) if 2 <= (r >> 1) < 6 and 14 + (r >> 1) < F // 2 else -1 for r in range(32)]
    out = torch.from_numpy(t).to(device)
    _maps_cache[key] = out
    return out


def mlp_pack_bwd_bf16(weights, F):
    _need_narrow(weights, "mlp_pack_bwd_bf16")
    n = _lib.lib().mvsnerf_mlp_packed_bwd_bf16_elems()
    packed = torch.empty(n, device=weights[0].device, dtype=torch.bfloat16)
    wp = _Ptr11(*[dev_f32(w, "weight") for w in weights])
    check(_lib.lib().mvsnerf_mlp_pack_bwd_bf16(wp, F, packed.data_ptr(), stream_ptr()), "mlp_pack_bwd_bf16")
    return packed


def mlp_pack_bwd(weights, F):
    _need_narrow(weights, "mlp_pack_bwd")
    n = _lib.lib().mvsnerf_mlp_packed_bwd_floats()
    packed = torch.empty(n, device=weights[0].device, dtype=torch.float32)
    wp = _Ptr11(*[dev_f32(w, "weight") for w in weights])
    check(_lib.lib().mvsnerf_mlp_pack_bwd(wp, F, packed.data_ptr(), stream_ptr()), "mlp_pack_bwd")
    return packed


_BwdSetup = collections.namedtuple("_BwdSetup", "grads packed_bwd gslots ws maps gwp gbp g_in g_ptr")


def _bwd_setup(mlp_params, F, bf16, n_points, g_in, dev):
    """What both ray-march backwards hold before their MLP stage on n_points points: grads (the 22 gradient tensors, in mlp_params' order), packed_bwd
    (the weight re-pack for the transposed products), gslots, ws, maps, the pointer arrays gwp / gbp into grads, and g_in with g_ptr - the incoming
    gradients, contiguous and kept alive until the launch, and their addresses (0 for None).  n_points = 0: grads only, every other field None."""
    _cl_cache.pop("last", None)              # do not keep the step's volume storage past its backward (channels_last_volume)
    # 22 gradient tensors of their own, zeroed by ONE multi-tensor launch.  (They used to be views of one zero-filled buffer: autograd's
    # AccumulateGrad clones a gradient that does not own its storage - 22 device copies per step in the kernel trace.)
    grads = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in mlp_params]
    torch._foreach_zero_(grads)
    if not n_points:
        return _BwdSetup(grads, *[None] * 8)
    lib = _lib.lib()
    f32 = dict(device=dev, dtype=torch.float32)
    g_in = [None if g is None else g.contiguous() for g in g_in]
    weights = [p.detach() for p in mlp_params[0::2]]
    return _BwdSetup(grads, mlp_pack_bwd_bf16(weights, F) if bf16 else mlp_pack_bwd(weights, F),
                     torch.empty(lib.mvsnerf_mlp_gradslot_floats(n_points) // (2 if bf16 else 1), **f32),
                     torch.empty(lib.mvsnerf_mlp_bwd_workspace_floats(), **f32), _mlp_bwd_maps(F, dev),
                     _Ptr11(*[g.data_ptr() for g in grads[0::2]]), _Ptr11(*[g.data_ptr() for g in grads[1::2]]),
                     g_in, [0 if g is None else dev_f32(g, "grad") for g in g_in])


class RayMarchFunction(torch.autograd.Function):
    """rendering() (renderer.py:138-165) with gradients to the neural volume and the 22 MLP tensors.
    Inputs that never carry gradients in the reference's losses (rays, source images, cameras) are not differentiated."""

    @staticmethod
    def forward(ctx, volume, imgs, w2cs, intrinsics, rays_pts, rays_ndc, z_vals, rays_dir, white_bkgd, packed, dp_samples, *mlp_params):
        """ONE FFI call (mvsnerf_raymarch_train_fwd): lookups -> MLP training forward with activation store -> compositing."""
        _need_narrow(packed, "raymarch_train")
        lib = _lib.lib()
        vol_cl = channels_last_volume(volume)
        D, H, W, C = vol_cl.shape
        N, S = z_vals.shape
        V = imgs.shape[0]
        F = 8 + 4 * V
        if C not in (8, F):
            raise RuntimeError(f"ray march: the volume has {C} channels; expected 8 or 8 + 4V = {F}")
        bf16 = training_mlp_mode() == "bf16"            # 'fp32' or 'bf16': _train_entry has refused every other mode
        dev = rays_pts.device
        f32 = dict(device=dev, dtype=torch.float32)
        feat = torch.empty((N, S, F), **f32)
        raw = torch.empty((N, S, 4), **f32)
        saved = torch.empty(lib.mvsnerf_mlp_saved_floats(N * S) // (2 if bf16 else 1), **f32)      # bf16 mode: two-byte slots
        dirs = torch.empty((N, 3), **f32)
        rgb, disp, acc, depth = (torch.empty(sh, **f32) for sh in ((N, 3), (N,), (N,), (N,)))
        weights, alpha = torch.empty((N, S), **f32), torch.empty((N, S), **f32)
        packed_b = mlp_pack_bf16([p.detach() for p in mlp_params[0::2]], F) if bf16 else None
        icl = channels_last_images(imgs) if C == 8 else None
        vp, vl = vol_ptr_layout(vol_cl)
        a = _lib.RaymarchTrainArgs(
            vol=vp, vol_layout=vl, D=D, H=H, W=W, C=C,
            imgs_nhwc4=0 if icl is None else icl.data_ptr(), V=V, IH=imgs.shape[2], IW=imgs.shape[3],
            w2c=dev_f32(w2cs, "w2cs"), K=dev_f32(intrinsics, "intrinsics"), packed_mlp=packed.data_ptr(),
            packed_mlp_bf16=0 if packed_b is None else packed_b.data_ptr(), bf16=int(bf16),
            rays_pts=dev_f32(rays_pts, "rays_pts"), rays_ndc=dev_f32(rays_ndc, "rays_ndc"), z_vals=dev_f32(z_vals, "z_vals"),
            rays_dir=dev_f32(rays_dir, "rays_dir"), N=N, S=S, white_bkgd=int(bool(white_bkgd)),
            dirs_tmp=dirs.data_ptr(), input_feat=feat.data_ptr(), raw=raw.data_ptr(), saved=saved.data_ptr(),
            rgb_map=rgb.data_ptr(), disp=disp.data_ptr(), acc=acc.data_ptr(), weights=weights.data_ptr(), depth=depth.data_ptr(), alpha=alpha.data_ptr())
        check(lib.mvsnerf_raymarch_train_fwd(ctypes.byref(a), stream_ptr()), "raymarch_train_fwd")
        ctx.save_for_backward(rays_ndc, z_vals, raw, saved, packed, *mlp_params)
        ctx.meta = (tuple(volume.shape), (D, H, W, C), N, S, F, bool(white_bkgd), bf16, bool(dp_samples))
        ctx.mark_non_differentiable(feat, raw)
        return rgb, feat, weights, depth, alpha, raw

    @staticmethod
    def backward(ctx, g_rgb, g_feat, g_weights, g_depth, g_alpha, g_raw):
        """The weight re-pack for the transposed products + ONE FFI call (mvsnerf_raymarch_bwd): compositing backward -> MLP data and
        weight gradients -> trilinear scatter into the volume gradient."""
        rays_ndc, z_vals, raw, saved, packed, *mlp_params = ctx.saved_tensors
        vshape, (D, H, W, C), N, S, F, white, bf16, dp_samples = ctx.meta
        f32 = dict(device=raw.device, dtype=torch.float32)
        b = _bwd_setup(mlp_params, F, bf16, N * S, (g_rgb, g_depth, g_weights, g_alpha), raw.device)
        d_raw = torch.empty((N, S, 4), **f32)
        d_feat = torch.empty((N * S, C), **f32)         # C = 8: the volume features only; C = F: the colour volume is a parameter too
        gvol_cl = torch.zeros((D, H, W, C), **f32) if ctx.needs_input_grad[0] else None
        # The call scatters into the volume gradient itself unless the scatter has to run behind it (_volume_grad): on the sample gradients of all
        # ranks (data-parallel fine-tuning), or through the fixed-point accumulators of VOLUME_BWD_DETERMINISTIC (mvsnerf_volume_sample_bwd_det)
        in_call = gvol_cl is not None and not (_exchange_samples(dp_samples) or VOLUME_BWD_DETERMINISTIC)
        a = _lib.RaymarchBwdArgs(
            packed_mlp=packed.data_ptr(), packed_bwd=b.packed_bwd.data_ptr(), bf16=int(bf16), F=F,
            raw=raw.data_ptr(), saved=saved.data_ptr(), z_vals=z_vals.data_ptr(), rays_ndc=rays_ndc.data_ptr(), N=N, S=S, white_bkgd=int(white),
            g_rgb=b.g_ptr[0], g_depth=b.g_ptr[1], g_weights=b.g_ptr[2], g_alpha=b.g_ptr[3],
            d_raw=d_raw.data_ptr(), gslots=b.gslots.data_ptr(), d_feat=d_feat.data_ptr(), n_feat_out=C,
            gw=ctypes.cast(b.gwp, ctypes.POINTER(ctypes.c_void_p)), gb=ctypes.cast(b.gbp, ctypes.POINTER(ctypes.c_void_p)),
            maps=b.maps.data_ptr(), workspace=b.ws.data_ptr(),
            gvol=gvol_cl.data_ptr() if in_call else 0, D=D, H=H, W=W, C=C)
        check(_lib.lib().mvsnerf_raymarch_bwd(ctypes.byref(a), stream_ptr()), "raymarch_bwd")
        g_vol = _volume_grad(gvol_cl, d_feat, rays_ndc.reshape(-1, 3), dp_samples, vshape, have_rows=not in_call)
        return (g_vol, None, None, None, None, None, None, None, None, None, None, *b.grads)


VOLUME_BWD_DETERMINISTIC = False   # True: the volume gradient's scatter through 64-bit fixed-point accumulators (mvsnerf_volume_sample_bwd_det; integer atomics
                                   # commute: one call gives the same bits in whatever order its rows arrive, so two runs are bit-identical) - two extra passes and
                                   # 8 bytes of zeroed workspace per volume element (300 MB at config 2) instead of float atomics.  N ranks: for a zeroed gvol,
                                   # volume_grad_from_all_ranks gives every rank the bits of ONE scatter call on all ranks' rows, divided by world


def _scatter_hip(gvol_cl, ndc, g):
    D, H, W, C = gvol_cl.shape
    lib = _lib.lib()
    if VOLUME_BWD_DETERMINISTIC:
        ws = torch.zeros(lib.mvsnerf_volume_sample_bwd_det_workspace_words(D, H, W, C), device=gvol_cl.device, dtype=torch.int64)
        check(lib.mvsnerf_volume_sample_bwd_det(D, H, W, C, ndc.data_ptr(), ndc.shape[0], g.data_ptr(), g.shape[-1], gvol_cl.data_ptr(), ws.data_ptr(), stream_ptr()),
              "volume_sample_bwd_det")
        return
    check(lib.mvsnerf_volume_sample_bwd(D, H, W, C, ndc.data_ptr(), ndc.shape[0], g.data_ptr(), C, gvol_cl.data_ptr(), stream_ptr()), "volume_sample_bwd")


def volume_grad_from_gathered_rows(allrows, cnts, width, gvol_cl, scatter=_scatter_hip):
    """The part of volume_grad_from_all_ranks behind its collectives, a pure function of the gathered buffer: allrows (world * width, C + 4) holds rank r's
    rows [d_feat (C) | ndc (3) | pad] at [r * width, r * width + cnts[r]).  ONE `scatter` call on the concatenation of the ranks' valid rows in rank order,
    then gvol_cl /= world.  One call, so that under VOLUME_BWD_DETERMINISTIC there is one fixed-point scale, one rounding per contribution and one workspace
    whatever the number of ranks: for a zeroed gvol_cl the result is the single-call scatter of all ranks' rows, divided by world, bit for bit and whatever
    the order of the shards.  With float atomics it is that value to their summation-order noise."""
    C = gvol_cl.shape[-1]
    world = len(cnts)
    if all(n == width for n in cnts):
        rows = allrows
    else:
        rows = torch.cat([allrows[r * width:r * width + n] for r, n in enumerate(cnts)])
    if rows.shape[0]:
        scatter(gvol_cl, rows[:, C:C + 3].contiguous(), rows[:, :C].contiguous())     # `scatter` is replaceable so that the CPU (gloo) tests can drive this exchange
    gvol_cl.div_(world)
    return gvol_cl


def volume_grad_from_all_ranks(d_feat, ndc, gvol_cl, group=None, scatter=_scatter_hip):
    """Data-parallel gradient of a learnable RefVolume WITHOUT reducing the volume-sized tensor (SURVEY.md 5 / 8e "Fine-tune").

    The volume gradient is the trilinear scatter of the per-sample feature gradients d_feat (P_local x C).  A dense all-reduce of it moves
    2 x (world-1)/world x 150-246 MB per rank and step over xGMI; the SAMPLE gradients of all ranks are 36 B + 12 B (NDC) per sample -
    6 MB for 1024 x 128 samples in total.  So: ONE all_gather of the counts and ONE of the [d_feat | ndc] rows, then every rank scatters the
    samples of ALL ranks into its own gradient volume in one call (volume_grad_from_gathered_rows; 0.16 ms for 131 072 samples) and scales by
    1/world - the same mean-over-ranks FlatGradAllReduce gives the other parameters.  Every rank ends with the full gradient; the volume
    parameter takes no part in the flat all-reduce.

    For a zeroed gvol_cl the result equals the single-call scatter of all ranks' rows (rank order) divided by world.  Under
    VOLUME_BWD_DETERMINISTIC that holds bit for bit, so the replicas agree with each other and with one rank that holds every row.  With the
    float-atomic scatter it holds to the atomics' summation-order noise, so replicas can differ in the last bits; MVSSystemFinetune
    re-broadcasts the volume from rank 0 every `args.dp_volume_resync` steps."""
    import torch.distributed as dist
    from . import distributed as DD
    C = d_feat.shape[1]
    P = d_feat.shape[0]
    world = dist.get_world_size(group)
    # shards may differ by one ray: gather the counts, pad to the largest
    cnt = torch.tensor([P], device=d_feat.device, dtype=torch.int64)
    cnts = torch.empty(world, device=d_feat.device, dtype=torch.int64)
    DD.all_gather_into_tensor(cnts, cnt, group=group)
    cnts = [int(c) for c in cnts.tolist()]
    width = max(cnts)
    row = torch.zeros((width, C + 4), device=d_feat.device, dtype=torch.float32)          # [d_feat (C) | ndc (3) | pad] -> 16-byte rows
    row[:P, :C] = d_feat
    row[:P, C:C + 3] = ndc
    allrows = torch.empty((world * width, C + 4), device=d_feat.device, dtype=torch.float32)
    DD.all_gather_into_tensor(allrows, row, group=group)
    return volume_grad_from_gathered_rows(allrows, cnts, width, gvol_cl, scatter)


def _exchange_samples(dp_samples):
    """dp_samples with a collective to run: the volume scatter runs on the sample gradients of ALL ranks (volume_grad_from_all_ranks)."""
    from . import distributed as DD
    return bool(dp_samples) and DD._collective_needed()


def _volume_grad(gvol_cl, d_feat, ndc_rows, dp_samples, vshape, have_rows, scatter=_scatter_hip):
    """The end of both ray-march backwards: gvol_cl (D,H,W,C; None: the volume takes no gradient, and None is returned) in the caller's layout -
    (C,D,H,W), or (1,C,D,H,W) for a five-entry vshape - after the rows d_feat (P,C) at ndc_rows (P,3) have been scattered into it when have_rows.
    Under dp_samples with a collective to run that is volume_grad_from_all_ranks, which a rank without rows enters with one row that scatters zeros;
    otherwise `scatter` (replaceable for the CPU tests), and without rows nothing is left to do: mvsnerf_raymarch_bwd scattered inside the call."""
    if gvol_cl is None:
        return None
    if _exchange_samples(dp_samples):
        if not have_rows:
            d_feat, ndc_rows = gvol_cl.new_zeros((1, gvol_cl.shape[-1])), gvol_cl.new_zeros((1, 3))
        volume_grad_from_all_ranks(d_feat, ndc_rows, gvol_cl, scatter=scatter)
    elif have_rows:
        scatter(gvol_cl, ndc_rows, d_feat)
    g_vol = gvol_cl.permute(3, 0, 1, 2)
    return g_vol.unsqueeze(0) if len(vshape) == 5 else g_vol


def _train_entry(net, views, op):
    """(the 22 MLP tensors as [weight, bias] * 11 in MLP_ORDER, net.packed(8 + 4V)) of a differentiable ray march, V = views.shape[0], after the refusals
    that come before anything is packed or launched: netwidth 256, a precision mode training does not run; net.packed refuses net_type v2 under bf16."""
    if getattr(net.nerf, "W", 128) != 128:
        raise _wide_refusal(op)
    if training_mlp_mode() not in ("fp32", "bf16"):
        raise RuntimeError(f"training runs the MLP in 'fp32' or 'bf16' (ops.set_mlp_precision), not {MLP_PRECISION!r}")
    params = [t for l in net.nerf._linears() for t in (l.weight, l.bias)]
    return params, net.packed(8 + 4 * views.shape[0])


def raymarch_train(volume, imgs, w2cs, intrinsics, net, rays_pts, rays_ndc, z_vals, rays_dir, white_bkgd=False, dp_samples=False):
    """Differentiable rendering(): `net` is a models.MVSNeRF; returns the dict of ops.raymarch.
    dp_samples: data-parallel volume gradient by exchanging sample gradients (volume_grad_from_all_ranks)."""
    params, packed = _train_entry(net, imgs, "raymarch_train")
    rgb, feat, weights, depth, alpha, raw = RayMarchFunction.apply(
        volume, imgs, w2cs, intrinsics, rays_pts, rays_ndc, z_vals, rays_dir, white_bkgd, packed, dp_samples, *params)
    return {"rgb_map": rgb, "input_feat": feat, "weights": weights, "depth": depth, "alpha": alpha, "raw": raw}


class SparseRayMarchFunction(torch.autograd.Function):
    """RayMarchFunction with the radiance MLP - training forward, data gradient, weight gradients - run on the LIVE samples only (ops.live_samples
    of `density` at `thr`).  A dead sample's raw is the constant (0,0,0,0): it hands no gradient to the MLP or the volume, and the live
    rows' gradients are those of "dense compositing with the dead rows zeroed".  The stages are the stable-tier entries RayMarchFunction's two calls
    chain, with N = n_live, S = 1, between live_samples / expand_rows (forward) and compact_rows (backward)."""

    @staticmethod
    def forward(ctx, volume, imgs, w2cs, intrinsics, rays_pts, rays_ndc, z_vals, rays_dir, density, thr, white_bkgd, packed, dp_samples, *mlp_params):
        """_sparse_march on mvsnerf_mlp_fwd_train (mvsnerf_mlp_fwd_bf16_train under training_mlp_mode() == "bf16"), its activation store sized for the live points."""
        _need_narrow(packed, "raymarch_sparse_train")
        lib = _lib.lib()
        vol_cl = channels_last_volume(volume)
        D, H, W, C = vol_cl.shape
        N, S = z_vals.shape
        F = 8 + 4 * w2cs.shape[0]
        if C not in (8, F):
            raise RuntimeError(f"ray march: the volume has {C} channels; expected 8 or 8 + 4V = {F}")
        bf16 = training_mlp_mode() == "bf16"
        f32 = dict(device=rays_ndc.device, dtype=torch.float32)
        kept = []

        def mlp(ndc_l, feat, dirs, n_live):
            raw_c = torch.empty((n_live, 4), **f32)
            saved = torch.empty(lib.mvsnerf_mlp_saved_floats(n_live) // (2 if bf16 else 1), **f32)      # per LIVE point; bf16 mode: two-byte slots
            kept.append(saved)
            io = (F, ndc_l.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, n_live, 1, raw_c.data_ptr(), saved.data_ptr(), stream_ptr())
            if bf16:
                packed_b = mlp_pack_bf16([p.detach() for p in mlp_params[0::2]], F)
                check(lib.mvsnerf_mlp_fwd_bf16_train(packed_b.data_ptr(), packed.data_ptr(), *io), "mlp_fwd_bf16_train")
            else:
                check(lib.mvsnerf_mlp_fwd_train(packed.data_ptr(), *io), "mlp_fwd_train")
            return raw_c
        (idx, count, ndc_l, raw_c, raw, n_live), (rgb, _, _, weights, depth, alpha) = _sparse_march(
            vol_cl, imgs, w2cs, intrinsics, rays_pts, rays_ndc, z_vals, rays_dir, density, thr, white_bkgd, mlp)
        saved = kept[0] if kept else raw_c              # no live sample: nothing is stored, the backward reads nothing
        ctx.save_for_backward(z_vals, raw, raw_c, ndc_l, idx, count, packed, saved, *mlp_params)
        ctx.meta = (tuple(volume.shape), (D, H, W, C), N, S, F, bool(white_bkgd), bf16, bool(dp_samples), n_live)
        ctx.mark_non_differentiable(raw)
        return rgb, weights, depth, alpha, raw, n_live

    @staticmethod
    def backward(ctx, g_rgb, g_weights, g_depth, g_alpha, g_raw, _g_n_live):
        """mvsnerf_composite_bwd on the dense raw -> compact_rows to (n_live,4) -> the MLP backward on the live rows -> the volume scatter on the
        compact NDC rows (_volume_grad: float atomics, VOLUME_BWD_DETERMINISTIC, or volume_grad_from_all_ranks under dp_samples).  Without a live
        sample none of these is launched and every gradient is zero."""
        lib = _lib.lib()
        z_vals, raw, raw_c, ndc_l, idx, count, packed, saved, *mlp_params = ctx.saved_tensors
        vshape, (D, H, W, C), N, S, F, white, bf16, dp_samples, n_live = ctx.meta
        f32 = dict(device=raw.device, dtype=torch.float32)
        b = _bwd_setup(mlp_params, F, bf16, n_live, (g_rgb, g_depth, g_weights, g_alpha), raw.device)
        gvol_cl = torch.zeros((D, H, W, C), **f32) if ctx.needs_input_grad[0] else None
        d_feat = torch.empty((n_live, C), **f32)
        if n_live:
            d_raw = torch.empty((N * S, 4), **f32)
            check(lib.mvsnerf_composite_bwd(raw.data_ptr(), z_vals.data_ptr(), N, S, int(white), b.g_ptr[0], b.g_ptr[1], 0, b.g_ptr[2], b.g_ptr[3],
                                            d_raw.data_ptr(), stream_ptr()), "composite_bwd")
            d_raw_c = compact_rows(d_raw, idx, count, n_live)
            fn = lib.mvsnerf_mlp_bwd_bf16 if bf16 else lib.mvsnerf_mlp_bwd
            check(fn(packed.data_ptr(), b.packed_bwd.data_ptr(), F, raw_c.data_ptr(), d_raw_c.data_ptr(), saved.data_ptr(), n_live, 1, b.gslots.data_ptr(),
                     d_feat.data_ptr(), C, b.gwp, b.gbp, b.maps.data_ptr(), b.ws.data_ptr(), stream_ptr()), "mlp_bwd_bf16" if bf16 else "mlp_bwd")
        g_vol = _volume_grad(gvol_cl, d_feat, ndc_l, dp_samples, vshape, have_rows=bool(n_live))
        return (g_vol, None, None, None, None, None, None, None, None, None, None, None, None, *b.grads)


def raymarch_sparse_train(volume, imgs, w2cs, intrinsics, net, rays_pts, rays_ndc, z_vals, rays_dir, density, thr, white_bkgd=False, dp_samples=False):
    """Differentiable rendering() with empty space skipped: ops.raymarch_train's step with the MLP - training forward, data gradient and
    the weight-gradient GEMMs - run on the samples that ops.live_samples(density, rays_ndc, thr) calls live.  `net` is a models.MVSNeRF (netwidth
    128); volume (1,C,D,H,W) | (C,D,H,W) with C = 8 (imgs (V,3,H,W), w2cs (V,4,4), intrinsics (V,3,3) for the colour lookup) or C = 8 + 4V (a colour
    volume: imgs / intrinsics / rays_pts are not read); density (D',H',W') fp32.  The 22 MLP tensors and the volume receive gradients; rays, images,
    cameras and `density` do not.
    The forward is _sparse_march's sequence - ONE host read of the live count, the step's only synchronisation - and the backward
    SparseRayMarchFunction.backward's.  A dead sample's raw is the constant (0,0,0,0); with no live sample at all nothing but live_samples,
    expand_rows and the compositing is launched, and every gradient is zero.
    Returns a dict: rgb_map (N,3), weights (N,S), depth (N,), alpha (N,S), raw (N,S,4; not differentiable), n_live (int).  There is no input_feat:
    the dense (N,S,F) feature tensor is never formed."""
    thr = _thr_f32(thr, "raymarch_sparse_train")
    if not torch.is_tensor(density) or density.dim() != 3:
        raise RuntimeError(f"raymarch_sparse_train: density must be (D,H,W), got {tuple(getattr(density, 'shape', ()))}")
    params, packed = _train_entry(net, w2cs, "raymarch_sparse_train")
    rgb, weights, depth, alpha, raw, n_live = SparseRayMarchFunction.apply(
        volume, imgs, w2cs, intrinsics, rays_pts, rays_ndc, z_vals, rays_dir, density.detach(), thr, white_bkgd, packed, dp_samples, *params)
    return {"rgb_map": rgb, "weights": weights, "depth": depth, "alpha": alpha, "raw": raw, "n_live": n_live}


# ------------------------------------------------------------------ frame metrics
METRICS_ROW = 15                 # MVSNERF_METRICS_ROW of include/mvsnerf_hip_internal.h; the entries of a row:
(M_SSE, M_N, M_SSE_CROP, M_N_CROP, M_SSE_MASK, M_N_MASK, M_SSIM0, M_SSIM1, M_SSIM2, M_N_SSIM, M_ABS_ERR, M_ACC0, M_ACC1, M_ACC2, M_N_DEPTH) = range(METRICS_ROW)


def frame_metrics_workspace_bytes(K, H, W, win_size=7):
    return int(_lib.lib().mvsnerf_frame_metrics_workspace_bytes(K, H, W, win_size))


def frame_metrics(pred, gt, depth_pred=None, depth_gt=None, win_size=7, data_range=2.0, K1=0.01, K2=0.03, gt_scale=1.0 / 200.0,
                  thresholds=(0.01, 0.05, 0.1), out=None, workspace=None):
    """The evaluation record of K frames (mvsnerf_frame_metrics_fwd): pred, gt (K,H,W,3) or (H,W,3) on the GPU (fp32; contiguous, or copied to
    that on the device), depth_pred / depth_gt (K,H,W) or (H,W) or both None -> (K, METRICS_ROW) float64 on the GPU: sums and counts, see the M_* indices (a mean squared error is
    row[M_SSE] / (3 row[M_N])).  Two launches on the current stream, no host synchronisation.  out / workspace: caller-owned buffers of a loop
    ((K, METRICS_ROW) float64; at least frame_metrics_workspace_bytes(K, H, W, win_size) bytes of float64)."""
    _need_no_grad(pred, gt, depth_pred, depth_gt, op="frame_metrics")
    if not (torch.is_tensor(pred) and torch.is_tensor(gt)) or pred.shape != gt.shape or pred.dim() not in (3, 4) or pred.shape[-1] != 3:
        raise RuntimeError(f"frame_metrics: pred and gt must both be (K,H,W,3) or (H,W,3), got {tuple(getattr(pred, 'shape', ()))} and {tuple(getattr(gt, 'shape', ()))}")
    K = 1 if pred.dim() == 3 else int(pred.shape[0])
    H, W = int(pred.shape[-3]), int(pred.shape[-2])
    if (depth_pred is None) != (depth_gt is None):
        raise RuntimeError("frame_metrics: depth_pred and depth_gt come together")
    if depth_gt is not None and not (tuple(depth_pred.shape) == tuple(depth_gt.shape) == tuple(pred.shape[:-1])):
        raise RuntimeError(f"frame_metrics: depth_pred and depth_gt must be {tuple(pred.shape[:-1])}, got {tuple(depth_pred.shape)} and {tuple(depth_gt.shape)}")
    if len(thresholds) != 3:
        raise RuntimeError("frame_metrics: three depth thresholds")
    keep = _Keep()        # render_view's frame is a strided view of its (N,4) rgb + depth rows: such inputs are made contiguous on the device first
    ptrs = [keep(pred, "frame_metrics: pred"), keep(gt, "frame_metrics: gt")]
    ptrs += [0, 0] if depth_gt is None else [keep(depth_pred, "frame_metrics: depth_pred"), keep(depth_gt, "frame_metrics: depth_gt")]
    need = frame_metrics_workspace_bytes(K, H, W, win_size)
    if out is None:
        out = torch.empty((K, METRICS_ROW), device=pred.device, dtype=torch.float64)
    elif not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (K, METRICS_ROW) and out.device == pred.device):
        raise RuntimeError(f"frame_metrics: out must be a contiguous ({K},{METRICS_ROW}) float64 tensor on {pred.device}")
    if workspace is None:
        workspace = torch.empty((max(need, 8) // 8,), device=pred.device, dtype=torch.float64)
    elif not (workspace.is_cuda and workspace.dtype == torch.float64 and workspace.is_contiguous() and workspace.numel() * 8 >= need
              and workspace.device == pred.device):
        raise RuntimeError(f"frame_metrics: workspace must be a contiguous float64 tensor of at least {need} bytes on {pred.device}")
    thr = (ctypes.c_double * 3)(*[float(t) for t in thresholds])
    check(_lib.lib().mvsnerf_frame_metrics_fwd(*ptrs, K, H, W, int(win_size), float(data_range), float(K1), float(K2), float(gt_scale), thr,
                                               out.data_ptr(), workspace.data_ptr(), stream_ptr()), "frame_metrics_fwd")
    return out


# ------------------------------------------------------------------ LPIPS-VGG layers (csrc/lpips.hip; evaluate.LPIPS strings them together)
def lpips_conv_packed_floats(Cin, Cout):
    """Floats of one packed conv layer (weights in MFMA fragment order, then the bias); 0 for a (Cin, Cout) the kernels do not carry.  No GPU needed."""
    return int(_lib.lib().mvsnerf_lpips_conv_packed_floats(int(Cin), int(Cout)))


def lpips_head_workspace_bytes(K, h, w, C):
    return int(_lib.lib().mvsnerf_lpips_head_workspace_bytes(int(K), int(h), int(w), int(C)))


def _lpips_act(x, name, C=None):
    if not (torch.is_tensor(x) and x.dim() == 4 and (C is None or x.shape[-1] == C)):
        raise RuntimeError(f"{name}: expected a (N,H,W,{'C' if C is None else C}) tensor, got {tuple(getattr(x, 'shape', ()))}")
    dev_f32(x, name)
    return tuple(int(s) for s in x.shape)


def lpips_conv_pack(weight, bias):
    """weight (Cout,Cin,3,3), bias (Cout,) on the GPU -> the packed layer of lpips_conv.  (Cin, Cout) = (3, 64) or both in {64,128,256,512}."""
    _need_no_grad(weight, bias, op="lpips_conv_pack")
    if not (torch.is_tensor(weight) and weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3) and torch.is_tensor(bias) and tuple(bias.shape) == (weight.shape[0],)):
        raise RuntimeError(f"lpips_conv_pack: weight (Cout,Cin,3,3) and bias (Cout,), got {tuple(getattr(weight, 'shape', ()))} and {tuple(getattr(bias, 'shape', ()))}")
    Cout, Cin = int(weight.shape[0]), int(weight.shape[1])
    n = lpips_conv_packed_floats(Cin, Cout)
    if n == 0:
        raise RuntimeError(f"lpips_conv_pack: no kernel for a 3x3 convolution {Cin} -> {Cout}")
    keep = _Keep()
    pw, pb = keep(weight, "lpips_conv_pack: weight"), keep(bias, "lpips_conv_pack: bias")
    packed = torch.empty((n,), device=weight.device, dtype=torch.float32)
    check(_lib.lib().mvsnerf_lpips_conv_pack(pw, pb, Cin, Cout, packed.data_ptr(), stream_ptr()), "lpips_conv_pack")
    return packed


def lpips_conv(x, packed, Cout):
    """conv3x3 + bias + ReLU (stride 1, zero padding 1) of a channel-last (N,H,W,Cin) fp32 tensor -> (N,H,W,Cout).  Cin == 3 is conv1_1: x is an image in
    [0,1] and the kernel's loader applies LPIPS's scaling layer to it (padding stays 0 after the scaling)."""
    _need_no_grad(x, packed, op="lpips_conv")
    N, H, W, Cin = _lpips_act(x, "lpips_conv: x")
    if lpips_conv_packed_floats(Cin, Cout) == 0 or not torch.is_tensor(packed) or packed.numel() != lpips_conv_packed_floats(Cin, Cout):
        raise RuntimeError(f"lpips_conv: packed does not hold a {Cin} -> {Cout} layer")
    out = torch.empty((N, H, W, int(Cout)), device=x.device, dtype=torch.float32)
    check(_lib.lib().mvsnerf_lpips_conv_fwd(x.data_ptr(), dev_f32(packed, "lpips_conv: packed"), N, H, W, Cin, int(Cout), out.data_ptr(), stream_ptr()),
          "lpips_conv_fwd")
    return out


def lpips_pool(x):
    """maxpool 2x2 / stride 2, floor mode, of a channel-last (N,H,W,C) fp32 tensor -> (N,H//2,W//2,C)."""
    _need_no_grad(x, op="lpips_pool")
    N, H, W, C = _lpips_act(x, "lpips_pool: x")
    out = torch.empty((N, H // 2, W // 2, C), device=x.device, dtype=torch.float32)
    check(_lib.lib().mvsnerf_lpips_pool_fwd(x.data_ptr(), N, H, W, C, out.data_ptr(), stream_ptr()), "lpips_pool_fwd")
    return out


def lpips_head(f0, f1, lin, layer_out=None, total=None, accumulate=False):
    """One LPIPS tap layer: f0, f1 (K,h,w,C) fp32, lin (C,) -> layer_out (K,) float64 on the GPU, the frame means of
    sum_c lin_c (f0_c / n0 - f1_c / n1)^2 with n = sqrt(sum_c f_c^2) + 1e-10.  total (K,) float64, if given, receives the value too (accumulate=False) or has it
    added.  Two launches, no atomics, no host synchronisation."""
    _need_no_grad(f0, f1, lin, op="lpips_head")
    K, h, w, C = _lpips_act(f0, "lpips_head: f0")
    if _lpips_act(f1, "lpips_head: f1") != (K, h, w, C) or not torch.is_tensor(lin) or tuple(lin.shape) != (C,):
        raise RuntimeError(f"lpips_head: f1 must be {(K, h, w, C)} and lin ({C},), got {tuple(f1.shape)} and {tuple(getattr(lin, 'shape', ()))}")
    need = lpips_head_workspace_bytes(K, h, w, C)
    if need == 0:
        raise RuntimeError(f"lpips_head: no kernel for C = {C}")
    if layer_out is None:
        layer_out = torch.empty((K,), device=f0.device, dtype=torch.float64)
    for t, name in ((layer_out, "layer_out"), (total, "total")):
        if t is not None and not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (K,) and t.device == f0.device):
            raise RuntimeError(f"lpips_head: {name} must be a contiguous ({K},) float64 tensor on {f0.device}")
    workspace = torch.empty((need // 8,), device=f0.device, dtype=torch.float64)
    check(_lib.lib().mvsnerf_lpips_head_fwd(f0.data_ptr(), f1.data_ptr(), dev_f32(lin, "lpips_head: lin"), K, h, w, C, layer_out.data_ptr(),
                                            0 if total is None else total.data_ptr(), int(bool(accumulate)), workspace.data_ptr(), stream_ptr()),
          "lpips_head_fwd")
    return layer_out


# ------------------------------------------------------------------ 8-bit video frames (csrc/frames.hip)
_JET = {}


def jet_lut(device):
    """The default colour table of the depth panel, (256,3) uint8 in RGB order: the jet ramp in closed form.  For i = 0..255, x = i / 255:
    r = clamp(1.5 - |4x - 3|, 0, 1), g = clamp(1.5 - |4x - 2|, 0, 1), b = clamp(1.5 - |4x - 1|, 0, 1), each round(255 c).  255 c is always an
    integer or a half, so it is formed in integers (510 c = clamp(765 - 2 |4i - 765 + 255 k|, 0, 510), k = 0, 1, 2) and halves round UP.
    cv2's COLORMAP_JET bytes are not pinned by this (cv2 is not in this image); a caller who wants them passes cv2's own table as `lut`."""
    key = str(torch.device(device))
    if key not in _JET:
        i = torch.arange(256, dtype=torch.int64).view(256, 1)
        k = torch.tensor([0, 1, 2], dtype=torch.int64).view(1, 3)
        twice = (765 - 2 * (4 * i - 765 + 255 * k).abs()).clamp(0, 510)
        _JET[key] = ((twice + 1) // 2).to(torch.uint8).to(device)
    return _JET[key]


def depth_range(depth):
    """utils.py:35-38 on the device: x0 = nan_to_num(depth) -> tensor([min{x0 : x0 > 0}, max x0]) (2,) fp32 on the GPU; the minimum is +inf when no
    element is positive.  Two launches on the current stream, no host synchronisation; two runs give the same bits."""
    _need_no_grad(depth, op="depth_range")
    if not torch.is_tensor(depth) or depth.numel() < 1:
        raise RuntimeError("depth_range: a non-empty tensor on the GPU")
    keep = _Keep()
    ptr = keep(depth, "depth_range: depth")
    n = depth.numel()
    out = torch.empty((2,), device=depth.device, dtype=torch.float32)
    ws = torch.empty((int(_lib.lib().mvsnerf_depth_range_workspace_floats(n)),), device=depth.device, dtype=torch.float32)
    check(_lib.lib().mvsnerf_depth_range_fwd(ptr, n, out.data_ptr(), ws.data_ptr(), stream_ptr()), "depth_range_fwd")
    return out


def frame_u8(rgb, depth=None, minmax=None, lut=None, crop=(0, 0), out=None):
    """One 8-bit frame of the reference's video notebook (mvsnerf_frame_u8_fwd): rgb (H,W,3) -> trunc(clamp(rgb, 0, 1) * 255); with depth (H,W) a second
    panel to its right, lut[trunc(255 (nan_to_num(depth) - mi) / (ma - mi + 1e-8))] (visualize_depth_numpy, utils.py:35-44, the index saturated to
    0..255); crop = (rows, columns) removed from every side of each panel first.  Returns uint8 (H - 2 rows, (W - 2 columns) * panels, 3) on the GPU.
    rgb=None writes the depth panel alone.  minmax: a (2,) device tensor or a pair of floats; None: ops.depth_range(depth), on the device.
    lut: (256,3) uint8, None: jet_lut (RGB).  out: where to write - any uint8 tensor of that shape whose memory is contiguous, e.g. frame k of a
    (K,H',Wout,3) tensor (no alignment needed).  One launch (three with minmax=None), no host synchronisation unless minmax is a pair of floats."""
    _need_no_grad(rgb, depth, op="frame_u8")
    if rgb is None and depth is None:
        raise RuntimeError("frame_u8: rgb, depth or both")
    ref = rgb if rgb is not None else depth
    if not (torch.is_tensor(ref) and ref.is_cuda):
        raise RuntimeError("frame_u8: tensors on the GPU")
    if rgb is not None and not (rgb.dim() == 3 and rgb.shape[-1] == 3):
        raise RuntimeError(f"frame_u8: rgb must be (H,W,3), got {tuple(rgb.shape)}")
    H, W = int(ref.shape[0]), int(ref.shape[1])
    if depth is not None and tuple(depth.shape) != (H, W):
        raise RuntimeError(f"frame_u8: depth must be ({H},{W}), got {tuple(depth.shape)}")
    ch, cw = int(crop[0]), int(crop[1])
    if ch < 0 or cw < 0 or 2 * ch >= H or 2 * cw >= W:
        raise RuntimeError(f"frame_u8: crop {(ch, cw)} leaves nothing of a {H} x {W} frame")
    dev = ref.device
    keep = _Keep()
    p_rgb = keep(rgb, "frame_u8: rgb") if rgb is not None else 0
    p_depth = p_mm = p_lut = 0
    if depth is not None:
        p_depth = keep(depth, "frame_u8: depth")
        if minmax is None:
            minmax = depth_range(keep.alive[-1])
        elif not torch.is_tensor(minmax):
            minmax = torch.tensor([float(minmax[0]), float(minmax[1])], dtype=torch.float32).to(dev)
        if minmax.numel() != 2:
            raise RuntimeError("frame_u8: minmax is (mi, ma)")
        p_mm = keep(minmax.to(dev).reshape(2), "frame_u8: minmax")
        lut = jet_lut(dev) if lut is None else torch.as_tensor(lut)
        if tuple(lut.shape) != (256, 3) or lut.dtype != torch.uint8:
            raise RuntimeError(f"frame_u8: lut must be (256,3) uint8, got {tuple(lut.shape)} {lut.dtype}")
        lut = lut.to(dev).contiguous()
        p_lut = lut.data_ptr()
    shape = (H - 2 * ch, (W - 2 * cw) * ((rgb is not None) + (depth is not None)), 3)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.uint8)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.device == dev and tuple(out.shape) == shape and out.is_contiguous()):
        raise RuntimeError(f"frame_u8: out must be a contiguous uint8 tensor of shape {shape} on {dev}")
    check(_lib.lib().mvsnerf_frame_u8_fwd(p_rgb, p_depth, H, W, p_mm, p_lut, ch, cw, int(depth is not None), out.data_ptr(), stream_ptr()), "frame_u8_fwd")
    return out


# ------------------------------------------------------------------ depth maps -> point cloud (csrc/depth_fusion.hip)
def _fusion_bank(images, c2ws, intrinsics, op):
    M, H, W = _bank_images(images, op)
    if tuple(c2ws.shape) != (M, 3, 4) or tuple(intrinsics.shape) != (M, 3, 3):
        raise RuntimeError(f"{op}: c2ws ({M},3,4) and intrinsics ({M},3,3) expected, got {tuple(c2ws.shape)}, {tuple(intrinsics.shape)}")
    return M, H, W


def _fusion_map(t, dtype, shape, dev, name, op):
    if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == shape and t.device == dev and t.is_contiguous()):
        raise RuntimeError(f"{op}: {name} must be a contiguous {shape} {dtype} tensor on {dev}, got {tuple(getattr(t, 'shape', ()))} "
                           f"{getattr(t, 'dtype', None)} {getattr(t, 'device', None)}")
    return t.data_ptr()


def depth_consistency(images, c2ws, w2cs, intrinsics, depths, src_ids, pix_thr=1.0, rel_thr=0.01, min_views=3, valid=None, alpha=True):
    """The cross-view geometric-consistency filter of the MVSNet line of work over the M depth maps of a bank (mvsnerf_depth_consistency_fwd; the
    definition is in include/mvsnerf_hip_internal.h): depths (M,H,W) fp32, src_ids (M,n_src) int32 on the device (-1: no view), valid (M,H,W) uint8 | None,
    w2cs (M,3,4) the inverses of c2ws -> (seen (M,H,W) int32 bit masks, fused (M,H,W) fp32, mask (M,H,W) uint8).  alpha=False leaves the bank's alpha
    bytes unread (a bank built from three-channel images holds 255 everywhere).  One launch, no atomics, every output element written."""
    op = "depth_consistency"
    _need_no_grad(depths, c2ws, w2cs, intrinsics, op=op)
    M, H, W = _fusion_bank(images, c2ws, intrinsics, op)
    dev = images.device
    if tuple(w2cs.shape) != (M, 3, 4):
        raise RuntimeError(f"{op}: w2cs must be ({M},3,4), got {tuple(w2cs.shape)}")
    p_depth = _fusion_map(depths, torch.float32, (M, H, W), dev, "depths", op)
    p_valid = 0 if valid is None else _fusion_map(valid, torch.uint8, (M, H, W), dev, "valid", op)
    if not (torch.is_tensor(src_ids) and src_ids.dim() == 2 and src_ids.shape[0] == M):
        raise RuntimeError(f"{op}: src_ids must be ({M},n_src)")
    n_src = int(src_ids.shape[1])
    p_src = _fusion_map(src_ids, torch.int32, (M, n_src), dev, "src_ids", op)
    c = _Keep()
    seen = torch.empty((M, H, W), device=dev, dtype=torch.int32)
    fused = torch.empty((M, H, W), device=dev, dtype=torch.float32)
    mask = torch.empty((M, H, W), device=dev, dtype=torch.uint8)
    check(_lib.lib().mvsnerf_depth_consistency_fwd(p_depth, p_valid, images.data_ptr() if alpha else 0, c(c2ws, "c2ws"), c(w2cs, "w2cs"),
                                                   c(intrinsics, "intrinsics"), p_src, M, H, W, n_src, float(pix_thr), float(rel_thr), int(min_views),
                                                   seen.data_ptr(), fused.data_ptr(), mask.data_ptr(), stream_ptr()), "depth_consistency_fwd")
    return seen, fused, mask


def point_cloud(images, c2ws, intrinsics, fused, seen, mask, capacity, out=None):
    """The pixels with mask != 0 as a coloured point cloud in flat-ray-index order (mvsnerf_point_cloud_fwd: count -> scan -> write, no atomics, two runs
    give the same bytes) -> (points (capacity,3) fp32 = o + d * fused, colors (capacity,3) uint8, n_views (capacity,) uint8 = popcount(seen),
    index (capacity,) int64, count (1,) int64 on the device).  count always holds the true total; rows >= min(count, capacity) are not written.
    capacity == 0 runs the count alone.  out: the four output tensors to write into (at least capacity rows each); nothing is read from the device."""
    op = "point_cloud"
    _need_no_grad(fused, c2ws, intrinsics, op=op)
    M, H, W = _fusion_bank(images, c2ws, intrinsics, op)
    dev = images.device
    capacity = int(capacity)
    if capacity < 0:
        raise RuntimeError(f"{op}: capacity must be >= 0, got {capacity}")
    p_fused = _fusion_map(fused, torch.float32, (M, H, W), dev, "fused", op)
    p_seen = _fusion_map(seen, torch.int32, (M, H, W), dev, "seen", op)
    p_mask = _fusion_map(mask, torch.uint8, (M, H, W), dev, "mask", op)
    lib = _lib.lib()
    ws_bytes = int(lib.mvsnerf_point_cloud_workspace_bytes(M * H * W))
    if ws_bytes == 0:
        raise RuntimeError(f"{op}: {M} x {H} x {W} pixels are outside what the compaction indexes (fewer than 2^31)")
    if out is None:
        out = (torch.empty((capacity, 3), device=dev, dtype=torch.float32), torch.empty((capacity, 3), device=dev, dtype=torch.uint8),
               torch.empty((capacity,), device=dev, dtype=torch.uint8), torch.empty((capacity,), device=dev, dtype=torch.int64))
    else:
        for t, dt, tail, name in zip(out, (torch.float32, torch.uint8, torch.uint8, torch.int64), ((3,), (3,), (), ()), ("points", "colors", "n_views", "index")):
            if not (torch.is_tensor(t) and t.dtype == dt and t.device == dev and t.is_contiguous() and t.dim() == 1 + len(tail)
                    and tuple(t.shape[1:]) == tail and t.shape[0] >= capacity):
                raise RuntimeError(f"{op}: out {name} must be a contiguous (>= {capacity},{','.join(map(str, tail))}) {dt} tensor on {dev}")
    points, colors, n_views, index = out
    count = torch.empty((1,), device=dev, dtype=torch.int64)
    ws = torch.empty((ws_bytes // 4,), device=dev, dtype=torch.int32)
    c = _Keep()
    ptr = (lambda t: t.data_ptr()) if capacity > 0 else (lambda t: 0)    # (an empty tensor has no address to hand over)
    check(lib.mvsnerf_point_cloud_fwd(images.data_ptr(), c(c2ws, "c2ws"), c(intrinsics, "intrinsics"), M, H, W, p_fused, p_seen, p_mask, capacity,
                                      ptr(points), ptr(colors), ptr(n_views), ptr(index), count.data_ptr(), ws.data_ptr(), stream_ptr()), "point_cloud_fwd")
    return points, colors, n_views, index, count


# ------------------------------------------------------------------ a density volume -> a triangle mesh (csrc/mesh.hip)
MESH_MAX_NODES = 1 << 27


def _box6(box, op):
    """(lo, hi) of a world box, 2 x 3 numbers read on the host, as the float[6] the C entries take."""
    vals = [float(v) for v in torch.as_tensor(box, dtype=torch.float32).reshape(-1).tolist()]
    if len(vals) != 6:
        raise RuntimeError(f"{op}: box must hold (lo, hi), 2 x 3 numbers")
    return (ctypes.c_float * 6)(*vals)


def mesh_extract(field, level, positions=None, box=None, capacity=None, valid=None):
    """Marching tetrahedra over the Kuhn split of the cells of field (D,H,W) fp32 (mvsnerf_mesh_extract_fwd; the definition is in DESIGN.md 4n and
    include/mvsnerf_hip_internal.h) -> (vertices (V,3) fp32, ndc (V,3) fp32, vertex_edge (V,) int64, faces (T,3) int32, count (2,) int64 on the device).
    positions: the (D,H,W,3) fp32 table of node positions; box: (lo, hi) as 2 x 3 numbers, read on the host; neither: vertices are grid coordinates.
    capacity None: the count runs alone, is read from the device once, and the outputs have exactly V and T rows.  A pair (max_vertices, max_faces):
    nothing is read from the device, the outputs have that many rows, count holds the true totals and rows past them (or past the capacity) are not
    written.  classify -> scan -> vertices -> faces, no atomics: two runs give the same bytes.
    valid: a contiguous (D,H,W) uint8 node mask on the field's device (mvsnerf_mesh_extract_masked_fwd): only edges between valid nodes carry vertices and
    only tetrahedra of four valid nodes emit faces."""
    op = "mesh_extract"
    _need_no_grad(field, positions, op=op)
    if not (torch.is_tensor(field) and field.dim() == 3):
        raise RuntimeError(f"{op}: field must be a (D,H,W) tensor")
    D, H, W = (int(v) for v in field.shape)
    dev = field.device
    p_field = dev_f32(field, f"{op}: field")
    p_pos = 0
    if positions is not None:
        if tuple(positions.shape) != (D, H, W, 3):
            raise RuntimeError(f"{op}: positions must be ({D},{H},{W},3), got {tuple(positions.shape)}")
        p_pos = dev_f32(positions, f"{op}: positions")
    p_valid = 0 if valid is None else _fusion_map(valid, torch.uint8, (D, H, W), dev, "valid", op)
    c_box = None if box is None else _box6(box, op)
    lib = _lib.lib()
    ws_bytes = int(lib.mvsnerf_mesh_workspace_bytes(D, H, W))
    if ws_bytes == 0:
        raise RuntimeError(f"{op}: a ({D},{H},{W}) field is outside what the kernels index (every dimension >= 2, at most 2^27 nodes)")
    ws = torch.empty(((ws_bytes + 3) // 4,), device=dev, dtype=torch.int32)
    count = torch.empty((2,), device=dev, dtype=torch.int64)

    def run(cap_v, cap_f):
        out = (torch.empty((cap_v, 3), device=dev, dtype=torch.float32), torch.empty((cap_v, 3), device=dev, dtype=torch.float32),
               torch.empty((cap_v,), device=dev, dtype=torch.int64), torch.empty((cap_f, 3), device=dev, dtype=torch.int32))
        ptr = [t.data_ptr() if t.numel() else 0 for t in out]            # (an empty tensor has no address to hand over)
        check(lib.mvsnerf_mesh_extract_masked_fwd(p_field, p_valid, D, H, W, float(level), p_pos, c_box, cap_v, cap_f, *ptr, count.data_ptr(),
                                                  ws.data_ptr(), stream_ptr()), "mesh_extract_masked_fwd")
        return out

    if capacity is None:
        run(0, 0)
        cap_v, cap_f = (int(v) for v in count.tolist())                  # the one host read
        if cap_v == 0 and cap_f == 0:
            return (torch.empty((0, 3), device=dev, dtype=torch.float32), torch.empty((0, 3), device=dev, dtype=torch.float32),
                    torch.empty((0,), device=dev, dtype=torch.int64), torch.empty((0, 3), device=dev, dtype=torch.int32), count)
    else:
        cap_v, cap_f = int(capacity[0]), int(capacity[1])
        if cap_v < 0 or cap_f < 0:
            raise RuntimeError(f"{op}: capacity must be a pair of numbers >= 0, got {capacity}")
    return (*run(cap_v, cap_f), count)


def mesh_dirs(vertices, origin):
    """vertices (n,3) fp32, origin (3,) fp32 on the device -> (n,3) rows vertices - origin (mvsnerf_mesh_dirs_fwd)."""
    _need_no_grad(vertices, origin, op="mesh_dirs")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or origin.numel() != 3:
        raise RuntimeError(f"mesh_dirs: vertices (n,3) and origin (3,), got {tuple(vertices.shape)} and {tuple(origin.shape)}")
    n = int(vertices.shape[0])
    out = torch.empty((n, 3), device=vertices.device, dtype=torch.float32)
    check(_lib.lib().mvsnerf_mesh_dirs_fwd(dev_f32(vertices, "mesh_dirs: vertices") if n else 0, dev_f32(origin, "mesh_dirs: origin"), n,
                                           out.data_ptr() if n else 0, stream_ptr()), "mesh_dirs_fwd")
    return out


def mesh_rgb_u8(raw):
    """raw (n,4) fp32 (the MLP's rgb + sigma rows) -> (n,3) uint8 = trunc(clamp(rgb, 0, 1) * 255), NaN -> 0 (mvsnerf_mesh_rgb_u8_fwd: frame_u8's rule)."""
    _need_no_grad(raw, op="mesh_rgb_u8")
    if raw.dim() != 2 or raw.shape[1] != 4:
        raise RuntimeError(f"mesh_rgb_u8: raw must be (n,4), got {tuple(raw.shape)}")
    n = int(raw.shape[0])
    out = torch.empty((n, 3), device=raw.device, dtype=torch.uint8)
    check(_lib.lib().mvsnerf_mesh_rgb_u8_fwd(dev_f32(raw, "mesh_rgb_u8: raw") if n else 0, n, out.data_ptr() if n else 0, stream_ptr()), "mesh_rgb_u8_fwd")
    return out


# ------------------------------------------------------------------ depth maps -> a TSDF volume (csrc/tsdf.hip)
def tsdf_integrate(images, w2cs, intrinsics, depths, box, dims, trunc, valid=None, alpha=True, views=None, z_min=0.0):
    """The M depth maps of a bank integrated into a truncated signed distance volume over the world box (lo, hi) (mvsnerf_tsdf_integrate_fwd; the
    definition is in DESIGN.md 4o and include/mvsnerf_hip_internal.h): depths (M,H,W) fp32, w2cs (M,3,4) the inverses of the bank's poses, valid (M,H,W)
    uint8 | None, views a 1-D int32 tensor of view ids on the device (integrated in its order) | None for every view, dims = (D,H,W) nodes ->
    (tsdf (D,H,W) fp32, weight (D,H,W) int32, colors (D,H,W,4) uint8).  alpha=False leaves the bank's alpha bytes untested.  One launch, one thread per
    node, no atomics, every output element written."""
    op = "tsdf_integrate"
    _need_no_grad(depths, w2cs, intrinsics, op=op)
    M, H, W = _bank_images(images, op)
    dev = images.device
    if tuple(w2cs.shape) != (M, 3, 4) or tuple(intrinsics.shape) != (M, 3, 3):
        raise RuntimeError(f"{op}: w2cs ({M},3,4) and intrinsics ({M},3,3) expected, got {tuple(w2cs.shape)}, {tuple(intrinsics.shape)}")
    p_depth = _fusion_map(depths, torch.float32, (M, H, W), dev, "depths", op)
    p_valid = 0 if valid is None else _fusion_map(valid, torch.uint8, (M, H, W), dev, "valid", op)
    p_views, n_views = _view_list(views, dev, op)
    if views is None:
        n_views = M
    c_box = _box6(box, op)
    D, Hn, Wn = (int(v) for v in dims)
    if min(D, Hn, Wn) < 2 or D * Hn * Wn > MESH_MAX_NODES:
        raise RuntimeError(f"{op}: a ({D},{Hn},{Wn}) grid is outside what the kernels index (every dimension >= 2, at most 2^27 nodes)")
    c = _Keep()
    tsdf = torch.empty((D, Hn, Wn), device=dev, dtype=torch.float32)
    weight = torch.empty((D, Hn, Wn), device=dev, dtype=torch.int32)
    colors = torch.empty((D, Hn, Wn, 4), device=dev, dtype=torch.uint8)
    check(_lib.lib().mvsnerf_tsdf_integrate_fwd(p_depth, p_valid, images.data_ptr(), int(bool(alpha)), c(w2cs, "w2cs"), c(intrinsics, "intrinsics"), p_views,
                                                n_views, M, H, W, c_box, D, Hn, Wn, float(trunc), float(z_min), tsdf.data_ptr(), weight.data_ptr(),
                                                colors.data_ptr(), stream_ptr()), "tsdf_integrate_fwd")
    return tsdf, weight, colors


def tsdf_vertex_colors(tsdf, colors, vertex_edge, count):
    """tsdf (D,H,W) fp32 and colors (D,H,W,4) uint8 of a TSDF volume, vertex_edge (rows,) int64 and count (>= 1,) int64 of a mesh of its zero level, all on
    one device -> (rows,3) uint8: the two end nodes' colours interpolated at the zero crossing of the edge (mvsnerf_tsdf_vertex_colors_fwd).  Rows past
    min(count[0], rows) are left 0; nothing is read from the device."""
    op = "tsdf_vertex_colors"
    _need_no_grad(tsdf, op=op)
    if not (torch.is_tensor(tsdf) and tsdf.dim() == 3):
        raise RuntimeError(f"{op}: tsdf must be a (D,H,W) tensor")
    D, H, W = (int(v) for v in tsdf.shape)
    dev = tsdf.device
    p_tsdf = dev_f32(tsdf, f"{op}: tsdf")
    p_col = _fusion_map(colors, torch.uint8, (D, H, W, 4), dev, "colors", op)
    if not (torch.is_tensor(vertex_edge) and vertex_edge.dim() == 1):
        raise RuntimeError(f"{op}: vertex_edge must be a (rows,) tensor")
    rows = int(vertex_edge.shape[0])
    p_edge = _fusion_map(vertex_edge, torch.int64, (rows,), dev, "vertex_edge", op)
    if not (torch.is_tensor(count) and count.dtype == torch.int64 and count.device == dev and count.dim() == 1 and count.numel() >= 1
            and count.is_contiguous()):
        raise RuntimeError(f"{op}: count must be a contiguous int64 tensor of at least one element on {dev} (TriangleMesh.count)")
    out = torch.zeros((rows, 3), device=dev, dtype=torch.uint8)
    check(_lib.lib().mvsnerf_tsdf_vertex_colors_fwd(p_tsdf, p_col, D, H, W, p_edge if rows else 0, count.data_ptr(), rows, out.data_ptr() if rows else 0,
                                                    stream_ptr()), "tsdf_vertex_colors_fwd")
    return out


# ------------------------------------------------------------------ point grid, nearest neighbour, cloud metrics, points on a mesh (csrc/cloud_metrics.hip)
GRID_MAX_CELLS = 1 << 24
CLOUD_METRICS_MAX_TAUS = 8
CLOUD_METRICS_ROW = 2 + CLOUD_METRICS_MAX_TAUS       # sum of the finite distances, their number, the numbers below each tau
MESH_SAMPLE_MAX_N = 1024


def _cloud_rows(t, name, op):
    """A contiguous (n,3) fp32 tensor on the current GPU, n < 2^31 -> (n, pointer or 0 for n == 0)."""
    if not (torch.is_tensor(t) and t.dim() == 2 and t.shape[1] == 3):
        raise RuntimeError(f"{op}: {name} must be an (n,3) tensor, got {tuple(getattr(t, 'shape', ()))}")
    n = int(t.shape[0])
    if n >= 1 << 31:
        raise RuntimeError(f"{op}: {name} holds {n} rows; the kernels index fewer than 2^31")
    return n, (dev_f32(t, f"{op}: {name}") if n else 0)


def grid_bounds(points):
    """points (n,3) fp32 -> (6,) fp32 on the device: min xyz, max xyz over the rows whose coordinates are all finite (+inf, -inf when there is none).  Two
    launches, min / max only: the same bits every run (mvsnerf_grid_bounds_fwd)."""
    op = "grid_bounds"
    _need_no_grad(points, op=op)
    n, p = _cloud_rows(points, "points", op)
    lib = _lib.lib()
    ws = torch.empty((int(lib.mvsnerf_grid_bounds_workspace_bytes(n)) // 4,), device=points.device, dtype=torch.float32)
    out = torch.empty((6,), device=points.device, dtype=torch.float32)
    check(lib.mvsnerf_grid_bounds_fwd(p, n, out.data_ptr(), ws.data_ptr(), stream_ptr()), "grid_bounds_fwd")
    return out


def grid_build(points, lo, cell, dims):
    """The uniform grid over points (n,3) fp32 (mvsnerf_grid_build_fwd): lo three host numbers, cell the edge, dims = (dx, dy, dz) cells ->
    (cell_start (dx dy dz + 1,) int32, records (n,4) fp32: x, y, z and the bits of the original row, grouped by cell; the first cell_start[-1] rows are
    written).  A point outside the box lands in a border cell; a row with a non-finite coordinate is left out.  The order inside a cell may differ
    between runs."""
    op = "grid_build"
    _need_no_grad(points, op=op)
    n, p = _cloud_rows(points, "points", op)
    dx, dy, dz = (int(v) for v in dims)
    lib = _lib.lib()
    ws_bytes = int(lib.mvsnerf_grid_build_workspace_bytes(n, dx, dy, dz))
    if ws_bytes == 0:
        raise RuntimeError(f"{op}: a grid of {dx} x {dy} x {dz} cells is outside what the kernels index (every dimension >= 1, at most 2^24 cells)")
    dev = points.device
    cell_start = torch.empty((dx * dy * dz + 1,), device=dev, dtype=torch.int32)
    records = torch.empty((n, 4), device=dev, dtype=torch.float32)
    ws = torch.empty((ws_bytes // 4,), device=dev, dtype=torch.int32)
    c_lo = (ctypes.c_float * 3)(*[float(v) for v in lo])
    check(lib.mvsnerf_grid_build_fwd(p, n, c_lo, float(cell), dx, dy, dz, cell_start.data_ptr(), records.data_ptr() if n else 0, ws.data_ptr(),
                                     stream_ptr()), "grid_build_fwd")
    return cell_start, records


def grid_nearest(lo, cell, dims, cell_start, records, query, max_dist):
    """The exact nearest grid point within max_dist of every row of query (n,3) fp32 (mvsnerf_grid_nearest_fwd) -> (dist (n,) fp32, index (n,) int32):
    the lowest original index among equal squared distances, +inf and -1 where nothing is within max_dist or the query is not finite."""
    op = "grid_nearest"
    _need_no_grad(query, op=op)
    n, p = _cloud_rows(query, "query", op)
    dx, dy, dz = (int(v) for v in dims)
    dev = query.device
    p_start = _fusion_map(cell_start, torch.int32, (dx * dy * dz + 1,), dev, "cell_start", op)
    if not (torch.is_tensor(records) and records.dtype == torch.float32 and records.dim() == 2 and records.shape[1] == 4 and records.device == dev
            and records.is_contiguous()):
        raise RuntimeError(f"{op}: records must be a contiguous (n,4) float32 tensor on {dev}")
    dist = torch.empty((n,), device=dev, dtype=torch.float32)
    index = torch.empty((n,), device=dev, dtype=torch.int32)
    c_lo = (ctypes.c_float * 3)(*[float(v) for v in lo])
    check(_lib.lib().mvsnerf_grid_nearest_fwd(c_lo, float(cell), dx, dy, dz, p_start, records.data_ptr() if records.shape[0] else 0, p, n, float(max_dist),
                                              dist.data_ptr() if n else 0, index.data_ptr() if n else 0, stream_ptr()), "grid_nearest_fwd")
    return dist, index


def cloud_metrics_row(dist, taus):
    """dist (n,) fp32 on the device, taus up to 8 host numbers -> (CLOUD_METRICS_ROW,) float64 on the device: the sum of the finite distances, their
    number, the number of distances below each tau (fp32 compare), zeros behind (mvsnerf_cloud_metrics_fwd: two launches, fixed order, no atomics)."""
    op = "cloud_metrics_row"
    _need_no_grad(dist, op=op)
    if not (torch.is_tensor(dist) and dist.dim() == 1):
        raise RuntimeError(f"{op}: dist must be an (n,) tensor")
    n = int(dist.shape[0])
    taus = [float(t) for t in taus]
    if len(taus) > CLOUD_METRICS_MAX_TAUS:
        raise RuntimeError(f"{op}: at most {CLOUD_METRICS_MAX_TAUS} thresholds, got {len(taus)}")
    p = dev_f32(dist, f"{op}: dist") if n else 0
    lib = _lib.lib()
    ws_bytes = int(lib.mvsnerf_cloud_metrics_workspace_bytes(n))
    if ws_bytes == 0:
        raise RuntimeError(f"{op}: {n} distances are outside what the kernels index (fewer than 2^31)")
    ws = torch.empty((ws_bytes // 8,), device=dist.device, dtype=torch.float64)
    out = torch.empty((CLOUD_METRICS_ROW,), device=dist.device, dtype=torch.float64)
    c_taus = (ctypes.c_float * max(len(taus), 1))(*taus)
    check(lib.mvsnerf_cloud_metrics_fwd(p, n, c_taus, len(taus), out.data_ptr(), ws.data_ptr(), stream_ptr()), "cloud_metrics_fwd")
    return out


def mesh_sample(vertices, faces, spacing, capacity=None, mesh_count=None):
    """Points on the faces (T,3) int32 of vertices (V,3) fp32 at about `spacing` apart (mvsnerf_mesh_sample_fwd; the lattice is written out in DESIGN.md 4p)
    -> (points (P,3) fp32, face (P,) int32, count (2,) int64 on the device: the true number of points, the largest subdivision n of any face).
    capacity None: the count runs alone and is read from the device once; a face that needs n > 1024 raises.  An integer: nothing is read from the
    device, the outputs have that many rows, rows past count[0] are not written and a face with n > 1024 emits nothing (count[1] tells).
    mesh_count: the (2,) int64 device counts of a mesh extracted with a capacity: rows past them are not read."""
    op = "mesh_sample"
    _need_no_grad(vertices, op=op)
    V, p_v, T, p_f, p_mc = _mesh_rows(vertices, faces, mesh_count, op)
    dev = vertices.device
    lib = _lib.lib()
    ws_bytes = int(lib.mvsnerf_mesh_sample_workspace_bytes(T))
    if ws_bytes == 0:
        raise RuntimeError(f"{op}: {T} faces are outside what the kernels index (fewer than 2^31)")
    ws = torch.empty((ws_bytes // 8,), device=dev, dtype=torch.int64)
    count = torch.empty((2,), device=dev, dtype=torch.int64)

    def run(cap):
        points = torch.empty((cap, 3), device=dev, dtype=torch.float32)
        face = torch.empty((cap,), device=dev, dtype=torch.int32)
        check(lib.mvsnerf_mesh_sample_fwd(p_v, V, p_f, T, p_mc, float(spacing), cap, points.data_ptr() if cap else 0, face.data_ptr() if cap else 0,
                                          count.data_ptr(), ws.data_ptr(), stream_ptr()), "mesh_sample_fwd")
        return points, face

    if capacity is None:
        run(0)
        total, n_max = (int(v) for v in count.tolist())                  # the one host read
        if n_max > MESH_SAMPLE_MAX_N:
            raise RuntimeError(f"{op}: unsupported shape: a face needs {n_max} subdivisions at spacing {float(spacing)} (at most {MESH_SAMPLE_MAX_N}); "
                               "sample with a larger spacing")
        if total >= 1 << 31:
            raise RuntimeError(f"{op}: unsupported shape: {total} points (fewer than 2^31); sample with a larger spacing")
        capacity = total
    return (*run(int(capacity)), count)


# ------------------------------------------------------------------ a mesh in the scene's cameras: rasteriser, face visibility, mesh filter (csrc/raster.hip)
RASTER_MAX_VIEWS = 65535
RASTER_MAX_IMAGE = 1 << 15


def _mesh_rows(vertices, faces, mesh_count, op):
    """(V, vertices pointer, T, faces pointer, mesh_count pointer) of a mesh on the current GPU."""
    V, p_v = _cloud_rows(vertices, "vertices", op)
    dev = vertices.device
    if not (torch.is_tensor(faces) and faces.dim() == 2 and faces.shape[1] == 3):
        raise RuntimeError(f"{op}: faces must be a (T,3) tensor, got {tuple(getattr(faces, 'shape', ()))}")
    T = int(faces.shape[0])
    p_f = _fusion_map(faces, torch.int32, (T, 3), dev, "faces", op) if T else 0
    p_mc = 0 if mesh_count is None else _fusion_map(mesh_count, torch.int64, (2,), dev, "mesh_count", op)
    return V, p_v, T, p_f, p_mc


def _view_list(views, dev, op):
    if views is None:
        return 0, 0
    if not (torch.is_tensor(views) and views.dim() == 1 and views.numel() >= 1):
        raise RuntimeError(f"{op}: views must be a 1-D tensor of at least one view id")
    n = int(views.numel())
    return _fusion_map(views, torch.int32, (n,), dev, "views", op), n


def mesh_raster(vertices, faces, w2cs, intrinsics, hw, colors=None, views=None, cull=0, z_min=0.0, background=(255, 255, 255), mesh_count=None):
    """The z-buffer rasteriser (mvsnerf_mesh_raster_fwd; the definition is in DESIGN.md 4r and include/mvsnerf_hip_internal.h): vertices (V,3) fp32, faces
    (T,3) int32, colors (V,3) uint8 | None, w2cs (M,3,4) and intrinsics (M,3,3) fp32, hw = (H, W), views a 1-D int32 device tensor of view ids (output slot a
    shows view views[a]) | None for every view -> (depth (n,H,W) fp32, 0 = nothing hit; face (n,H,W) int32, -1 = nothing; colors (n,H,W,3) uint8 | None).
    cull: 0 both windings, +1 drops A > 0, -1 drops A < 0.  mesh_count: the (2,) int64 device counts of a mesh extracted with a capacity.  Order-free atomic
    min on 64-bit words: two runs give the same bytes.  Nothing is read from the device."""
    op = "mesh_raster"
    _need_no_grad(vertices, w2cs, intrinsics, op=op)
    V, p_v, T, p_f, p_mc = _mesh_rows(vertices, faces, mesh_count, op)
    dev = vertices.device
    if not (torch.is_tensor(w2cs) and w2cs.dim() == 3 and tuple(w2cs.shape[1:]) == (3, 4) and w2cs.shape[0] >= 1):
        raise RuntimeError(f"{op}: w2cs must be (M,3,4), got {tuple(getattr(w2cs, 'shape', ()))}")
    M = int(w2cs.shape[0])
    p_w2c = _fusion_map(w2cs, torch.float32, (M, 3, 4), dev, "w2cs", op)
    p_K = _fusion_map(intrinsics, torch.float32, (M, 3, 3), dev, "intrinsics", op)
    p_col = 0 if colors is None else (_fusion_map(colors, torch.uint8, (V, 3), dev, "colors", op) if V else 0)
    p_views, n_views = _view_list(views, dev, op)
    n = n_views if views is not None else M
    H, W = int(hw[0]), int(hw[1])
    bg = [int(b) for b in background]
    if len(bg) != 3 or min(bg) < 0 or max(bg) > 255:
        raise RuntimeError(f"{op}: background must be three bytes, got {background!r}")
    lib = _lib.lib()
    ws_bytes = int(lib.mvsnerf_mesh_raster_workspace_bytes(T, n, H, W))
    if ws_bytes == 0:
        raise RuntimeError(f"{op}: unsupported shape: {T} faces in {n} views of {H} x {W} (at least 1 x 1 and at most {RASTER_MAX_IMAGE} a side, at most "
                           f"{RASTER_MAX_VIEWS} views, at most 2^22 workgroups of 256 (face, view) pairs)")
    ws = torch.empty((ws_bytes // 8,), device=dev, dtype=torch.int64)
    depth = torch.empty((n, H, W), device=dev, dtype=torch.float32)
    face = torch.empty((n, H, W), device=dev, dtype=torch.int32)
    has_colors = colors is not None and V > 0
    out_colors = torch.empty((n, H, W, 3), device=dev, dtype=torch.uint8) if has_colors else None
    check(lib.mvsnerf_mesh_raster_fwd(p_v, V, p_f, T, p_col, p_mc, p_w2c, p_K, p_views, n_views, M, H, W, int(cull), float(z_min),
                                      bg[0] | bg[1] << 8 | bg[2] << 16, depth.data_ptr(), face.data_ptr(), out_colors.data_ptr() if has_colors else 0,
                                      ws.data_ptr(), stream_ptr()), "mesh_raster_fwd")
    if colors is not None and not has_colors:                               # a mesh without a vertex: every pixel is background
        out_colors = torch.tensor(bg, dtype=torch.uint8).to(dev).expand(n, H, W, 3).contiguous()
    return depth, face, out_colors


def mesh_face_views(face, n_faces, views=None, n_bank=None, mesh_count=None):
    """face (n,H,W) int32 face maps (mesh_raster's) -> (n_views (T,) int32: the views in which a face owns at least one pixel, seen (T, ceil(M / 32)) int32:
    bit m & 31 of word m >> 5 says so for view m).  views: the 1-D int32 device tensor mesh_raster was given (map a shows view views[a]) with n_bank = M, or
    None: map a is view a.  Entries outside [0, min(mesh_count[1], T)) are ignored.  Integer atomic OR: order-free (mvsnerf_mesh_face_views_fwd)."""
    op = "mesh_face_views"
    if not (torch.is_tensor(face) and face.is_cuda and face.dim() == 3 and face.numel() > 0):
        raise RuntimeError(f"{op}: face must be a non-empty (n,H,W) tensor on the GPU")
    n, H, W = (int(v) for v in face.shape)
    dev = face.device
    if dev.index != torch.cuda.current_device():
        raise RuntimeError(f"{op}: face is on {dev} but the current device is cuda:{torch.cuda.current_device()}")
    p_face = _fusion_map(face, torch.int32, (n, H, W), dev, "face", op)
    p_views, n_views = _view_list(views, dev, op)
    if views is not None and n_views != n:
        raise RuntimeError(f"{op}: {n} face maps but {n_views} view ids")
    M = n if views is None else int(n_bank)
    T = int(n_faces)
    p_mc = 0 if mesh_count is None else _fusion_map(mesh_count, torch.int64, (2,), dev, "mesh_count", op)
    words = (M + 31) // 32
    seen = torch.empty((T, words), device=dev, dtype=torch.int32)
    count = torch.empty((T,), device=dev, dtype=torch.int32)
    check(_lib.lib().mvsnerf_mesh_face_views_fwd(p_face, n, H, W, p_views, M, T, p_mc, seen.data_ptr() if T else 0, count.data_ptr() if T else 0,
                                                 stream_ptr()), "mesh_face_views_fwd")
    return count, seen


def mesh_filter(vertices, faces, keep, ndc=None, vertex_edge=None, colors=None, mesh_count=None):
    """The faces with keep (T,) uint8 != 0, in order, and the vertices they use, in order, renumbered (mvsnerf_mesh_filter_fwd) ->
    (vertices, ndc | None, vertex_edge | None, colors | None, vertex_index (V',) int64, faces (T',3) int32, face_index (T',) int64, count (2,) int64 on the
    device).  The two totals are read from the device once.  mark -> count -> scan -> write, no atomics: stable, the same bytes every run."""
    op = "mesh_filter"
    _need_no_grad(vertices, op=op)
    V, p_v, T, p_f, p_mc = _mesh_rows(vertices, faces, mesh_count, op)
    dev = vertices.device
    p_keep = _fusion_map(keep, torch.uint8, (T,), dev, "keep", op) if T else 0
    p_ndc = 0 if ndc is None or not V else _fusion_map(ndc, torch.float32, (V, 3), dev, "ndc", op)
    p_edge = 0 if vertex_edge is None or not V else _fusion_map(vertex_edge, torch.int64, (V,), dev, "vertex_edge", op)
    p_col = 0 if colors is None or not V else _fusion_map(colors, torch.uint8, (V, 3), dev, "colors", op)
    lib = _lib.lib()
    ws_bytes = int(lib.mvsnerf_mesh_filter_workspace_bytes(V, T))
    if ws_bytes == 0:
        raise RuntimeError(f"{op}: {V} vertices and {T} faces are outside what the kernels index (fewer than 2^31)")
    ws = torch.empty(((ws_bytes + 3) // 4,), device=dev, dtype=torch.int32)
    count = torch.empty((2,), device=dev, dtype=torch.int64)

    def run(cv, cf):
        out = (torch.empty((cv, 3), device=dev, dtype=torch.float32),
               None if ndc is None else torch.empty((cv, 3), device=dev, dtype=torch.float32),
               None if vertex_edge is None else torch.empty((cv,), device=dev, dtype=torch.int64),
               None if colors is None else torch.empty((cv, 3), device=dev, dtype=torch.uint8),
               torch.empty((cv,), device=dev, dtype=torch.int64), torch.empty((cf, 3), device=dev, dtype=torch.int32),
               torch.empty((cf,), device=dev, dtype=torch.int64))
        ptr = [t.data_ptr() if t is not None and t.numel() else 0 for t in out]
        check(lib.mvsnerf_mesh_filter_fwd(p_v, p_ndc, p_edge, p_col, V, p_f, T, p_mc, p_keep, cv, cf, *ptr, count.data_ptr(), ws.data_ptr(), stream_ptr()),
              "mesh_filter_fwd")
        return out

    run(0, 0)
    cv, cf = (int(v) for v in count.tolist())                            # the one host read
    return (*run(cv, cf), count)
