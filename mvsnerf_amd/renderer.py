"""Drop-in for the reference's renderer.py (same callables) on libmvsnerf_hip.so.

`rendering` takes the fused one-call path (ops.raymarch) whenever it is handed what
`create_nerf_mvs` builds; every individual function is also HIP-backed so that code calling them
piecemeal (notebooks, render_density) keeps working.
"""
import torch

from . import ops
from .utils import index_point_feature, build_color_volume, normal_vect  # noqa: F401  (reference re-exports)


def depth2dist(z_vals, cos_angle):
    """renderer.py:5-11.  Kept for API parity; raw2alpha ignores its result (renderer.py:18-26)."""
    d = z_vals[..., 1:] - z_vals[..., :-1]
    d = torch.cat([d, torch.full_like(d[..., :1], 1e10)], -1)
    return d * cos_angle.unsqueeze(-1)


def raw2alpha(sigma, dist=None, net_type="v0"):
    """renderer.py:18-26 -> (alpha, weights, alpha_softmax).  `dist` is ignored, as in the reference.
    The third return value (softmax of sigma over the samples, renderer.py:24) is consumed by nobody in the reference; it is
    computed here eagerly with one torch call so that the 3-tuple is complete.  Not on the hot path: rendering() composites
    inside the fused kernel and never calls this function."""
    raw = torch.zeros((*sigma.shape, 4), device=sigma.device, dtype=torch.float32)
    raw[..., 3] = sigma
    _, _, _, weights, _, alpha = ops.composite(raw, torch.zeros_like(sigma), False)
    return alpha, weights, torch.softmax(sigma, 1)


def raw2outputs(raw, z_vals, dists=None, white_bkgd=False, net_type="v2"):
    """renderer.py:65-92 -> (rgb_map, disp_map, acc_map, weights, depth_map, alpha)."""
    return ops.composite(raw.contiguous(), z_vals.contiguous(), white_bkgd)


def batchify(fn, chunk):
    """renderer.py:28-40.  The fused MLP kernel needs no chunking; kept for callers that pass plain modules."""
    if chunk is None:
        return fn

    def ret(inputs, alpha_only):
        f = fn.forward_alpha if alpha_only else fn
        return torch.cat([f(inputs[i:i + chunk]) for i in range(0, inputs.shape[0], chunk)], 0)
    return ret


def run_network_mvs(pts, viewdirs, alpha_feat, fn, embed_fn, embeddirs_fn, netchunk=1024):
    """renderer.py:42-63.  pts (N,S,3) NDC, viewdirs (N,3) or None, alpha_feat (N,S,F) -> (N,S,4|1).
    With our MVSNeRF + Embedder(10) the 63-wide embedding and the 86-wide concat are never built."""
    from .models import MVSNeRF, Embedder
    fused_ok = (isinstance(fn, MVSNeRF) and isinstance(embed_fn, Embedder) and embed_fn.fusable
                and embeddirs_fn is None and alpha_feat is not None)
    if not fused_ok:
        raise NotImplementedError(
            "run_network_mvs: only the configurations the reference trains are built as a HIP kernel "
            "(MVSNeRF net_type v0 or v2, pts embedder multires=10, no dir embedder, alpha_feat given)")
    if viewdirs is not None and viewdirs.dim() == 3:
        raise NotImplementedError("run_network_mvs: per-sample view directions are not on the hot path")
    N, S = pts.shape[:2]
    raw = fn.query(pts, alpha_feat, viewdirs, N, S)
    return raw.view(N, S, -1)


def gen_dir_feature(w2c_ref, rays_dir):
    """renderer.py:111-122: rays_dir @ w2c_ref[:3,:3]^T (caller passes unit directions)."""
    return ops.dir_feature(rays_dir.contiguous(), w2c_ref.contiguous(), normalize=False)


def gen_pts_feats(imgs, volume_feature, rays_pts, pose_ref, rays_ndc, feat_dim, img_feat=None, img_downscale=1.0,
                  use_color_volume=False, net_type="v0"):
    """renderer.py:124-136: [8 volume channels | V x (r,g,b,mask)] written in place into one (N,S,feat_dim) tensor."""
    from .models import RefVolume
    vol = volume_feature.feat_volume if isinstance(volume_feature, RefVolume) else volume_feature
    ops._need_no_grad(vol, op="gen_pts_feats (gather)")                                  # on the caller's tensor: the channel-last view is always detached
    vol_cl = ops.channels_last_volume(vol)
    if use_color_volume:
        # renderer.py:134-135 (--use_color_volume fine-tuning): the colours were projected into the volume once
        # (train_mvs_nerf_finetuning_pl.py:72-82), so the per-sample feature is ONE lookup of the (8 + 4V)-channel volume
        if vol_cl.shape[-1] != feat_dim:
            raise RuntimeError(f"use_color_volume: the volume has {vol_cl.shape[-1]} channels, feat_dim is {feat_dim}")
        return ops.volume_sample(vol_cl, rays_ndc.contiguous())
    N, S = rays_pts.shape[:2]
    V = imgs.shape[1]
    if feat_dim != 8 + 4 * V:
        raise RuntimeError(f"feat_dim {feat_dim} != 8 + 4*V ({V} views)")
    if img_feat is not None:          # renderer.py:126-127,133: feat_dim grows by V*Cf; columns [8 | V x (rgb, Cf feature channels, mask)]
        if img_feat.shape[1] != V:        # the reference's cat (utils.py:329) would raise on mismatched view counts; here columns would stay unwritten
            raise RuntimeError(f"gen_pts_feats: img_feat holds {img_feat.shape[1]} views, imgs {V}")
        feat_dim += V * img_feat.shape[2]
        out = torch.empty((N, S, feat_dim), device=rays_pts.device, dtype=torch.float32)
        ops.volume_sample(vol_cl, rays_ndc.contiguous(), out=out, out_stride=feat_dim)
        ops.color_feat_sample(imgs[0].contiguous(), img_feat[0, :V].contiguous(), pose_ref["w2cs"][:V].contiguous(),
                              pose_ref["intrinsics"][:V].contiguous(), rays_pts.contiguous(), with_mask=True, out=out,
                              out_ptr=out.data_ptr() + 8 * 4, out_stride=feat_dim)
        return out
    out = torch.empty((N, S, feat_dim), device=rays_pts.device, dtype=torch.float32)
    ops.volume_sample(vol_cl, rays_ndc.contiguous(), out=out, out_stride=feat_dim)
    ops.color_sample(imgs[0].contiguous(), pose_ref["w2cs"][:V].contiguous(), pose_ref["intrinsics"][:V].contiguous(),
                     rays_pts.contiguous(), with_mask=True, out=out, out_ptr=out.data_ptr() + 8 * 4, out_stride=feat_dim)
    return out


WIDE_TRAINING_MSG = ("training at netwidth 256 is not built: the wide MLP kernel (csrc/mlp_wide.hip) is a no-grad forward; render under "
                     "torch.no_grad(), or train a netwidth-128 network")

_scene = [None]


def _scene_views(imgs, pose_ref, V):
    """(imgs[0], w2cs[:V], intrinsics[:V], channel-last images) of the scene a render loop keeps passing: the three slices / contiguous()
    calls and the transpose-cache lookup cost ~10 us per rendering() call, more than the 4 kernel launches.  One entry, keyed on the
    identity and version of the three tensors (the entry holds them, so an id cannot be recycled while it is compared)."""
    w2cs, K = pose_ref["w2cs"], pose_ref["intrinsics"]
    hit = _scene[0]
    if (hit is not None and hit[0] is imgs and hit[1] is w2cs and hit[2] is K and hit[3] == (V, imgs._version, w2cs._version, K._version)):
        return hit[4]
    im0 = imgs[0].contiguous()
    val = (im0, w2cs[:V].contiguous(), K[:V].contiguous(), ops.channels_last_images(im0) if ops.FUSED_GATHER else None)
    _scene[0] = (imgs, w2cs, K, (V, imgs._version, w2cs._version, K._version), val)
    return val


def rendering(args, pose_ref, rays_pts, rays_ndc, depth_candidates, rays_o, rays_dir,
              volume_feature=None, imgs=None, network_fn=None, img_feat=None, network_query_fn=None, white_bkgd=False, **kwargs):
    """renderer.py:138-165.  Returns (rgb_map, input_feat, weights, depth_map, alpha, {}) - note that the
    reference's callers name the 2nd/3rd entries `disp`/`acc` (train_mvs_nerf_pl.py:123)."""
    from .models import MVSNeRF, RefVolume
    color_vol = bool(getattr(args, "use_color_volume", False))
    fusable = (pose_ref is not None and isinstance(network_fn, MVSNeRF) and img_feat is None and getattr(network_query_fn, "_mvsnerf_fused", False))
    vol = volume_feature.feat_volume if isinstance(volume_feature, RefVolume) else volume_feature
    if isinstance(network_fn, MVSNeRF) and network_fn.wide:
        # netwidth 256: the no-grad network query on the wide fp32 kernel between the individually HIP-backed pieces below (no one-call ray
        # march, no backward at this width) - refused here, before anything is enqueued, when the call wants gradients
        if torch.is_grad_enabled() and ((vol is not None and vol.requires_grad) or any(p.requires_grad for p in network_fn.parameters())):
            raise NotImplementedError(WIDE_TRAINING_MSG)
        fusable = False
    fusable = fusable and vol is not None
    needs_grad = fusable and torch.is_grad_enabled() and (vol.requires_grad or any(p.requires_grad for p in network_fn.parameters()))
    fused = fusable and (not color_vol or needs_grad)     # a colour volume is rendered piecewise below, trained through raymarch_train
    if fused:
        V = imgs.shape[1]
        if args.feat_dim != 8 + 4 * V:
            raise RuntimeError(f"args.feat_dim {args.feat_dim} != 8 + 4*V ({V} views)")
        if color_vol and vol.shape[-4] != args.feat_dim:
            raise RuntimeError(f"use_color_volume: the volume has {vol.shape[-4]} channels, feat_dim is {args.feat_dim}")
        if needs_grad:      # training: same kernels + activation store, gradients to the volume and the MLP
            out = ops.raymarch_train(vol, imgs[0].contiguous(), pose_ref["w2cs"][:V].contiguous(),
                                     pose_ref["intrinsics"][:V].contiguous(), network_fn, rays_pts.contiguous(),
                                     rays_ndc.contiguous(), depth_candidates.contiguous(), rays_dir.contiguous(), white_bkgd,
                                     dp_samples=getattr(args, "dp_volume_grad", "allreduce") == "samples" and vol.requires_grad)
        else:
            sc = _scene_views(imgs, pose_ref, V)
            out = ops.raymarch(ops.channels_last_volume(vol), sc[0], sc[1], sc[2],
                               network_fn.packed(args.feat_dim), rays_pts.contiguous(), rays_ndc.contiguous(),
                               depth_candidates.contiguous(), rays_dir.contiguous(), white_bkgd, want=(), imgs_cl=sc[3],
                               **network_fn.packed_alt(args.feat_dim, fresh=True))
        rendering.last_raw = out["raw"]          # sigma lives in raw[...,3]; kept for parity tests / density queries
        return out["rgb_map"], out["input_feat"], out["weights"], out["depth"], out["alpha"], {}

    # generic composition of the individually HIP-backed pieces (same order as the reference)
    # rays_dir/|rays_dir| then rotation into the reference camera (renderer.py:142-147), one kernel
    angle = ops.dir_feature(rays_dir.contiguous(), pose_ref["w2cs"][0].contiguous() if pose_ref is not None else None, normalize=True)
    input_feat = gen_pts_feats(imgs, volume_feature, rays_pts, pose_ref, rays_ndc, args.feat_dim, img_feat,
                               args.img_downscale, args.use_color_volume, args.net_type)
    raw = network_query_fn(rays_ndc, angle, input_feat, network_fn)
    rendering.last_raw = raw
    rgb_map, _, _, weights, depth_map, alpha = raw2outputs(raw, depth_candidates, None, white_bkgd, args.net_type)
    return rgb_map, input_feat, weights, depth_map, alpha, {}


def rendering_batched(args, pose_ref, ray_batches, volume_feature=None, imgs=None, network_fn=None, network_query_fn=None, white_bkgd=False, **kwargs):
    """K calls of rendering() (renderer.py:138-165) on one scene as ONE host call: ray_batches = [(rays_pts, rays_ndc, depth_candidates, rays_o,
    rays_dir), ...] (rendering()'s positional ray arguments).  Returns the list of rendering()'s 6-tuples.  No gradients (inference loops:
    validation_step's chunk loop, notebooks' render loops); an extension - the reference has no such entry, its loop body is rendering().
    With args.use_color_volume the feature rows come from the (8 + 4V)-channel volume (ops.raymarch_colorvol_batched), still one host call."""
    from .models import MVSNeRF, RefVolume
    vol = volume_feature.feat_volume if isinstance(volume_feature, RefVolume) else volume_feature
    if not (pose_ref is not None and isinstance(network_fn, MVSNeRF) and getattr(network_query_fn, "_mvsnerf_fused", False) and vol is not None):
        raise NotImplementedError("rendering_batched: the fused configuration only (what create_nerf_mvs builds); call rendering() per batch otherwise")
    if network_fn.wide:      # netwidth 256 has no batched entry: rendering() once per batch, the same tuples
        return [rendering(args, pose_ref, *b, volume_feature=volume_feature, imgs=imgs, network_fn=network_fn, network_query_fn=network_query_fn,
                          white_bkgd=white_bkgd, **kwargs) for b in ray_batches]
    V = imgs.shape[1]
    if args.feat_dim != 8 + 4 * V:
        raise RuntimeError(f"args.feat_dim {args.feat_dim} != 8 + 4*V ({V} views)")
    if bool(getattr(args, "use_color_volume", False)):
        # renderer.py:134-135: the feature row is one lookup of the (8 + 4V)-channel volume - the same one host call, the colour-volume gather
        # (ops.gather_colorvol's kernel) in place of the image gather
        if vol.shape[-4] != args.feat_dim:
            raise RuntimeError(f"use_color_volume: the volume has {vol.shape[-4]} channels, feat_dim is {args.feat_dim}")
        outs = ops.raymarch_colorvol_batched(ops.channels_last_volume(vol), pose_ref["w2cs"][:V].contiguous(), network_fn.packed(args.feat_dim),
                                             [(b[1].contiguous(), b[2].contiguous(), b[4].contiguous()) for b in ray_batches], white_bkgd,
                                             **network_fn.packed_alt(args.feat_dim, fresh=True))
        if outs:
            rendering.last_raw = outs[-1]["raw"]
        return [(o["rgb_map"], o["input_feat"], o["weights"], o["depth"], o["alpha"], {}) for o in outs]
    sc = _scene_views(imgs, pose_ref, V)
    packed = network_fn.packed(args.feat_dim)
    outs = ops.raymarch_batched(ops.channels_last_volume(vol), sc[0], sc[1], sc[2], packed,
                                [(b[0].contiguous(), b[1].contiguous(), b[2].contiguous(), b[4].contiguous()) for b in ray_batches],
                                white_bkgd, imgs_cl=sc[3], **network_fn.packed_alt(args.feat_dim, fresh=True))
    if outs:
        rendering.last_raw = outs[-1]["raw"]
    return [(o["rgb_map"], o["input_feat"], o["weights"], o["depth"], o["alpha"], {}) for o in outs]


def render_density(network_fn, rays_pts, density_feature, network_query_fn, chunk=1024 * 5):
    """renderer.py:167-177: sigma-only queries (forward_alpha path)."""
    out = []
    dev = density_feature.device
    for i in range(0, rays_pts.shape[0], chunk):
        out.append(network_query_fn(rays_pts[i:i + chunk].to(dev), None, density_feature[i:i + chunk], network_fn))
    return torch.cat(out)
