"""Training entry points of the reference on the HIP hot path, without pytorch_lightning (not in this image).

`MVSSystem` mirrors `train_mvs_nerf_pl.py:34-288`: same constructor argument (`args` from opt.py), same
`decode_batch / unpreprocess / configure_optimizers / training_step(batch, batch_nb) -> {'loss': loss} / save_ckpt`
methods, same batch dict schema (data/dtu.py:199-211 collated with B=1), same `self.log` keys, same checkpoint keys.
A real `pytorch_lightning.LightningModule` can be mixed in unchanged; `_ModuleShim` provides the three attributes
the step uses (`log`, `global_step`, `device`) when Lightning is absent.

Multi-GPU (one process per GPU, gradients averaged by ONE flat-buffer all-reduce -
mvsnerf_amd.distributed.FlatGradAllReduce, RCCL over xGMI on GPUs), two modes selected by `args.dp_mode`:
  "scene" (DEFAULT for generalizable training; north_star's "source-view triplets" sharding) each rank takes a DIFFERENT
          (scan, ref view) sample and its own 1024 rays - what Lightning DDP + DistributedSampler would give the reference
          (train_mvs_nerf_pl.py:306,313): the effective batch is `world` scenes per step and the WHOLE step (encoder included) is
          divided; the only exchange is the 1.9 MB flat all-reduce.  BN batch statistics are per rank (DDP without SyncBN); the
          running-stat buffers are broadcast from rank 0 at the end of fit_steps and before save_ckpt (DDP's broadcast_buffers).
  "ray"   every rank encodes the SAME scene sample and draws the same pixel ids / jitter (ONE base seed broadcast from rank 0 at
          the start of fit_steps, step i uses base + i), renders its slice of the rays and back-propagates through its slice AND
          the replicated encoder: the step equals the 1-GPU step on the same batch, but the encoder's ~8.5 of ~10 ms are repeated on
          every rank (bounded speed-up, <= ~1.2x at 8 GPUs by construction).  It is the right mode where no encoder runs per step
          (per-scene fine-tuning, MVSSystemFinetune), not for this class.
Nothing here has run on more than one GPU (the dev boxes have one): every multi-GPU statement is by construction + world-size-2 gloo
tests, UNMEASURED on hardware.

`args.use_amp` (the reference's `precision=16 if args.use_amp`, train_mvs_nerf_pl.py:317-318; BASELINE config 3 "bf16"): the ray-march MLP
trains on v_mfma_f32_32x32x16_bf16 - forward with a 16-bit activation store, data- and weight-gradient GEMMs - and the encoder on
v_mfma_f32_16x16x32_bf16: conv0 of CostRegNet (74.5 % of the encoder's FLOPs) from a bf16 cost volume (csrc/conv_bf16.hip), conv1 .. conv11 and
FeatureNet from their fp32 activations rounded on load (csrc/conv3d_bf16.hip, csrc/wgrad_bf16.hip) - forward, data and weight gradients alike -
with fp32 accumulation, fp32 master weights and an fp32 gradient all-reduce.  The plane sweep's arithmetic and InPlaceABN (statistics,
normalisation, its backward) stay fp32, as autocast keeps grid_sample and batch norm.
"""
import os

import torch
import torch.nn as nn

from . import distributed as D
from . import ops
from .models import MVSNeRF, create_nerf_mvs
from .renderer import rendering, WIDE_TRAINING_MSG
from .utils import build_rays, build_rays_test, img2mse


_UNPRE = {}


def _adam_kw(params):
    """torch's single-kernel Adam when every parameter lives on the GPU (same update rule as the reference's torch.optim.Adam; the default
    multi-tensor path makes ~8 passes over the parameters - 0.6 ms per fine-tuning step for the 150 MB learnable volume)."""
    ps = list(params)
    return {"fused": True} if ps and all(p.is_cuda and p.dtype == torch.float32 for p in ps) else {}


def _adam(params, lr):
    """The reference's torch.optim.Adam(betas=(0.9, 0.999)).  fp32 parameters on the GPU: mvsnerf_amd.optim.Adam - the same update, state_dict and
    hooks with ONE launch per step for all tensors (torch's fused Adam: three ~25 us launches for the 78 tensors of the generalizable step)."""
    ps = list(params)
    if ps and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in ps):
        from .optim import Adam
        return Adam(ps, lr=lr, betas=(0.9, 0.999))
    return torch.optim.Adam(ps, lr=lr, betas=(0.9, 0.999), **_adam_kw(ps))


def mse2psnr2(x):
    """utils.py:28-30.  A device tensor stays on the device (no host synchronisation inside the training step)."""
    import math
    if torch.is_tensor(x):
        return -10.0 * torch.log(x.detach().clamp_min(1e-20)) / math.log(10.0)
    return -10.0 * math.log(max(x, 1e-20)) / math.log(10.0)


class SL1Loss(nn.Module):
    """reference train_mvs_nerf_pl.py:22-32."""

    def __init__(self, levels=3):
        super().__init__()
        self.loss = nn.SmoothL1Loss(reduction="mean")

    def forward(self, depth_pred, depth_gt, mask=None):
        if mask is None:
            mask = depth_gt > 0
        return self.loss(depth_pred[mask], depth_gt[mask]) * 2 ** (1 - 2)


class _ModuleShim(nn.Module):
    """What `training_step` needs from LightningModule."""

    def __init__(self):
        super().__init__()
        self.global_step = 0
        self.logged = {}

    def log(self, key, value, prog_bar=False, **kw):
        # tensors are kept as (detached) device tensors: reading one is the only host synchronisation, and it is the reader's
        self.logged[key] = value.detach() if torch.is_tensor(value) else float(value)

    def logged_values(self):
        """The last logged metrics as Python floats (synchronises with the device)."""
        return {k: float(v) for k, v in self.logged.items()}

    @property
    def device(self):
        return next(self.parameters()).device


# ------------------------------------------------------------------ empty-space skipping: what the three systems share
def _threshold(value, who):
    """A density threshold (skip_empty=, args.skip_empty_train) as a float; NaN is refused - by ops._thr_f32, the package's one NaN test."""
    return ops._thr_f32(value, who)


def _need_fused(net, kw, who):
    """The sparse paths run the fused configuration only: an MVSNeRF whose network query the ray-march kernels embed (what create_nerf_mvs builds)."""
    if not (isinstance(net, MVSNeRF) and getattr(kw.get("network_query_fn"), "_mvsnerf_fused", False)):
        raise NotImplementedError(f"{who}: the fused configuration only (what create_nerf_mvs builds)")


def _sparse_config(system, vol, V, who):
    """(network, colour volume?) of a system's sparse paths (ops.node_density, ops.raymarch_sparse) on `vol` with V source views, after the refusals:
    the fused configuration, and a volume whose channels are what args.feat_dim and args.use_color_volume say."""
    args, kw = system.args, system.render_kwargs_train
    net = kw.get("network_fn")
    _need_fused(net, kw, who)
    color_vol = bool(getattr(args, "use_color_volume", False))
    if args.feat_dim != 8 + 4 * V or vol.shape[-4] != (args.feat_dim if color_vol else 8):
        raise RuntimeError(f"{who}: volume with {vol.shape[-4]} channels, feat_dim {args.feat_dim}, {V} source views")
    return net, color_vol


def _sparse_sources(system, vol, pose, V, imgs, who):
    """The scene arguments of ops.raymarch_sparse, as its keywords, for a system that renders `vol` from V source views (after _sparse_config's
    refusals): imgs and intrinsics (None for a colour volume, which holds the colours itself), w2cs, packed, white_bkgd and the kernel choice of
    MVSNeRF.packed_alt."""
    args, kw = system.args, system.render_kwargs_train
    net, color_vol = _sparse_config(system, vol, V, who)
    return dict(imgs=None if color_vol else imgs.contiguous(), w2cs=pose["w2cs"][:V].contiguous(),
                intrinsics=None if color_vol else pose["intrinsics"][:V].contiguous(), packed=net.packed(args.feat_dim),
                white_bkgd=bool(kw.get("white_bkgd", getattr(args, "white_bkgd", False))), **net.packed_alt(args.feat_dim))


def _density_sources(net, F, vol, pose, V, imgs=None, **camera):
    """Every argument of ops.node_density but dilate, as keywords, for the nodes of a system's volume `vol`.  imgs: the V source images of an
    8-channel volume, with `camera` - near_far, ref_hw, pad[, lindisp] of the reference view the volume is aligned with; its intrinsics and pose are
    pose's first - for the nodes' world positions; None for a colour volume (one lookup per node, no camera)."""
    src = {} if imgs is None else dict(imgs=imgs.contiguous(), intrinsics=pose["intrinsics"][:V].contiguous(),
                                       camera=dict(K_ref=pose["intrinsics"][0], c2w_ref=pose["c2ws"][0], **camera))
    return dict(vol_cl=ops.channels_last_volume(vol), packed=net.packed(F), w2cs=pose["w2cs"][:V].contiguous(), **src, **net.packed_alt(F))


def _early_stop(early_stop, stop_every, who):
    """early_stop= / stop_every= of a render call after ops._early_stop_args' refusals: None (no early stop), or (eps, stop_every)."""
    return None if early_stop is None else ops._early_stop_args(early_stop, stop_every, f"{who}(early_stop=)")


def _device_count(device_count, skip_empty, stop, who):
    """device_count= of a render call as a bool after its refusals, which need no library: it belongs to the sparse paths, and the
    bf16-family MLP modes have no counted kernels."""
    if not device_count:
        return False
    if skip_empty is None and stop is None:
        raise ValueError(f"{who}: device_count=True is a switch of the skip_empty / early_stop paths; pass one of them with it")
    mode = ops.inference_mlp_mode()
    if mode in ("bf16", "bf16x3", "bf16x6"):
        raise NotImplementedError(f"{who}(device_count=True): the {mode!r} MLP kernels take their row count from the host only; device counts run "
                                  "under 'auto', 'fp32' and 'fp16x3'")
    return True


def _render_sparse_batches(system, n_rows, B, make_batch, march_kw, early_stop=None, device_count=False):
    """A frame of n_rows rays with empty space skipped, per sub-batch of B rays: make_batch(idx) -> (pts, ndc, z, dirs) of rays [idx * B, (idx + 1) * B)
    -> ops.raymarch_sparse(**march_kw: vol_cl, imgs, w2cs, intrinsics, packed, density, thr, white_bkgd and the kernel choice) - one host read of
    the live count per sub-batch.  The sub-batches are sharded over the ranks (distributed.render_frame); system.last_live_fraction is this rank's
    live samples over its samples.  Returns (rgb (n_rows,3), depth (n_rows,)).
    early_stop: (eps, stop_every) of _early_stop - the sub-batch call is ops.raymarch_early_stop (march_kw with or without density /
    thr), one host read per segment of stop_every samples; last_live_fraction then counts the samples that reached the MLP, and
    system.last_stopped_fraction is this rank's stopped rays over its rays.
    device_count: the sub-batch calls run with device_count=True - no host read per sub-batch or segment; the counts are summed on
    the device and read ONCE, after the frame's last sub-batch has been enqueued, for the two fractions."""
    live = [0, 0, 0, 0]             # live samples, samples, stopped rays, rays
    kw = dict(march_kw, device_count=True) if device_count else march_kw

    def render_batch(idx):
        pts, ndc, z, dirs = make_batch(idx)
        if early_stop is None:
            o = ops.raymarch_sparse(rays_pts=pts, rays_ndc=ndc, z_vals=z, rays_dir=dirs, **kw)
        else:
            o = ops.raymarch_early_stop(rays_pts=pts, rays_ndc=ndc, z_vals=z, rays_dir=dirs, eps=early_stop[0], stop_every=early_stop[1], **kw)
            live[2] = live[2] + (o["n_stopped"].long() if device_count else o["n_stopped"])
            live[3] += z.shape[0]
        live[0] = live[0] + (o["n_live"].long() if device_count else o["n_live"])       # (int64 device sums: a frame can hold more than 2^31 samples)
        live[1] += z.numel()
        return o["rgb_map"], o["depth"]
    out = D.render_frame(render_batch, 1, n_rows, B)
    if torch.is_tensor(live[0]):                                 # device_count: the frame's one host read, behind its last sub-batch
        live[0], live[2] = torch.stack([live[0], live[2] if torch.is_tensor(live[2]) else torch.zeros_like(live[0])]).tolist()
    system.last_live_fraction = live[0] / live[1] if live[1] else 0.0
    if early_stop is not None:
        system.last_stopped_fraction = live[2] / live[3] if live[3] else 0.0
    return out


class MVSSystem(_ModuleShim):
    """reference train_mvs_nerf_pl.py:34-288 (generalizable training)."""

    def __init__(self, args, n_depth_planes=128):
        super().__init__()
        self.args = args
        self.n_views = getattr(args, "n_views", 3)                       # extension (config 4: 5 views); the reference fixes 3
        self.args.feat_dim = 8 + self.n_views * 4                        # :38
        self.idx = 0
        self.loss = SL1Loss()
        self.learning_rate = args.lrate
        kw_train, kw_test, _, self.grad_vars = create_nerf_mvs(args, use_mvs=True, dir_embedder=False, pts_embedder=True)   # :45
        for k in ("N_samples", "ndc", "lindisp"):                        # filter_keys, utils.py:418-424
            kw_train.pop(k, None)
        self.render_kwargs_train, self.render_kwargs_test = kw_train, kw_test
        self.MVSNet = kw_train.pop("network_mvs")                        # registered as sub-module `MVSNet` like the reference
        self.MVSNet.D = n_depth_planes
        self.network_fn = kw_train["network_fn"]                         # registers the MLP parameters
        self.render_kwargs_train["NDC_local"] = False
        self.eval_metric = [0.01, 0.05, 0.1]
        self._allreduce = None

    # -- data plumbing -------------------------------------------------------------------------
    def decode_batch(self, batch):
        """:56-62 - move to device, squeeze the B=1 dim of the pose tensors."""
        dev = self.device
        data = {k: (v.to(dev, torch.float32, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}
        pose_ref = {k: data[k].squeeze(0) if data[k].dim() > 3 or k == "near_fars" else data[k]
                    for k in ("w2cs", "intrinsics", "c2ws", "near_fars")}
        return data, pose_ref

    @staticmethod
    def unpreprocess(data, shape=(1, 1, 3, 1, 1)):
        """:64-71 - undo the ImageNet normalisation (colour lookups use raw [0,1] images)."""
        key = (data.device, data.dtype)
        if key not in _UNPRE:                     # built once per device: a torch.tensor(list, device=...) is a synchronous upload
            _UNPRE[key] = (torch.tensor([-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225], device=data.device, dtype=data.dtype),
                           torch.tensor([1 / 0.229, 1 / 0.224, 1 / 0.225], device=data.device, dtype=data.dtype))
        mean, std = _UNPRE[key]
        return (data - mean.view(*shape)) / std.view(*shape)

    def configure_optimizers(self):
        """:84-88."""
        self.optimizer = _adam(self.grad_vars, self.learning_rate)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=self.args.num_epochs, eta_min=1e-7)
        return [self.optimizer], [sched]

    # -- the step ------------------------------------------------------------------------------
    def training_step(self, batch, batch_nb):
        """:104-168.  Returns {'loss': loss}; gradients are left to the caller (Lightning or `fit_steps`)."""
        args = self.args
        if getattr(args, "skip_empty_train", None) is not None:
            raise ValueError("MVSSystem.training_step: args.skip_empty_train is set, but generalizable training encodes a new scene every step and "
                             "holds no density volume to test samples against; the switch is for MVSSystemFinetune and MVSSystemFusion (DESIGN.md 4g)")
        batch = dict(batch)
        batch.pop("scan", None)
        data_mvs, pose_ref = self.decode_batch(batch)
        imgs, proj_mats = data_mvs["images"], data_mvs["proj_mats"]
        near_fars, depths_h = data_mvs["near_fars"], data_mvs["depths_h"]

        nv = self.n_views
        from . import encoder as _enc
        with _enc.encoder_precision("bf16" if getattr(args, "use_amp", False) else _enc.ENCODER_PRECISION):   # :317-318 precision=16: conv0 .. conv11 and FeatureNet on bf16
            volume_feature, _, _ = self.MVSNet(imgs[:, :nv], proj_mats[:, :nv], near_fars[0, 0], pad=args.pad)      # :113
        imgs = self.unpreprocess(imgs)
        N_rays, N_samples = args.batch_size, args.N_samples
        rays_pts, rays_dir, target_s, rays_NDC, depth_candidates, rays_o, rays_depth, _ = build_rays(
            imgs, depths_h, pose_ref, pose_ref["w2cs"], pose_ref["c2ws"], pose_ref["intrinsics"], near_fars, N_rays, N_samples, pad=args.pad)  # :119
        loss_scale, depth_scale, depth_term = 1.0, None, None
        n_masked_all = (rays_depth > 0).sum() if (rays_depth is not None and getattr(args, "with_depth", False)) else None
        if self.dp_mode() == "ray":                                      # same draw on all ranks (seeded in fit_steps), local slice
            (rays_pts, rays_dir, target_s, rays_NDC, depth_candidates, rays_depth, rays_o), loss_scale = D.shard_ray_batch(
                (rays_pts, rays_dir, target_s, rays_NDC, depth_candidates, rays_depth, rays_o), N_rays)     # rays_o is (3, N): sliced in dim 1
        # --use_amp (train_mvs_nerf_pl.py:317-318 `precision=16`): the MLP's forward / backward GEMMs on the bf16 matrix cores with
        # fp32 accumulation, master weights and gradients; the encoder runs its bf16 kernels under the context above (encoder.py)
        with ops.mlp_precision("bf16" if getattr(args, "use_amp", False) else ops.MLP_PRECISION):
            rgb, disp, acc, depth_pred, alpha, ret = rendering(args, pose_ref, rays_pts, rays_NDC, depth_candidates, rays_o, rays_dir,
                                                               volume_feature, imgs[:, :-1], img_feat=None, **self.render_kwargs_train)   # :123
        loss = 0
        if getattr(args, "with_depth", False):
            mask = rays_depth > 0
            if getattr(args, "with_depth_loss", False):
                if self.dp_mode() == "ray" and D.world_rank()[0] > 1:
                    # The depth term is a mean over the MASKED rays of the whole draw.  A rank's slice (128 rays at 8 GPUs) may hold none of
                    # them: a local masked mean would then be NaN, and the flat all-reduce would hand that NaN to every rank.  So: local masked
                    # SUM (0 for an empty slice) x world / global masked count - every rank holds the full draw before slicing, so the global
                    # count is local knowledge (device tensors, no host sync); the rank-averaged gradient is that of the global mean.
                    dsum = torch.nn.functional.smooth_l1_loss(depth_pred[mask], rays_depth[mask], reduction="sum") * 2 ** (1 - 2)
                    depth_term = dsum / mask.sum().clamp_min(1)                     # reported: local mean (0 when the slice has no masked ray)
                    depth_scale = dsum * float(D.world_rank()[0]) / n_masked_all.clamp_min(1)   # back-propagated
                else:
                    depth_term = self.loss(depth_pred, rays_depth, mask)
                loss = loss + depth_term
            with torch.no_grad():                                        # :130-138
                err = (depth_pred - rays_depth)[mask].abs()
                for t in self.eval_metric:
                    self.log(f"train/acc_l_{t}mm", (err < t).float().mean(), prog_bar=False)
                self.log("train/abs_err", err.mean(), prog_bar=True)
        img_loss = img2mse(rgb, target_s)                                # :143
        loss = loss + img_loss
        with torch.no_grad():
            self.log("train/loss", loss, prog_bar=True)
            self.log("train/img_mse_loss", img_loss)
            if getattr(args, "with_depth", False):                       # :152-155: PSNR over the masked rays, PSNR_out over the rest
                self.log("train/PSNR", mse2psnr2(img2mse(rgb[mask], target_s[mask])), prog_bar=True)
                self.log("train/PSNR_out", mse2psnr2(img2mse(rgb[~mask], target_s[~mask])), prog_bar=True)
            else:
                self.log("train/PSNR", mse2psnr2(img_loss), prog_bar=True)
        if self.global_step % 20000 == 19999:
            if self.dp_mode() == "scene":
                self.sync_buffers()                                       # collective: every rank takes part, rank 0 writes
            if D.world_rank()[1] == 0:                                    # one writer (ranks hold identical weights after the all-reduce)
                self.save_ckpt(f"{self.global_step}")
        # ray mode with N_rays % world != 0: the tensor that is back-propagated is weighted so that the rank-AVERAGED gradient is that of
        # the global mean; what is reported / logged stays the plain local mean ('loss_unscaled')
        if loss_scale == 1.0 and depth_scale is None:
            return {"loss": loss}
        scaled = img_loss * loss_scale + (0 if depth_term is None else (depth_scale if depth_scale is not None else depth_term * loss_scale))
        return {"loss": scaled, "loss_unscaled": loss.detach()}

    @torch.no_grad()
    def encode_scene(self, batch):
        """The scene encode of render_view alone: MVSNet on the batch's source views -> the neural volume (1,8,D,h,w).  The reference's video path encodes a scene
        ONCE and renders every camera pose of the path from that volume (renderer_video.ipynb cell 8: `volume_feature` outside the pose loop); pass the result to
        render_view(..., volume=...) for the same.  Under tile-parallel inference this is what removes the replicated encode from the per-frame time."""
        data_mvs, pose_ref = self.decode_batch(dict(batch))
        imgs, proj_mats, near_fars = data_mvs["images"], data_mvs["proj_mats"], pose_ref["near_fars"]
        V = imgs.shape[1] - 1
        self.MVSNet.train()                                              # :182 batch-statistics ABN also at inference
        return self.MVSNet(imgs[:, :V], proj_mats[:, :V], near_fars[0], pad=self.args.pad)[0]

    @torch.no_grad()
    def scene_density(self, batch, volume=None, dilate=0):
        """The density volume of the encoded scene in the RENDERER's frame -> (D,h,w) fp32: ops.node_density over the nodes of `volume`
        (encode_scene(batch) when None) - at every node the sigma-only output of the lookups and the MLP entry render_view's ray march runs there
        (DESIGN.md 4f).  Views and cameras are taken from the batch exactly as render_view takes them (all but the last view are sources, view 0 is the
        reference); the nodes' world positions for the colour lookup come from the reference view's OWN intrinsics, pose and near / far - what the volume
        is aligned with.  dilate: widen the occupied region by that many voxels (ops.max_dilate3d).  This is what render_view(skip_empty=) tests
        samples against; build it once per scene (render_path_skip_empty does)."""
        args = self.args
        data_mvs, pose_ref = self.decode_batch(dict(batch))
        imgs, near_fars = data_mvs["images"], pose_ref["near_fars"]
        H, W = int(imgs.shape[-2]), int(imgs.shape[-1])
        V = imgs.shape[1] - 1
        vol = self.encode_scene(batch) if volume is None else volume
        net, color_vol = _sparse_config(self, vol, V, "skip_empty / scene_density")
        return ops.node_density(dilate=dilate, **_density_sources(net, args.feat_dim, vol, pose_ref, V, None if color_vol else self.unpreprocess(imgs)[0, :V],
                                                                  near_far=near_fars[0], ref_hw=(H, W), pad=args.pad))

    @torch.no_grad()
    def render_view(self, batch, chunk=None, whole_frame_off=False, target=None, batch_rays=16384, volume=None, skip_empty=None, density=None, dilate=0,
                    device_count=False, early_stop=None, stop_every=32):
        """The rendering part of validation_step (:172-254): encode once, then the chunk loop over the target view's
        pixels - tile-parallel over ranks (contiguous chunk ranges + one all_gather).  Returns (rgb (H,W,3), depth (H,W)).
        whole_frame_off=True keeps the per-chunk Python loop (build_rays_test + rendering per chunk) instead of the single
        mvsnerf_render_pixels_fwd call; both produce the same pixels.
        target (extension, BASELINE config 5): dict(hw=(H,W), intrinsic (3,3), c2w (4,4)[, near_far (2,)]) renders a camera whose
        pixel grid differs from the source views' (e.g. 1008x756 rays over 960x640 sources).  The reference normalises the NDC
        coordinates with the *target* size and intrinsics (utils.py:252-253, fine when all views share both); with `target` the
        reference view's own intrinsics and size are used, which is what the volume is aligned with.
        batch_rays: rays per sub-batch inside the library call (free parameter: the pixels do not depend on it; measured on a 512x640
        frame: 1024 -> 85.5 ms, 4096 -> 81.7, 16384 -> 80.5, 65536 -> 80.9; the workspace is 16 KB per ray).
        volume: the result of encode_scene(batch) - the encode is skipped (a camera path over one scene; the pixels are the same).
        skip_empty: None (default) is the dense render above, untouched.  A float is the density threshold of DESIGN.md 4e: samples whose trilinear
        cell in `density` holds no value above it are not sent through the MLP - their raw is (0,0,0,0), the others have the bits of the dense
        sequence (ops.raymarch_sparse).  The frame then runs per sub-batch of batch_rays pixels (_render_sparse_batches on ops.raygen), the sub-batches
        sharded over the ranks, one host read of the live count per sub-batch; `self.last_live_fraction` is this rank's live samples over its samples.
        netwidth 256, net_type v2 and colour volumes take the same path.  density: (D,h,w) of the volume in use - default
        scene_density(batch, volume, dilate), built on every call: a camera path should build it once (render_path_skip_empty does) and pass it.  dilate is
        read only when the density is built here.
        early_stop: None (default) changes nothing.  A float eps in [0, 1) stops a ray at the first multiple of stop_every samples in front of which its
        transmittance is < eps (ops.raymarch_early_stop per sub-batch, one host read per segment; rgb moves by at most eps, depth by
        eps max|z|).  Alone it needs no density volume; with skip_empty a sample reaches the MLP iff its ray is alive and its cell is live.
        `self.last_stopped_fraction` is this rank's stopped rays over its rays, last_live_fraction the samples that reached the MLP.
        device_count: False (default) changes nothing.  True (with skip_empty or early_stop only, not under the bf16-family modes) runs
        the sub-batches without a host read - the same pixels; the two fractions come from one host read behind the frame's last sub-batch."""
        stop = _early_stop(early_stop, stop_every, "render_view")          # refusals first: nothing below needs the library before them
        device_count = _device_count(device_count, skip_empty, stop, "render_view")
        if stop is not None and whole_frame_off:
            raise ValueError("render_view: early_stop runs its own per-sub-batch loop; it cannot be combined with whole_frame_off=True")
        if skip_empty is not None:
            if whole_frame_off:
                raise ValueError("render_view: skip_empty runs its own per-sub-batch loop; it cannot be combined with whole_frame_off=True")
            skip_empty = _threshold(skip_empty, "render_view(skip_empty=)")
            if density is not None and (density.dim() != 3 or (volume is not None and tuple(density.shape) != tuple(volume.shape[-3:]))):
                raise RuntimeError(f"render_view: density must be the (D,h,w) of the volume in use, got {tuple(density.shape)}"
                                   + ("" if volume is None else f" for a volume {tuple(volume.shape)}"))
        elif density is not None:
            raise ValueError("render_view: density= is read by the skip_empty path only; pass skip_empty= (a threshold) with it")
        args = self.args
        chunk = chunk or args.chunk
        data_mvs, pose_ref = self.decode_batch(dict(batch))
        imgs, proj_mats, near_fars = data_mvs["images"], data_mvs["proj_mats"], pose_ref["near_fars"]
        H, W = int(imgs.shape[-2]), int(imgs.shape[-1])
        V = imgs.shape[1] - 1                                            # source views (3 in the reference's batches, :193)
        if volume is None:
            self.MVSNet.train()                                          # :182 batch-statistics ABN also at inference
            volume_feature, _, _ = self.MVSNet(imgs[:, :V], proj_mats[:, :V], near_fars[0], pad=args.pad)
        else:
            volume_feature = volume
        imgs = self.unpreprocess(imgs)
        world_to_ref, tgt_to_world, intrinsic = pose_ref["w2cs"][0], pose_ref["c2ws"][-1], pose_ref["intrinsics"][-1]
        k_ref, ref_hw, nf_tgt = None, None, near_fars[-1]
        if target is not None:
            dev = imgs.device
            ref_hw, (H, W) = (H, W), (int(target["hw"][0]), int(target["hw"][1]))
            intrinsic, tgt_to_world = target["intrinsic"].to(dev, torch.float32), target["c2w"].to(dev, torch.float32)
            k_ref = pose_ref["intrinsics"][0]
            if "near_far" in target:
                nf_tgt = target["near_far"].to(dev, torch.float32)

        kw = self.render_kwargs_train
        net = kw["network_fn"]
        if skip_empty is not None or stop is not None:
            src = _sparse_sources(self, volume_feature, pose_ref, V, imgs[0, :-1], "skip_empty / early_stop / scene_density")
            if skip_empty is not None:
                if density is None:
                    density = self.scene_density(batch, volume=volume_feature, dilate=dilate)
                if tuple(density.shape) != tuple(volume_feature.shape[-3:]):
                    raise RuntimeError(f"render_view: density {tuple(density.shape)} is not the (D,h,w) of the volume {tuple(volume_feature.shape)}")
                src.update(density=density.to(imgs.device, torch.float32).contiguous(), thr=skip_empty)
            k_render = intrinsic if intrinsic.dim() == 2 else intrinsic.mean(0)
            k_ndc = k_render if k_ref is None else k_ref
            nf_t, nf_r = nf_tgt.reshape(-1)[:2].contiguous(), near_fars[0].reshape(-1)[:2].contiguous()
            B = max(int(batch_rays), 1)

            def make_batch(idx):
                first = idx * B
                pts, dirs, ndc, z, _ = ops.raygen(H, W, k_render, tgt_to_world, k_ndc, world_to_ref, nf_t, nf_r, args.N_samples, pad=args.pad,
                                                  first_pixel=first, n_rays=min(B, H * W - first), ref_hw=ref_hw)
                return pts, ndc, z, dirs
            rgb, depth = _render_sparse_batches(self, H * W, B, make_batch, dict(src, vol_cl=ops.channels_last_volume(volume_feature)), early_stop=stop,
                                                device_count=device_count)
            return rgb.reshape(H, W, 3), depth.reshape(H, W)
        fused = (isinstance(net, MVSNeRF) and getattr(kw.get("network_query_fn"), "_mvsnerf_fused", False)
                 and not getattr(args, "use_color_volume", False) and args.feat_dim == 8 + 4 * V and not whole_frame_off
                 and not net.wide)                       # netwidth 256 has no whole-frame entry: the per-chunk loop below
        if target is not None and not fused:
            raise RuntimeError("render_view(target=...) needs the fused ray-march path (MVSNeRF + fused network_query_fn)")
        if fused:
            # one FFI call per rank: the chunk loop (build_rays_test + rendering per chunk) runs inside the library
            k_render = intrinsic if intrinsic.dim() == 2 else intrinsic.mean(0)
            nf_t, nf_r = nf_tgt.reshape(-1)[:2].contiguous(), near_fars[0].reshape(-1)[:2].contiguous()
            vol_cl = ops.channels_last_volume(volume_feature)
            src = imgs[0, :-1].contiguous()

            def render_range(first, n):
                o = ops.render_pixels(vol_cl, src, pose_ref["w2cs"][:V].contiguous(), pose_ref["intrinsics"][:V].contiguous(),
                                      net.packed(args.feat_dim), H, W, k_render, tgt_to_world, k_render if k_ref is None else k_ref,
                                      world_to_ref, nf_t, nf_r, args.N_samples, first_pixel=first, n_pixels=n, pad=args.pad,
                                      white_bkgd=kw.get("white_bkgd", False), ref_hw=ref_hw, batch_rays=batch_rays,
                                      **net.packed_alt(args.feat_dim))
                return o["rgb"], o["depth"]
            rgb, depth = D.render_frame_pixels(render_range, H, W, chunk, device=imgs.device)
            return rgb.reshape(H, W, 3), depth.reshape(H, W)

        def render_chunk(idx):
            rays_pts, rays_dir, rays_NDC, depth_candidates, rays_o, _ = build_rays_test(
                H, W, tgt_to_world, world_to_ref, intrinsic, near_fars, near_fars[-1], args.N_samples, pad=args.pad, chunk=chunk, idx=idx)
            rgb, _, _, depth_pred, _, _ = rendering(args, pose_ref, rays_pts, rays_NDC, depth_candidates, rays_o, rays_dir,
                                                    volume_feature, imgs[:, :-1], img_feat=None, **self.render_kwargs_train)
            return rgb, depth_pred
        rgb, depth = D.render_frame(render_chunk, H, W, chunk)
        return rgb.reshape(H, W, 3), depth.reshape(H, W)

    @torch.no_grad()
    def render_path(self, batch, c2ws_render, hw=None, intrinsic=None, near_far=None, depth_panel=True, crop=False, minmax=None, cmap=None, volume=None):
        """The reference's video loop (renderer_video.ipynb): the scene is encoded ONCE (or `volume` = encode_scene(batch) is used), every pose of
        c2ws_render (K,4,4) is rendered with render_view(batch, volume=, target=) and written as an 8-bit `rgb | depth` frame by ops.frame_u8 straight
        into frame k of the result: uint8 (K, H', W' * panels, 3) on the device, nothing visits the host and the loop never waits on the device.
        hw / intrinsic / near_far: the rendered camera (defaults: the batch's image size, the last view's intrinsics and near / far).
        depth_panel=False: colours only.  crop=True: H // 20 rows and W // 20 columns off every side of each panel, as the notebook; or (rows, columns).
        minmax: the depth range of the colour map - a pair or a (2,) tensor; default the source views' near / far, as the notebooks.
        cmap: a (256,3) uint8 table (default ops.jet_lut, RGB).  utils.save_frames writes the result as PNGs.
        With empty space skipped: render_path_skip_empty (this method's parameter list is pinned by tests/test_render_path_refs.py)."""
        return self._render_path(batch, c2ws_render, hw, intrinsic, near_far, depth_panel, crop, minmax, cmap, volume, None, 0)

    @torch.no_grad()
    def render_path_skip_empty(self, batch, c2ws_render, skip_empty, dilate=0, device_count=False, **render_path_kw):
        """render_path with render_view's skip_empty (a density threshold): the scene is encoded once, its density volume is built ONCE per
        path next to the encode (scene_density(batch, volume, dilate)), and both are handed to every render_view call.  render_path_kw: render_path's
        keywords (hw, intrinsic, near_far, depth_panel, crop, minmax, cmap, volume).  `self.last_live_fraction` is the last frame's.
        device_count: render_view's - one host read per frame, for the fraction, instead of one per sub-batch."""
        skip_empty = _threshold(skip_empty, "render_path_skip_empty(skip_empty=)")       # before the encode; render_view parses it again per frame
        device_count = _device_count(device_count, skip_empty, None, "render_path_skip_empty")
        names = ("hw", "intrinsic", "near_far", "depth_panel", "crop", "minmax", "cmap", "volume")
        unknown = sorted(set(render_path_kw) - set(names))
        if unknown:
            raise TypeError(f"render_path_skip_empty: unexpected keyword(s) {unknown}; render_path's are {list(names)}")
        kw = dict(hw=None, intrinsic=None, near_far=None, depth_panel=True, crop=False, minmax=None, cmap=None, volume=None)
        kw.update(render_path_kw)
        return self._render_path(batch, c2ws_render, *(kw[n] for n in names), skip_empty, dilate, device_count)

    def _render_path(self, batch, c2ws_render, hw, intrinsic, near_far, depth_panel, crop, minmax, cmap, volume, skip_empty, dilate, device_count=False):
        batch = batch_to_device({k: v for k, v in batch.items() if k != "scan"}, self.device)
        _, pose_ref = self.decode_batch(batch)
        dev = self.device
        H, W = (int(batch["images"].shape[-2]), int(batch["images"].shape[-1])) if hw is None else (int(hw[0]), int(hw[1]))
        intrinsic = pose_ref["intrinsics"][-1] if intrinsic is None else torch.as_tensor(intrinsic).to(dev, torch.float32)
        near_far = pose_ref["near_fars"][-1] if near_far is None else torch.as_tensor(near_far).to(dev, torch.float32)
        c2ws = _path_poses(c2ws_render, dev)
        if c2ws.shape[-2] == 3:
            c2ws = torch.cat([c2ws, torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev).expand(c2ws.shape[0], 1, 4)], 1)
        crop, mm, lut, frames = _frame_setup(c2ws.shape[0], H, W, depth_panel, crop, minmax, cmap, pose_ref["near_fars"][0], dev)
        vol = self.encode_scene(batch) if volume is None else volume
        sparse = {} if skip_empty is None else dict(skip_empty=skip_empty, density=self.scene_density(batch, volume=vol, dilate=dilate),
                                                    device_count=device_count)
        for k in range(c2ws.shape[0]):
            rgb, depth = self.render_view(batch, volume=vol, target=dict(hw=(H, W), intrinsic=intrinsic, c2w=c2ws[k], near_far=near_far), **sparse)
            ops.frame_u8(rgb, depth if depth_panel else None, minmax=mm, lut=lut, crop=crop, out=frames[k])
        return frames

    @torch.no_grad()
    def validation_step(self, batch, batch_nb):
        """:172-254.  Renders the batch's last view from the first three (render_view: encode + the chunk loop, tile-parallel over the
        ranks) and returns the reference's per-sample log dict: 'val_psnr', 'val_depth_loss_r', 'val_abs_err', 'mask_sum',
        'val_acc_{t}mm' for t in eval_metric (sums over the mask, as the reference - validation_epoch_end divides by mask_sum).
        Left out: the TensorBoard image grids (`self.logger.experiment.add_images`) and the PNG dump (cv2 colour maps / imageio are
        not in this image); `args.img_downscale = rand*0.75+0.25` (:187) is drawn like the reference but, like there, consumed by
        nothing on the img_feat=None path."""
        args = self.args
        batch = dict(batch)
        batch.pop("scan", None)
        from .evaluate import abs_error, acc_threshold
        from .utils import mse2psnr
        log = {k: torch.tensor([0.0], dtype=torch.float64) for k in
               ["val_psnr", "val_depth_loss_r", "val_abs_err", "mask_sum"] + [f"val_acc_{i}mm" for i in self.eval_metric]}      # init_log, utils.py:23-26
        args.img_downscale = float(torch.rand((1,)) * 0.75 + 0.25)                                       # :187
        rgb, depth_r = self.render_view(batch)                                                          # (H,W,3), (H,W)
        rgb = torch.clamp(rgb.permute(2, 0, 1), 0, 1).cpu()                                             # :207
        depth_r = depth_r.cpu()
        tgt = self.unpreprocess(batch["images"].to(torch.float32).cpu())[0, -1]                            # :193 + :208
        img_err_abs = (rgb - tgt).abs()
        if getattr(args, "with_depth", False):
            depth_gt = batch["depths_h"][0, -1].to(torch.float32).cpu()
            mask = depth_gt > 0
            log["val_psnr"] = mse2psnr(torch.mean(img_err_abs[:, mask] ** 2))                             # :213
            log["val_depth_loss_r"] = self.loss(depth_r, depth_gt, mask)                                # :220
            log["val_abs_err"] = abs_error(depth_r, depth_gt, mask).sum()                               # :229
            for t in self.eval_metric:
                log[f"val_acc_{t}mm"] = acc_threshold(depth_r, depth_gt, mask, t).sum()                 # :230-232
            log["mask_sum"] = mask.float().sum()
        else:
            log["val_psnr"] = mse2psnr(torch.mean(img_err_abs ** 2))                                      # :215
        self.idx += 1
        self.last_val_images = {"rgb": rgb, "depth": depth_r, "err": img_err_abs}                       # what the reference's image grids show
        return log

    def validation_epoch_end(self, outputs):
        """:256-275: the 'val/*' keys."""
        st = lambda k: torch.stack([torch.as_tensor(x[k], dtype=torch.float64).reshape(()) for x in outputs])
        mask_sum = st("mask_sum").sum()
        self.log("val/d_loss_r", st("val_depth_loss_r").mean(), prog_bar=False)
        self.log("val/PSNR", st("val_psnr").mean(), prog_bar=False)
        self.log("val/abs_err", st("val_abs_err").sum() / mask_sum, prog_bar=False)
        for t in self.eval_metric:
            self.log(f"val/acc_{t}mm", st(f"val_acc_{t}mm").sum() / mask_sum, prog_bar=False)

    def save_ckpt(self, name="latest"):
        """:277-288 - same dict keys as the reference's .tar checkpoints."""
        save_dir = f"runs_new/{getattr(self.args, 'expname', 'exp')}/ckpts/"
        os.makedirs(save_dir, exist_ok=True)
        path = f"{save_dir}/{name}.tar"
        torch.save({"global_step": self.global_step, "network_fn_state_dict": self.render_kwargs_train["network_fn"].state_dict(),
                    "network_mvs_state_dict": self.MVSNet.state_dict()}, path)
        return path

    # -- minimal trainer -----------------------------------------------------------------------
    def dp_mode(self):
        """"ray" | "scene" (module docstring); anything else is rejected loudly."""
        mode = getattr(self.args, "dp_mode", "scene")
        if mode not in ("ray", "scene"):
            raise ValueError(f"args.dp_mode must be 'ray' or 'scene', got {mode!r}")
        return mode

    def fit_steps(self, batches, optimizer=None):
        """Lightning-free loop: training_step -> backward -> (flat-buffer all-reduce) -> Adam step.
        dp_mode "ray": `batches` is the same list on every rank; "scene": the list is sharded round-robin over the ranks
        (distributed.scene_shard) and every rank seeds its own pixel-id / jitter streams."""
        if optimizer is None:
            optimizer = self.configure_optimizers()[0][0]
        if self._allreduce is None:
            self._allreduce = D.FlatGradAllReduce(self.grad_vars)
        world, rank = D.world_rank()
        mode = self.dp_mode()
        if world > 1 and mode == "scene":
            batches = D.scene_shard(list(batches))
            if not getattr(self, "_scene_seeded", False):
                torch.manual_seed(torch.initial_seed() + 7919 * rank)      # independent draws per rank from here on
                self._scene_seeded = True
        losses = []
        base_seed = D.common_seed(self.device) if (world > 1 and mode == "ray") else None   # ONE broadcast + host read per call, not per step
        for i, batch in enumerate(batches):
            if base_seed is not None:
                torch.manual_seed(base_seed + i)                             # same pixel ids (CPU RNG) and jitter (device RNG) everywhere
            optimizer.zero_grad(set_to_none=True)
            out = self.training_step(batch, i)
            out["loss"].backward()
            self._allreduce()
            optimizer.step()
            self.global_step += 1
            losses.append(out.get("loss_unscaled", out["loss"]).detach())
        if world > 1 and mode == "scene":
            self.sync_buffers()
        return [float(l) for l in losses]                                   # one host synchronisation, after the last step is enqueued

    def sync_buffers(self):
        """Scene-sharded DP: every rank updates the InPlaceABN running statistics from its own scenes.  Like DDP's default
        broadcast_buffers=True, rank 0's buffers become everybody's (one flat broadcast); the forward pass never reads them
        (MVSNet runs in train mode, batch statistics), so it only matters for what save_ckpt writes."""
        if not D._collective_needed():
            return
        bufs = [b for b in self.MVSNet.buffers() if b.is_floating_point()]
        if not bufs:
            return
        flat = torch.cat([b.reshape(-1) for b in bufs])
        D.broadcast(flat, src=0)
        off = 0
        for b in bufs:
            b.copy_(flat[off:off + b.numel()].view_as(b))
            off += b.numel()


def synthetic_batch(H=512, W=640, seed=1234, **rig_kw):
    """A `MVSDatasetDTU.__getitem__`-shaped batch (collated, B=1) from the seeded synthetic rig."""
    from .synth import make_rig
    rig = make_rig(H, W, seed=seed, **rig_kw)
    return {"images": rig["images"], "proj_mats": rig["proj_mats"], "w2cs": rig["w2cs"], "c2ws": rig["c2ws"],
            "intrinsics": rig["intrinsics"], "near_fars": rig["near_fars"], "depths_h": torch.zeros(1, 4, 1, 1)}


def batch_to_device(batch, device):
    """The collated batch with its tensors on `device` (what a pinned-memory DataLoader + prefetcher hands the step): training_step then
    issues no host-to-device copy of its own."""
    return {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}


def default_args(**over):
    """opt.py defaults of the fields the hot path reads (the reference parses them with configargparse)."""
    import types
    d = dict(expname="exp", pad=24, batch_size=1024, num_epochs=8, pts_dim=3, dir_dim=3, net_type="v0", netdepth=6, netwidth=128,
             lrate=5e-4, chunk=1024, netchunk=1024, ckpt=None, N_samples=128, N_importance=0, perturb=1.0, use_viewdirs=True,
             i_embed=0, multires=10, multires_views=4, raw_noise_std=0.0, white_bkgd=False, img_downscale=1.0,
             use_color_volume=False, with_depth=False, with_depth_loss=False, feat_dim=20, dp_mode="scene", use_amp=False)
    d.update(over)
    return types.SimpleNamespace(**d)


# ------------------------------------------------------------------ per-scene fine-tuning (reference train_mvs_nerf_finetuning_pl.py)
def dda(rays_o, rays_d, bbox_3D):
    """reference data/ray_utils.py:143-150: entry and exit depth (N,1) of each ray against the axis-aligned box bbox_3D (2,3).  Host-side torch
    (ops.ray_march_bbox holds the same arithmetic on the device)."""
    inv = 1.0 / (rays_d + 1e-6)
    t = torch.stack(((bbox_3D[:1] - rays_o) * inv, (bbox_3D[1:] - rays_o) * inv))
    return (torch.max(torch.min(t, dim=0)[0], dim=-1, keepdim=True)[0],
            torch.min(torch.max(t, dim=0)[0], dim=-1, keepdim=True)[0])


def ray_marcher(rays, N_samples=64, lindisp=False, perturb=0, bbox_3D=None):
    """reference data/ray_utils.py:152-197: rays (N,8) = [o(3) | d(3) | near | far] -> z-sampled points.
    Host-side torch like the reference (it owns the jitter draw); with bbox_3D (2,3) near / far come from dda and the whole
    march is one kernel behind the draw (ops.ray_march_bbox)."""
    n = rays.shape[0]
    if bbox_3D is not None:
        with torch.no_grad():
            jitter = torch.rand((n, N_samples), device=rays.device) if perturb > 0 else None
            pts, _, z = ops.ray_march_bbox(rays, bbox_3D, N_samples, lindisp=lindisp, perturb=perturb, jitter=jitter)
        return pts, rays[:, 0:3], rays[:, 3:6], z
    rays_o, rays_d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8]
    steps = torch.linspace(0, 1, N_samples, device=rays.device)
    z = near * (1 - steps) + far * steps if not lindisp else 1 / (1 / near * (1 - steps) + 1 / far * steps)
    z = z.expand(n, N_samples)
    if perturb > 0:
        mid = 0.5 * (z[:, :-1] + z[:, 1:])
        upper, lower = torch.cat([mid, z[:, -1:]], -1), torch.cat([z[:, :1], mid], -1)
        z = lower + (upper - lower) * (perturb * torch.rand(z.shape, device=rays.device))
    return rays_o.unsqueeze(1) + rays_d.unsqueeze(1) * z.unsqueeze(2), rays_o, rays_d, z


def sample_pdf(bins, weights, N_samples, det=False, pytest=False, u=None):
    """reference data/ray_utils.py:96-139.  The uniform draw stays here (torch.rand on the device like :109, or `u` supplied);
    CDF construction + inversion is one HIP kernel (one wave per ray)."""
    if pytest:
        raise NotImplementedError("sample_pdf(pytest=True) overwrites u with numpy's RNG in the reference; pass u= instead")
    shape = list(weights.shape[:-1]) + [N_samples]
    if u is None:
        u = (torch.linspace(0.0, 1.0, steps=N_samples, device=weights.device).expand(shape) if det
             else torch.rand(shape, device=weights.device))
    return ops.sample_pdf(bins.detach(), weights.detach(), u.contiguous())


def ray_marcher_fine(rays, density_volume, z_vals, pts_NDC, N_importance=64, lindisp=False, u=None):
    """reference data/ray_utils.py:199-224: importance samples from the density volume merged into the coarse depths.
    Returns (xyz (N,S+NI,3), rays_o, rays_d, z_vals (N,S+NI)).  Density lookup, weights, sample_pdf and the sort are one
    kernel; `u` is the torch.rand draw of sample_pdf (drawn here when not supplied)."""
    rays_o, rays_d = rays[:, 0:3], rays[:, 3:6]
    if u is None:
        u = torch.rand((rays.shape[0], N_importance), device=rays.device)
    with torch.no_grad():
        z = ops.ray_marcher_fine_z(density_volume.detach(), pts_NDC.detach(), z_vals.detach(), u)
        xyz, _ = ops.ray_points(rays_o, rays_d, z)
    return xyz, rays_o, rays_d, z


def _skip_empty_train(args):
    """The switch of DESIGN.md 4g, read from args so that default_args stays as it is: None (args.skip_empty_train unset or None: the dense step), or
    (threshold, dilate, refresh): args.skip_empty_dilate (default 1 voxel, 4f's recommendation) and args.skip_empty_refresh (default 200 steps,
    train_mvs_nerf_finetuning_pl.py:144-145's cadence)."""
    thr = getattr(args, "skip_empty_train", None)
    if thr is None:
        return None
    thr = _threshold(thr, "args.skip_empty_train")
    refresh = int(getattr(args, "skip_empty_refresh", 200))
    if refresh < 1:
        raise ValueError(f"args.skip_empty_refresh must be >= 1 step, got {refresh}")
    return thr, int(getattr(args, "skip_empty_dilate", 1)), refresh


def _refresh_train_density(system, sparse, build_density):
    """The training density of a system with args.skip_empty_train set: `system.train_density` (D,H,W), build_density(dilate) on first use and at
    every later multiple of args.skip_empty_refresh steps (an assigned tensor is kept until then).  system.density_volume is not touched."""
    _, dilate, refresh = sparse
    _need_fused(system.network_fn, system.render_kwargs_train, "args.skip_empty_train")
    if getattr(system, "train_density", None) is None or (system.global_step > 0 and system.global_step % refresh == 0):
        system.train_density = build_density(dilate)


def _sparse_training_render(system, sparse, volume, imgs, w2cs, intrinsics, pts, ndc, z_vals, rays_d, dp_samples):
    """The render call of a fine-tuning step with args.skip_empty_train set: ops.raymarch_sparse_train against system.train_density.  Sets
    system.last_live_fraction (live samples over samples of this step).  Returns rgb_map."""
    thr = sparse[0]
    net, kw = system.network_fn, system.render_kwargs_train
    white = bool(kw.get("white_bkgd", getattr(system.args, "white_bkgd", False)))
    o = ops.raymarch_sparse_train(volume, imgs, w2cs, intrinsics, net, pts.contiguous(), ndc.contiguous(), z_vals.contiguous(), rays_d.contiguous(),
                                  system.train_density, thr, white_bkgd=white, dp_samples=dp_samples)
    system.last_live_fraction = o["n_live"] / z_vals.numel() if z_vals.numel() else 0.0
    return o["rgb_map"]


def _fit_loop(system, steps, optimizer):
    """The optimisation loop of the per-scene systems, over an iterable of callables that each run one training step and return {'loss'}:
    step -> backward -> gradient exchange -> Adam; with args.dp_volume_grad == "samples" the volume is re-broadcast from rank 0 every
    args.dp_volume_resync steps (default 200) so that last-bit differences of the atomics-ordered scatters cannot add up.  Returns the losses."""
    if optimizer is None:
        optimizer = system.configure_optimizers()[0][0]
    if system._allreduce is None:
        system._allreduce = D.FlatGradAllReduce(system.grad_vars)
    resync = int(getattr(system.args, "dp_volume_resync", 200))
    losses = []
    for step in steps:
        optimizer.zero_grad(set_to_none=True)
        out = step()
        out["loss"].backward()
        system._allreduce()
        optimizer.step()
        system.global_step += 1
        if getattr(system.args, "dp_volume_grad", "allreduce") == "samples" and resync > 0 and system.global_step % resync == 0 and D._collective_needed():
            D.broadcast(ops.channels_last_volume(system.volume.feat_volume.data), src=0)     # the (D,H,W,C) view of the same memory
        losses.append(out["loss"].detach())
    return [float(l) for l in losses]                                   # one host synchronisation, after the last step is enqueued


def _scene_index_batches(scene, n_steps, batch_size, seed):
    """The index batches of n_steps steps over a rays.SceneRays bank: scene.epoch(batch_size) after scene.epoch, every epoch's permutation drawn
    from ONE generator on the bank's device seeded with `seed` (the global generators are not touched)."""
    g = torch.Generator(device=scene.device).manual_seed(int(seed))
    n_steps, done = int(n_steps), 0
    while done < n_steps:
        for idx in scene.epoch(int(batch_size), generator=g):
            if done == n_steps:
                return
            done += 1
            yield idx


class MVSSystemFinetune(_ModuleShim):
    """reference train_mvs_nerf_finetuning_pl.py:32-189: the scene is encoded ONCE (`init_volume`), the 8-channel
    volume becomes a learnable `RefVolume` (checkpoint key `volume.feat_volume`) and only the ray march runs per step;
    gradients flow to the MLP and to the volume (trilinear scatter kernel)."""

    def __init__(self, args, source_views, n_depth_planes=128):
        """source_views = (imgs (1,V,3,H,W) normalised, proj_mats (1,V,3,4), near_far (2,), pose_source dict) -
        what `dataset.read_source_views()` returns in the reference."""
        super().__init__()
        from .models import RefVolume
        self.args = args
        self.args.feat_dim = 8 + 4 * int(getattr(args, "n_views", 3))       # :39 hard-wires 3 source views (8 + 3*4); n_views is the config-4 extension
        if int(args.netwidth) == ops.WIDE_WIDTH:                            # this system trains the MLP; before anything is built or loaded
            raise NotImplementedError(f"MVSSystemFinetune: {WIDE_TRAINING_MSG}")
        if getattr(args, "use_color_volume", False) and getattr(args, "use_density_volume", False):
            raise NotImplementedError("--use_color_volume together with --use_density_volume: update_density_volume would concatenate the "
                                      "colours to a volume that already holds them (train_mvs_nerf_finetuning_pl.py:96); not supported")
        kw_train, _, _, self.grad_vars = create_nerf_mvs(args, use_mvs=True, dir_embedder=False, pts_embedder=True)
        for k in ("N_samples", "ndc", "lindisp"):
            kw_train.pop(k, None)
        self.render_kwargs_train = kw_train
        self.MVSNet = kw_train.pop("network_mvs")
        self.MVSNet.D = n_depth_planes
        self.network_fn = kw_train["network_fn"]
        imgs, proj_mats, near_far, pose = source_views
        dev = next(self.MVSNet.parameters()).device
        self.near_far_source = near_far.to(dev)
        self.pose_source = {k: v.to(dev) for k, v in pose.items()}
        # init_volume :57-66: a checkpoint written by save_ckpt of THIS class carries the optimised volume - resume from it
        # instead of re-encoding (the reference does the same); otherwise encode the scene once
        vol = None
        ck_path = getattr(args, "ckpt", None)
        if ck_path and ck_path != "None" and os.path.exists(ck_path):
            ckpts = torch.load(ck_path, map_location="cpu", weights_only=False)
            if "volume" in ckpts:
                vol = ckpts["volume"]["feat_volume"].to(dev, torch.float32)
                self.volume_from_ckpt = True
        if vol is None:
            self.volume_from_ckpt = False
            self.MVSNet.train()                                           # :62
            with torch.no_grad():
                vol, _, _ = self.MVSNet(imgs.to(dev), proj_mats.to(dev), self.near_far_source, pad=args.pad, lindisp=getattr(args, "use_disp", False))
        self.imgs = MVSSystem.unpreprocess(imgs.to(dev))
        # importance sampling from a density volume (:73-86): voxel positions + per-voxel colour features, once per scene
        self.density_volume = None
        use_cv, use_dv = bool(getattr(args, "use_color_volume", False)), bool(getattr(args, "use_density_volume", False))
        if use_cv or use_dv:
            from .utils import build_color_volume
            Dv, Hv, Wv = vol.shape[-3:]
            vox_pts = self._voxel_points(Dv, Hv, Wv)
            with torch.no_grad():
                self.color_feature = build_color_volume(vox_pts, self.pose_source, self.imgs, with_mask=True)   # (D*H, W, 4V)
            if use_cv and vol.shape[1] == 8:
                # :79-80: the projected colours become 4V extra channels of the learnable volume (a checkpoint written by this class
                # already holds all 8+4V channels; the reference would concatenate a second copy there, :66 + :80)
                cf = self.color_feature.reshape(Dv, Hv, Wv, -1).permute(3, 0, 1, 2).unsqueeze(0)
                vol = torch.cat((vol, cf), dim=1)
            if use_dv:
                self.vox_pts = vox_pts
        self.volume = RefVolume(vol.detach())
        self.grad_vars = [p for p in self.network_fn.parameters()] + list(self.volume.parameters())    # MVSNet stays frozen here
        self._allreduce = None
        # Data parallelism (rays of the scene's all-rays buffer sharded over the ranks): args.dp_volume_grad selects how the gradient of
        # the 150-246 MB volume is combined - "samples" (default): all_gather of the per-sample feature gradients + a local scatter on
        # every rank (ops.volume_grad_from_all_ranks: 6 MB per step instead of a volume-sized all-reduce); "allreduce": the volume joins
        # the flat all-reduce of the MLP gradients.
        if not hasattr(args, "dp_volume_grad"):
            args.dp_volume_grad = "samples"
        if args.dp_volume_grad not in ("samples", "allreduce"):
            raise ValueError("args.dp_volume_grad must be 'samples' or 'allreduce'")
        if args.dp_volume_grad == "samples":
            self._allreduce = D.FlatGradAllReduce([p for p in self.network_fn.parameters()])           # the volume gradient arrives complete

    def _voxel_points(self, Dv, Hv, Wv):
        """:73-77: the voxel centres of the reference frustum, (D*H, W, 3)."""
        from .utils import get_ptsvolume
        intrinsic, c2w = self.pose_source["intrinsics"][0].clone(), self.pose_source["c2ws"][0]
        intrinsic[:2] /= 4
        return get_ptsvolume(Hv - 2 * self.args.pad, Wv - 2 * self.args.pad, Dv, self.args.pad, self.near_far_source, intrinsic, c2w).contiguous()

    def _render_space_density(self, dilate=0):
        """The renderer-consistent density of the current volume and MLP -> (D,H,W): what update_density_volume(render_space=True) assigns to
        self.density_volume and what a step with args.skip_empty_train keeps in self.train_density."""
        V = self.imgs.shape[1]
        vol = self.volume.feat_volume.detach()
        H, W = self.imgs.shape[-2:]
        with torch.no_grad():
            return ops.node_density(dilate=dilate, **_density_sources(
                self.network_fn, self.args.feat_dim, vol, self.pose_source, V, self.imgs[0] if vol.shape[1] == 8 else None, near_far=self.near_far_source,
                ref_hw=(int(H), int(W)), pad=self.args.pad, lindisp=bool(getattr(self.args, "use_disp", False))))

    def update_density_volume(self, render_space=False, dilate=0):
        """:91-99: sigma of every voxel centre from the current volume + MLP (forward_alpha queries), -> (D,H,W).
        Under --use_density_volume the voxel positions and colour features are the ones __init__ built.  Any other system builds what is missing
        on first use (render_rays(skip_empty=) needs the density of a scene that was fine-tuned without importance sampling); a colour volume's
        feature rows are its own 8 + 4V channels - the colours were projected into it once, :79-80.
        render_space=False (default) is that reference-faithful volume, bit for bit: like :76,98 it hands the MLP the WORLD positions of the voxel
        centres as its point input, where the renderer hands it NDC coordinates (renderer.py:156) - so its values are not the sigma the ray march
        sees at those voxels.  It is what the reference's importance sampling (args.N_importance) was trained and tuned with: keep it for that.
        render_space=True builds the renderer-consistent volume instead (ops.node_density: the ray march's own lookups and MLP entry at the nodes'
        NDC coordinates; dilate widens the occupied region, ops.max_dilate3d) - the one to use with render_rays(skip_empty=): a sample is dropped
        because the density the renderer would compute around it is below the threshold, not because another function of the same weights is
        (DESIGN.md 4e, 4f).  dilate is read with render_space=True only."""
        if render_space:
            self.density_volume = self._render_space_density(dilate)
            return
        from .renderer import render_density
        with torch.no_grad():
            Dv, Hv, Wv = self.volume.feat_volume.shape[-3:]
            vol_cl = ops.channels_last_volume(self.volume.feat_volume.detach())                     # (D,H,W,8) or (D,H,W,8+4V)
            if getattr(self, "vox_pts", None) is None:
                self.vox_pts = self._voxel_points(Dv, Hv, Wv)
            C = vol_cl.shape[-1]
            if C == self.args.feat_dim and C != 8:
                features = vol_cl.reshape(Dv * Hv, Wv, C)
            else:
                if getattr(self, "color_feature", None) is None:
                    from .utils import build_color_volume
                    self.color_feature = build_color_volume(self.vox_pts, self.pose_source, self.imgs, with_mask=True)   # (D*H, W, 4V)
                features = torch.cat((vol_cl.reshape(Dv * Hv, Wv, 8), self.color_feature), -1)       # = cat(...).permute(0,2,3,4,1) :96
            self.density_volume = render_density(self.network_fn, self.vox_pts, features,
                                                 self.render_kwargs_train["network_query_fn"]).reshape(Dv, Hv, Wv)

    def training_step(self, batch, batch_nb):
        """:140-189.  batch = {'rays': (1,B,8), 'rgbs': (1,B,3)} from the all-rays buffer.
        args.skip_empty_train (None / unset: the dense step below, untouched): a density threshold - the MLP's forward and backward run on the samples
        that are live against self.train_density, the renderer-consistent density of the scene dilated by args.skip_empty_dilate voxels (default 1) and
        rebuilt every args.skip_empty_refresh steps (default 200); ops.raymarch_sparse_train, DESIGN.md 4g.  self.last_live_fraction is the step's."""
        args = self.args
        self._step_prologue()
        rays, target = batch["rays"].squeeze(0).to(self.imgs.device), batch["rgbs"].squeeze(0).to(self.imgs.device)
        lindisp = getattr(args, "use_disp", False)
        pts, rays_o, rays_d, z_vals = ray_marcher(rays, N_samples=args.N_samples, lindisp=lindisp, perturb=args.perturb)
        pts, ndc = self._to_ndc(rays_o, rays_d, z_vals)
        return self._step_body(rays, target, rays_o, rays_d, z_vals, pts, ndc)

    def _step_prologue(self):
        """What a step does before it forms its rays: the training density of args.skip_empty_train and the density volume of :144-145."""
        sparse = _skip_empty_train(self.args)
        if sparse is not None:
            _refresh_train_density(self, sparse, self._render_space_density)
        if getattr(self.args, "use_density_volume", False) and 0 == self.global_step % 200:         # :144-145
            self.update_density_volume()

    def _ref_camera(self):
        """The reference camera of get_ndc_coordinate (:150-156) in the form ops.scene_rays_march takes: (w2c, K, near_far, (H, W), pad)."""
        H, W = self.imgs.shape[-2:]
        return self.pose_source["w2cs"][0], self.pose_source["intrinsics"][0], self.near_far_source, (H, W), self.args.pad

    def _to_ndc(self, rays_o, rays_d, z):
        """o + d*z and get_ndc_coordinate (:150-156) in one kernel."""
        w2c, K, nf, hw, pad = self._ref_camera()
        return ops.ray_points(rays_o, rays_d, z, w2c, K, nf, ref_hw=hw, pad=pad, lindisp=getattr(self.args, "use_disp", False))

    def _step_body(self, rays, target, rays_o, rays_d, z_vals, pts, ndc):
        """A step behind ray_marcher / get_ndc_coordinate (:158-189), shared by training_step (rays from the batch) and fit_scene (rays, depths, points
        and NDC coordinates from one ops.scene_rays_march launch): importance sampling, the render, the loss."""
        args = self.args
        sparse = _skip_empty_train(args)
        if self.density_volume is not None and getattr(args, "N_importance", 0) > 0:                # :158-163
            pts, rays_o, rays_d, z_vals = ray_marcher_fine(rays, self.density_volume, z_vals, ndc, N_importance=args.N_importance)
            pts, ndc = self._to_ndc(rays_o, rays_d, z_vals)
        with ops.mlp_precision("bf16" if getattr(args, "use_amp", False) else ops.MLP_PRECISION):
            if sparse is not None:
                V = self.imgs.shape[1]
                vol = self.volume.feat_volume
                rgbs = _sparse_training_render(self, sparse, vol, self.imgs[0].contiguous(), self.pose_source["w2cs"][:V].contiguous(),
                                               self.pose_source["intrinsics"][:V].contiguous(), pts, ndc, z_vals, rays_d,
                                               getattr(args, "dp_volume_grad", "allreduce") == "samples" and vol.requires_grad)
            else:
                rgbs, _, _, depth_pred, _, _ = rendering(args, self.pose_source, pts, ndc, z_vals, rays_o, rays_d, self.volume, self.imgs,
                                                         **self.render_kwargs_train)
        img_loss = img2mse(rgbs, target)
        with torch.no_grad():
            self.log("train/loss", img_loss, prog_bar=True)
            self.log("train/PSNR", mse2psnr2(img_loss), prog_bar=True)
        return {"loss": img_loss}

    # -- rendering the fine-tuned scene (train_mvs_nerf_finetuning_pl.py:192-252) ---------------------
    @torch.no_grad()
    def render_rays(self, rays, chunk=None, batch_rays=16384, u=None, whole_frame_off=False, skip_empty=None, device_count=False, early_stop=None,
                    stop_every=32):
        """The rendering part of the fine-tuning script's validation_step (:204-237) for the dataset's rays (N,8) = [o | d | near | far]: per
        chunk ray_marcher -> get_ndc_coordinate -> [ray_marcher_fine, when a density volume exists and args.N_importance > 0] -> rendering, from
        the learnt `self.volume` (8 channels + the source images, or the (8 + 4V)-channel colour volume of --use_color_volume).  Returns
        (rgb (N,3), depth (N,)).  One library call per rank (ops.render_rays: the chunk loop runs inside the library), the rays sharded over the
        ranks in contiguous chunk ranges exactly as MVSSystem.render_view shards pixels.
        u: the (N, N_importance) uniform draw of sample_pdf (drawn once with torch.rand when None).  batch_rays: rays per sub-batch inside the
        library call (free parameter: the results do not depend on it).  whole_frame_off=True runs the reference's per-chunk Python loop
        (ray_marcher -> ops.ray_points -> ray_marcher_fine -> rendering) instead; both produce the same values.
        skip_empty: None (default) is the dense render above, untouched.  A float is a density threshold: samples whose trilinear cell in
        `self.density_volume` (update_density_volume()) holds no value above it are not sent through the MLP - their raw is (0,0,0,0), the
        others have the bits of the dense sequence (ops.raymarch_sparse).  The frame then runs per sub-batch of batch_rays rays (ray_marcher ->
        ops.ray_points -> [ray_marcher_fine] -> ops.raymarch_sparse: _render_sparse_batches), the sub-batches sharded over the ranks, one host read of the live count per
        sub-batch; `self.last_live_fraction` is this rank's live samples over its samples.
        early_stop / stop_every: as MVSSystem.render_view - alone it needs no density volume, with skip_empty it uses that one;
        with N_importance > 0 the merged depths are simply a larger S.  `self.last_stopped_fraction` is this rank's stopped rays over its rays.
        device_count: as MVSSystem.render_view - the sparse sub-batches without a host read, the same values."""
        stop = _early_stop(early_stop, stop_every, "render_rays")          # refusals first: nothing below needs the library before them
        device_count = _device_count(device_count, skip_empty, stop, "render_rays")
        if stop is not None and whole_frame_off:
            raise ValueError("render_rays: early_stop runs its own per-sub-batch loop; it cannot be combined with whole_frame_off=True")
        if skip_empty is not None:
            if whole_frame_off:
                raise ValueError("render_rays: skip_empty runs its own per-sub-batch loop; it cannot be combined with whole_frame_off=True")
            skip_empty = _threshold(skip_empty, "render_rays(skip_empty=)")
            if getattr(self, "density_volume", None) is None:
                raise RuntimeError("render_rays: skip_empty needs the scene's density volume; call update_density_volume() first")
        args = self.args
        chunk = int(chunk or args.chunk)
        dev = self.imgs.device
        rays = rays.reshape(-1, 8).to(dev, torch.float32).contiguous()
        N = rays.shape[0]
        if N == 0:
            return torch.empty((0, 3), device=dev), torch.empty((0,), device=dev)
        lindisp = bool(getattr(args, "use_disp", False))
        white = bool(self.render_kwargs_train.get("white_bkgd", getattr(args, "white_bkgd", False)))
        H, W = self.imgs.shape[-2:]
        w2c_ref, K_ref = self.pose_source["w2cs"][0], self.pose_source["intrinsics"][0]
        NI = int(getattr(args, "N_importance", 0) or 0)
        fine = self.density_volume is not None and NI > 0
        if fine:
            u = torch.rand((N, NI), device=dev) if u is None else u.to(dev, torch.float32).contiguous()
            if tuple(u.shape) != (N, NI):
                raise RuntimeError(f"render_rays: u must be ({N}, {NI}), got {tuple(u.shape)}")
        kw = self.render_kwargs_train
        V = self.imgs.shape[1]
        vol = self.volume.feat_volume
        who = "render_rays (whole_frame_off=True runs the per-chunk loop)"

        def march(idx, n):          # rays [idx * n, (idx + 1) * n) -> (pts, ndc, z, rays_o, rays_d): the per-chunk Python loop's and the sparse loop's samples
            r = rays[idx * n:(idx + 1) * n]
            _, rays_o, rays_d, z = ray_marcher(r, N_samples=args.N_samples, lindisp=lindisp)
            pts, ndc = ops.ray_points(rays_o, rays_d, z, w2c_ref, K_ref, self.near_far_source, ref_hw=(H, W), pad=args.pad, lindisp=lindisp)
            if fine:
                pts, rays_o, rays_d, z = ray_marcher_fine(r, self.density_volume, z, ndc, N_importance=NI, u=u[idx * n:(idx + 1) * n].contiguous())
                pts, ndc = ops.ray_points(rays_o, rays_d, z, w2c_ref, K_ref, self.near_far_source, ref_hw=(H, W), pad=args.pad, lindisp=lindisp)
            return pts, ndc, z, rays_o, rays_d

        if whole_frame_off:
            def render_chunk(idx):
                pts, ndc, z, rays_o, rays_d = march(idx, chunk)
                rgb, _, _, depth, _, _ = rendering(args, self.pose_source, pts, ndc, z, rays_o, rays_d.contiguous(), self.volume, self.imgs, **kw)
                return rgb, depth
            return D.render_frame(render_chunk, 1, N, chunk)

        if skip_empty is not None or stop is not None:
            src = _sparse_sources(self, vol, self.pose_source, V, self.imgs[0], who)
            if skip_empty is not None:
                src.update(density=self.density_volume, thr=skip_empty)
            B = max(int(batch_rays), 1)

            def make_batch(idx):
                pts, ndc, z, _, rays_d = march(idx, B)
                return pts, ndc, z.contiguous(), rays_d.contiguous()
            return _render_sparse_batches(self, N, B, make_batch, dict(src, vol_cl=ops.channels_last_volume(vol)), early_stop=stop, device_count=device_count)
        net, color_vol = _sparse_config(self, vol, V, who)
        vol_cl = ops.channels_last_volume(vol)
        t = torch.linspace(0, 1, args.N_samples, device=dev)
        src = {} if color_vol else dict(imgs=self.imgs[0].contiguous(), w2cs=self.pose_source["w2cs"][:V].contiguous(),
                                        intrinsics=self.pose_source["intrinsics"][:V].contiguous())
        if fine:
            src.update(density=self.density_volume, u=u)

        def render_range(first, n):
            o = ops.render_rays(vol_cl, rays, t, net.packed(args.feat_dim), K_ref, w2c_ref, self.near_far_source, (H, W), V, first_ray=first, n_rays=n,
                                pad=args.pad, lindisp=lindisp, white_bkgd=white, batch_rays=batch_rays, **src, **net.packed_alt(args.feat_dim))
            return o["rgb"], o["depth"]
        return D.render_frame_pixels(render_range, 1, N, chunk, device=dev)

    @torch.no_grad()
    def render_path(self, c2ws_render, hw, focal, depth_panel=True, crop=False, minmax=None, cmap=None, device_count=False, **render_rays_kw):
        """The video loop of renderer_video.ipynb for the fine-tuned scene: per pose of c2ws_render (K,4,4) the notebook's rays (get_ray_directions(H, W,
        focal) / get_rays, the source near / far) -> render_rays -> ops.frame_u8 into frame k.  Returns uint8 (K, H', W' * panels, 3) on the device;
        depth_panel / crop / minmax / cmap as MVSSystem.render_path (minmax defaults to the source near / far); device_count and the other keywords go to
        render_rays (device_count=True with skip_empty / early_stop: one host read per frame)."""
        _device_count(device_count, render_rays_kw.get("skip_empty"), render_rays_kw.get("early_stop"), "render_path")
        return _render_path_rays(self, c2ws_render, hw, focal, self.near_far_source, depth_panel, crop, minmax, cmap, self.imgs.device,
                                 device_count=device_count, **render_rays_kw)

    @torch.no_grad()
    def validation_step(self, batch, batch_nb):
        """:192-252.  batch = {'rays': (1,N,8) | (N,8), 'rgbs': (1,H,W,3) | (H,W,3) | (N,3)} - one view of the val split.  Renders the rays
        (render_rays) and returns the reference's log dict: 'val_psnr_all'.  Left out, as in MVSSystem.validation_step: the TensorBoard
        image grids and the PNG dump; `last_val_images` keeps what they show.  The reference re-scales the reference intrinsics and the pad
        by imgScale_test / imgScale_train (:215-218); only ratio 1 is supported."""
        args = self.args
        ratio = float(getattr(args, "imgScale_test", 1.0)) / float(getattr(args, "imgScale_train", 1.0))
        if ratio != 1.0:
            raise NotImplementedError("validation_step: imgScale_test / imgScale_train != 1 re-scales the reference intrinsics and the volume's pad "
                                      f"(train_mvs_nerf_finetuning_pl.py:215-218); only ratio 1 is supported, got {ratio}")
        from .utils import mse2psnr
        rays = batch["rays"].reshape(-1, 8)
        img = batch["rgbs"].to(torch.float32).cpu()
        img = img[0] if img.dim() == 4 else img                                                          # (H,W,3) or (N,3)
        rgb, depth = self.render_rays(rays)
        rgb = torch.clamp(rgb.cpu().reshape(img.shape), 0, 1)                                           # :237
        depth = depth.cpu().reshape(img.shape[:-1])
        img_err_abs = (rgb - img).abs()
        log = {"val_psnr_all": mse2psnr(torch.mean(img_err_abs ** 2))}                                    # :240
        self.idx = getattr(self, "idx", 0) + 1
        self.last_val_images = {"rgb": rgb, "depth": depth, "err": img_err_abs}
        return log

    def validation_epoch_end(self, outputs):
        """:254-276 (the with_depth keys need logs this validation_step does not produce, as in the reference's own)."""
        self.log("val/PSNR_all", torch.stack([torch.as_tensor(x["val_psnr_all"], dtype=torch.float64).reshape(()) for x in outputs]).mean(), prog_bar=True)

    def save_ckpt(self, name="latest"):
        """:277-291 of the fine-tuning script: adds the `volume` state dict."""
        save_dir = f"runs_fine_tuning/{getattr(self.args, 'expname', 'exp')}/ckpts/"
        os.makedirs(save_dir, exist_ok=True)
        path = f"{save_dir}/{name}.tar"
        torch.save({"global_step": self.global_step, "network_fn_state_dict": self.network_fn.state_dict(),
                    "volume": self.volume.state_dict(), "network_mvs_state_dict": self.MVSNet.state_dict()}, path)
        return path

    def dp_mode(self):
        return "data"          # every rank feeds its own slice of the all-rays buffer; nothing to slice or re-seed in the step

    def fit_steps(self, batches, optimizer=None):
        """training_step -> backward -> gradient exchange -> Adam; with args.dp_volume_grad == "samples" the volume is re-broadcast from
        rank 0 every args.dp_volume_resync steps (default 200) so that last-bit differences of the atomics-ordered scatters cannot add up."""
        return _fit_loop(self, ((lambda batch=batch, i=i: self.training_step(batch, i)) for i, batch in enumerate(batches)), optimizer)

    def fit_scene(self, scene, n_steps, batch_size=None, seed=0, optimizer=None):
        """fit_steps fed by a rays.SceneRays bank instead of batches: n_steps steps over the index batches of scene.epoch(batch_size) (default
        args.batch_size; a new epoch starts when one is exhausted) shuffled by a generator seeded with `seed`.  Each step is ONE
        ops.scene_rays_march launch - rays, target colours, stratified depths, points and their NDC coordinates in the reference camera - and then
        the body of training_step; with args.perturb > 0 a step draws torch.rand((B, S)) from the global device generator, the one draw
        ray_marcher makes.  The step of training_step on {'rays', 'rgbs'} = scene.gather(idx) computes the same bits.  Returns the
        losses; one host synchronisation, after the last step is enqueued."""
        args = self.args
        S, lindisp, ref = int(args.N_samples), getattr(args, "use_disp", False), self._ref_camera()

        def step(idx):
            self._step_prologue()
            jitter = torch.rand((idx.shape[0], S), device=idx.device) if args.perturb > 0 else None
            m = scene.march(idx, S, perturb=args.perturb, jitter=jitter, lindisp=lindisp, ref=ref)
            rays = m["rays"]
            return self._step_body(rays, m["rgbs"], rays[:, 0:3], rays[:, 3:6], m["z_vals"], m["pts"], m["ndc"])
        batches = _scene_index_batches(scene, n_steps, batch_size or args.batch_size, seed)
        return _fit_loop(self, ((lambda idx=idx: step(idx)) for idx in batches), optimizer)

    def configure_optimizers(self):
        self.optimizer = _adam(self.grad_vars, self.args.lrate)
        return [self.optimizer], []


# ------------------------------------------------------------------ fused-scene fine-tuning (reference train_mvs_nerf_fusion_finetuning_pl.py)
def get_ray_directions(H, W, focal, center=None):
    """reference data/ray_utils.py:12-29: camera-space directions (H,W,3) of every pixel, no half-pixel offset; focal = (fx, fy) or one number."""
    f = torch.as_tensor(focal, dtype=torch.float32).reshape(-1)
    fx, fy = (f[0], f[0]) if f.numel() == 1 else (f[0], f[1])
    j, i = torch.meshgrid(torch.linspace(0, H - 1, H), torch.linspace(0, W - 1, W), indexing="ij")
    cent = center if center is not None else [W / 2, H / 2]
    return torch.stack([(i - cent[0]) / fx, (j - cent[1]) / fy, torch.ones_like(i)], -1)


def get_rays(directions, c2w):
    """reference data/ray_utils.py:32-53: (rays_o, rays_d), both (H*W, 3), un-normalised directions."""
    rays_d = directions @ c2w[:3, :3].T
    return c2w[:3, 3].expand(rays_d.shape).reshape(-1, 3), rays_d.reshape(-1, 3)


# ------------------------------------------------------------------ camera path -> 8-bit frames (reference renderer_video.ipynb)
def _path_poses(c2ws_render, dev):
    """(K,4,4) | (K,3,4) poses (numpy from utils.gen_render_path / pose_spherical_dtu, or tensors) as one fp32 device tensor: one upload for the path."""
    c2ws = torch.as_tensor(c2ws_render).to(dev, torch.float32)
    if c2ws.dim() != 3 or c2ws.shape[-1] != 4 or c2ws.shape[-2] not in (3, 4):
        raise ValueError(f"render_path: c2ws_render must be (K,4,4) or (K,3,4), got {tuple(c2ws.shape)}")
    return c2ws


def _frame_setup(K, H, W, depth_panel, crop, minmax, cmap, near_far, dev):
    """What every frame of a path shares, built once so that the loop issues launches only: the crop (the notebook's H // 20, W // 20), the depth
    range as a device tensor (default: the source near / far, `visualize_depth_numpy(depth, near_far_source)`), the colour table, the output."""
    crop = (H // 20, W // 20) if crop is True else ((0, 0) if not crop else (int(crop[0]), int(crop[1])))
    if minmax is None:
        minmax = near_far
    mm = (minmax.to(dev, torch.float32) if torch.is_tensor(minmax) else torch.tensor([float(minmax[0]), float(minmax[1])]).to(dev)).reshape(-1)[:2].contiguous()
    lut = ops.jet_lut(dev) if cmap is None else torch.as_tensor(cmap).reshape(256, 3).to(dev, torch.uint8).contiguous()
    frames = torch.empty((K, H - 2 * crop[0], (W - 2 * crop[1]) * (2 if depth_panel else 1), 3), device=dev, dtype=torch.uint8)
    return crop, mm, lut, frames


def _path_rays(directions, c2w, near_far):
    """The notebook's (H*W, 8) rays of one pose: get_rays, then the source near / far in columns 6 and 7."""
    rays_o, rays_d = get_rays(directions, c2w)
    nf = near_far.reshape(-1)
    return torch.cat([rays_o, rays_d, nf[0] * torch.ones_like(rays_o[:, :1]), nf[1] * torch.ones_like(rays_o[:, :1])], 1)


def _render_path_rays(system, c2ws_render, hw, focal, near_far, depth_panel, crop, minmax, cmap, dev, **kw):
    """render_path of the systems that render rays: per pose the notebook's rays -> system.render_rays -> ops.frame_u8 into frame k."""
    H, W = int(hw[0]), int(hw[1])
    c2ws = _path_poses(c2ws_render, dev)
    near_far = near_far.to(dev, torch.float32)
    crop, mm, lut, frames = _frame_setup(c2ws.shape[0], H, W, depth_panel, crop, minmax, cmap, near_far, dev)
    directions = get_ray_directions(H, W, focal).to(dev)
    for k in range(c2ws.shape[0]):
        rgb, depth = system.render_rays(_path_rays(directions, c2ws[k], near_far), **kw)
        ops.frame_u8(rgb.reshape(H, W, 3), depth.reshape(H, W) if depth_panel else None, minmax=mm, lut=lut, crop=crop, out=frames[k])
    return frames


class MVSSystemFusion(_ModuleShim):
    """reference train_mvs_nerf_fusion_finetuning_pl.py:78-382: a scene that one triplet of source views cannot cover.  Every camera of the scene is
    rendered at quarter resolution from its three nearest views and every sample's 20-channel feature row and alpha are splatted into ONE
    canonical volume over a world-space box (`fuse_local_volumes`, fusion.VolumeFuser: colliding writes are accumulated, bit-reproducibly);
    that volume becomes the learnable `RefVolume` (checkpoint key `volume.feat_volume`) which is fine-tuned and rendered with rays clipped to the
    box, through the colour-volume ray march.
    Left out: importance sampling (`args.N_importance > 0` raises - the reference's own calls, :259-260 and :312-313, hand `N_importance=` and
    `density_volume=` to a ray_marcher without such parameters and raise TypeError as shipped) and the reference's `update_density_volume` with it;
    the method of that name here is an extension - the renderer-consistent density render_rays(skip_empty=) tests samples against."""

    def __init__(self, args, views, bbox_3d, img_wh, focal, n_depth_planes=128):
        """views: one entry per scene camera, (imgs (1,3,3,H,W) normalised, proj_mats (1,3,3,4), near_far (2,), pose_source dict, c2w (4,4) | (3,4)) -
        what `dataset.read_source_views(pair_idx=...)` returns for the camera's three nearest views (:143), then the camera's own pose.
        bbox_3d (2,3): the scene box; img_wh = (W, H) and focal of the full-resolution images (:130-132)."""
        super().__init__()
        if int(getattr(args, "N_importance", 0) or 0) > 0:
            raise NotImplementedError("MVSSystemFusion: args.N_importance > 0 - the reference's fusion script cannot run it either (its ray_marcher "
                                      "takes neither N_importance= nor density_volume=, data/ray_utils.py:152-156)")
        if int(args.pad) % 4:
            raise ValueError(f"MVSSystemFusion: args.pad must be a multiple of 4 (the quarter-resolution march pads by pad / 4), got {args.pad}")
        if int(args.netwidth) == ops.WIDE_WIDTH:                          # this system trains the MLP; before anything is built or loaded
            raise NotImplementedError(f"MVSSystemFusion: {WIDE_TRAINING_MSG}")
        self.args = args
        self.args.feat_dim = 8 + 12                                       # :82
        if not hasattr(args, "fusion_N_samples"):
            args.fusion_N_samples = 128                                   # :159, a literal there
        if not hasattr(args, "fusion_volume_dim"):
            args.fusion_volume_dim = [128, 128, 128]                      # :101
        self.volume_dim = [int(v) for v in args.fusion_volume_dim]
        self.idx = 0
        kw_train, _, _, self.grad_vars = create_nerf_mvs(args, use_mvs=True, dir_embedder=False, pts_embedder=True)      # :89
        for k in ("N_samples", "ndc", "lindisp"):
            kw_train.pop(k, None)
        self.render_kwargs_train = kw_train
        self.MVSNet = kw_train.pop("network_mvs")
        self.MVSNet.D = n_depth_planes
        self.network_fn = kw_train["network_fn"]
        self.views = list(views)
        self.img_wh, self.focal = (int(img_wh[0]), int(img_wh[1])), focal
        self.register_buffer("bbox_3d", torch.as_tensor(bbox_3d, dtype=torch.float32).reshape(2, 3).clone(), persistent=False)
        self.volume = None
        self._allreduce = None

    # -- fusion ------------------------------------------------------------------------------------
    @torch.no_grad()
    def fuse_local_volumes(self):
        """:117-203.  Call once the module is on its device and the weights are loaded.  With torch.distributed initialised the views are split over
        the ranks in contiguous ranges and the integer accumulators are all-reduced: every rank ends with the same bits as one process."""
        import copy
        from .fusion import VolumeFuser
        from .models import RefVolume
        args = copy.copy(self.args)
        args.use_color_volume = False                                     # :100
        dev = self.bbox_3d.device
        fuser = VolumeFuser(self.volume_dim, args.feat_dim, dev)
        W, H = self.img_wh
        H, W = H // 4, W // 4                                             # :131
        directions = get_ray_directions(H, W, torch.as_tensor(self.focal, dtype=torch.float32) / 4.0).to(dev)      # :132
        box_lo, box_size = self.bbox_3d[0].view(1, 1, 3), (self.bbox_3d[1] - self.bbox_3d[0]).view(1, 1, 3)
        world, rank = D.world_rank()
        lo, hi = D.shard_range(len(self.views), world, rank)
        self.MVSNet.train()                                               # batch-statistics ABN, as every encode of the reference
        for i, (imgs, proj_mats, near_far, pose, c2w) in enumerate(self.views):
            if i == 0:
                self.pose_source_ref = {k: v.to(dev) for k, v in pose.items()}       # :146-147
                self.imgs_ref = MVSSystem.unpreprocess(imgs.to(dev))
            if not lo <= i < hi:
                continue
            imgs, near_far = imgs.to(dev), near_far.to(dev, torch.float32)
            pose = {k: v.to(dev) for k, v in pose.items()}
            volume_feature, _, _ = self.MVSNet(imgs, proj_mats.to(dev), near_far, pad=args.pad)       # :144
            imgs = MVSSystem.unpreprocess(imgs)
            rays_o, rays_d = get_rays(directions, torch.as_tensor(c2w, dtype=torch.float32).to(dev))            # :149
            rays = torch.cat([rays_o, rays_d, near_far[0] * torch.ones_like(rays_o[:, :1]), near_far[1] * torch.ones_like(rays_o[:, :1])], 1)
            intrinsic_ref = pose["intrinsics"][0].clone()
            intrinsic_ref[:2] *= 0.25                                     # :164
            for c0 in range(0, rays.shape[0], args.chunk):                # :156
                pts, ro, rd, z = ray_marcher(rays[c0:c0 + args.chunk], N_samples=args.fusion_N_samples)
                pts, ndc = ops.ray_points(ro, rd, z, pose["w2cs"][0], intrinsic_ref, near_far, ref_hw=(H, W), pad=args.pad // 4)     # :162-168
                _, ray_feat, _, _, ray_alpha, _ = rendering(args, pose, pts, ndc, z, ro, rd.contiguous(), volume_feature, imgs,
                                                            **self.render_kwargs_train)                      # :171-174
                fuser.add(ray_feat, (pts - box_lo) / box_size, ray_alpha)                                     # :176-177
        fuser.all_reduce()
        feat_volume, self.density_volume = fuser.finish()                 # :190-192, :199
        self.volume = RefVolume(feat_volume).to(dev)                      # :200
        self.grad_vars = [p for p in self.network_fn.parameters()] + list(self.volume.parameters())      # :105 (MVSNet is not stepped: no gradient reaches it)
        self.args.use_color_volume = True                                 # :106
        return fuser

    def _need_volume(self):
        if self.volume is None:
            raise RuntimeError("MVSSystemFusion: call fuse_local_volumes() first (after .to(device) and loading the weights)")

    # -- the step ----------------------------------------------------------------------------------
    def training_step(self, batch, batch_nb):
        """:251-291.  batch = {'rays': (1,B,8), 'rgbs': (1,B,3)}.
        args.skip_empty_train (None / unset: the dense step below, untouched): as MVSSystemFinetune.training_step - the training density
        self.train_density is ops.node_density of the box volume; self.density_volume, the (1,1,D,H,W) density of the splat, is not touched."""
        self._need_volume()
        args = self.args
        sparse = _skip_empty_train(args)
        if int(getattr(args, "N_importance", 0) or 0) > 0:
            raise NotImplementedError("MVSSystemFusion: args.N_importance > 0 is not supported (see the class docstring)")
        dev = self.bbox_3d.device
        rays, target = batch["rays"].reshape(-1, 8).to(dev, torch.float32), batch["rgbs"].reshape(-1, 3).to(dev, torch.float32)
        with torch.no_grad():                                             # :259-263
            jitter = torch.rand((rays.shape[0], args.N_samples), device=dev) if args.perturb > 0 else None
            pts, ndc, z_vals = ops.ray_march_bbox(rays, self.bbox_3d, args.N_samples, lindisp=getattr(args, "use_disp", False),
                                                  perturb=args.perturb, jitter=jitter)
        if sparse is not None:
            _refresh_train_density(self, sparse, self._node_density)
        with ops.mlp_precision("bf16" if getattr(args, "use_amp", False) else ops.MLP_PRECISION):
            if sparse is not None:
                vol = self.volume.feat_volume
                rgbs = _sparse_training_render(self, sparse, vol, None, self.pose_source_ref["w2cs"][:(args.feat_dim - 8) // 4].contiguous(), None,
                                               pts, ndc, z_vals, rays[:, 3:6],
                                               getattr(args, "dp_volume_grad", "allreduce") == "samples" and vol.requires_grad)
            else:
                rgbs, _, _, _, _, _ = rendering(args, self.pose_source_ref, pts, ndc, z_vals, rays[:, 0:3], rays[:, 3:6].contiguous(), self.volume,
                                                self.imgs_ref, **self.render_kwargs_train)                       # :266-267
        img_loss = img2mse(rgbs, target)
        with torch.no_grad():
            self.log("train/loss", img_loss, prog_bar=True)
            self.log("train/img_mse_loss", img_loss)
            self.log("train/PSNR", mse2psnr2(img_loss), prog_bar=True)
        return {"loss": img_loss}

    def fit_scene(self, scene, n_steps, batch_size=None, seed=0, optimizer=None):
        """MVSSystemFinetune.fit_scene for the fused scene: every step gathers its rays and colours from the rays.SceneRays bank (ops.scene_rays_gather,
        one launch) and runs training_step on them - the march against the box stays ops.ray_march_bbox.  Returns the losses."""
        self._need_volume()
        batches = _scene_index_batches(scene, n_steps, batch_size or self.args.batch_size, seed)

        def step(i, idx):
            rays, rgbs = scene.gather(idx)
            return self.training_step({"rays": rays[None], "rgbs": rgbs[None]}, i)
        return _fit_loop(self, ((lambda i=i, idx=idx: step(i, idx)) for i, idx in enumerate(batches)), optimizer)

    # -- rendering the fused scene -----------------------------------------------------------------
    @torch.no_grad()
    def update_density_volume(self, dilate=0):
        """The density of the fused, fine-tuned scene in the renderer's frame: ops.node_density over the nodes of the box volume (a colour volume: one
        lookup per node, no camera; the node coordinates are box coordinates, x -> W, y -> H, z -> D, as ops.ray_march_bbox forms them) ->
        self.density_volume, in the (1,1,D,H,W) shape fuse_local_volumes leaves.  Until the first call that attribute is the FUSED density of the
        splat (fusion.VolumeFuser.finish: the alpha sums over the weight sums of the per-view renders, with the reference's corner weights), which
        knows nothing of what fine-tuning did to the volume since; dilate widens the occupied region (ops.max_dilate3d)."""
        dens = self._node_density(dilate)
        self.density_volume = dens.view(1, 1, *dens.shape)
        return self.density_volume

    @torch.no_grad()
    def _node_density(self, dilate=0):
        """ops.node_density over the nodes of the box volume -> (D,H,W): what update_density_volume reshapes into self.density_volume and what a step
        with args.skip_empty_train keeps in self.train_density."""
        self._need_volume()
        F = self.args.feat_dim
        return ops.node_density(dilate=dilate, **_density_sources(self.network_fn, F, self.volume.feat_volume.detach(), self.pose_source_ref, (F - 8) // 4))

    @torch.no_grad()
    def render_rays(self, rays, chunk=None, batch_rays=65536, skip_empty=None, device_count=False, early_stop=None, stop_every=32):
        """The rendering part of validation_step (:307-324) for rays (N,8): per chunk ops.ray_march_bbox -> rendering, the chunks of up to batch_rays
        rays issued as one renderer.rendering_batched call; chunk ranges are sharded over the ranks as in MVSSystemFinetune.render_rays.
        Returns (rgb (N,3), depth (N,)).
        skip_empty: None (default) is the dense render above, untouched.  A float is a density threshold: per sub-batch of batch_rays
        rays ops.ray_march_bbox -> ops.raymarch_sparse (_render_sparse_batches) against `self.density_volume` - the fused density of the splat, or the renderer-consistent one
        after update_density_volume(); the sub-batches are sharded over the ranks and `self.last_live_fraction` is this rank's live samples over its
        samples.
        early_stop / stop_every: as MVSSystem.render_view; alone it reads no density volume.  `self.last_stopped_fraction` is this
        rank's stopped rays over its rays.
        device_count: as MVSSystem.render_view - the sparse sub-batches without a host read, the same values."""
        from .renderer import rendering_batched
        stop = _early_stop(early_stop, stop_every, "render_rays")          # refusals first: nothing below needs the library before them
        device_count = _device_count(device_count, skip_empty, stop, "render_rays")
        if skip_empty is not None:
            skip_empty = _threshold(skip_empty, "render_rays(skip_empty=)")
        self._need_volume()
        args = self.args
        chunk = int(chunk or args.chunk)
        dev = self.bbox_3d.device
        rays = rays.reshape(-1, 8).to(dev, torch.float32).contiguous()
        N = rays.shape[0]
        if N == 0:
            return torch.empty((0, 3), device=dev), torch.empty((0,), device=dev)
        if skip_empty is not None or stop is not None:
            vol = self.volume.feat_volume
            src = _sparse_sources(self, vol, self.pose_source_ref, (args.feat_dim - 8) // 4, None, "render_rays(skip_empty= / early_stop=)")
            if skip_empty is not None:                   # (1,1,D,H,W) as finish() leaves it
                src.update(density=self.density_volume.reshape(vol.shape[-3:]).to(dev, torch.float32).contiguous(), thr=skip_empty)
            lindisp = getattr(args, "use_disp", False)
            B = max(int(batch_rays), 1)
            t = torch.linspace(0, 1, args.N_samples, device=dev)

            def make_batch(idx):
                r = rays[idx * B:(idx + 1) * B]
                pts, ndc, z = ops.ray_march_bbox(r, self.bbox_3d, args.N_samples, lindisp=lindisp, t=t)
                return pts, ndc, z, r[:, 3:6].contiguous()
            return _render_sparse_batches(self, N, B, make_batch, dict(src, vol_cl=ops.channels_last_volume(vol)), early_stop=stop, device_count=device_count)
        n_chunks = (N + chunk - 1) // chunk
        world, rank = D.world_rank()
        lo, hi = D.shard_range(n_chunks, world, rank)
        t = torch.linspace(0, 1, args.N_samples, device=dev)
        group = max(1, int(batch_rays) // chunk)
        rows = []
        for g0 in range(lo, hi, group):
            batches = []
            for idx in range(g0, min(g0 + group, hi)):
                r = rays[idx * chunk:(idx + 1) * chunk]
                pts, ndc, z = ops.ray_march_bbox(r, self.bbox_3d, args.N_samples, lindisp=getattr(args, "use_disp", False), t=t)
                batches.append((pts, ndc, z, r[:, 0:3], r[:, 3:6].contiguous()))
            outs = rendering_batched(args, self.pose_source_ref, batches, self.volume, self.imgs_ref, **self.render_kwargs_train)
            rows += [torch.cat([o[0], o[3][:, None]], 1) for o in outs]
        return D._assemble_frame(torch.cat(rows, 0) if rows else None, 1, N, chunk, n_chunks, world, None, dev)

    @torch.no_grad()
    def render_path(self, c2ws_render, hw, focal, depth_panel=True, crop=False, minmax=None, cmap=None, device_count=False, **render_rays_kw):
        """MVSSystemFinetune.render_path for the fused scene: the rays of each pose carry the first camera's source near / far (render_rays clips them to
        the box), which is also the default depth range of the colour map."""
        _device_count(device_count, render_rays_kw.get("skip_empty"), render_rays_kw.get("early_stop"), "render_path")
        self._need_volume()
        return _render_path_rays(self, c2ws_render, hw, focal, torch.as_tensor(self.views[0][2]), depth_panel, crop, minmax, cmap, self.bbox_3d.device,
                                 device_count=device_count, **render_rays_kw)

    @torch.no_grad()
    def validation_step(self, batch, batch_nb):
        """:294-343.  batch = {'rays': (1,N,8) | (N,8), 'rgbs': (1,H,W,3) | (H,W,3) | (N,3)} -> {'val_psnr_all'}; the image grids and the PNG dump
        are left out as in the other systems (`last_val_images` keeps what they show)."""
        from .utils import mse2psnr
        img = batch["rgbs"].to(torch.float32).cpu()
        img = img[0] if img.dim() == 4 else img
        rgb, depth = self.render_rays(batch["rays"].reshape(-1, 8))
        rgb = torch.clamp(rgb.cpu().reshape(img.shape), 0, 1)            # :327
        depth = depth.cpu().reshape(img.shape[:-1])
        img_err_abs = (rgb - img).abs()
        self.idx += 1
        self.last_val_images = {"rgb": rgb, "depth": depth, "err": img_err_abs}
        return {"val_psnr_all": mse2psnr(torch.mean(img_err_abs ** 2))}  # :330

    validation_epoch_end = MVSSystemFinetune.validation_epoch_end
    save_ckpt = MVSSystemFinetune.save_ckpt                               # :370-382, the fine-tuning script's keys
    configure_optimizers = MVSSystemFinetune.configure_optimizers
