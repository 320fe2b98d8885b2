"""The training rays of a scene, resident on the device.

The reference's per-scene datasets build an all-rays buffer on the CPU (`read_meta`, data/dtu_ft.py:143-188 and data/blender.py:49-85: 32 bytes
per ray and 12 per colour) and a shuffling DataLoader serves it in 1024-row batches.  What they compute - get_ray_directions, get_rays, the
[o | d | near | far] rows, ToTensor, the RGBA blend onto white, the epoch shuffle - is held here as 4 bytes per pixel plus the cameras, and a
batch of ray indices becomes rays, colours, depths, points and NDC coordinates in one launch (csrc/scene_rays.hip).  Reading the files stays
with the caller: the bank takes the decoded 8-bit images and the cameras.
"""
import numpy as np
import torch

from . import ops
from .synth import IMAGENET_MEAN, IMAGENET_STD


class SceneRays:
    """SceneRays(images, c2ws, intrinsics, near_far, depths=None, device="cuda")
        images      (M,H,W,3|4) uint8, as decoded from the scene's PNGs (RGBA is blended onto white, data/blender.py:70)
        c2ws        (M,4,4) | (M,3,4) camera-to-world poses
        intrinsics  (M,3,3) | (3,3) full-resolution K
        near_far    (M,2) | (2,)
        depths      (M,H,W) ground-truth depth maps of the validation views, or None
    A flat ray index is view-major, then row-major: the order of torch.cat(all_rays, 0)."""

    def __init__(self, images, c2ws, intrinsics, near_far, depths=None, device="cuda"):
        images = torch.as_tensor(images)
        if images.dtype != torch.uint8:
            raise TypeError(f"SceneRays: images must be uint8, as decoded from the scene's 8-bit files, got {images.dtype} "
                            "(a float image would be quantised silently)")
        if images.dim() != 4 or images.shape[-1] not in (3, 4):
            raise ValueError(f"SceneRays: images must be (M,H,W,3) or (M,H,W,4), got {tuple(images.shape)}")
        M, H, W = (int(v) for v in images.shape[:3])
        if min(M, H, W) < 1:
            raise ValueError(f"SceneRays: an empty bank, images {tuple(images.shape)}")
        self._init_cameras(M, H, W, c2ws, intrinsics, near_far, depths, device)
        self.has_alpha = images.shape[-1] == 4
        if not self.has_alpha:
            images = torch.cat((images, torch.full((M, H, W, 1), 255, dtype=torch.uint8, device=images.device)), -1)
        self.images = images.to(self.device).contiguous()

    def _init_cameras(self, M, H, W, c2ws, intrinsics, near_far, depths, device):
        """Everything of the bank but its images, for M views of H x W pixels."""
        c2w64 = torch.as_tensor(c2ws).to("cpu", torch.float64)
        if c2w64.dim() != 3 or c2w64.shape[0] != M or tuple(c2w64.shape[1:]) not in ((4, 4), (3, 4)):
            raise ValueError(f"SceneRays: c2ws must be ({M},4,4) or ({M},3,4) for {M} images, got {tuple(c2w64.shape)}")
        if c2w64.shape[1] == 3:
            c2w64 = torch.cat((c2w64, torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(M, 1, 4)), 1)
        K64 = torch.as_tensor(intrinsics).to("cpu", torch.float64)
        if tuple(K64.shape) == (3, 3):
            K64 = K64.expand(M, 3, 3)
        if tuple(K64.shape) != (M, 3, 3):
            raise ValueError(f"SceneRays: intrinsics must be ({M},3,3) or (3,3) for {M} images, got {tuple(K64.shape)}")
        nf = torch.as_tensor(near_far).to("cpu", torch.float32)
        if tuple(nf.shape) == (2,):
            nf = nf.expand(M, 2)
        if tuple(nf.shape) != (M, 2):
            raise ValueError(f"SceneRays: near_far must be ({M},2) or (2,) for {M} images, got {tuple(nf.shape)}")
        if depths is not None:
            depths = torch.as_tensor(depths)
            if tuple(depths.shape) != (M, H, W):
                raise ValueError(f"SceneRays: depths must be ({M},{H},{W}), got {tuple(depths.shape)}")
        self.device = torch.device(device)
        self.n_views, self.hw, self.n_rays = M, (H, W), M * H * W
        self._c2w64, self._K64 = c2w64.contiguous(), K64.contiguous()                   # the host's cameras, for source_views
        self.c2ws = c2w64[:, :3, :4].to(torch.float32).to(self.device).contiguous()
        self.intrinsics = K64.to(torch.float32).to(self.device).contiguous()
        self.near_far = nf.to(self.device).contiguous()
        self.depths = None if depths is None else depths.to(self.device, torch.float32).contiguous()
        self._t = {}

    @classmethod
    def from_images(cls, images, c2ws, intrinsics, near_far, img_wh, resample="lanczos", depths=None, device="cuda"):
        """The bank from the scene's images at the size they were decoded at: `np.asarray(Image.open(p))` of every view, resized on the device to
        img_wh = (W, H) exactly as `Image.resize(img_wh, Image.LANCZOS)` of Pillow resizes them (data/dtu_ft.py:163, data/blender.py:66,
        data/llff.py:344; resample="bilinear": Image.BILINEAR, data/dtu.py:160) - the same bytes as SceneRays(<the Pillow-resized images>, ...).
            images      (M,Hin,Win,3|4) uint8, or a sequence of (H_i,W_i,3|4) uint8 arrays whose sizes may differ (one channel count for all)
            intrinsics, depths    those of the RESIZED images, as the reference's datasets hold them after their own scaling
        One image at a time: upload, resize into that view's slot of the bank (ops.resample_u8); the device holds the bank, one source image
        (briefly also its three-channel form) and the horizontal pass's output.  RGBA is resampled premultiplied, as Pillow resizes mode RGBA.
        Refused: an image more than 100 times as tall as wide whose height shrinks (Pillow 12 runs the vertical pass first for those)."""
        if resample not in ops.RESAMPLE_SUPPORT:
            raise ValueError(f"SceneRays.from_images: resample must be one of {sorted(ops.RESAMPLE_SUPPORT)}, got {resample!r}")
        W, H = (int(v) for v in img_wh)
        if min(W, H) < 1:
            raise ValueError(f"SceneRays.from_images: img_wh must be (W, H) >= 1, got {tuple(img_wh)}")
        views = [torch.as_tensor(v) for v in images]                                    # (a 4-D array iterates over its views)
        if not views:
            raise ValueError("SceneRays.from_images: no images")
        for v in views:
            if v.dtype != torch.uint8:
                raise TypeError(f"SceneRays.from_images: images must be uint8, as decoded from the scene's 8-bit files, got {v.dtype} "
                                "(a float image would be quantised silently)")
            if v.dim() != 3 or v.shape[-1] not in (3, 4) or v.shape[-1] != views[0].shape[-1] or min(v.shape[:2]) < 1:
                raise ValueError(f"SceneRays.from_images: every image must be (H,W,3) or (H,W,4) with one channel count, got {tuple(v.shape)}")
            if v.shape[0] > 100 * v.shape[1] and H < v.shape[0]:
                raise ValueError(f"SceneRays.from_images: a {v.shape[0]} x {v.shape[1]} image (more than 100 times as tall as wide) made lower: "
                                 "Pillow 12 resizes such an image vertically first, the device resampler does not")
        self = cls.__new__(cls)
        M = len(views)
        self._init_cameras(M, H, W, c2ws, intrinsics, near_far, depths, device)
        self.has_alpha = views[0].shape[-1] == 4
        self.images = torch.empty((M, H, W, 4), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            for m, v in enumerate(views):
                src = v.to(self.device)
                if not self.has_alpha:
                    src = torch.nn.functional.pad(src, (0, 1), value=255)
                ops.resample_u8(src.contiguous()[None], (H, W), resample=resample, premultiply=self.has_alpha, out=self.images[m:m + 1])
        return self

    def _bank(self):
        return self.images, self.c2ws, self.intrinsics, self.near_far

    def _idx(self, idx):
        return torch.as_tensor(idx).to(self.device, torch.int64).reshape(-1).contiguous()

    @torch.no_grad()
    def gather(self, idx):
        """(rays (B,8), rgbs (B,3)) = all_rays[idx], all_rgbs[idx]."""
        rays, rgbs, _, _ = ops.scene_rays_gather(*self._bank(), self.depths, self._idx(idx))
        return rays, rgbs

    @torch.no_grad()
    def march(self, idx, N_samples, perturb=0.0, jitter=None, lindisp=False, ref=None):
        """One launch for the front end of a fine-tuning step: {'rays' (B,8), 'rgbs' (B,3), 'z_vals' (B,S), 'pts' (B,S,3), 'ndc' (B,S,3) | None}.
        jitter: the (B,S) torch.rand draw, required when perturb > 0; ref = (w2c_ref, K_ref, near_far_ref, (H_ref, W_ref), pad)."""
        S = int(N_samples)
        if S not in self._t:
            self._t = {S: torch.linspace(0, 1, S, device=self.device)}
        rays, rgbs, z, pts, ndc = ops.scene_rays_march(*self._bank(), self._idx(idx), S, t=self._t[S], jitter=jitter, perturb=perturb, lindisp=lindisp,
                                                       ref=ref)
        return {"rays": rays, "rgbs": rgbs, "z_vals": z, "pts": pts, "ndc": ndc}

    @torch.no_grad()
    def view(self, m):
        """The split='val' item of DTU_ft.__getitem__ (data/dtu_ft.py:210-218) for view m: (rays (H*W,8), image (H,W,3), depth (H,W) | None)."""
        m = int(m)
        if not 0 <= m < self.n_views:
            raise IndexError(f"SceneRays.view: view {m} of {self.n_views}")
        H, W = self.hw
        idx = torch.arange(m * H * W, (m + 1) * H * W, device=self.device, dtype=torch.int64)
        rays, rgbs, depth, _ = ops.scene_rays_gather(*self._bank(), self.depths, idx, want_depth=self.depths is not None)
        return rays, rgbs.reshape(H, W, 3), None if depth is None else depth.reshape(H, W)

    def epoch(self, batch_size, generator=None):
        """The index batches of one shuffled pass over the scene's rays: one torch.randperm on the bank's device, the last batch short
        (drop_last=False, the DataLoader default the reference trains with)."""
        B = int(batch_size)
        if B < 1:
            raise ValueError(f"SceneRays.epoch: batch_size must be >= 1, got {batch_size}")
        perm = torch.randperm(self.n_rays, device=self.device, generator=generator)
        for i in range(0, self.n_rays, B):
            yield perm[i:i + B]

    def source_views(self, ids, on_device=False):
        """read_source_views (data/dtu_ft.py:72-119) for the views `ids`, the first being the reference view: (imgs (1,V,3,H,W) ImageNet-normalised,
        proj_mats (1,V,3,4), near_far (2,), pose_source {'c2ws', 'w2cs' (V,4,4), 'intrinsics' (V,3,3) full resolution}) - what the systems' constructors
        take.  proj = (K/4 [R|t])_v (K/4 [R|t])_ids[0]^-1, rows 0:3, the identity for the first id; float64 on the host, rounded once.  near_far is
        that of ids[-1] (:88 leaves the last one read).  RGBA images are blended onto white (data/blender.py:135).  on_device=True: imgs is formed on
        the bank's device in one launch (ops.source_images) and stays there, the same bits; the default pulls the views' bytes to the host and forms it
        there."""
        ids = [int(i) for i in ids]
        if not ids or min(ids) < 0 or max(ids) >= self.n_views:
            raise IndexError(f"SceneRays.source_views: ids {ids} of {self.n_views} views")
        c2w = self._c2w64[ids].numpy()
        w2c = np.linalg.inv(c2w)
        K = self._K64[ids].numpy()
        projs = []
        for i in range(len(ids)):
            P = np.eye(4)
            Kq = K[i].copy()
            Kq[:2] /= 4.0                                                               # 4 times downscale in the feature space
            P[:3, :4] = Kq @ w2c[i][:3, :4]
            if i == 0:
                ref_inv = np.linalg.inv(P)
                projs.append(np.eye(4))
            else:
                projs.append(P @ ref_inv)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        if on_device:
            with torch.cuda.device(self.device):
                imgs = ops.source_images(self.images, torch.as_tensor(ids, device=self.device), IMAGENET_MEAN, IMAGENET_STD).unsqueeze(0)
        else:
            px = self.images[torch.as_tensor(ids, device=self.device)].cpu().to(torch.float32).div(255)      # ToTensor
            rgb = px[..., :3] * px[..., 3:] + (1 - px[..., 3:])                          # blend A to RGB
            rgb = rgb.permute(0, 3, 1, 2).contiguous()
            mean, std = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
            imgs = rgb.sub_(mean).div_(std).unsqueeze(0)                                 # T.Normalize
        pose = {"c2ws": f32(c2w), "w2cs": f32(w2c), "intrinsics": f32(K)}
        return imgs, f32(np.stack(projs)[:, :3]).unsqueeze(0), self.near_far[ids[-1]].cpu().clone(), pose
