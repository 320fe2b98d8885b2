"""Fusing per-view neural volumes into one scene volume (reference train_mvs_nerf_fusion_finetuning_pl.py:35-76, 117-203).

`VolumeFuser` owns the 64-bit fixed-point accumulators of mvsnerf_volume_fuse_splat (csrc/fusion.hip): every sample's feature row, its alpha
and its weight are splatted to the eight surrounding voxels of a world-space box with the reference's arithmetic - quirks included, see
include/mvsnerf_hip_internal.h - and every colliding write is ADDED (the reference's `vol[..., idx] += x` keeps one of them on a GPU).
Integer sums commute: the accumulators are bit-identical from run to run, for any order of the views, for any split over `add` calls,
fusers (`merge`) or ranks (`all_reduce`)."""
import torch

from . import _lib
from ._lib import check, dev_f32, stream_ptr
from .ops import _Keep, _need_no_grad

HEADER_WORDS = 8          # FUSE_HEADER_WORDS of csrc/fusion.hip: [0] refused contributions, [1] log2 of the scale
SCALE_LOG2 = 32           # a word counts multiples of 2^-32
LIMIT = 2.0 ** 20         # a contribution at or beyond it (or not finite) is refused


class VolumeFuser:
    def __init__(self, volume_dim, C, device):
        """volume_dim = [W, H, D] (the reference's self.volume_dim, :101), C feature channels (a multiple of 4, 4..40)."""
        self.W, self.H, self.D = (int(v) for v in volume_dim)
        self.C = int(C)
        words = int(_lib.lib().mvsnerf_volume_fuse_workspace_words(self.D, self.H, self.W, self.C))
        if words == 0:
            raise RuntimeError(f"VolumeFuser: volume_dim {list(volume_dim)} (every size >= 2) with {C} channels (a multiple of 4, 4..40) is not supported")
        self.device = torch.device(device)
        self.ws = torch.zeros(words, device=self.device, dtype=torch.int64)

    # -- filling ---------------------------------------------------------------------------------
    def add(self, ray_feat, ray_ndc, ray_alpha):
        """update_volume(:35-76) of one batch: ray_feat (..., C), ray_ndc (..., 3) box coordinates (x -> W, y -> H, z -> D), ray_alpha (...)."""
        _need_no_grad(ray_feat, ray_ndc, ray_alpha, op="VolumeFuser.add")
        if ray_feat.shape[-1] != self.C or ray_ndc.shape[-1] != 3:
            raise RuntimeError(f"VolumeFuser.add: ray_feat (..., {self.C}) and ray_ndc (..., 3), got {tuple(ray_feat.shape)} and {tuple(ray_ndc.shape)}")
        P = ray_ndc.numel() // 3
        if ray_feat.numel() != P * self.C or ray_alpha.numel() != P:
            raise RuntimeError(f"VolumeFuser.add: {P} points, but ray_feat {tuple(ray_feat.shape)} and ray_alpha {tuple(ray_alpha.shape)}")
        if P == 0:
            return self
        c = _Keep()         # like every op, the launch goes to the current device's stream: tensors of another device raise (dev_f32)
        check(_lib.lib().mvsnerf_volume_fuse_splat(self.D, self.H, self.W, self.C, c(ray_ndc.reshape(P, 3), "ray_ndc"), P,
                                                   c(ray_feat.reshape(P, self.C), "ray_feat"), self.C, c(ray_alpha.reshape(P), "ray_alpha"),
                                                   self._ws_ptr(), stream_ptr()), "volume_fuse_splat")
        return self

    def _ws_ptr(self):
        if self.ws.device.index != torch.cuda.current_device():
            raise RuntimeError(f"VolumeFuser: the accumulator is on {self.ws.device} but the current device is cuda:{torch.cuda.current_device()}")
        return self.ws.data_ptr()

    def merge(self, other):
        """Adds another fuser's sums: an integer add.  Raises when either side holds refused contributions."""
        if (other.W, other.H, other.D, other.C) != (self.W, self.H, self.D, self.C):
            raise RuntimeError("VolumeFuser.merge: the two accumulators differ in shape")
        self._check(), other._check()
        self.ws[HEADER_WORDS:] += other.ws[HEADER_WORDS:].to(self.device)
        self.ws[1] = torch.maximum(self.ws[1], other.ws[1].to(self.device))       # log2 of the scale: set once either side was splatted into
        return self

    def all_reduce(self, group=None):
        """ONE torch.distributed SUM over the int64 buffer (header included: the refusal counts add up); a no-op without a process group."""
        from . import distributed as D
        if D._collective_needed(group):
            D.all_reduce(self.ws, group=group)
            self.ws[1] = SCALE_LOG2
        self._check()
        return self

    # -- reading ---------------------------------------------------------------------------------
    def _check(self):
        n = int(self.ws[0])
        if n:
            raise RuntimeError(f"VolumeFuser: {n} contribution(s) were refused (|weight * value| >= 2^20 or not finite); the accumulator is invalid")

    def accumulators(self):
        """The int64 words as (D, H, W, C + 4): C feature sums, the alpha sum, the weight sum, 2 pad words; a view."""
        return self.ws[HEADER_WORDS:].view(self.D, self.H, self.W, self.C + 4)

    def sums(self):
        """(feat (C,D,H,W), alpha (D,H,W), weight (D,H,W)) in float64: the words times 2^-32 (exact below 2^21)."""
        self._check()
        a = self.accumulators().to(torch.float64) * 2.0 ** -SCALE_LOG2
        return a[..., :self.C].permute(3, 0, 1, 2).contiguous(), a[..., self.C].contiguous(), a[..., self.C + 1].contiguous()

    def finish(self):
        """fuse_local_volumes :190-192 -> (feat_volume (1,C,D,H,W), density_volume (1,1,D,H,W)) fp32."""
        self._check()
        feat = torch.empty((1, self.C, self.D, self.H, self.W), device=self.device, dtype=torch.float32)
        dens = torch.empty((1, 1, self.D, self.H, self.W), device=self.device, dtype=torch.float32)
        check(_lib.lib().mvsnerf_volume_fuse_finish(self.D, self.H, self.W, self.C, self._ws_ptr(), dev_f32(feat, "feat_volume"),
                                                    dev_f32(dens, "density_volume"), stream_ptr()), "volume_fuse_finish")
        return feat, dens
