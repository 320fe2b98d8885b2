"""Timing of empty-space skipping (MVSSystemFinetune.render_rays(skip_empty=), ops.raymarch_sparse) against the dense render of the same frame.

  --mode frame    per size, MLP mode and occupied share f of the depth planes: a synthetic band density volume (f of the planes at 1, the rest 0) is
                  assigned to the system, then render_rays(rays) - the untouched default path - and render_rays(rays, skip_empty=0.0) are timed in
                  alternating pairs, device-synchronised, after a warm-up of both at that shape.  Reported: every pair's two times, the MEASURED
                  live fraction, whether the sparse frame won every pair, and the check of the timed outputs: the sparse frame against the dense
                  sequence with the dead rows zeroed (ops.gather -> ops.mlp_forward -> zero -> ops.composite per sub-batch) - torch.equal in fp32;
                  in "auto" both frames' errors against that fp32 frame.  Also the algorithmic bytes of the new kernels per frame and, from a
                  device-event timing of live_samples + expand_rows on one sub-batch, their share of the HBM peak (a cross-check: the kernel times
                  proper come from the trace below).
  --mode trace    one sparse frame per size at the band nearest f = 0.1, nothing else: meant to run under `rocprofv3 --kernel-trace --stats`.

Algorithmic bytes per sample of the new kernels: 12 B of NDC read + 16 B of raw written once (expand_rows) and read once (composite); per LIVE sample
4 B of index + up to 36 B of compact rows (NDC, world point, ray direction; 24 B for a colour volume).

Sizes as bench_finetune_render.py: "3view" = 512x640 rays, 3 views, 128 planes, 128 samples; "config4" = 800x800, 5 views, 192 planes.
Prints one JSON line per measurement and writes them all to --out.
"""
import argparse
import json

import torch

from bench_finetune_render import HBM_PEAK, SIZES, _frame_rays, _system, _timed

SHARES = (1.0, 0.5, 0.25, 0.1, 0.03)


def band_volume(like, share):
    """(D,H,W) density with round(share * D) depth planes (at least one) in the middle at 1 and the rest at 0."""
    D = like.shape[0]
    k = min(D, max(1, int(round(share * D))))
    lo = (D - k) // 2
    d = torch.zeros_like(like)
    d[lo:lo + k] = 1.0
    return d


def masked_dense_frame(ft, rays, thr, B):
    """The dense sequence with the dead rows zeroed, per sub-batch of B rays: what the sparse frame must equal.  The dead rows are the complement of
    ops.live_samples' index list (held to the torch oracle by tests/test_gpu_sparse_render.py)."""
    from mvsnerf_amd import ops, train
    a = ft.args
    H, W = ft.imgs.shape[-2:]
    V = ft.imgs.shape[1]
    w2c, K = ft.pose_source["w2cs"][0], ft.pose_source["intrinsics"][0]
    w2cs, Ks, imgs = ft.pose_source["w2cs"][:V].contiguous(), ft.pose_source["intrinsics"][:V].contiguous(), ft.imgs[0].contiguous()
    vol_cl = ops.channels_last_volume(ft.volume.feat_volume)
    net, F = ft.network_fn, a.feat_dim
    rgbs, depths = [], []
    for i in range(0, rays.shape[0], B):
        r = rays[i:i + B]
        _, ro, rd, z = train.ray_marcher(r, N_samples=a.N_samples)
        pts, ndc = ops.ray_points(ro, rd, z, w2c, K, ft.near_far_source, ref_hw=(H, W), pad=a.pad)
        N, S = z.shape
        if vol_cl.shape[-1] == 8:
            feat, dirs = ops.gather(vol_cl, imgs, w2cs, Ks, pts, ndc, rd.contiguous())
        else:
            feat, dirs = ops.gather_colorvol(vol_cl, ndc, rd.contiguous(), w2c.contiguous())
        raw = ops.mlp_forward(net.packed(F), F, ndc.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, N, S, 0, ndc.device, **net.packed_alt(F))
        count, idx, _, _, _ = ops.live_samples(ft.density_volume, ndc, thr)
        live = torch.zeros(N * S, dtype=torch.bool, device=ndc.device)
        live[idx[:int(count.item())].long()] = True
        raw = torch.where(live[:, None], raw, torch.zeros_like(raw)).view(N, S, 4)
        rgb, _, _, _, depth, _ = ops.composite(raw, z.contiguous(), bool(getattr(a, "white_bkgd", False)))
        rgbs.append(rgb)
        depths.append(depth)
    return torch.cat(rgbs), torch.cat(depths)


def new_kernel_bytes(P, n_live, colour):
    return P * (12 + 16 + 16) + n_live * (4 + (24 if colour else 36))


def kernels_event_us(ft, rays, B, reps=10):
    """Device-event time of live_samples + expand_rows on the first sub-batch of the frame (median of reps), with its sample and live counts."""
    from mvsnerf_amd import ops, train
    a = ft.args
    H, W = ft.imgs.shape[-2:]
    r = rays[:B]
    _, ro, rd, z = train.ray_marcher(r, N_samples=a.N_samples)
    pts, ndc = ops.ray_points(ro, rd, z, ft.pose_source["w2cs"][0], ft.pose_source["intrinsics"][0], ft.near_far_source, ref_hw=(H, W), pad=a.pad)
    rd = rd.contiguous()
    P = z.numel()
    count, idx, *_ = ops.live_samples(ft.density_volume, ndc, 0.0, pts, rd)
    n = int(count.item())
    src = torch.zeros((n, 4), device=ndc.device)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        count, idx, *_ = ops.live_samples(ft.density_volume, ndc, 0.0, pts, rd)
        ops.expand_rows(src, idx, count, P)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ts)[len(ts) // 2], P, n


def frame_mode(sizes, pairs, shares, batch_rays, results):
    from mvsnerf_amd import ops
    for size in sizes:
        ft, rig, pose = _system(size)
        ft.update_density_volume()                              # builds the voxel positions on first use; replaced by the bands below
        learnt = ft.density_volume
        rays = _frame_rays(rig, pose, size)
        P = rays.shape[0] * ft.args.N_samples
        for mode in ("fp32", "auto"):
            for share in shares:
                ft.density_volume = band_volume(learnt, share)
                with ops.mlp_precision(mode), torch.no_grad():
                    dense = lambda: ft.render_rays(rays, batch_rays=batch_rays)
                    sparse = lambda: ft.render_rays(rays, batch_rays=batch_rays, skip_empty=0.0)
                    d_out, s_out = dense(), sparse()            # warm-up of both paths at this shape
                    frac = ft.last_live_fraction
                    with ops.mlp_precision("fp32"):
                        want = masked_dense_frame(ft, rays, 0.0, batch_rays)
                    if mode == "fp32":
                        check = dict(outputs_equal=bool(torch.equal(s_out[0], want[0]) and torch.equal(s_out[1], want[1])))
                    else:
                        auto = masked_dense_frame(ft, rays, 0.0, batch_rays)
                        check = dict(e_sparse_rgb=float((s_out[0] - want[0]).abs().max()), e_dense_rgb=float((auto[0] - want[0]).abs().max()),
                                     e_sparse_depth=float((s_out[1] - want[1]).abs().max()), e_dense_depth=float((auto[1] - want[1]).abs().max()))
                    del want
                    t_dense, t_sparse = [], []
                    for _ in range(pairs):
                        t_dense.append(_timed(dense)[0])
                        t_sparse.append(_timed(sparse)[0])
                    ev_us, P_b, n_b = kernels_event_us(ft, rays, batch_rays)
                n_live = int(round(frac * P))
                by = new_kernel_bytes(P_b, n_b, colour=False)
                r = dict(kind="frame", size=size, mlp=mode, planes_share=share, live_fraction=round(frac, 5), rays=int(rays.shape[0]), samples=P,
                         batch_rays=batch_rays, dense_ms=[round(t, 3) for t in t_dense], sparse_ms=[round(t, 3) for t in t_sparse],
                         sparse_wins_every_pair=all(s < d for s, d in zip(t_sparse, t_dense)),
                         speedup_median=round(sorted(t_dense)[len(t_dense) // 2] / sorted(t_sparse)[len(t_sparse) // 2], 3), **check,
                         new_kernels_algorithmic_bytes_per_frame=new_kernel_bytes(P, n_live, colour=False),
                         new_kernels_one_batch=dict(samples=P_b, live=n_b, algorithmic_bytes=by, event_us=round(ev_us, 2),
                                                    share_of_hbm_peak=round(by / (ev_us * 1e-6) / HBM_PEAK, 4)))
                results.append(r)
                print(json.dumps(r), flush=True)
        del ft
        torch.cuda.empty_cache()


def trace_mode(sizes, batch_rays):
    from mvsnerf_amd import ops
    for size in sizes:
        ft, rig, pose = _system(size)
        ft.update_density_volume()
        ft.density_volume = band_volume(ft.density_volume, 0.1)
        rays = _frame_rays(rig, pose, size)
        with torch.no_grad():
            ft.render_rays(rays, batch_rays=batch_rays, skip_empty=0.0)
        torch.cuda.synchronize()
        print(json.dumps(dict(kind="trace", size=size, mlp=ops.MLP_PRECISION, live_fraction=round(ft.last_live_fraction, 5))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("frame", "trace"), default="frame")
    ap.add_argument("--sizes", default="3view,config4")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--shares", default=",".join(str(s) for s in SHARES))
    ap.add_argument("--batch-rays", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_render.py measures on the GPU; none found")
    results = []
    sizes = a.sizes.split(",")
    if a.mode == "frame":
        frame_mode(sizes, a.pairs, [float(s) for s in a.shares.split(",")], a.batch_rays, results)
    else:
        trace_mode(sizes, a.batch_rays)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
