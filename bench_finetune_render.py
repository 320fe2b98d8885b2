"""Timing of the fine-tuned-scene render (MVSSystemFinetune.render_rays, ops.gather_colorvol) against the code paths that existed before it.

  --mode frame    frame time of render_rays (one library call) vs render_rays(whole_frame_off=True) (the per-chunk Python loop:
                  ray_marcher -> ops.ray_points -> [ray_marcher_fine] -> rendering), device-synchronised, warmed up, alternating pairs,
                  for a colour volume and for an 8-channel volume with importance sampling, in the fp32 and the default MLP modes.
  --mode lookup   the lookups alone on one (P, C): ops.gather_colorvol vs ops.volume_sample (volume_sample_generic_kernel) + ops.dir_feature;
                  meant to run under `rocprofv3 --kernel-trace --stats` (kernel times come from the trace; the device-event times printed here
                  are a cross-check).  Algorithmic bytes per sample: 8 corners x 4C bytes read + 4F bytes written.

Sizes: "config4" = 800x800 rays, 5 source views, 192 depth planes, 128 samples (BASELINE config 4); "3view" = 512x640, 3 views, 128 planes.
Prints one JSON line per measurement and writes them all to --out.
"""
import argparse
import json
import time

import torch

SIZES = {"config4": dict(H=800, W=800, V=5, D=192, S=128), "3view": dict(H=512, W=640, V=3, D=128, S=128), "tiny": dict(H=64, W=96, V=3, D=16, S=32)}
HBM_PEAK = 8.0e12      # bytes/s, MI355X


def _system(size, **over):
    from mvsnerf_amd import train
    from mvsnerf_amd.synth import make_rig, pose_ref_of
    s = SIZES[size]
    V = s["V"]
    base = (0.0, 0.25, -0.25, 0.12, -0.12, 0.1)
    rig = make_rig(s["H"], s["W"], n_views=V + 1, seed=9, baselines=base[:V] + (0.1,), smooth=True)
    pose = pose_ref_of(rig)
    src = (rig["images"][:, :V], rig["proj_mats"][:, :V], rig["near_fars"][0, 0], {k: v[:V] for k, v in pose.items()})
    args = train.default_args(pad=24 if size != "tiny" else 4, N_samples=s["S"], n_views=V, **over)
    ft = train.MVSSystemFinetune(args, src, n_depth_planes=s["D"]).to("cuda")
    return ft, rig, pose


def _frame_rays(rig, pose, size):
    """The rays of the held-out view's whole pixel grid, (H*W, 8)."""
    from mvsnerf_amd import ops
    s = SIZES[size]
    H, W, V = s["H"], s["W"], s["V"]
    dev = "cuda"
    K, c2w, nf = pose["intrinsics"][V].to(dev), pose["c2ws"][V].to(dev), rig["near_fars"][0, V].to(dev)
    _, dirs, _, _, _ = ops.raygen(H, W, K, c2w, K, pose["w2cs"][0].to(dev), nf, nf, 1, n_rays=H * W)
    n = H * W
    return torch.cat([c2w[:3, 3].expand(n, 3), dirs, nf[0].expand(n, 1), nf[1].expand(n, 1)], 1).contiguous()


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def frame_mode(sizes, pairs, results):
    from mvsnerf_amd import ops
    cases = [(sz, "colour_volume", dict(use_color_volume=True)) for sz in sizes] + [(sizes[-1], "importance", dict(use_density_volume=True, N_importance=64))]
    for size, name, over in cases:
        if size == "tiny" and "N_importance" in over:
            over = dict(over, N_importance=16)
        ft, rig, pose = _system(size, **over)
        if name == "importance":
            ft.update_density_volume()
        rays = _frame_rays(rig, pose, size)
        u = torch.rand((rays.shape[0], ft.args.N_importance), device="cuda") if name == "importance" else None
        for mode in ("fp32", "auto"):
            with ops.mlp_precision(mode):
                one = lambda: ft.render_rays(rays, u=u)
                loop = lambda: ft.render_rays(rays, u=u, whole_frame_off=True)
                a, b = one(), loop()                            # warm-up of both paths, and the outputs agree
                same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
                t_one, t_loop = [], []
                for _ in range(pairs):
                    t_one.append(_timed(one)[0])
                    t_loop.append(_timed(loop)[0])
            r = dict(kind="frame", size=size, case=name, mlp=mode, rays=int(rays.shape[0]), channels=int(ft.volume.feat_volume.shape[1]),
                     one_call_ms=[round(t, 3) for t in t_one], loop_ms=[round(t, 3) for t in t_loop], outputs_equal=same,
                     one_call_wins_every_pair=all(x < y for x, y in zip(t_one, t_loop)))
            results.append(r)
            print(json.dumps(r), flush=True)
        del ft
        torch.cuda.empty_cache()


def lookup_mode(sizes, reps, results):
    from mvsnerf_amd import ops
    g = torch.Generator().manual_seed(0)
    for size in sizes:
        s = SIZES[size]
        C = 8 + 4 * s["V"]
        pad = 24 if size != "tiny" else 4
        D, Hv, Wv = s["D"], s["H"] // 4 + 2 * pad, s["W"] // 4 + 2 * pad
        N, S = 16384, s["S"]
        vol = torch.randn((D, Hv, Wv, C), device="cuda")
        # rays that walk depth through the volume, as a frame's do
        xy = torch.rand((N, 1, 2), generator=g).expand(N, S, 2) + 0.02 * torch.linspace(0, 1, S).view(1, S, 1)
        ndc = torch.cat([xy, torch.linspace(0, 1, S).view(1, S, 1).expand(N, S, 1)], -1).contiguous().cuda()
        rays_dir = torch.randn((N, 3), generator=g).cuda()
        w2c = torch.eye(4, device="cuda")
        new = lambda: ops.gather_colorvol(vol, ndc, rays_dir, w2c)
        old = lambda: (ops.volume_sample(vol, ndc), ops.dir_feature(rays_dir, w2c, normalize=True))
        with torch.no_grad():
            a, b = new(), old()
            same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
            t = {"new": [], "old": []}
            for _ in range(reps):
                for k, fn in (("new", new), ("old", old)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(); e1.record(); e1.synchronize()
                    t[k].append(e0.elapsed_time(e1) * 1e3)
        P = N * S
        alg_bytes = P * (8 * 4 * C + 4 * C)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        r = dict(kind="lookup", size=size, P=P, C=C, volume=[D, Hv, Wv], algorithmic_bytes=alg_bytes, outputs_equal=same,
                 event_us_median=dict(gather_colorvol=round(med["new"], 2), generic_plus_dir_feature=round(med["old"], 2)),
                 event_bytes_per_s=dict(gather_colorvol=alg_bytes / (med["new"] * 1e-6), generic_plus_dir_feature=alg_bytes / (med["old"] * 1e-6)),
                 event_share_of_hbm_peak=dict(gather_colorvol=round(alg_bytes / (med["new"] * 1e-6) / HBM_PEAK, 4),
                                              generic_plus_dir_feature=round(alg_bytes / (med["old"] * 1e-6) / HBM_PEAK, 4)))
        results.append(r)
        print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("frame", "lookup"), required=True)
    ap.add_argument("--sizes", default="config4,3view")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune_render.py measures on the GPU; none found")
    results = []
    sizes = a.sizes.split(",")
    if a.mode == "frame":
        frame_mode(sizes, a.pairs, results)
    else:
        lookup_mode(sizes, a.reps, results)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
