"""Timing of empty-space skipping on a PRETRAINED scene (MVSSystem.scene_density, render_view(skip_empty=, density=)) against the dense render_view of
the same frame, the same run.

  --mode frame    the synthetic 512 x 640 3-view scene with the checkpoint's weights, encoded once (volume = encode_scene(batch)); per MLP mode ("fp32",
                  "auto"):
                    density   scene_density(batch, volume) alone, with dilate 0 and 1: device-synchronised wall times.
                    (a) band  synthetic band volumes (a share f of the depth planes at 1, the rest 0, thr = 0): the path's cost at a known live fraction.
                    (b) own   the scene's own scene_density with dilate in {0, 1} at thr in {0, 0.01, 0.1}: live fraction, and PSNR / largest absolute RGB
                              difference of the sparse frame against the dense frame of the same mode.
                  Every row: alternating pairs of device-synchronised times, dense render_view(volume=) then sparse render_view(volume=, skip_empty=,
                  density=), after a warm-up of both; the measured live fraction; whether the sparse frame won every pair; the median ratio.
  --mode trace    one density build (dilate 1) and one sparse frame, nothing else: meant to run under `rocprofv3 --kernel-trace --stats` (no counters in
                  that run) for the times of voxel_points_kernel and max_dilate_axis_kernel.

Algorithmic bytes of the new kernels: voxel_points 24 B per node (two 12-byte rows written, nothing read; 12 B for a box volume); max_dilate3d 8 B per
voxel and pass (4 read, 4 written; the neighbours come from cache), three passes for r > 0.
Prints one JSON line per measurement and writes them all to --out.
"""
import argparse
import json

import torch

from bench_common import H_IMG, W_IMG, _psnr
from bench_finetune_render import HBM_PEAK, _timed
from bench_sparse_render import SHARES, band_volume

THRESHOLDS = (0.0, 0.01, 0.1)


def _scene(dev):
    from bench_extras import load_system
    from mvsnerf_amd import train
    system = load_system(dev)
    batch = train.batch_to_device(train.synthetic_batch(H_IMG, W_IMG, seed=1234), dev)
    with torch.no_grad():
        vol = system.encode_scene(batch)
    return system, batch, vol


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _pairs(dense, sparse, pairs):
    t_dense, t_sparse = [], []
    for _ in range(pairs):
        t_dense.append(_timed(dense)[0])
        t_sparse.append(_timed(sparse)[0])
    return dict(dense_ms=[round(t, 3) for t in t_dense], sparse_ms=[round(t, 3) for t in t_sparse],
                sparse_wins_every_pair=all(s < d for s, d in zip(t_sparse, t_dense)), speedup_median=round(_median(t_dense) / _median(t_sparse), 3))


def frame_mode(pairs, shares, batch_rays, results):
    from mvsnerf_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    system, batch, vol = _scene(dev)
    grid = tuple(vol.shape[-3:])
    nodes = grid[0] * grid[1] * grid[2]

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)
    for mode in ("fp32", "auto"):
        with ops.mlp_precision(mode), torch.no_grad():
            dense = lambda: system.render_view(batch, volume=vol, batch_rays=batch_rays)
            d_out = dense()
            t_frame = _median([_timed(dense)[0] for _ in range(pairs)])
            own = {}
            for dilate in (0, 1):
                build = lambda: system.scene_density(batch, volume=vol, dilate=dilate)
                own[dilate] = build()                                # warm-up, and the volume (b) uses
                ts = [_timed(build)[0] for _ in range(pairs)]
                emit(dict(kind="density", mlp=mode, grid=grid, nodes=nodes, dilate=dilate, build_ms=[round(t, 3) for t in ts], dense_frame_ms=round(t_frame, 3),
                          build_over_dense_frame=round(_median(ts) / t_frame, 3), share_above_0=round(float((own[dilate] > 0).float().mean()), 4),
                          share_above_0p01=round(float((own[dilate] > 0.01).float().mean()), 4), share_above_0p1=round(float((own[dilate] > 0.1).float().mean()), 4),
                          max=round(float(own[dilate].max()), 3)))
            for share in shares:                                     # (a) the path's cost at a known live fraction
                band = band_volume(own[0], share)
                sparse = lambda: system.render_view(batch, volume=vol, batch_rays=batch_rays, skip_empty=0.0, density=band)
                s_out = sparse()
                frac = system.last_live_fraction
                same = bool(torch.equal(s_out[0], d_out[0]) and torch.equal(s_out[1], d_out[1])) if frac == 1.0 else None
                emit(dict(kind="band", mlp=mode, planes_share=share, live_fraction=round(frac, 5), batch_rays=batch_rays, **_pairs(dense, sparse, pairs),
                          equals_dense_frame_when_all_live=same))
            for dilate in (0, 1):                                    # (b) the scene's own density
                for thr in THRESHOLDS:
                    sparse = lambda: system.render_view(batch, volume=vol, batch_rays=batch_rays, skip_empty=thr, density=own[dilate])
                    s_out = sparse()
                    frac = system.last_live_fraction
                    emit(dict(kind="own", mlp=mode, thr=thr, dilate=dilate, live_fraction=round(frac, 5), batch_rays=batch_rays, **_pairs(dense, sparse, pairs),
                              psnr_vs_dense=_psnr(s_out[0].clamp(0, 1), d_out[0].clamp(0, 1)), max_abs_rgb_diff=round(float((s_out[0] - d_out[0]).abs().max()), 6),
                              max_abs_depth_diff=round(float((s_out[1] - d_out[1]).abs().max()), 6)))


def trace_mode(batch_rays):
    from mvsnerf_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    system, batch, vol = _scene(dev)
    with torch.no_grad():
        dens = system.scene_density(batch, volume=vol, dilate=1)
        system.render_view(batch, volume=vol, batch_rays=batch_rays, skip_empty=0.01, density=dens)
    torch.cuda.synchronize()
    grid = tuple(vol.shape[-3:])
    nodes = grid[0] * grid[1] * grid[2]
    print(json.dumps(dict(kind="trace", mlp=ops.MLP_PRECISION, grid=grid, nodes=nodes, live_fraction=round(system.last_live_fraction, 5),
                          voxel_points_bytes=24 * nodes, max_dilate_bytes_per_pass=8 * nodes, hbm_peak_bytes_per_s=HBM_PEAK)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("frame", "trace"), default="frame")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--shares", default=",".join(str(s) for s in SHARES))
    ap.add_argument("--batch-rays", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_skip.py measures on the GPU; none found")
    results = []
    if a.mode == "frame":
        frame_mode(a.pairs, [float(s) for s in a.shares.split(",")], a.batch_rays, results)
    else:
        trace_mode(a.batch_rays)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
