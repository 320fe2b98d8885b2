"""Timing of a fine-tuning step with empty space skipped (args.skip_empty_train, ops.raymarch_sparse_train) against the dense step
of the same run.

  --mode step     config 4 of BASELINE.json as far as a synthetic scene allows (800x800, 5 source views, 192 planes; 1024 rays x 128 samples per step;
                  "bf16" = use_amp, config 4's MLP mode, and "fp32").  Per MLP mode and occupied share f of the depth planes a band density volume
                  (f of the planes at 1, the rest 0: bench_sparse_render.py's protocol) is ASSIGNED to the system's train_density, with a refresh
                  interval longer than the run, so that the measured live fraction is the band's.  Timed: training_step + backward, host wall clock
                  between device synchronisations, in ONE process, after a warm-up of both paths, in alternating (dense, sparse) pairs - the dense
                  time is the same run's dense step.  Reported per row: every pair's two times, the medians, the measured live fraction, whether the
                  sparse step won every pair; then per mode the live fraction at which the two medians meet (linear interpolation between the rows
                  on either side).  The f = 1.0 row is the price of the feature: every sample live, plus live_samples, the host read, expand_rows and
                  compact_rows.
  --mode trace    one warm-up and one sparse step at f = 0.1, nothing else: meant to run under `rocprofv3 --kernel-trace --stats`.

Prints one JSON line per measurement and writes them all to --out.
"""
import argparse
import json

import torch

from bench_finetune_render import SIZES, _frame_rays, _system, _timed
from bench_sparse_render import band_volume

SHARES = (1.0, 0.5, 0.25, 0.1)


def _setup(size, mode, n_rays):
    ft, rig, pose = _system(size, use_amp=(mode == "bf16"), batch_size=n_rays)
    g = torch.Generator().manual_seed(7)
    rays = _frame_rays(rig, pose, size)
    pick = torch.randperm(rays.shape[0], generator=g)[:n_rays].to(rays.device)
    batch = {"rays": rays[pick][None].contiguous(), "rgbs": torch.rand((1, n_rays, 3), generator=g).to(rays.device)}
    ft.args.skip_empty_dilate, ft.args.skip_empty_refresh = 1, 10 ** 9
    return ft, batch


def _step(ft, batch, thr):
    """training_step + backward with the switch at `thr` (None: the dense step)"""
    ft.args.skip_empty_train = thr
    ft.zero_grad(set_to_none=True)
    out = ft.training_step(batch, 0)
    out["loss"].backward()
    return out["loss"].detach()


def _median(ts):
    return sorted(ts)[len(ts) // 2]


def _break_even(rows):
    """live fraction at which the sparse median meets the dense median: linear interpolation of (sparse - dense) between neighbouring rows"""
    pts = sorted((r["live_fraction"], r["sparse_median_ms"] - r["dense_median_ms"]) for r in rows)
    for (f0, d0), (f1, d1) in zip(pts, pts[1:]):
        if d0 <= 0 < d1:
            return round(f0 + (f1 - f0) * (0 - d0) / (d1 - d0), 4)
    return None if pts[0][1] > 0 else ">= %.3f" % pts[-1][0]


def step_mode(size, modes, shares, pairs, n_rays, results):
    from mvsnerf_amd import ops
    for mode in modes:
        ft, batch = _setup(size, mode, n_rays)
        like = torch.zeros(tuple(ft.volume.feat_volume.shape[-3:]), device="cuda")
        rows = []
        with ops.mlp_precision("fp32"):          # use_amp sets bf16 inside the step; outside it nothing here runs the MLP
            for share in shares:
                ft.train_density = band_volume(like, share)
                for _ in range(2):               # warm-up of both paths
                    _step(ft, batch, None)
                    _step(ft, batch, 0.0)
                t_dense, t_sparse, fracs = [], [], []
                for _ in range(pairs):
                    t_dense.append(_timed(lambda: _step(ft, batch, None))[0])
                    t_sparse.append(_timed(lambda: _step(ft, batch, 0.0))[0])
                    fracs.append(ft.last_live_fraction)
                r = dict(kind="step", size=size, mlp=mode, rays=n_rays, samples=n_rays * ft.args.N_samples, planes_share=share,
                         live_fraction=round(sum(fracs) / len(fracs), 5), dense_ms=[round(t, 3) for t in t_dense], sparse_ms=[round(t, 3) for t in t_sparse],
                         dense_median_ms=round(_median(t_dense), 3), sparse_median_ms=round(_median(t_sparse), 3),
                         speedup_median=round(_median(t_dense) / _median(t_sparse), 3),
                         sparse_wins_every_pair=all(s < d for s, d in zip(t_sparse, t_dense)))
                rows.append(r)
                results.append(r)
                print(json.dumps(r), flush=True)
        r = dict(kind="break_even", size=size, mlp=mode, live_fraction=_break_even(rows))
        results.append(r)
        print(json.dumps(r), flush=True)
        del ft
        torch.cuda.empty_cache()


def trace_mode(size, modes, n_rays):
    for mode in modes:
        ft, batch = _setup(size, mode, n_rays)
        ft.train_density = band_volume(torch.zeros(tuple(ft.volume.feat_volume.shape[-3:]), device="cuda"), 0.1)
        _step(ft, batch, 0.0)
        _step(ft, batch, 0.0)
        torch.cuda.synchronize()
        print(json.dumps(dict(kind="trace", size=size, mlp=mode, live_fraction=round(ft.last_live_fraction, 5))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("step", "trace"), default="step")
    ap.add_argument("--size", default="config4", choices=sorted(SIZES))
    ap.add_argument("--mlp", default="bf16,fp32")
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--shares", default=",".join(str(s) for s in SHARES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_train.py measures on the GPU; none found")
    results = []
    modes = a.mlp.split(",")
    if a.mode == "step":
        step_mode(a.size, modes, [float(s) for s in a.shares.split(",")], a.pairs, a.rays, results)
    else:
        trace_mode(a.size, modes, a.rays)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
