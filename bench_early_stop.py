"""Timing of early ray termination (render_rays(early_stop=), ops.raymarch_early_stop) against the same frame without it.

  --mode frame    per size and MLP mode: the fine-tuning system of bench_finetune_render.py with its network's alpha_linear.bias raised by --sigma-bias
                  (every sample the MLP sees then has sigma around that value: a band of a dozen samples is opaque) and a density volume of TWO bands of
                  depth planes - the first at 0.2 .. 0.3 of the depth range, the second, occupied but occluded, at 0.6 .. 0.7.  Rows, each timed in
                  alternating pairs (yardstick, new path), device-synchronised, after a warm-up of both at that shape:
                    skip_empty            render_rays(skip_empty=0.0)                                  against the dense render_rays()
                    early_stop            render_rays(early_stop=1e-2, stop_every=G)                   against the dense render_rays()
                    both                  render_rays(skip_empty=0.0, early_stop=1e-2, stop_every=G)   against render_rays(skip_empty=0.0)
                    eps0 / both_eps0      the same two with early_stop=0.0: the price when nothing stops
                  for G in --stop-every (16, 32, 64).  The yardstick of every ratio is the same run's call WITHOUT early_stop - the parent's code path.
                  Reported: every pair's two times, the medians, whether the new path won every pair, the MEASURED last_live_fraction and
                  last_stopped_fraction, and the check of the timed outputs: max |rgb diff| and max |depth diff| against the yardstick frame next to
                  the bound eps + S 2^-22 (times max z); for eps = 0 torch.equal in fp32.
  --mode trace    one frame of `both` at stop_every 32, nothing else: meant to run under `rocprofv3 --kernel-trace --stats`.

Algorithmic bytes of the new kernels, per sample of a sub-batch (S samples per ray, K = ceil(S / G) segments): raw is zero-filled once (16 B) and read
by ops.composite (16 B); ray_transmittance reads 16 B of every sample but the last segment's (the 64-byte lines that hold the 4 B of sigma it needs) and
4 + 4 B of ray_T per ray and segment; live_samples_range reads 4 B of ray_T per window element's ray (cached) and 12 B of NDC when a density is given;
per sample that reaches the MLP 4 B of index, 12 B of NDC read, up to 36 B of compact rows written, and 4 + 16 + 16 B in scatter_rows.
Prints one JSON line per measurement and writes them all to --out.
"""
import argparse
import json

import torch

from bench_finetune_render import SIZES, _frame_rays, _system, _timed

EPS = 1e-2


def two_bands(like):
    """(D,H,W) density: planes [0.2 D, 0.3 D) and [0.6 D, 0.7 D) at 1, the rest 0 - an opaque surface and an occupied region behind it."""
    D = like.shape[0]
    d = torch.zeros_like(like)
    d[int(0.2 * D):max(int(0.3 * D), int(0.2 * D) + 1)] = 1.0
    d[int(0.6 * D):max(int(0.7 * D), int(0.6 * D) + 1)] = 1.0
    return d


def new_kernel_bytes(N, S, G, n_live, with_density):
    """The algorithmic bytes of one sub-batch's zero fill, ray_transmittance, live_samples_range and scatter_rows launches (see the module docstring)."""
    K = -(-S // G)
    P = N * S
    return P * 16 + (P - N * (S - (K - 1) * G)) * 16 + N * (K - 1) * 8 + (P * 12 if with_density else 0) + n_live * (4 + 12 + 36 + 36)


def _median(ts):
    return sorted(ts)[len(ts) // 2]


def _system_for_bench(size, sigma_bias):
    ft, rig, pose = _system(size)
    with torch.no_grad():
        ft.network_fn.nerf.alpha_linear.bias += sigma_bias
    ft.update_density_volume()                                  # builds the voxel positions on first use; replaced by the bands
    ft.density_volume = two_bands(ft.density_volume)
    return ft, _frame_rays(rig, pose, size)


def frame_mode(sizes, pairs, stop_every, batch_rays, sigma_bias, results):
    from mvsnerf_amd import ops
    for size in sizes:
        ft, rays = _system_for_bench(size, sigma_bias)
        S, n_rays = ft.args.N_samples, int(rays.shape[0])
        zmax = float(rays[:, 7].max())
        tol = EPS + S * 2.0 ** -22
        for mode in ("fp32", "auto"):
            with ops.mlp_precision(mode), torch.no_grad():
                dense = lambda: ft.render_rays(rays, batch_rays=batch_rays)
                skip = lambda: ft.render_rays(rays, batch_rays=batch_rays, skip_empty=0.0)
                rows = [("skip_empty", None, None, dense, skip)]
                for G in stop_every:
                    rows += [("early_stop", EPS, G, dense, lambda G=G: ft.render_rays(rays, batch_rays=batch_rays, early_stop=EPS, stop_every=G)),
                             ("both", EPS, G, skip, lambda G=G: ft.render_rays(rays, batch_rays=batch_rays, skip_empty=0.0, early_stop=EPS, stop_every=G))]
                rows += [("eps0", 0.0, 32, dense, lambda: ft.render_rays(rays, batch_rays=batch_rays, early_stop=0.0)),
                         ("both_eps0", 0.0, 32, skip, lambda: ft.render_rays(rays, batch_rays=batch_rays, skip_empty=0.0, early_stop=0.0))]
                for name, eps, G, yard, new in rows:
                    ft.last_stopped_fraction = None
                    y_out, n_out = yard(), new()                 # warm-up of both paths at this shape
                    live, stopped = ft.last_live_fraction, ft.last_stopped_fraction
                    e_rgb, e_depth = float((n_out[0] - y_out[0]).abs().max()), float((n_out[1] - y_out[1]).abs().max())
                    check = dict(max_rgb_diff=e_rgb, max_depth_diff=e_depth)
                    if eps is None:
                        pass                                    # skip_empty against dense: another frame by design (the network is not told the bands)
                    elif eps == 0.0:
                        check["outputs_equal"] = bool(torch.equal(n_out[0], y_out[0]) and torch.equal(n_out[1], y_out[1]))
                    else:
                        check.update(bound_rgb=tol, bound_depth=tol * zmax, within_bound=bool(e_rgb <= tol and e_depth <= tol * zmax))
                    del y_out, n_out
                    t_yard, t_new = [], []
                    for _ in range(pairs):
                        t_yard.append(_timed(yard)[0])
                        t_new.append(_timed(new)[0])
                    r = dict(kind="frame", size=size, mlp=mode, row=name, eps=eps, stop_every=G, sigma_bias=sigma_bias, rays=n_rays, samples=n_rays * S,
                             batch_rays=batch_rays, yardstick="dense" if yard is dense else "skip_empty", live_fraction=round(live, 5),
                             stopped_fraction=None if stopped is None else round(stopped, 5),
                             yardstick_ms=[round(t, 3) for t in t_yard], new_ms=[round(t, 3) for t in t_new],
                             yardstick_median_ms=round(_median(t_yard), 3), new_median_ms=round(_median(t_new), 3),
                             new_wins_every_pair=all(n < y for n, y in zip(t_new, t_yard)), speedup_median=round(_median(t_yard) / _median(t_new), 3), **check)
                    if eps is not None:
                        r["new_kernels_algorithmic_bytes_per_frame"] = new_kernel_bytes(n_rays, S, G, int(round(live * n_rays * S)), name.startswith("both"))
                    results.append(r)
                    print(json.dumps(r), flush=True)
        del ft
        torch.cuda.empty_cache()


def trace_mode(sizes, batch_rays, sigma_bias):
    from mvsnerf_amd import ops
    for size in sizes:
        ft, rays = _system_for_bench(size, sigma_bias)
        with torch.no_grad():
            ft.render_rays(rays, batch_rays=batch_rays, skip_empty=0.0, early_stop=EPS, stop_every=32)
        torch.cuda.synchronize()
        print(json.dumps(dict(kind="trace", size=size, mlp=ops.MLP_PRECISION, live_fraction=round(ft.last_live_fraction, 5),
                              stopped_fraction=round(ft.last_stopped_fraction, 5))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("frame", "trace"), default="frame")
    ap.add_argument("--sizes", default="3view")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--stop-every", default="16,32,64")
    ap.add_argument("--batch-rays", type=int, default=16384)
    ap.add_argument("--sigma-bias", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_early_stop.py measures on the GPU; none found")
    unknown = [s for s in a.sizes.split(",") if s not in SIZES]
    if unknown:
        raise SystemExit(f"bench_early_stop.py: unknown size(s) {unknown}; known: {list(SIZES)}")
    results = []
    if a.mode == "frame":
        frame_mode(a.sizes.split(","), a.pairs, [int(g) for g in a.stop_every.split(",")], a.batch_rays, a.sigma_bias, results)
    else:
        trace_mode(a.sizes.split(","), a.batch_rays, a.sigma_bias)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
