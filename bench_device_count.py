"""Timing of device_count=True (the sparse and early-stopped renders without a host read per sub-batch) against the same call without
it - the host-count path, which is the parent's code, unchanged - in the method of bench_sparse_render.py and bench_early_stop.py: one process, both
paths warmed up at the shape, alternating pairs of device-synchronised host-clock times of a whole frame.

  --mode frame    per size and MLP mode ("fp32", "auto"), on the fine-tuning system of bench_finetune_render.py:
                    dense                 render_rays() twice per pair (the spread of the clock, and the frame the others are to beat)
                    skip_empty            render_rays(skip_empty=0.0, device_count=True) against render_rays(skip_empty=0.0) on band volumes with a plane
                                          share of --shares (bench_sparse_render.band_volume)
                    early_stop / both     early_stop=1e-2, stop_every in --stop-every, alone and with skip_empty=0.0, on bench_early_stop's two-band
                    eps0 / both_eps0      scene (alpha_linear.bias raised by --sigma-bias); the eps = 0 rows: nothing stops
                  Per row: both times of every pair, the medians, whether device_count won every pair, the measured live and stopped fractions, and
                  torch.equal of the timed outputs (rgb, depth) and of the fractions against the host-count frame.
  --mode kernel   one launch against the other at the same n, by device events (median of --reps): ops.mlp_forward(N = n) against
                  ops.mlp_forward(N = cap, count = n) for cap = 16384 x 128 rows and n in {cap, cap / 10, 0}, per kernel ("fp32", "auto", "fp16x3",
                  netwidth 256), and ops.gather likewise.  n = 0 is the price of the workgroups that exit (the host-count path enqueues nothing).
                  --lib PATH loads another build of the library (the tile-walk probe -DMVS_COUNTED_WALK of csrc/mlp_f16x3.hip and mlp_wide.hip).
  --mode trace    one device_count frame of skip_empty at a plane share of 0.1, nothing else: meant to run under `rocprofv3 --kernel-trace --stats`.

Prints one JSON line per measurement and writes them all to --out.
"""
import argparse
import json

import torch

from bench_finetune_render import SIZES, _frame_rays, _system, _timed
from bench_sparse_render import SHARES, band_volume
from bench_early_stop import EPS, two_bands


def _median(ts):
    return sorted(ts)[len(ts) // 2]


def _row(ft, yard, new, pairs, **tags):
    ft.last_stopped_fraction = None
    y_out = yard()                                              # warm-up of both paths at this shape
    y_frac = (ft.last_live_fraction, ft.last_stopped_fraction)
    n_out = new()
    n_frac = (ft.last_live_fraction, ft.last_stopped_fraction)
    equal = bool(torch.equal(n_out[0], y_out[0]) and torch.equal(n_out[1], y_out[1]))
    del y_out, n_out
    t_yard, t_new = [], []
    for _ in range(pairs):
        t_yard.append(_timed(yard)[0])
        t_new.append(_timed(new)[0])
    return dict(kind="frame", **tags, live_fraction=None if n_frac[0] is None else round(n_frac[0], 5),
                stopped_fraction=None if n_frac[1] is None else round(n_frac[1], 5), host_count_ms=[round(t, 3) for t in t_yard],
                device_count_ms=[round(t, 3) for t in t_new], host_count_median_ms=round(_median(t_yard), 3),
                device_count_median_ms=round(_median(t_new), 3), device_count_wins_every_pair=all(n < y for n, y in zip(t_new, t_yard)),
                speedup_median=round(_median(t_yard) / _median(t_new), 3), outputs_equal=equal, fractions_equal=n_frac == y_frac)


def frame_mode(sizes, pairs, shares, stop_every, batch_rays, sigma_bias, results):
    from mvsnerf_amd import ops
    for size in sizes:
        ft, rig, pose = _system(size)
        ft.update_density_volume()                              # builds the voxel positions on first use; replaced by the bands below
        learnt = ft.density_volume
        rays = _frame_rays(rig, pose, size)
        tags = dict(size=size, rays=int(rays.shape[0]), samples=int(rays.shape[0]) * ft.args.N_samples, batch_rays=batch_rays)
        render = lambda **kw: ft.render_rays(rays, batch_rays=batch_rays, **kw)

        def emit(r):
            results.append(r)
            print(json.dumps(r), flush=True)
        for mode in ("fp32", "auto"):
            with ops.mlp_precision(mode), torch.no_grad():
                ft.last_live_fraction = None
                emit(_row(ft, render, render, pairs, row="dense", mlp=mode, **tags))        # (both columns are the dense frame)
                for share in shares:
                    ft.density_volume = band_volume(learnt, share)
                    emit(_row(ft, lambda: render(skip_empty=0.0), lambda: render(skip_empty=0.0, device_count=True), pairs, row="skip_empty", mlp=mode,
                              planes_share=share, **tags))
        # the two-band scene of bench_early_stop.py: an opaque surface and an occupied region behind it
        with torch.no_grad():
            ft.network_fn.nerf.alpha_linear.bias += sigma_bias
        ft.density_volume = two_bands(learnt)
        for mode in ("fp32", "auto"):
            with ops.mlp_precision(mode), torch.no_grad():
                rows = []
                for G in stop_every:
                    rows += [("early_stop", EPS, G, dict(early_stop=EPS, stop_every=G)), ("both", EPS, G, dict(skip_empty=0.0, early_stop=EPS, stop_every=G))]
                rows += [("eps0", 0.0, 32, dict(early_stop=0.0)), ("both_eps0", 0.0, 32, dict(skip_empty=0.0, early_stop=0.0))]
                for name, eps, G, kw in rows:
                    emit(_row(ft, lambda: render(**kw), lambda: render(device_count=True, **kw), pairs, row=name, mlp=mode, eps=eps, stop_every=G,
                              sigma_bias=sigma_bias, **tags))
        del ft
        torch.cuda.empty_cache()


def _event_us(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return round(_median(ts), 2)


def kernel_mode(reps, lib, results):
    from mvsnerf_amd import _lib, models, ops
    if lib:
        _lib.LIB_PATH = lib
    dev, F, cap = "cuda", 20, 16384 * 128
    g = torch.Generator().manual_seed(0)
    ndc, feat = torch.rand((cap, 3), generator=g).to(dev), torch.randn((cap, F), generator=g).to(dev)
    dirs = torch.nn.functional.normalize(torch.randn((cap, 3), generator=g), dim=-1).to(dev)
    out = torch.empty((cap, 4), device=dev)
    nets = {}
    for width in (128, 256):
        torch.manual_seed(width)
        nets[width] = models.MVSNeRF(D=6, W=width, input_ch_pts=63, input_ch_views=3, input_ch_feat=F, skips=[4], net_type="v0").to(dev)
    with torch.no_grad():
        for name, mode, width in (("fp32", "fp32", 128), ("auto", "auto", 128), ("fp16x3", "fp16x3", 128), ("wide", "fp32", 256)):
            with ops.mlp_precision(mode):
                m = nets[width]
                packed, alt = m.packed(F), m.packed_alt(F)
                q = lambda N, **kw: ops.mlp_forward(packed, F, ndc.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, N, 1, 0, dev, out=out[:N], **alt, **kw)
                for n in (cap, cap // 10, 0):
                    count = torch.tensor([n], dtype=torch.int32, device=dev)
                    host = (lambda: q(n)) if n else (lambda: None)          # at n = 0 the host-count path enqueues nothing
                    counted = lambda: q(cap, count=count)
                    host(), counted()
                    r = dict(kind="kernel", op="mlp_forward", kernel=name, cap=cap, n=n, host_count_us=_event_us(host, reps),
                             device_count_us=_event_us(counted, reps), library=lib or "product")
                    results.append(r)
                    print(json.dumps(r), flush=True)
        vol = torch.randn((128, 176, 208, 8), device=dev)
        imgs = torch.rand((3, 3, 512, 640), device=dev)
        w2cs, Ks = torch.eye(4, device=dev).repeat(3, 1, 1), torch.tensor([[400.0, 0, 320], [0, 400, 256], [0, 0, 1]], device=dev).repeat(3, 1, 1)
        pts = torch.cat([ndc[:, :2] - 0.5, ndc[:, 2:] + 2.0], -1).contiguous()
        bufs = (torch.empty((cap, 1, F), device=dev), torch.empty((cap, 3), device=dev))
        for n in (cap, cap // 10, 0):
            count = torch.tensor([n], dtype=torch.int32, device=dev)
            host = (lambda: ops.gather(vol, imgs, w2cs, Ks, pts[:n].view(n, 1, 3), ndc[:n].view(n, 1, 3), dirs[:n], out=(bufs[0][:n], bufs[1][:n]))) \
                if n else (lambda: None)
            counted = lambda: ops.gather(vol, imgs, w2cs, Ks, pts.view(cap, 1, 3), ndc.view(cap, 1, 3), dirs, count=count, out=bufs)
            host(), counted()
            r = dict(kind="kernel", op="gather", cap=cap, n=n, host_count_us=_event_us(host, reps), device_count_us=_event_us(counted, reps),
                     library=lib or "product")
            results.append(r)
            print(json.dumps(r), flush=True)


def trace_mode(sizes, batch_rays):
    from mvsnerf_amd import ops
    for size in sizes:
        ft, rig, pose = _system(size)
        ft.update_density_volume()
        ft.density_volume = band_volume(ft.density_volume, 0.1)
        rays = _frame_rays(rig, pose, size)
        with torch.no_grad():
            ft.render_rays(rays, batch_rays=batch_rays, skip_empty=0.0, device_count=True)
        torch.cuda.synchronize()
        print(json.dumps(dict(kind="trace", size=size, mlp=ops.MLP_PRECISION, live_fraction=round(ft.last_live_fraction, 5))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("frame", "kernel", "trace"), default="frame")
    ap.add_argument("--sizes", default="3view,config4")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shares", default=",".join(str(s) for s in SHARES))
    ap.add_argument("--stop-every", default="16,32,64")
    ap.add_argument("--batch-rays", type=int, default=16384)
    ap.add_argument("--sigma-bias", type=float, default=1.0)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_count.py measures on the GPU; none found")
    unknown = [s for s in a.sizes.split(",") if s not in SIZES]
    if unknown:
        raise SystemExit(f"bench_device_count.py: unknown size(s) {unknown}; known: {list(SIZES)}")
    results = []
    if a.mode == "frame":
        frame_mode(a.sizes.split(","), a.pairs, [float(s) for s in a.shares.split(",")], [int(g) for g in a.stop_every.split(",")], a.batch_rays,
                   a.sigma_bias, results)
    elif a.mode == "kernel":
        kernel_mode(a.reps, a.lib, results)
    else:
        trace_mode(a.sizes.split(","), a.batch_rays)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
