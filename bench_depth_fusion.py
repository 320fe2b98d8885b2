"""Time of the depth-map fusion (geometry.fuse_depths, csrc/depth_fusion.hip) on a DTU-sized scene: 49 views of 512 x 640, n_src = 4, the
defaults pix_thr = 1, rel_thr = 0.01, min_views = 3.

The scene is the analytic rig of the tests (tests/depth_fusion_refs.py: the plane z = 150 and a sphere of radius 120, cameras on an arc of +-14 degrees at
distance 600 with parallel optical axes, fx = fy = 1.1 W), ray-cast here in float64 on the device, so the depth maps are consistent wherever a surface is
visible.  Medians over --reps repetitions after --warmup unrecorded ones, by device events, in alternating rounds:
    consistency       ops.depth_consistency: one launch over M H W pixels
    compaction        ops.point_cloud at the known capacity: count, scan, write
    fuse_depths       geometry.fuse_depths(capacity=None): the inverse cameras, both of the above, the count alone first and its one host read
    torch_eager       the same definition in torch ops on the same GPU (gathers for the taps, then nonzero and indexing): the baseline, since nothing in
                      the library fused depth maps before
and the achieved bytes/s of the two kernels' compulsory traffic against the 8.0 TB/s HBM3E peak (6.29 TB/s is what a float4 copy reaches):
    consistency       per pixel the depth read once (4) and seen, fused, mask written (9), plus 4 bytes per source if every source view's depth map comes
                      from HBM once ("bytes_with_taps"; the taps of neighbouring pixels share cache lines)
    compaction        the mask read twice (2 per pixel); per kept pixel fused, seen and the colour read (12) and 24 bytes of rows written
Nothing is asserted about the order of the timings.  Prints one JSON line and writes it to --out (default profiles/depth_fusion.json).  The result is not
pinned against any external fusion tool."""
import argparse
import json
import math

import numpy as np
import torch

PLANE_Z, SPHERE_R, DIST = 150.0, 120.0, 600.0
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
SIZES = {"dtu": (49, 512, 640), "tiny": (5, 24, 40)}


def _median(v):
    return sorted(v)[len(v) // 2]


def rig_cameras(M, H, W):
    """c2w (M,4,4), K (M,3,3) float64: the recipe of tests/depth_fusion_refs.rig_cameras with parallel optical axes"""
    c2w, K = np.zeros((M, 4, 4)), np.zeros((M, 3, 3))
    for m in range(M):
        a = np.deg2rad(14.0) * (2.0 * m / max(M - 1, 1) - 1.0)
        roll = np.deg2rad(3.0 * (m - (M - 1) / 2.0) * 4.0 / max(M - 1, 1))
        c, s = np.cos(roll), np.sin(roll)
        c2w[m, :3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
        c2w[m, :3, 3] = [DIST * np.sin(a), 25.0 * ((m % 3) - 1) + 0.4 * m, -DIST * np.cos(a)]
        c2w[m, 3, 3] = 1.0
        K[m] = [[1.1 * W, 0.0, 0.5 * (W - 1) + 0.3 - 0.01 * m], [0.0, 1.1 * W, 0.5 * (H - 1) - 0.2 + 0.007 * m], [0.0, 0.0, 1.0]]
    return c2w, K


def ray_cast(c2w, K, H, W, dev):
    """(M,H,W) fp32 depth of the first hit with the sphere or the plane, float64 arithmetic on the device"""
    out = []
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    for m in range(c2w.shape[0]):
        c, k = torch.from_numpy(c2w[m]).to(dev), torch.from_numpy(K[m]).to(dev)
        d = torch.stack([(x - k[0, 2]) / k[0, 0], (y - k[1, 2]) / k[1, 1], torch.ones_like(x)], -1) @ c[:3, :3].T
        o = c[:3, 3]
        tp = (PLANE_Z - o[2]) / d[..., 2]
        a, b, cc = (d * d).sum(-1), (d * o).sum(-1), (o * o).sum() - SPHERE_R ** 2
        disc = b * b - a * cc
        ts = torch.where(disc >= 0, (-b - torch.sqrt(disc.clamp_min(0))) / a, torch.full_like(a, math.inf))
        ts = torch.where(ts > 0, ts, torch.full_like(ts, math.inf))
        out.append(torch.minimum(tp, ts).to(torch.float32))
    return torch.stack(out).contiguous()


def torch_eager(images, c2w, w2c, K, depth, src, pix_thr, rel_thr, min_views):
    """The definition of include/mvsnerf_hip_internal.h in torch ops, all views at once, one source column at a time -> (points, colors, n_views, index, fused, seen)"""
    M, H, W = depth.shape
    y, x = torch.meshgrid(torch.arange(H, device=depth.device, dtype=torch.float32), torch.arange(W, device=depth.device, dtype=torch.float32), indexing="ij")
    usable = torch.isfinite(depth) & (depth > 0) & (images[..., 3] != 0)

    def lift(c, k, px, py, z):      # c (M,3,4), k (M,3,3) -> three (M,H,W)
        dx, dy = (px - k[:, 0, 2, None, None]) / k[:, 0, 0, None, None], (py - k[:, 1, 2, None, None]) / k[:, 1, 1, None, None]
        return [c[:, i, 3, None, None] + (dx * c[:, i, 0, None, None] + dy * c[:, i, 1, None, None] + c[:, i, 2, None, None]) * z for i in range(3)]

    def cam(w, P):
        return [w[:, i, 0, None, None] * P[0] + w[:, i, 1, None, None] * P[1] + w[:, i, 2, None, None] * P[2] + w[:, i, 3, None, None] for i in range(3)]
    P = lift(c2w, K, x, y, depth)
    flat_d, flat_u = depth.reshape(-1), usable.reshape(-1)
    total, n = torch.where(usable, depth, torch.zeros_like(depth)), torch.zeros_like(depth, dtype=torch.int32)
    seen = torch.zeros_like(n)
    for j in range(src.shape[1]):
        s = src[:, j].long()
        have = (s >= 0)[:, None, None]
        sc = s.clamp_min(0)
        q = cam(w2c[sc], P)
        ks = K[sc]
        u, v = ks[:, 0, 0, None, None] * q[0] / q[2] + ks[:, 0, 2, None, None], ks[:, 1, 1, None, None] * q[1] / q[2] + ks[:, 1, 2, None, None]
        inside = have & usable & (q[2] > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        uc, vc = torch.where(inside, u, torch.zeros_like(u)), torch.where(inside, v, torch.zeros_like(v))
        x0, y0 = uc.floor().clamp_max(W - 2), vc.floor().clamp_max(H - 2)
        ax, ay = uc - x0, vc - y0
        t = sc[:, None, None] * (H * W) + y0.long() * W + x0.long()
        z00, z01, z10, z11 = flat_d[t], flat_d[t + 1], flat_d[t + W], flat_d[t + W + 1]
        ok = inside & flat_u[t] & flat_u[t + 1] & flat_u[t + W] & flat_u[t + W + 1]
        zs = (z00 * (1 - ax) + z01 * ax) * (1 - ay) + (z10 * (1 - ax) + z11 * ax) * ay
        b = cam(w2c, lift(c2w[sc], ks, uc, vc, torch.where(ok, zs, torch.ones_like(zs))))
        ex = K[:, 0, 0, None, None] * b[0] / b[2] + K[:, 0, 2, None, None] - x
        ey = K[:, 1, 1, None, None] * b[1] / b[2] + K[:, 1, 2, None, None] - y
        c = ok & (b[2] > 0) & (torch.sqrt(ex * ex + ey * ey) < pix_thr) & ((b[2] - depth).abs() / depth < rel_thr)
        seen |= c.int() << j
        total = total + torch.where(c, b[2], torch.zeros_like(b[2]))
        n += c
    fused = torch.where(usable, total / (n + 1), torch.zeros_like(total))
    index = torch.nonzero(((n >= min_views) & usable).reshape(-1)).reshape(-1)
    Pf = lift(c2w, K, x, y, fused)
    points = torch.stack([p.reshape(-1)[index] for p in Pf], -1)
    return points, images.reshape(-1, 4)[index, :3], n.reshape(-1)[index].to(torch.uint8), index, fused, seen


def measure(name, reps, warmup, n_src):
    from mvsnerf_amd import geometry, ops
    from mvsnerf_amd.rays import SceneRays
    M, H, W = SIZES[name]
    dev = torch.device("cuda", torch.cuda.current_device())
    c2w, K = rig_cameras(M, H, W)
    depths = ray_cast(c2w, K, H, W, dev)
    g = torch.Generator().manual_seed(0)
    scene = SceneRays(torch.randint(0, 256, (M, H, W, 3), generator=g, dtype=torch.uint8), c2w, K, (300.0, 1000.0), device=dev)
    src_np = geometry.nearest_source_ids(scene, n_src)
    src = torch.from_numpy(src_np).to(dev)
    w2cs = torch.from_numpy(np.ascontiguousarray(np.linalg.inv(c2w)[:, :3, :4], dtype=np.float32)).to(dev)
    bank = (scene.images, scene.c2ws, scene.intrinsics)
    seen, fused, mask = ops.depth_consistency(scene.images, scene.c2ws, w2cs, scene.intrinsics, depths, src, alpha=False)
    N = int(ops.point_cloud(*bank, fused, seen, mask, 0)[4].item())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        def run():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run
    loops = {"consistency": timed(lambda: ops.depth_consistency(scene.images, scene.c2ws, w2cs, scene.intrinsics, depths, src, alpha=False)),
             "compaction": timed(lambda: ops.point_cloud(*bank, fused, seen, mask, N)),
             "fuse_depths": timed(lambda: geometry.fuse_depths(scene, depths, src_ids=src_np)),
             "torch_eager": timed(lambda: torch_eager(scene.images, scene.c2ws, w2cs, scene.intrinsics, depths, src, 1.0, 0.01, 3))}
    ms = {k: [] for k in loops}
    with torch.no_grad():
        for i in range(warmup + reps):
            for k, fn in loops.items():
                t = fn()
                if i >= warmup:
                    ms[k].append(t)
        cloud = geometry.fuse_depths(scene, depths, src_ids=src_np)
        theirs = torch_eager(scene.images, scene.c2ws, w2cs, scene.intrinsics, depths, src, 1.0, 0.01, 3)
    med = {k: _median(v) for k, v in ms.items()}
    n_px = M * H * W
    b_cons, b_taps, b_comp = 13 * n_px, (13 + 4 * n_src) * n_px, 2 * n_px + 36 * N
    # the eager restatement rounds in another order, so a pair within rounding of a threshold may fall on the other side (and then moves the average by
    # up to rel_thr z / 2): the clouds are compared where both kept the pixel, and the points where both also saw the same sources
    both = torch.isin(cloud.index, theirs[3])
    sel = torch.isin(theirs[3], cloud.index)
    same = cloud.seen.reshape(-1)[cloud.index[both]] == theirs[5].reshape(-1)[theirs[3][sel]]
    diff = (cloud.points[both] - theirs[0][sel]).abs().amax(-1)
    dmax = float(diff.max()) if bool(both.any()) else None
    dmax_same = float(diff[same].max()) if bool(same.any()) else None
    tb = lambda b, t_ms: round(b / (t_ms * 1e-3) / 1e12, 3)
    return dict(kind="depth_fusion", size=name, views=M, hw=[H, W], n_src=n_src, reps=reps, pixels=n_px, points=N, kept_fraction=round(N / n_px, 4),
                median_ms={k: round(v, 3) for k, v in med.items()}, min_ms={k: round(min(v), 3) for k, v in ms.items()},
                max_ms={k: round(max(v), 3) for k, v in ms.items()},
                bytes={"consistency": b_cons, "consistency_with_taps": b_taps, "compaction": b_comp},
                tb_per_s={"consistency": tb(b_cons, med["consistency"]), "consistency_with_taps": tb(b_taps, med["consistency"]),
                          "compaction": tb(b_comp, med["compaction"])},
                of_hbm_peak={"consistency": round(tb(b_cons, med["consistency"]) * 1e12 / HBM_PEAK, 3),
                             "consistency_with_taps": round(tb(b_taps, med["consistency"]) * 1e12 / HBM_PEAK, 3),
                             "compaction": round(tb(b_comp, med["compaction"]) * 1e12 / HBM_PEAK, 3)},
                hbm_peak_tb_per_s=HBM_PEAK / 1e12, hbm_copy_tb_per_s=HBM_COPY / 1e12,
                eager={"points": int(theirs[3].numel()), "common": int(both.sum()), "common_with_other_sources": int((~same).sum()),
                       "max_abs_point_diff_on_common": dmax, "max_abs_point_diff_same_sources": dmax_same})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="dtu")
    ap.add_argument("--n-src", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/depth_fusion.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_fusion.py measures on the GPU; none found")
    r = measure(a.size, a.reps, a.warmup, a.n_src)
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
