"""Time of the TSDF fusion and its mesh (geometry.fuse_tsdf, geometry.tsdf_mesh; csrc/tsdf.hip, csrc/mesh.hip) on a DTU-sized scene: 49 views
of 512 x 640 integrated into 128^3 and into 256^3 nodes.

The scene is the analytic rig of the tests (tests/depth_fusion_refs.py: the plane z = 150 and a sphere of radius 120, cameras on an arc of +-14 degrees at
distance 600, fx = fy = 1.1 W), ray-cast here in float64 on the device; the box is the tests' (-160,-150,-140)..(160,150,170) and trunc the default, 3 x the
longest voxel edge.  Medians over --reps repetitions after --warmup unrecorded ones, by device events, in alternating rounds:
    fuse_tsdf           geometry.fuse_tsdf: the inverse cameras on the host and ONE launch over the nodes, the view loop inside
    tsdf_mesh           geometry.tsdf_mesh(colors=True, capacity=None): negate, the weight mask, the masked mesher (count, its one host read, the sized run), the
                        vertex colours
    tsdf_mesh_bare      the same with colors=False
    chain               fuse_tsdf then tsdf_mesh
    torch_restatement   the same definition of the volume in vectorised torch ops on the same GPU (all nodes at once, one view at a time): the baseline, since
                        nothing in the library fused a TSDF before
and, per kernel, the device time of one chain in a run of its own under `rocprofv3 --kernel-trace --stats` (this file with --mode trace in a child process;
kernel_us is null, with the reason, when that run gives no statistics).  The achieved bytes/s of the integration's compulsory traffic over its kernel time
(the device-event time of fuse_tsdf when there is no kernel time) against the 8.0 TB/s HBM3E peak: 12 B per node written (tsdf, weight, colours) and the
depth maps and images read once (8 B per pixel); next to it the VALU bound, the arithmetic of steps 1 and 2 for every (node, view) pair (COUNTED_FLOPS of
them, an IEEE division counted as one though it is about ten instructions) over 78.6 TFLOP/s - half the 157.3 TFLOP/s fp32 vector peak, which counts a fused
multiply-add as two and the definition forbids fusing - and which of the two is the larger.  Nothing is asserted about the order of the
timings; `same_as_restatement` compares the library's volume with the baseline's where both agree on the weight.  Prints one JSON line holding a result per
size and writes it to --out (default profiles/tsdf.json).  Not pinned against any external fusion tool."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

from bench_depth_fusion import ray_cast, rig_cameras

HBM_PEAK, FP32_VALU_PEAK = 8.0e12, 78.6e12
COUNTED_FLOPS = 18 + 8 + 4             # per (node, view): q = w2c X (9 products, 9 sums), u + 0.5 and v + 0.5 (2 products, 2 quotients, 4 sums), sdf / trunc, min, sum
SIZES = {"n128": (49, 512, 640, (128, 128, 128)), "n256": (49, 512, 640, (256, 256, 256)), "tiny": (5, 24, 32, (9, 11, 13))}
BOX = ((-160.0, -150.0, -140.0), (160.0, 150.0, 170.0))
KERNELS = ("tsdf_integrate_kernel", "tsdf_vertex_colors_kernel", "mesh_classify_kernel", "mesh_scan_kernel", "mesh_vertices_kernel", "mesh_faces_kernel")


def _median(v):
    return sorted(v)[len(v) // 2]


def torch_tsdf(images, w2c, K, depth, box, dims, trunc, z_min=0.0):
    """The definition of DESIGN.md 4o in torch ops, fp32 -> (tsdf, weight, colors)"""
    dev = depth.device
    M, Hi, Wi = depth.shape
    D, H, W = dims
    lo, hi = (torch.tensor(b, dtype=torch.float32, device=dev) for b in box)
    size = hi - lo
    k, j, i = torch.meshgrid(torch.arange(D, device=dev, dtype=torch.float32), torch.arange(H, device=dev, dtype=torch.float32),
                             torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    X, Y, Z = lo[0] + i / (W - 1) * size[0], lo[1] + j / (H - 1) * size[1], lo[2] + k / (D - 1) * size[2]
    usable = torch.isfinite(depth) & (depth > 0) & (images[..., 3] != 0)
    tsum = torch.zeros((D, H, W), device=dev)
    wsum = torch.zeros((D, H, W), device=dev, dtype=torch.int32)
    csum = torch.zeros((D, H, W, 3), device=dev, dtype=torch.int32)
    cw = torch.zeros((D, H, W), device=dev, dtype=torch.int32)
    for m in range(M):
        w, kk = w2c[m], K[m]
        q = [((w[r, 0] * X + w[r, 1] * Y) + w[r, 2] * Z) + w[r, 3] for r in range(3)]
        up, vp = kk[0, 0] * q[0] / q[2] + kk[0, 2] + 0.5, kk[1, 1] * q[1] / q[2] + kk[1, 2] + 0.5
        inside = (q[2] > z_min) & (up >= 0) & (up < Wi) & (vp >= 0) & (vp < Hi)
        t = torch.where(inside, vp.floor().long() * Wi + up.floor().long(), torch.zeros((), dtype=torch.long, device=dev))
        sdf = depth[m].reshape(-1)[t] - q[2]
        hit = inside & usable[m].reshape(-1)[t] & (sdf >= -trunc)
        near = hit & (sdf <= trunc)
        tsum = tsum + torch.where(hit, (sdf / trunc).clamp_max(1.0), torch.zeros_like(sdf))
        wsum += hit
        csum += torch.where(near[..., None], images[m].reshape(-1, 4)[t][..., :3].int(), torch.zeros((), dtype=torch.int32, device=dev))
        cw += near
    tsdf = torch.where(wsum > 0, tsum / wsum, torch.ones_like(tsum))
    colors = torch.zeros((D, H, W, 4), device=dev, dtype=torch.uint8)
    den = (2 * cw).clamp_min(1)[..., None]
    colors[..., :3] = torch.where((cw > 0)[..., None], (2 * csum + cw[..., None]) // den, torch.zeros_like(csum)).to(torch.uint8)
    colors[..., 3] = torch.where(cw > 0, 255, 0).to(torch.uint8)
    return tsdf, wsum, colors


def _scene(name, dev):
    from mvsnerf_amd.rays import SceneRays
    M, H, W, dims = SIZES[name]
    c2w, K = rig_cameras(M, H, W)
    depths = ray_cast(c2w, K, H, W, dev)
    depths = torch.where(torch.isfinite(depths), depths, torch.zeros_like(depths))      # a ray that hits nothing: a hole
    g = torch.Generator().manual_seed(0)
    scene = SceneRays(torch.randint(0, 256, (M, H, W, 3), generator=g, dtype=torch.uint8), c2w, K, (300.0, 1000.0), device=dev)
    return scene, depths, c2w, dims


def trace(name):
    """one chain behind one warm-up chain, nothing else: what the kernel trace of the child process records"""
    from mvsnerf_amd import geometry
    dev = torch.device("cuda", torch.cuda.current_device())
    scene, depths, _, dims = _scene(name, dev)
    for _ in range(2):
        geometry.tsdf_mesh(geometry.fuse_tsdf(scene, depths, BOX, dims))
    torch.cuda.synchronize()


def kernel_times(name):
    """({kernel: microseconds of its LAST launch's average over the two chains}, None) from a child process under rocprofv3, or (None, the reason)"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "tsdf", "--", sys.executable, os.path.abspath(__file__), "--mode", "trace", "--sizes", name]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        except (OSError, subprocess.TimeoutExpired) as e:
            return None, f"rocprofv3 did not run: {e}"
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return None, f"rocprofv3 exit {p.returncode}, {len(files)} statistics files: {p.stderr[-300:]}"
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                for k in KERNELS:
                    if k in row["Name"]:
                        out[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2)}
        return (out, None) if "tsdf_integrate_kernel" in out else (None, "no tsdf_integrate_kernel in the statistics")


def measure(name, reps, warmup, profile):
    from mvsnerf_amd import geometry
    M, H, W, dims = SIZES[name]
    dev = torch.device("cuda", torch.cuda.current_device())
    scene, depths, c2w, dims = _scene(name, dev)
    w2cs = torch.from_numpy(np.ascontiguousarray(np.linalg.inv(c2w)[:, :3, :4], dtype=np.float32)).to(dev)
    vol = geometry.fuse_tsdf(scene, depths, BOX, dims)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        def run():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run
    loops = {"fuse_tsdf": timed(lambda: geometry.fuse_tsdf(scene, depths, BOX, dims)),
             "tsdf_mesh": timed(lambda: geometry.tsdf_mesh(vol)),
             "tsdf_mesh_bare": timed(lambda: geometry.tsdf_mesh(vol, colors=False)),
             "chain": timed(lambda: geometry.tsdf_mesh(geometry.fuse_tsdf(scene, depths, BOX, dims))),
             "torch_restatement": timed(lambda: torch_tsdf(scene.images, w2cs, scene.intrinsics, depths, BOX, dims, vol.trunc))}
    ms = {k: [] for k in loops}
    with torch.no_grad():
        for i in range(warmup + reps):
            for k, fn in loops.items():
                t = fn()
                if i >= warmup:
                    ms[k].append(t)
        mesh = geometry.tsdf_mesh(vol)
        theirs = torch_tsdf(scene.images, w2cs, scene.intrinsics, depths, BOX, dims, vol.trunc)
    # the eager restatement may contract or reorder, so a node within rounding of a pixel boundary may tap the neighbouring pixel
    agree = vol.weight == theirs[1]
    same = dict(weight_agrees=round(float(agree.float().mean()), 6),
                max_abs_tsdf_diff_where_it_does=float((vol.tsdf - theirs[0])[agree].abs().max()),
                colors_equal_where_it_does=round(float((vol.colors == theirs[2]).all(-1)[agree].float().mean()), 6))
    med = {k: _median(v) for k, v in ms.items()}
    per_kernel, why = kernel_times(name) if profile else (None, "not asked for (--no-profile)")
    nodes = dims[0] * dims[1] * dims[2]
    traffic = 12 * nodes + 8 * M * H * W
    t_int = per_kernel["tsdf_integrate_kernel"]["average_us"] * 1e-6 if per_kernel else med["fuse_tsdf"] * 1e-3
    t_bytes, t_valu = traffic / HBM_PEAK, COUNTED_FLOPS * nodes * M / FP32_VALU_PEAK
    tbs = traffic / t_int / 1e12
    return dict(kind="tsdf", size=name, views=M, hw=[H, W], dhw=list(dims), nodes=nodes, trunc=vol.trunc, reps=reps,
                observed_fraction=round(float((vol.weight > 0).float().mean()), 4), vertices=int(mesh.count[0]), faces=int(mesh.count[1]),
                median_ms={k: round(v, 4) for k, v in med.items()}, min_ms={k: round(min(v), 4) for k, v in ms.items()},
                max_ms={k: round(max(v), 4) for k, v in ms.items()}, kernel_us=per_kernel, kernel_us_missing_because=why,
                integrate_time_from="rocprofv3 kernel trace" if per_kernel else "device events around fuse_tsdf",
                bytes=traffic, tb_per_s=round(tbs, 4), of_hbm_peak=round(tbs * 1e12 / HBM_PEAK, 4), hbm_peak_tb_per_s=HBM_PEAK / 1e12,
                counted_flops_per_node_view=COUNTED_FLOPS, least_time_us={"bytes": round(t_bytes * 1e6, 2), "valu": round(t_valu * 1e6, 2)},
                bound_by="valu" if t_valu > t_bytes else "bytes", of_the_larger_bound=round(max(t_bytes, t_valu) / t_int, 4),
                same_as_restatement=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="bench", choices=("bench", "trace"))
    ap.add_argument("--sizes", default="n128,n256")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default="profiles/tsdf.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf.py measures on the GPU; none found")
    if a.mode == "trace":
        for name in a.sizes.split(","):
            trace(name)
        return
    line = json.dumps(dict(kind="tsdf", results=[measure(name, a.reps, a.warmup, not a.no_profile) for name in a.sizes.split(",")]))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
