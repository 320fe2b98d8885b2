"""Time of the mesh rasteriser and its two mesh tools (geometry.render_mesh, face_views, filter_mesh; csrc/raster.hip).

Mesh: the analytic 128^3 field of bench_mesh.py (two spheres and a slab, level 0) extracted over box = ((-1,-1,2), (1,1,4)), with seeded vertex colours.
Cameras: 49 views of 512 x 640 on a 7 x 7 fan of +-30 degrees around the box centre at distance 4, looking at it, focal 1.2 W.  Medians over --reps calls
after --warmup unrecorded ones, by device events, in alternating rounds:
    render_mesh     geometry.render_mesh(mesh, cameras=...): the host's camera inversion and uploads, the z-buffer clear, the five launches
    raster_only     ops.mesh_raster on cameras already on the device: the clear and the five launches alone
    face_views      geometry.face_views on the 49 face maps
    filter_mesh     geometry.filter_mesh(mesh, seen in >= 1 view): the count, its one host read, the run at that size
The JSON carries faces/s ((face, view) pairs set up per second of raster_only) and z-buffer bytes/s - the compulsory traffic of the 64-bit words: 8 B cleared
and 8 B read per pixel, plus the 11 B of depth, face and colour written - next to the 8.0 TB/s HBM3E peak as context (atomic traffic comes on top and is
not counted).  A first measurement: there is no earlier time and no gate.  Not pinned against any external rasteriser.  Prints one JSON line and writes it
to --out (default profiles/raster.json)."""
import argparse
import json
import math

import numpy as np
import torch

from bench_mesh import analytic_field

HBM_PEAK = 8.0e12
VIEWS, HW = 49, (512, 640)


def _median(v):
    return sorted(v)[len(v) // 2]


def fan_cameras(n_side, hw, centre, dist, half_angle_deg):
    """(c2w (n^2,4,4), K (3,3)) float64: OpenCV cameras (x right, y down, z forward) on an n x n fan of yaw / pitch around `centre`, looking at it"""
    H, W = hw
    c2w = np.zeros((n_side * n_side, 4, 4))
    angles = np.deg2rad(np.linspace(-half_angle_deg, half_angle_deg, n_side))
    for a, pitch in enumerate(angles):
        for b, yaw in enumerate(angles):
            f = np.array([math.sin(yaw) * math.cos(pitch), math.sin(pitch), math.cos(yaw) * math.cos(pitch)])
            x = np.cross(np.array([0.0, 1.0, 0.0]), f)
            x /= np.linalg.norm(x)
            m = a * n_side + b
            c2w[m, :3, :3], c2w[m, :3, 3], c2w[m, 3, 3] = np.stack([x, np.cross(f, x), f], 1), np.asarray(centre) - dist * f, 1.0
    K = np.array([[1.2 * W, 0.0, 0.5 * (W - 1)], [0.0, 1.2 * W, 0.5 * (H - 1)], [0.0, 0.0, 1.0]])
    return c2w, K


def measure(size, n_side, hw, reps, warmup):
    from mvsnerf_amd import geometry, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    H, W = hw
    box = ((-1.0, -1.0, 2.0), (1.0, 1.0, 4.0))
    mesh = geometry.extract_mesh(analytic_field(size, size, size, dev), 0.0, box=box)
    V, T = mesh.count.tolist()
    mesh.colors = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (V, 3)).astype(np.uint8)).to(dev)
    c2w, K = fan_cameras(n_side, hw, (0.0, 0.0, 3.0), 4.0, 30.0)
    M = c2w.shape[0]
    cams = (c2w, K, hw)
    w2c = torch.from_numpy(np.ascontiguousarray(np.linalg.inv(c2w)[:, :3, :4], dtype=np.float32)).to(dev)
    Ks = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(K, (M, 3, 3)), dtype=np.float32)).to(dev)
    img = geometry.render_mesh(mesh, cameras=cams)
    seen = geometry.face_views(img.face, T)
    keep = seen >= 1
    sub = geometry.filter_mesh(mesh, keep)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        def run():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run
    loops = {"render_mesh": timed(lambda: geometry.render_mesh(mesh, cameras=cams)),
             "raster_only": timed(lambda: ops.mesh_raster(mesh.vertices, mesh.faces, w2c, Ks, hw, colors=mesh.colors, mesh_count=mesh.count)),
             "face_views": timed(lambda: geometry.face_views(img.face, T)),
             "filter_mesh": timed(lambda: geometry.filter_mesh(mesh, keep))}
    ms = {k: [] for k in loops}
    with torch.no_grad():
        for i in range(warmup + reps):
            for k, fn in loops.items():
                t = fn()
                if i >= warmup:
                    ms[k].append(t)
        again = geometry.render_mesh(mesh, cameras=cams)
    med = {k: _median(v) for k, v in ms.items()}
    pixels = M * H * W
    zbytes = pixels * (8 + 8 + 11)
    t = med["raster_only"] * 1e-3
    return dict(kind="raster", mesh=f"analytic {size}^3", vertices=V, faces=T, views=M, hw=[H, W], reps=reps, warmup=warmup,
                median_ms={k: round(v, 4) for k, v in med.items()}, min_ms={k: round(min(v), 4) for k, v in ms.items()},
                max_ms={k: round(max(v), 4) for k, v in ms.items()},
                face_views_per_s=round(T * M / t, 1), zbuffer_bytes=zbytes, zbuffer_tb_per_s=round(zbytes / t / 1e12, 4),
                of_hbm_peak=round(zbytes / t / HBM_PEAK, 4), hbm_peak_tb_per_s=HBM_PEAK / 1e12,
                covered=round(float(img.mask.float().mean()), 4), faces_seen=int(keep.sum()), kept=sub.count.tolist(),
                two_runs_same_bytes=bool(torch.equal(again.face, img.face) and torch.equal(again.depth.view(torch.int32), img.depth.view(torch.int32))
                                         and torch.equal(again.colors, img.colors)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--side", type=int, default=7, help="the fan has side x side views")
    ap.add_argument("--hw", default="512,640")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="profiles/raster.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_raster.py measures on the GPU; none found")
    hw = tuple(int(v) for v in a.hw.split(","))
    line = json.dumps(measure(a.size, a.side, hw, a.reps, a.warmup))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
