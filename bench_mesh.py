"""Time of the mesh extraction (geometry.extract_mesh, csrc/mesh.hip) on the two volumes a fine-tuned scene has: the fused 128^3 box
volume and a 128 x 176 x 208 frustum volume.

The field is analytic and built on the device: two spheres and a slab (the maximum of their signed distances, in node units), level 0.  Medians over --reps
repetitions after --warmup unrecorded ones, by device events, in alternating rounds:
    extract_mesh          geometry.extract_mesh(capacity=None): the count alone, its one host read, then the run at exactly that size
    extract_mesh_sized    geometry.extract_mesh(capacity=(V, T)): no host read - classify, scan, vertices, faces
    count_only            classify and scan alone (both capacities 0)
    through_vertices      classify, scan and vertices (face capacity 0)
    torch_restatement     the vectorised torch restatement of the definition (tests/mesh_refs.py, fp32) on the same GPU: the baseline, since nothing in the
                          library extracted a mesh before
and, per kernel, the device time of each of the four launches of one sized run as the profiler records it (kernel_us; null when the profiler reports no
device activity - the differences of the three sized timings above then bound them).  The achieved bytes/s of the compulsory traffic of a sized run against
the 8.0 TB/s HBM3E peak (6.29 TB/s is what a float4 copy reaches): the field read once (4 B per node), mask and vbase written and read (10 B per node),
44 B per vertex (vertices, ndc, vertex_edge) and 12 B per face.  Nothing is asserted about the order of the timings; `same_as_restatement` says whether
the library's arrays equal the restatement's (faces and keys exactly, coordinates bit for bit).  Prints one JSON line holding a result per size and
writes it to --out (default profiles/mesh.json).  The mesh is not pinned against any external mesher."""
import argparse
import json
import os
import sys

import torch

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
SIZES = {"box128": (128, 128, 128), "frustum": (128, 176, 208), "tiny": (9, 11, 13)}
KERNELS = ("mesh_classify_kernel", "mesh_scan_kernel", "mesh_vertices_kernel", "mesh_faces_kernel")


def _median(v):
    return sorted(v)[len(v) // 2]


def analytic_field(D, H, W, dev):
    """max(two spheres, a slab) as signed distances in node units, (D,H,W) fp32; float64 arithmetic on the device"""
    k, j, i = torch.meshgrid(torch.arange(D, device=dev, dtype=torch.float64), torch.arange(H, device=dev, dtype=torch.float64),
                             torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    m = float(min(D, H, W))
    s1 = 0.23 * m - torch.sqrt((i - 0.31 * W) ** 2 + (j - 0.42 * H) ** 2 + (k - 0.37 * D) ** 2)
    s2 = 0.17 * m - torch.sqrt((i - 0.68 * W) ** 2 + (j - 0.57 * H) ** 2 + (k - 0.55 * D) ** 2)
    slab = 0.021 * m - (k - 0.803 * D + 0.013 * i).abs()
    return torch.maximum(torch.maximum(s1, s2), slab).to(torch.float32).contiguous()


def kernel_times(fn):
    """{kernel: device microseconds} of one call of fn, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            for name in KERNELS:
                if name in ev.name:
                    dur = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
                    if dur:
                        out[name] = round(out.get(name, 0.0) + float(dur), 2)
        return out if len(out) == len(KERNELS) else None
    except Exception:
        return None


def measure(name, reps, warmup):
    from mvsnerf_amd import geometry
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests"))
    import mesh_refs as R
    D, H, W = SIZES[name]
    dev = torch.device("cuda", torch.cuda.current_device())
    field = analytic_field(D, H, W, dev)
    box = ((-1.0, -1.0, 2.0), (1.0, 1.0, 4.0))
    V, T = geometry.extract_mesh(field, 0.0, box=box).count.tolist()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        def run():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run
    loops = {"extract_mesh": timed(lambda: geometry.extract_mesh(field, 0.0, box=box)),
             "extract_mesh_sized": timed(lambda: geometry.extract_mesh(field, 0.0, box=box, capacity=(V, T))),
             "count_only": timed(lambda: geometry.extract_mesh(field, 0.0, box=box, capacity=(0, 0))),
             "through_vertices": timed(lambda: geometry.extract_mesh(field, 0.0, box=box, capacity=(V, 0))),
             "torch_restatement": timed(lambda: R.extract(field, 0.0, box=box, dtype=torch.float32))}
    ms = {k: [] for k in loops}
    with torch.no_grad():
        for i in range(warmup + reps):
            for k, fn in loops.items():
                t = fn()
                if i >= warmup:
                    ms[k].append(t)
        mesh = geometry.extract_mesh(field, 0.0, box=box, capacity=(V, T))
        ref = R.extract(field, 0.0, box=box, dtype=torch.float32)
        per_kernel = kernel_times(lambda: geometry.extract_mesh(field, 0.0, box=box, capacity=(V, T)))
    bits = lambda t: t.contiguous().view(torch.int32)
    same = dict(count=mesh.count.tolist() == ref["count"].tolist(), faces=bool(torch.equal(mesh.faces, ref["faces"])),
                vertex_edge=bool(torch.equal(mesh.vertex_edge, ref["vertex_edge"])),
                vertices=bool(torch.equal(bits(mesh.vertices), bits(ref["vertices"]))), ndc=bool(torch.equal(bits(mesh.ndc), bits(ref["ndc"]))))
    med = {k: _median(v) for k, v in ms.items()}
    nodes = D * H * W
    traffic = 14 * nodes + 44 * V + 12 * T
    tbs = traffic / (med["extract_mesh_sized"] * 1e-3) / 1e12
    return dict(kind="mesh", size=name, dhw=[D, H, W], nodes=nodes, vertices=V, faces=T, reps=reps,
                median_ms={k: round(v, 4) for k, v in med.items()}, min_ms={k: round(min(v), 4) for k, v in ms.items()},
                max_ms={k: round(max(v), 4) for k, v in ms.items()}, kernel_us=per_kernel,
                stage_ms_by_difference={"classify_and_scan": round(med["count_only"], 4),
                                        "vertices": round(med["through_vertices"] - med["count_only"], 4),
                                        "faces": round(med["extract_mesh_sized"] - med["through_vertices"], 4)},
                bytes=traffic, tb_per_s=round(tbs, 3), of_hbm_peak=round(tbs * 1e12 / HBM_PEAK, 3),
                hbm_peak_tb_per_s=HBM_PEAK / 1e12, hbm_copy_tb_per_s=HBM_COPY / 1e12, same_as_restatement=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="box128,frustum")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/mesh.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py measures on the GPU; none found")
    line = json.dumps(dict(kind="mesh", results=[measure(name, a.reps, a.warmup) for name in a.sizes.split(",")]))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
