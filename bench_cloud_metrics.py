"""Time of the cloud scores (geometry.PointGrid, evaluate.cloud_metrics, geometry.sample_mesh; csrc/cloud_metrics.hip) on two analytic clouds:
points on a sphere of radius 150 in a 400-unit box with Gaussian radial noise (sigma 2 for the reconstruction, 0.5 for the scan), max_dist 20, 2^18 against
2^18 points and 2^21 against 2^21.

Medians over --reps repetitions after --warmup unrecorded ones, by device events on the current stream, in alternating rounds:
    grid_build          geometry.PointGrid(scan, max_dist): bounds, their one host read of six floats, count, scan, fill
    grid_build_box      the same with box= given: no host read
    nearest_pred_to_gt, nearest_gt_to_pred      grid.nearest, one per direction
    reduce              ops.cloud_metrics_row over one direction's distances (two launches)
    cloud_metrics       evaluate.cloud_metrics(pred, gt, max_dist): both grids, both queries, both reductions
    cloud_metrics_grids the same with grids= reused
and, per size, for `cell` = max_dist x each of --factors: the grid's dimensions, the build and the pred-to-gt query - the measurement behind
geometry.GRID_CELL_FACTOR - and the same query with the queries first sorted by their cell (torch.argsort of the flat cell number, timed separately): the
measurement behind NOT sorting inside the library.  At 2^18 also the same distances from a chunked torch.cdist on the same GPU (2048 queries a chunk), the
only way the library had before, and the largest |difference| where both find a neighbour.  sample_mesh: on the extract_mesh sphere of a 256^3 distance field
at a spacing of two thirds of a cell, with and without capacity=.
`of_hbm_peak` is the COMPULSORY traffic of a query (16 B per record read once, 12 B per query read, 8 B written) over its time against 8.0 TB/s: a lower
bound that says how far a gather-bound search is from streaming, not a share of what the kernel actually moves (every query re-reads the records of
the cells around it through L2).  Nothing is asserted about the timings.  Prints one JSON line and writes it to --out (default
profiles/cloud_metrics.json).  Not pinned against any external tool."""
import argparse
import json

import torch

HBM_PEAK = 8.0e12
SIZES = {"n18": 1 << 18, "n21": 1 << 21, "tiny": 1 << 10}
MAX_DIST, RADIUS, BOX = 20.0, 150.0, ((-200.0, -200.0, -200.0), (200.0, 200.0, 200.0))


def _median(v):
    return sorted(v)[len(v) // 2]


def noisy_sphere(n, sigma, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    d = torch.randn((n, 3), generator=g, device=dev)
    d = d / d.norm(dim=1, keepdim=True)
    return (d * (RADIUS + sigma * torch.randn((n, 1), generator=g, device=dev))).contiguous()


def cdist_nearest(query, target, max_dist, chunk=2048):
    dist = torch.empty((query.shape[0],), device=query.device)
    index = torch.empty((query.shape[0],), device=query.device, dtype=torch.int64)
    for b in range(0, query.shape[0], chunk):
        d, i = torch.cdist(query[b:b + chunk], target).min(dim=1)
        dist[b:b + chunk], index[b:b + chunk] = d, i
    return torch.where(dist <= max_dist, dist, torch.full_like(dist, float("inf"))), index


def _timer():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        def run():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run
    return timed


def _rounds(loops, reps, warmup):
    ms = {k: [] for k in loops}
    for i in range(warmup + reps):
        for k, fn in loops.items():
            t = fn()
            if i >= warmup:
                ms[k].append(t)
    return ({k: round(_median(v), 4) for k, v in ms.items()}, {k: round(min(v), 4) for k, v in ms.items()}, {k: round(max(v), 4) for k, v in ms.items()})


def measure(name, reps, warmup, factors):
    from mvsnerf_amd import evaluate, geometry, ops
    n = SIZES[name]
    dev = torch.device("cuda", torch.cuda.current_device())
    pred, gt = noisy_sphere(n, 2.0, 1, dev), noisy_sphere(n, 0.5, 2, dev)
    timed = _timer()
    with torch.no_grad():
        grid_gt, grid_pred = geometry.PointGrid(gt, MAX_DIST), geometry.PointGrid(pred, MAX_DIST)
        dist, index = grid_gt.nearest(pred)
        loops = {"grid_build": timed(lambda: geometry.PointGrid(gt, MAX_DIST)),
                 "grid_build_box": timed(lambda: geometry.PointGrid(gt, MAX_DIST, box=BOX)),
                 "nearest_pred_to_gt": timed(lambda: grid_gt.nearest(pred)),
                 "nearest_gt_to_pred": timed(lambda: grid_pred.nearest(gt)),
                 "reduce": timed(lambda: ops.cloud_metrics_row(dist, (0.5, 1.0, 2.0))),
                 "cloud_metrics": timed(lambda: evaluate.cloud_metrics(pred, gt, MAX_DIST)),
                 "cloud_metrics_grids": timed(lambda: evaluate.cloud_metrics(pred, gt, MAX_DIST, grids=(grid_gt, grid_pred)))}
        med, lo, hi = _rounds(loops, reps, warmup)
        # the choice of the cell edge, and sorted against unsorted queries
        cells = []
        for f in factors:
            grid = geometry.PointGrid(gt, MAX_DIST, cell=MAX_DIST * f)
            lo3 = torch.tensor(grid.lo, device=dev)
            key = ((pred - lo3) / grid.cell).floor().clamp_(min=0)
            dims = torch.tensor(grid.dims, device=dev, dtype=torch.float32)
            key = torch.minimum(key, dims - 1).long()
            flat = (key[:, 2] * grid.dims[1] + key[:, 1]) * grid.dims[0] + key[:, 0]
            order = torch.argsort(flat)
            pred_sorted = pred[order].contiguous()
            d_sorted, i_sorted = grid.nearest(pred_sorted)
            d_plain, i_plain = grid.nearest(pred)
            assert torch.equal(d_sorted, d_plain[order]) and torch.equal(i_sorted, i_plain[order]) and torch.equal(d_plain, dist) and torch.equal(i_plain, index)
            m, _, _ = _rounds({"build": timed(lambda: geometry.PointGrid(gt, MAX_DIST, cell=MAX_DIST * f)),
                               "nearest": timed(lambda: grid.nearest(pred)),
                               "nearest_sorted_queries": timed(lambda: grid.nearest(pred_sorted)),
                               "sort_queries": timed(lambda: pred[torch.argsort(flat)].contiguous())}, reps, warmup)
            occupied = int((grid.cell_start[1:] > grid.cell_start[:-1]).sum())
            cells.append(dict(factor=f, cell=grid.cell, dims=list(grid.dims), occupied_cells=occupied,
                              points_per_occupied_cell=round(n / max(occupied, 1), 2), median_ms=m))
        found = torch.isfinite(dist)
        out = dict(kind="cloud_metrics", size=name, n_pred=n, n_gt=n, max_dist=MAX_DIST, reps=reps, default_cell_factor=geometry.GRID_CELL_FACTOR,
                   default_dims=list(grid_gt.dims), found_fraction=round(float(found.float().mean()), 6), mean_dist=float(dist[found].double().mean()),
                   median_ms=med, min_ms=lo, max_ms=hi, cell_choice=cells)
        t = med["nearest_pred_to_gt"] * 1e-3
        out["nearest_mqueries_per_s"] = round(n / t / 1e6, 2)
        out["compulsory_bytes"] = 16 * n + 20 * n
        out["of_hbm_peak"] = round(out["compulsory_bytes"] / t / HBM_PEAK, 5)
        if n <= 1 << 18:
            cd, ci = cdist_nearest(pred, gt, MAX_DIST)
            m, _, _ = _rounds({"cdist_chunked": timed(lambda: cdist_nearest(pred, gt, MAX_DIST))}, max(reps // 3, 1), 1)
            both = torch.isfinite(cd) & found
            out["cdist_chunked_ms"] = m["cdist_chunked"]
            out["cdist_max_abs_diff"] = float((cd - dist)[both].abs().max())
            out["cdist_same_found"] = bool((torch.isfinite(cd) == found).all())
            out["cdist_index_agreement"] = round(float((ci[both] == index[both].long()).float().mean()), 6)
    return out


def measure_sampler(reps, warmup, n_grid):
    from mvsnerf_amd import geometry
    dev = torch.device("cuda", torch.cuda.current_device())
    timed = _timer()
    with torch.no_grad():
        ax = torch.linspace(BOX[0][0], BOX[1][0], n_grid, device=dev)
        z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
        mesh = geometry.extract_mesh(RADIUS - torch.sqrt(x * x + y * y + z * z), 0.0, box=BOX)
        h = (BOX[1][0] - BOX[0][0]) / (n_grid - 1)
        s = geometry.sample_mesh(mesh, h * 2 / 3)
        cap = int(s.count[0])
        med, lo, hi = _rounds({"sample_mesh": timed(lambda: geometry.sample_mesh(mesh, h * 2 / 3)),
                               "sample_mesh_capacity": timed(lambda: geometry.sample_mesh(mesh, h * 2 / 3, capacity=cap))}, reps, warmup)
    t = med["sample_mesh_capacity"] * 1e-3
    traffic = 16 * cap + 12 * int(mesh.faces.shape[0]) + 12 * int(mesh.vertices.shape[0])      # rows written, faces and vertices read once
    return dict(kind="sample_mesh", field=[n_grid] * 3, vertices=int(mesh.vertices.shape[0]), faces=int(mesh.faces.shape[0]), spacing=h * 2 / 3, points=cap,
                largest_n=int(s.count[1]), median_ms=med, min_ms=lo, max_ms=hi, bytes=traffic, of_hbm_peak=round(traffic / t / HBM_PEAK, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="n18,n21")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--factors", default="1,0.5,0.25,0.125")
    ap.add_argument("--mesh-grid", type=int, default=256)
    ap.add_argument("--out", default="profiles/cloud_metrics.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_metrics.py measures on the GPU; none found")
    factors = [float(f) for f in a.factors.split(",")]
    results = [measure(name, a.reps, a.warmup, factors) for name in a.sizes.split(",")]
    results.append(measure_sampler(a.reps, a.warmup, a.mesh_grid))
    line = json.dumps(dict(kind="cloud_metrics", hbm_peak_tb_per_s=HBM_PEAK / 1e12, results=results))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
