// Geometric scores of clouds and meshes: a uniform grid over a target cloud, the EXACT nearest neighbour within a radius, the DTU /
// Tanks-and-Temples reductions over the distances, and a deterministic sampler of points on a triangle mesh.  No counterpart in the reference.
//
// grid_bounds_kernel, grid_bounds_final_kernel   min / max of the rows of points (n,3) whose three coordinates are finite, per workgroup and then over the
//                         workgroups: min and max never round, so every order gives the same bits.  No finite row: lo = +inf, hi = -inf.
// grid_count_kernel       one thread per point; a row with a non-finite coordinate is left out; cell (per axis) = floorf((p - lo) * inv_cell) clamped to
//                         [0, dim - 1], flat cell = (cz dim_y + cy) dim_x + cx; counts[cell] += 1 (integer atomic: the sum does not depend on the order).
// grid_scan_part_kernel, grid_scan_top_kernel, grid_scan_kernel   the exclusive prefix of the cells + 1 counts in place -> cell_start (2048 entries per
//                         workgroup: sums, one workgroup over the sums, the offsets).
// grid_fill_kernel        slot = cursor[cell]++ (integer atomic on a copy of cell_start); records[slot] = (x, y, z, bits of the original index).  The order of
//                         the records INSIDE a cell differs between runs; nothing downstream depends on it (grid_nearest_kernel's minimum is over the pair
//                         (d2, original index)).
// grid_nearest_kernel     one thread per query.  d2 = (dx dx + dy dy) + dz dz in fp32, every operation rounded on its own; the result is the minimum of
//                         (d2, original index) in lexicographic order over the grid's points with d2 <= r2 = fl(max_dist max_dist), dist = sqrtf(d2) (IEEE),
//                         or (+inf, -1) when there is none or a coordinate of the query is not finite.  Cells are visited in Chebyshev rings around the
//                         query's clamped cell: ring r is every in-grid cell at Chebyshev distance exactly r, its x-runs scanned as one run of records.
//                         After ring r every unvisited point lies, on some axis, on the far side of one of the up to six planes of the cube of visited
//                         cells.  A point beyond the +a plane has cell index >= k = c_a + r + 1 >= 1, so fl(fl(p - lo) inv_cell) >= k, so p - lo >= k cell
//                         (1 - 4 2^-24) (three roundings, and the one of inv_cell); likewise p - lo < k cell (1 + 4 2^-24), k = c_a - r, beyond the -a plane
//                         (the clamp moves an index only towards the cube, never across the plane).  B = fl(fl(lo + fl(k cell)) - q) (resp. q - ...) differs
//                         from the real lower bound of |p - q| by less than 2e-6 (|k cell| + |lo| + |q|), which is subtracted, and a point at real distance
//                         >= L has a computed d2 >= L^2 (1 - 2^-21): the search stops when fl(L L) 0.999999 > the best d2 so far (r2 while nothing is found),
//                         L the smallest of the bounds of the planes that have cells behind them.  The test only ever keeps the search going longer than
//                         exact arithmetic would; it never trades exactness.  A query outside the box starts from the border cell it clamps to, and the same
//                         bounds hold for it.
// cloud_metrics_part_kernel, cloud_metrics_final_kernel   dist (n) fp32 -> the row [sum of the finite distances, their number, the number below tau_k (k < 8)]
//                         in double: 8192 distances per workgroup in a fixed order, then one workgroup over the partial rows in a fixed order.  d < tau_k is
//                         an fp32 compare.  No atomics; counts are whole numbers below 2^31, exact in a double.
// sample_count_kernel, sample_scan_kernel, sample_offsets_kernel, sample_points_kernel   per face n = max(1, ceilf(L / spacing)), L the longest edge,
//                         each edge sqrtf((dx dx + dy dy) + dz dz); a face with a non-finite vertex, a vertex number outside [0, V) or n > 1024 emits nothing
//                         (the largest n of any face leaves in count[1]).  The face emits the centroids of the n n congruent sub-triangles of its barycentric
//                         lattice: row j = 0..n-1, in a row i = 0..n-1-j, the upward triangle (i,j) - weights (3i+1, 3j+1) - then, while i < n-1-j, the
//                         downward one - (3i+2, 3j+2); point = ((wa A + wb B) + wc C) / (3n) per coordinate with wb, wc the two weights and wa = 3n - wb - wc.
//                         One thread per face counts, one workgroup scans the workgroups' sums (int64), one thread per OUTPUT point finds its face by
//                         bisection of the faces' offsets, so a large face does not hold a lane back.  Ordered by face, then by lattice order; no atomics.
// Arithmetic: fp32, every operation rounded on its own (no contraction), IEEE division and square root.
#include "common.h"
#include "scan_dev.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int CM_THREADS = 256;
constexpr int64_t CM_MAX_CELLS = (int64_t)1 << 24;
constexpr int CM_BOUNDS_ROWS = 8;                         // rows per thread of grid_bounds_kernel
constexpr int CM_SCAN_ITEMS = 8;                          // entries per thread of the cell scan: 2048 per workgroup
constexpr int CM_SCAN_TOP = 1024;
constexpr int CM_MAX_TAUS = 8;
constexpr int CM_ROW = 2 + CM_MAX_TAUS;
constexpr int CM_PART_ITEMS = 32;                         // distances per thread of cloud_metrics_part_kernel: 8192 per workgroup
constexpr int SM_MAX_N = 1024;
constexpr int SM_SCAN_THREADS = 1024;

struct PointGridDesc {
    float lo[3];
    float cell, inv_cell;
    int dim[3];                                           // x, y, z; dim_x dim_y dim_z <= 2^24
};

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// inside [0, dim - 1] whatever p is (fmaxf(NaN, 0) = 0)
__device__ __forceinline__ int cell_axis(const PointGridDesc& g, float p, int a)
{
    const float c = floorf((p - g.lo[a]) * g.inv_cell);
    return (int)fminf(fmaxf(c, 0.0f), (float)(g.dim[a] - 1));
}

// lo / hi of the workgroup's threads -> out[6] by thread 0; every thread of the workgroup calls it
__device__ __forceinline__ void block_bounds(float lo[3], float hi[3], float* __restrict__ out)
{
    __shared__ float s[CM_THREADS / 64][6];
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = mvs_wave_min_down(lo[k]); hi[k] = mvs_wave_max_down(hi[k]); }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) { s[threadIdx.x >> 6][k] = lo[k]; s[threadIdx.x >> 6][3 + k] = hi[k]; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) {
            out[k] = fminf(fminf(s[0][k], s[1][k]), fminf(s[2][k], s[3][k]));
            out[3 + k] = fmaxf(fmaxf(s[0][3 + k], s[1][3 + k]), fmaxf(s[2][3 + k], s[3][3 + k]));
        }
}

__global__ __launch_bounds__(CM_THREADS) void grid_bounds_kernel(const float* __restrict__ points, int64_t n, float* __restrict__ part)
{
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const int64_t base = (int64_t)blockIdx.x * (CM_THREADS * CM_BOUNDS_ROWS) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < CM_BOUNDS_ROWS; ++j) {
        const int64_t i = base + (int64_t)j * CM_THREADS;
        if (i < n) {
            const float p[3] = {points[i * 3 + 0], points[i * 3 + 1], points[i * 3 + 2]};
            if (finite3(p[0], p[1], p[2]))
                for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], p[k]); hi[k] = fmaxf(hi[k], p[k]); }
        }
    }
    block_bounds(lo, hi, part + (int64_t)blockIdx.x * 6);
}

__global__ __launch_bounds__(CM_THREADS) void grid_bounds_final_kernel(const float* __restrict__ part, int nb, float* __restrict__ bounds)
{
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < nb; b += CM_THREADS)
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], part[(int64_t)b * 6 + k]); hi[k] = fmaxf(hi[k], part[(int64_t)b * 6 + 3 + k]); }
    block_bounds(lo, hi, bounds);
}

__global__ __launch_bounds__(CM_THREADS) void grid_count_kernel(const float* __restrict__ points, int64_t n, PointGridDesc g, int* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (i >= n) return;
    const float x = points[i * 3 + 0], y = points[i * 3 + 1], z = points[i * 3 + 2];
    if (!finite3(x, y, z)) return;
    const int c = (cell_axis(g, z, 2) * g.dim[1] + cell_axis(g, y, 1)) * g.dim[0] + cell_axis(g, x, 0);      // < cells
    atomicAdd(&counts[c], 1);
}

// m entries, 2048 per workgroup: bsum[b] = the sum of workgroup b's entries
__global__ __launch_bounds__(CM_THREADS) void grid_scan_part_kernel(const int* __restrict__ v, int m, int* __restrict__ bsum)
{
    __shared__ int s_tot[CM_THREADS / 64];
    const int first = (blockIdx.x * CM_THREADS + threadIdx.x) * CM_SCAN_ITEMS;          // < 2^24 + 2^12
    int sum = 0;
#pragma unroll
    for (int j = 0; j < CM_SCAN_ITEMS; ++j)
        if (first + j < m) sum += v[first + j];
    const int pre = mvs_block_exclusive<CM_THREADS>(sum, s_tot);
    if (threadIdx.x == CM_THREADS - 1) bsum[blockIdx.x] = pre + sum;
}

// ONE workgroup: bsum[nb] -> its exclusive prefix, in place (nb <= 2^13 + 1; the total is the number of finite points, < 2^31)
__global__ __launch_bounds__(CM_SCAN_TOP) void grid_scan_top_kernel(int* __restrict__ bsum, int nb)
{
    __shared__ int s_tot[CM_SCAN_TOP / 64];
    mvs_block_scan_runs<CM_SCAN_TOP>(nb, [&](int i) { return bsum[i]; }, [&](int i, int pre) { bsum[i] = pre; }, s_tot);
}

// v[m] (counts) -> its exclusive prefix, in place, from the workgroups' offsets
__global__ __launch_bounds__(CM_THREADS) void grid_scan_kernel(int* __restrict__ v, int m, const int* __restrict__ boff)
{
    __shared__ int s_tot[CM_THREADS / 64];
    const int first = (blockIdx.x * CM_THREADS + threadIdx.x) * CM_SCAN_ITEMS;
    int c[CM_SCAN_ITEMS], sum = 0;
#pragma unroll
    for (int j = 0; j < CM_SCAN_ITEMS; ++j) {
        c[j] = first + j < m ? v[first + j] : 0;
        sum += c[j];
    }
    int run = boff[blockIdx.x] + mvs_block_exclusive<CM_THREADS>(sum, s_tot);
#pragma unroll
    for (int j = 0; j < CM_SCAN_ITEMS; ++j) {
        if (first + j < m) v[first + j] = run;
        run += c[j];
    }
}

__global__ __launch_bounds__(CM_THREADS) void grid_fill_kernel(const float* __restrict__ points, int64_t n, PointGridDesc g, int* __restrict__ cursor,
                                                               float4* __restrict__ records)
{
    const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (i >= n) return;
    const float x = points[i * 3 + 0], y = points[i * 3 + 1], z = points[i * 3 + 2];
    if (!finite3(x, y, z)) return;
    const int c = (cell_axis(g, z, 2) * g.dim[1] + cell_axis(g, y, 1)) * g.dim[0] + cell_axis(g, x, 0);
    const int slot = atomicAdd(&cursor[c], 1);            // cell_start[c] <= slot < cell_start[c + 1] <= n: the counts of grid_count_kernel on the same rows
    records[slot] = make_float4(x, y, z, __int_as_float((int)i));
}

// the records of cells c0..c1 (one x-run: contiguous) against the query
__device__ __forceinline__ void scan_cells(const int* __restrict__ cell_start, const float4* __restrict__ records, int c0, int c1, float qx, float qy,
                                           float qz, float& best, int& best_i)
{
    const int b = cell_start[c0], e = cell_start[c1 + 1];
    for (int j = b; j < e; ++j) {
        const float4 p = records[j];
        const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const int idx = __float_as_int(p.w);
        if (d2 < best || (d2 == best && idx < best_i)) { best = d2; best_i = idx; }
    }
}

__global__ __launch_bounds__(CM_THREADS) void grid_nearest_kernel(PointGridDesc g, const int* __restrict__ cell_start, const float4* __restrict__ records,
                                                                  const float* __restrict__ query, int64_t nq, float r2, float* __restrict__ dist,
                                                                  int* __restrict__ index)
{
    const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    if (i >= nq) return;
    const float q[3] = {query[i * 3 + 0], query[i * 3 + 1], query[i * 3 + 2]};
    float best = r2;
    int best_i = INT_MAX;                                 // nothing found: a point with d2 == r2 still wins against it
    if (finite3(q[0], q[1], q[2])) {
        const int cx = cell_axis(g, q[0], 0), cy = cell_axis(g, q[1], 1), cz = cell_axis(g, q[2], 2);
        const int c[3] = {cx, cy, cz};
        const int dx = g.dim[0], dy = g.dim[1], dz = g.dim[2];
        for (int r = 0;; ++r) {
            const int x0 = max(cx - r, 0), x1 = min(cx + r, dx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, dy - 1);
            const int z0 = max(cz - r, 0), z1 = min(cz + r, dz - 1);
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const int row = (z * dy + y) * dx;
                    if (z - cz == r || cz - z == r || y - cy == r || cy - y == r) {
                        scan_cells(cell_start, records, row + x0, row + x1, q[0], q[1], q[2], best, best_i);
                    } else {                                                            // (r > 0 here: r == 0 is the case above)
                        if (cx - r >= 0) scan_cells(cell_start, records, row + cx - r, row + cx - r, q[0], q[1], q[2], best, best_i);
                        if (cx + r < dx) scan_cells(cell_start, records, row + cx + r, row + cx + r, q[0], q[1], q[2], best, best_i);
                    }
                }
            float L = INFINITY;                                                         // stays +inf when the whole grid has been visited
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (c[a] + r + 1 <= g.dim[a] - 1) {
                    const float e = (float)(c[a] + r + 1) * g.cell;
                    const float B = (g.lo[a] + e) - q[a];
                    L = fminf(L, fmaxf(B - 2e-6f * ((fabsf(e) + fabsf(g.lo[a])) + fabsf(q[a])), 0.0f));
                }
                if (c[a] - r - 1 >= 0) {
                    const float e = (float)(c[a] - r) * g.cell;
                    const float B = q[a] - (g.lo[a] + e);
                    L = fminf(L, fmaxf(B - 2e-6f * ((fabsf(e) + fabsf(g.lo[a])) + fabsf(q[a])), 0.0f));
                }
            }
            if ((L * L) * 0.999999f > best) break;                                      // (+inf > best: best <= r2 is finite)
        }
    }
    const bool found = best_i != INT_MAX;
    dist[i] = found ? sqrtf(best) : INFINITY;
    index[i] = found ? best_i : -1;
}

struct MetricTaus {
    float t[CM_MAX_TAUS];
    int n;
};

// row[q] of the workgroup's threads -> out[q] by thread 0, waves added in order; every thread of the workgroup calls it
__device__ __forceinline__ void block_row_sum(double row[CM_ROW], double* __restrict__ out)
{
    __shared__ double s[CM_THREADS / 64][CM_ROW];
#pragma unroll
    for (int k = 0; k < CM_ROW; ++k) row[k] = mvs_wave_sum_down(row[k]);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < CM_ROW; ++k) s[threadIdx.x >> 6][k] = row[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < CM_ROW; ++k) out[k] = ((s[0][k] + s[1][k]) + s[2][k]) + s[3][k];
}

__global__ __launch_bounds__(CM_THREADS) void cloud_metrics_part_kernel(const float* __restrict__ dist, int64_t n, MetricTaus taus, double* __restrict__ part)
{
    double row[CM_ROW];
#pragma unroll
    for (int k = 0; k < CM_ROW; ++k) row[k] = 0.0;
    const int64_t base = (int64_t)blockIdx.x * (CM_THREADS * CM_PART_ITEMS) + threadIdx.x;
    for (int j = 0; j < CM_PART_ITEMS; ++j) {
        const int64_t i = base + (int64_t)j * CM_THREADS;
        if (i < n) {
            const float d = dist[i];
            if (isfinite(d)) { row[0] += (double)d; row[1] += 1.0; }
#pragma unroll
            for (int k = 0; k < CM_MAX_TAUS; ++k)
                if (k < taus.n && d < taus.t[k]) row[2 + k] += 1.0;
        }
    }
    block_row_sum(row, part + (int64_t)blockIdx.x * CM_ROW);
}

__global__ __launch_bounds__(CM_THREADS) void cloud_metrics_final_kernel(const double* __restrict__ part, int nb, double* __restrict__ out)
{
    double row[CM_ROW];
#pragma unroll
    for (int k = 0; k < CM_ROW; ++k) row[k] = 0.0;
    for (int b = threadIdx.x; b < nb; b += CM_THREADS)
        for (int k = 0; k < CM_ROW; ++k) row[k] += part[(int64_t)b * CM_ROW + k];
    block_row_sum(row, out);
}

struct MeshSoup {
    const float* vertices;             // [V][3]
    const int* faces;                  // [T][3]
    const int64_t* mesh_count;         // NULL, or {vertices, faces} that are meaningful (a mesh extracted with a capacity)
    int64_t V, T;
    float spacing;
};

__device__ __forceinline__ float edge_length(const float a[3], const float b[3])
{
    const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// the face's corners and its n: 0 = emits nothing (a row past the mesh's count, a vertex number outside the mesh, a non-finite vertex), otherwise
// max(1, ceilf(L / spacing)) clipped to 2^30 (a value above SM_MAX_N emits nothing either and is reported)
__device__ __forceinline__ int face_n(const MeshSoup& m, int64_t f, float A[3], float B[3], float C[3])
{
    int64_t V = m.V, T = m.T;
    if (m.mesh_count) { V = min(V, max(m.mesh_count[0], (int64_t)0)); T = min(T, max(m.mesh_count[1], (int64_t)0)); }
    if (f >= T) return 0;
    const int ia = m.faces[f * 3 + 0], ib = m.faces[f * 3 + 1], ic = m.faces[f * 3 + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) return 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { A[k] = m.vertices[(int64_t)ia * 3 + k]; B[k] = m.vertices[(int64_t)ib * 3 + k]; C[k] = m.vertices[(int64_t)ic * 3 + k]; }
    if (!finite3(A[0], A[1], A[2]) || !finite3(B[0], B[1], B[2]) || !finite3(C[0], C[1], C[2])) return 0;
    const float L = fmaxf(fmaxf(edge_length(A, B), edge_length(B, C)), edge_length(C, A));
    const float nf = ceilf(L / m.spacing);
    if (!(nf <= (float)(1 << 30))) return 1 << 30;        // an overflowed length or quotient
    return nf < 1.0f ? 1 : (int)nf;
}
__device__ __forceinline__ int face_points(int n) { return n > SM_MAX_N ? 0 : n * n; }            // <= 2^20

// bsum[b] = the points of workgroup b's 256 faces (< 2^28), bmax[b] = their largest n
__global__ __launch_bounds__(CM_THREADS) void sample_count_kernel(MeshSoup m, int64_t* __restrict__ bsum, int* __restrict__ bmax)
{
    __shared__ int s_tot[CM_THREADS / 64], s_max[CM_THREADS / 64];
    const int64_t f = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    float A[3], B[3], C[3];
    const int n = f < m.T ? face_n(m, f, A, B, C) : 0;
    const int mx = mvs_wave_max_down(n);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    const int total = mvs_block_sum<CM_THREADS>(mvs_wave_sum_down(face_points(n)), s_tot);             // (its barrier covers s_max too)
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = total;
        bmax[blockIdx.x] = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    }
}

// ONE workgroup: boff = exclusive prefix of bsum (int64), count[0] = the total, count[1] = the largest n
__global__ __launch_bounds__(SM_SCAN_THREADS) void sample_scan_kernel(const int64_t* __restrict__ bsum, const int* __restrict__ bmax, int nb,
                                                                      int64_t* __restrict__ boff, int64_t* __restrict__ count)
{
    __shared__ int64_t s_tot[SM_SCAN_THREADS / 64];
    __shared__ int s_max[SM_SCAN_THREADS / 64];
    int mx = 0;
    for (int i = threadIdx.x; i < nb; i += SM_SCAN_THREADS) mx = max(mx, bmax[i]);       // (a maximum: any order)
    mx = mvs_wave_max_down(mx);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    // nb <= 2^23: the run arithmetic stays below 2^23 + 2^10, and the total below 2^23 * 2^28.  (The scan's barrier covers s_max too.)
    const int64_t total = mvs_block_scan_runs<SM_SCAN_THREADS>(nb, [&](int i) { return bsum[i]; }, [&](int i, int64_t pre) { boff[i] = pre; }, s_tot);
    if (threadIdx.x == 0) {
        int all = 0;
        for (int w = 0; w < SM_SCAN_THREADS / 64; ++w) all = max(all, s_max[w]);
        count[0] = total;
        count[1] = all;
    }
}

// foff[f] = the first output row of face f
__global__ __launch_bounds__(CM_THREADS) void sample_offsets_kernel(MeshSoup m, const int64_t* __restrict__ boff, int64_t* __restrict__ foff)
{
    __shared__ int s_tot[CM_THREADS / 64];
    const int64_t f = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    float A[3], B[3], C[3];
    const int cnt = f < m.T ? face_points(face_n(m, f, A, B, C)) : 0;
    const int pre = mvs_block_exclusive<CM_THREADS>(cnt, s_tot);
    if (f < m.T) foff[f] = boff[blockIdx.x] + pre;
}

__global__ __launch_bounds__(CM_THREADS) void sample_points_kernel(MeshSoup m, const int64_t* __restrict__ foff, const int64_t* __restrict__ count,
                                                                   int64_t capacity, float* __restrict__ points, int* __restrict__ face)
{
    const int64_t p = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
    const int64_t live = count[0] < capacity ? count[0] : capacity;                      // the caller's rows and no others
    if (p >= live) return;
    int64_t lo = 0, hi = m.T - 1;                                                        // the LAST face with foff <= p: the faces before it that share its
    while (lo < hi) {                                                                    // offset emit nothing, and p < the total, so this face owns row p
        const int64_t mid = (lo + hi + 1) >> 1;
        if (foff[mid] <= p) lo = mid; else hi = mid - 1;
    }
    float A[3], B[3], C[3];
    const int n = face_n(m, lo, A, B, C);                                                // 1..1024: the face owns a row
    if (n < 1 || n > SM_MAX_N) return;
    const int s = (int)(p - foff[lo]);                                                   // < n n
    // row j: the largest j with j (2n - j) <= s, i.e. (n - j)^2 >= n^2 - s
    const int rest = n * n - s;                                                          // 1..2^20: exact in a float
    int h = (int)ceilf(sqrtf((float)rest));
    while (h * h < rest) ++h;
    while (h > 1 && (h - 1) * (h - 1) >= rest) --h;
    const int j = n - h;
    const int pos = s - j * (2 * n - j), i = pos >> 1, down = pos & 1;
    const float wb = (float)(3 * i + 1 + down), wc = (float)(3 * j + 1 + down), den = (float)(3 * n);
    const float wa = (den - wb) - wc;                                                    // small whole numbers: exact
#pragma unroll
    for (int k = 0; k < 3; ++k) points[p * 3 + k] = ((wa * A[k] + wb * B[k]) + wc * C[k]) / den;
    face[p] = (int)lo;
}

inline bool rows_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }

// dims >= 1 and dx dy dz <= 2^24
inline bool grid_cells(int dx, int dy, int dz, int64_t* cells)
{
    if (dx < 1 || dy < 1 || dz < 1) return false;
    const int64_t xy = (int64_t)dx * dy;
    if (xy > CM_MAX_CELLS) return false;
    *cells = xy * dz;
    return *cells <= CM_MAX_CELLS;
}
inline int64_t scan_blocks(int64_t m) { return (m + CM_THREADS * CM_SCAN_ITEMS - 1) / (CM_THREADS * CM_SCAN_ITEMS); }

// lo finite, cell finite and > 0 with a finite reciprocal
inline bool grid_desc(const float* lo, float cell, int dx, int dy, int dz, PointGridDesc* g)
{
    if (!(isfinite(lo[0]) && isfinite(lo[1]) && isfinite(lo[2]) && isfinite(cell) && cell > 0.0f && isfinite(1.0f / cell))) return false;
    *g = PointGridDesc{{lo[0], lo[1], lo[2]}, cell, 1.0f / cell, {dx, dy, dz}};
    return true;
}

}  // namespace

extern "C" size_t mvsnerf_grid_bounds_workspace_bytes(int64_t n)
{
    if (!rows_ok(n)) return 0;
    const int64_t nb = (n + CM_THREADS * CM_BOUNDS_ROWS - 1) / (CM_THREADS * CM_BOUNDS_ROWS);
    return (size_t)(nb > 0 ? nb : 1) * 6 * sizeof(float);
}

extern "C" int mvsnerf_grid_bounds_fwd(const float* points, int64_t n, float* bounds, void* workspace, void* stream)
{
    if (!bounds || !workspace || n < 0 || (n > 0 && !points)) return MVSNERF_EINVAL;
    if (!rows_ok(n)) return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(points, 4) || mvs_misaligned(bounds, 4) || mvs_misaligned(workspace, 4)) return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)((n + CM_THREADS * CM_BOUNDS_ROWS - 1) / (CM_THREADS * CM_BOUNDS_ROWS));      // <= 2^20
    float* part = static_cast<float*>(workspace);
    if (nb > 0) {
        grid_bounds_kernel<<<(unsigned)nb, CM_THREADS, 0, st>>>(points, n, part);
        MVS_LAUNCH_CHECK();
    }
    grid_bounds_final_kernel<<<1, CM_THREADS, 0, st>>>(part, nb, bounds);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// workspace: cursor int32 [cells] | bsum int32 [scan_blocks(cells + 1)]
extern "C" size_t mvsnerf_grid_build_workspace_bytes(int64_t n, int dx, int dy, int dz)
{
    int64_t cells;
    if (!rows_ok(n) || !grid_cells(dx, dy, dz, &cells)) return 0;
    return (size_t)(cells + scan_blocks(cells + 1)) * sizeof(int);
}

extern "C" int mvsnerf_grid_build_fwd(const float* points, int64_t n, const float* lo, float cell, int dx, int dy, int dz, int* cell_start, float* records,
                                      void* workspace, void* stream)
{
    if (!lo || !cell_start || !workspace || n < 0 || (n > 0 && (!points || !records))) return MVSNERF_EINVAL;
    int64_t cells;
    PointGridDesc g;
    if (!rows_ok(n) || !grid_cells(dx, dy, dz, &cells) || !grid_desc(lo, cell, dx, dy, dz, &g)) return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(points, 4) || mvs_misaligned(cell_start, 4) || mvs_misaligned(records, 16) || mvs_misaligned(workspace, 4)) return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int m = (int)cells + 1;
    const int nbs = (int)scan_blocks(m);                                                 // <= 2^13 + 1
    int* cursor = static_cast<int*>(workspace);
    int* bsum = cursor + cells;
    hipError_t e = hipMemsetAsync(cell_start, 0, (size_t)m * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    const unsigned nbp = mvs_cdiv(n, CM_THREADS);                                        // <= 2^23
    if (n > 0) {
        grid_count_kernel<<<nbp, CM_THREADS, 0, st>>>(points, n, g, cell_start);
        MVS_LAUNCH_CHECK();
    }
    grid_scan_part_kernel<<<(unsigned)nbs, CM_THREADS, 0, st>>>(cell_start, m, bsum);
    MVS_LAUNCH_CHECK();
    grid_scan_top_kernel<<<1, CM_SCAN_TOP, 0, st>>>(bsum, nbs);
    MVS_LAUNCH_CHECK();
    grid_scan_kernel<<<(unsigned)nbs, CM_THREADS, 0, st>>>(cell_start, m, bsum);
    MVS_LAUNCH_CHECK();
    if (n > 0) {
        e = hipMemcpyAsync(cursor, cell_start, (size_t)cells * sizeof(int), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return (int)e;
        grid_fill_kernel<<<nbp, CM_THREADS, 0, st>>>(points, n, g, cursor, reinterpret_cast<float4*>(records));
        MVS_LAUNCH_CHECK();
    }
    return MVSNERF_OK;
}

extern "C" int mvsnerf_grid_nearest_fwd(const float* lo, float cell, int dx, int dy, int dz, const int* cell_start, const float* records, const float* query,
                                        int64_t n_query, float max_dist, float* dist, int* index, void* stream)
{
    if (!lo || !cell_start || n_query < 0 || (n_query > 0 && (!query || !dist || !index))) return MVSNERF_EINVAL;
    int64_t cells;
    PointGridDesc g;
    if (!rows_ok(n_query) || !grid_cells(dx, dy, dz, &cells) || !grid_desc(lo, cell, dx, dy, dz, &g)) return MVSNERF_EUNSUPPORTED;
    const float r2 = max_dist * max_dist;
    if (!(isfinite(max_dist) && max_dist > 0.0f && isfinite(r2))) return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(cell_start, 4) || mvs_misaligned(records, 16) || mvs_misaligned(query, 4) || mvs_misaligned(dist, 4) || mvs_misaligned(index, 4)) return MVSNERF_EALIGN;
    if (n_query == 0) return MVSNERF_OK;
    grid_nearest_kernel<<<mvs_cdiv(n_query, CM_THREADS), CM_THREADS, 0, (hipStream_t)stream>>>(g, cell_start, reinterpret_cast<const float4*>(records), query,
                                                                                              n_query, r2, dist, index);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" size_t mvsnerf_cloud_metrics_workspace_bytes(int64_t n)
{
    if (!rows_ok(n)) return 0;
    const int64_t nb = (n + CM_THREADS * CM_PART_ITEMS - 1) / (CM_THREADS * CM_PART_ITEMS);
    return (size_t)(nb > 0 ? nb : 1) * CM_ROW * sizeof(double);
}

extern "C" int mvsnerf_cloud_metrics_fwd(const float* dist, int64_t n, const float* taus, int n_tau, double* out, void* workspace, void* stream)
{
    if (!out || !workspace || n < 0 || (n > 0 && !dist) || n_tau < 0 || (n_tau > 0 && !taus)) return MVSNERF_EINVAL;
    if (!rows_ok(n) || n_tau > CM_MAX_TAUS) return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(dist, 4) || mvs_misaligned(out, 8) || mvs_misaligned(workspace, 8)) return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    MetricTaus t{};
    t.n = n_tau;
    for (int k = 0; k < n_tau; ++k) t.t[k] = taus[k];
    const int nb = (int)((n + CM_THREADS * CM_PART_ITEMS - 1) / (CM_THREADS * CM_PART_ITEMS));         // <= 2^18
    double* part = static_cast<double*>(workspace);
    if (nb > 0) {
        cloud_metrics_part_kernel<<<(unsigned)nb, CM_THREADS, 0, st>>>(dist, n, t, part);
        MVS_LAUNCH_CHECK();
    }
    cloud_metrics_final_kernel<<<1, CM_THREADS, 0, st>>>(part, nb, out);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// workspace: foff int64 [T] | bsum int64 [nb] | boff int64 [nb] | bmax int32 [nb], nb = ceil(T / 256)
extern "C" size_t mvsnerf_mesh_sample_workspace_bytes(int64_t n_faces)
{
    if (!rows_ok(n_faces)) return 0;
    const int64_t nb = (n_faces + CM_THREADS - 1) / CM_THREADS;
    return (size_t)(n_faces + 2 * nb) * sizeof(int64_t) + (size_t)nb * sizeof(int) + 8;
}

extern "C" int mvsnerf_mesh_sample_fwd(const float* vertices, int64_t n_vertices, const int* faces, int64_t n_faces, const int64_t* mesh_count, float spacing,
                                       int64_t capacity, float* points, int* face, int64_t* count, void* workspace, void* stream)
{
    if (!count || !workspace || n_vertices < 0 || n_faces < 0 || capacity < 0) return MVSNERF_EINVAL;
    if ((n_vertices > 0 && !vertices) || (n_faces > 0 && !faces) || (capacity > 0 && (!points || !face))) return MVSNERF_EINVAL;
    if (!rows_ok(n_vertices) || !rows_ok(n_faces) || !rows_ok(capacity) || !(isfinite(spacing) && spacing > 0.0f)) return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(vertices, 4) || mvs_misaligned(faces, 4) || mvs_misaligned(mesh_count, 8) || mvs_misaligned(points, 4) || mvs_misaligned(face, 4) ||
        mvs_misaligned(count, 8) || mvs_misaligned(workspace, 8))
        return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)((n_faces + CM_THREADS - 1) / CM_THREADS);                       // <= 2^23
    int64_t* foff = static_cast<int64_t*>(workspace);
    int64_t* bsum = foff + n_faces;
    int64_t* boff = bsum + nb;
    int* bmax = reinterpret_cast<int*>(boff + nb);
    const MeshSoup m{vertices, faces, mesh_count, n_vertices, n_faces, spacing};
    if (nb > 0) {
        sample_count_kernel<<<(unsigned)nb, CM_THREADS, 0, st>>>(m, bsum, bmax);
        MVS_LAUNCH_CHECK();
    }
    sample_scan_kernel<<<1, SM_SCAN_THREADS, 0, st>>>(bsum, bmax, nb, boff, count);
    MVS_LAUNCH_CHECK();
    if (capacity == 0 || nb == 0) return MVSNERF_OK;                                     // the count alone: a caller sizing its outputs
    sample_offsets_kernel<<<(unsigned)nb, CM_THREADS, 0, st>>>(m, boff, foff);
    MVS_LAUNCH_CHECK();
    sample_points_kernel<<<mvs_cdiv(capacity, CM_THREADS), CM_THREADS, 0, st>>>(m, foff, count, capacity, points, face);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
