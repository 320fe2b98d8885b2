// A triangle mesh -> depth, face and colour maps in the scene's pinhole cameras: a z-buffer rasteriser, the views a face owns pixels in, and the stable
// compaction of a mesh to a subset of its faces (where the definition is written out; include/mvsnerf_hip_internal.h carries it too).  No
// counterpart in the reference.  Conventions are tsdf.hip's and depth_fusion.hip's: w2c [M][3][4], K [M][3][3], pixel centres at integer coordinates, depth =
// camera-space z, fp32 with every operation rounded on its own and IEEE division.  Vertices are snapped to a grid of 1/256 pixel and coverage is decided in
// int64, so the fill rule (top-left) is exact: shared edges are watertight and no pixel is hit twice.
//
// The z-buffer is one 64-bit word per pixel and view, float_bits(z) << 32 | face, all ones when empty, resolved with a no-return 64-bit unsigned atomic min
// (one global_atomic_umin_x2, no compare-and-swap loop).  z > 0, so the floats order as their bits: the smallest z wins, the lowest face number among equal
// z bits, whatever the arrival order - two runs give the same bytes.  A plain load in front of the atomic drops fragments that cannot win: the word only
// ever falls, so a stale value is no smaller than the current one and the test never drops a winner.
//
// raster_faces_kernel       one thread per (face, view), views in blockIdx.y: setup, then a loop over the face's clipped box (marching-tetrahedra faces
//                           cover a handful of pixels and consecutive faces are neighbours on screen).  A face whose box exceeds RS_BIG pixels in a
//                           direction is not rasterised here: its wave's ballot word and the workgroup's count go to the workspace.
// raster_big_scan_kernel    ONE workgroup: the exclusive prefix of the workgroups' counts and the total (scan_dev.h).
// raster_big_list_kernel    the big (face, view) items in item order (ballot ranks: stable, no atomics).
// raster_big_faces_kernel   a workgroup per listed item strides over its box.
// raster_resolve_kernel     one thread per pixel: reads the word, redoes the setup of the winning face and writes depth (the word's own bits), face, colour.
// mesh_face_views_kernel    one thread per pixel of the face maps: ORs bit m & 31 into seen[face][m >> 5] (integer atomic OR: order-free).
// filter_*                  mark the used vertices with plain stores of 1, then count -> scan -> write over the vertices (a remap table, -1 = dropped) and
//                           over the faces.
#include "scan_dev.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_SCAN_THREADS = 1024;
constexpr int RS_SUB_SHIFT = 8;                          // SUB = 256 sub-pixel positions per pixel
constexpr float RS_SUB = 256.0f;
constexpr float RS_MAX_SNAP = 8388608.0f;                // |X|, |Y| <= 2^23: every edge product fits int64 (differences < 2^25, products < 2^50)
constexpr int RS_BIG = 16;                               // a clipped box wider or higher than this goes to raster_big_faces_kernel
constexpr int RS_MAX_IMAGE = 1 << 15;                    // 256 x < 2^23 like a snapped vertex
constexpr int RS_MAX_VIEWS = 65535;                      // blockIdx.y
constexpr int64_t RS_MAX_BLOCKS = (int64_t)1 << 22;      // workgroups of raster_faces_kernel: an item number (block * 256 + thread) is an int32
constexpr int RS_BIG_GRID = 8192;                        // raster_big_faces_kernel's workgroups stride over the list: its length stays on the device
constexpr unsigned long long RS_EMPTY = ~0ull;

struct RasterMesh {
    const float* vertices;             // [V][3]
    const int* faces;                  // [T][3]
    const unsigned char* colors;       // [V][3] or NULL
    const int64_t* mesh_count;         // NULL, or {vertices, faces} that are meaningful (a mesh extracted with a capacity)
    int64_t V, T;
};

struct RasterViews {
    const float* w2c;                  // [M][3][4]
    const float* K;                    // [M][3][3]
    const int* view_ids;               // [slots] or NULL: every view, ascending
    int slots, M, H, W, cull;
    float z_min;
};

// a face after setup: b and c swapped where A < 0, so that A > 0
struct FaceSetup {
    int ia, ib, ic;
    int x[3], y[3];                    // snapped positions, 1/256 pixel
    float iz[3];                       // 1 / q.z
    int64_t A;
    int xs, xe, ys, ye;                // the snapped bounding box clipped to the image, in pixels (may be empty)
};

// e(x, y) = c + ax x + ay y at pixel (x, y): the edge function (xb-xa)(py-ya) - (yb-ya)(px-xa) at px = 256 x, py = 256 y; bias = 0 for a top-left edge
// (dy < 0, or dy == 0 and dx > 0) and -1 otherwise, so that the pixel is on the edge's inner side iff e + bias >= 0
struct EdgeEq {
    int64_t c, ax, ay;
    int bias;
};

__device__ __forceinline__ EdgeEq edge_eq(int xa, int ya, int xb, int yb)
{
    const int64_t dx = xb - xa, dy = yb - ya;
    EdgeEq e;
    e.c = dy * xa - dx * ya;                                                              // < 2^49
    e.ax = -(dy << RS_SUB_SHIFT);
    e.ay = dx << RS_SUB_SHIFT;
    e.bias = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
    return e;
}
__device__ __forceinline__ int64_t edge_at(const EdgeEq& e, int x, int y) { return e.c + e.ax * x + e.ay * y; }

__device__ __forceinline__ void live_counts(const RasterMesh& m, int64_t& V, int64_t& T)
{
    V = m.V; T = m.T;
    if (m.mesh_count) { V = min(V, max(m.mesh_count[0], (int64_t)0)); T = min(T, max(m.mesh_count[1], (int64_t)0)); }
}

__device__ __forceinline__ void to_camera(const float* __restrict__ w2c, const float P[3], float q[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = ((w2c[k * 4 + 0] * P[0] + w2c[k * 4 + 1] * P[1]) + w2c[k * 4 + 2] * P[2]) + w2c[k * 4 + 3];
}

// a vertex in a view: its snapped position and 1 / q.z; false when it is unusable
__device__ __forceinline__ bool snap_vertex(const float* __restrict__ w2c, const float* __restrict__ K, float z_min, const float* __restrict__ P, int& X, int& Y,
                                            float& iz)
{
    const float p[3] = {P[0], P[1], P[2]};
    float q[3];
    to_camera(w2c, p, q);
    const float u = K[0] * q[0] / q[2] + K[2], v = K[4] * q[1] / q[2] + K[5];
    const float fx = floorf(u * RS_SUB + 0.5f), fy = floorf(v * RS_SUB + 0.5f);
    iz = 1.0f / q[2];
    const bool ok = q[2] > z_min && isfinite(u) && isfinite(v) && fabsf(fx) <= RS_MAX_SNAP && fabsf(fy) <= RS_MAX_SNAP;       // a NaN fails
    X = ok ? (int)fx : 0;
    Y = ok ? (int)fy : 0;
    return ok;
}

// the setup of face f in view `view` (inside [0, M)); false when the face is dropped whole
__device__ __forceinline__ bool face_setup(const RasterMesh& m, const RasterViews& v, int view, int64_t f, FaceSetup& s)
{
    int64_t V, T;
    live_counts(m, V, T);
    if (f >= T) return false;
    const int ia = m.faces[f * 3 + 0], ib = m.faces[f * 3 + 1], ic = m.faces[f * 3 + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) return false;
    const float* w2c = v.w2c + (int64_t)view * 12;
    const float* K = v.K + (int64_t)view * 9;
    bool ok = snap_vertex(w2c, K, v.z_min, m.vertices + (int64_t)ia * 3, s.x[0], s.y[0], s.iz[0]);
    ok = snap_vertex(w2c, K, v.z_min, m.vertices + (int64_t)ib * 3, s.x[1], s.y[1], s.iz[1]) && ok;
    ok = snap_vertex(w2c, K, v.z_min, m.vertices + (int64_t)ic * 3, s.x[2], s.y[2], s.iz[2]) && ok;
    if (!ok) return false;
    int64_t A = (int64_t)(s.x[1] - s.x[0]) * (s.y[2] - s.y[0]) - (int64_t)(s.y[1] - s.y[0]) * (s.x[2] - s.x[0]);
    if (A == 0 || (v.cull > 0 && A > 0) || (v.cull < 0 && A < 0)) return false;
    s.ia = ia; s.ib = ib; s.ic = ic;
    if (A < 0) {
        A = -A;
        s.ib = ic; s.ic = ib;
        int t = s.x[1]; s.x[1] = s.x[2]; s.x[2] = t;
        t = s.y[1]; s.y[1] = s.y[2]; s.y[2] = t;
        const float z = s.iz[1]; s.iz[1] = s.iz[2]; s.iz[2] = z;
    }
    s.A = A;
    const int xl = min(min(s.x[0], s.x[1]), s.x[2]), xh = max(max(s.x[0], s.x[1]), s.x[2]);
    const int yl = min(min(s.y[0], s.y[1]), s.y[2]), yh = max(max(s.y[0], s.y[1]), s.y[2]);
    s.xs = max(0, (xl + 255) >> RS_SUB_SHIFT); s.xe = min(v.W - 1, xh >> RS_SUB_SHIFT);          // ceil and floor of a signed number: arithmetic shifts
    s.ys = max(0, (yl + 255) >> RS_SUB_SHIFT); s.ye = min(v.H - 1, yh >> RS_SUB_SHIFT);
    return true;
}

// the fragment of a covered pixel: t_k = b_k iz_k and z; false when it does not count
__device__ __forceinline__ bool fragment(const FaceSetup& s, int64_t e1, int64_t e2, float z_min, float t[3], float& z)
{
    const float fA = (float)s.A;
    const float b1 = (float)e1 / fA, b2 = (float)e2 / fA, b0 = (1.0f - b1) - b2;
    t[0] = b0 * s.iz[0]; t[1] = b1 * s.iz[1]; t[2] = b2 * s.iz[2];
    const float invz = (t[0] + t[1]) + t[2];
    z = 1.0f / invz;
    return isfinite(z) && z > z_min;
}

__device__ __forceinline__ void depth_test(unsigned long long* __restrict__ zbuf, int64_t p, float z, unsigned face)
{
    const unsigned long long key = (unsigned long long)__float_as_uint(z) << 32 | face;
    if (key < zbuf[p]) atomicMin(zbuf + p, key);                                          // (the word only falls: a stale load never drops a winner)
}

struct FaceEdges {
    EdgeEq e0, e1, e2;                 // the edges opposite vertex 0, 1, 2: e_k / A is vertex k's barycentric weight
};
__device__ __forceinline__ FaceEdges face_edges(const FaceSetup& s)
{
    return FaceEdges{edge_eq(s.x[1], s.y[1], s.x[2], s.y[2]), edge_eq(s.x[2], s.y[2], s.x[0], s.y[0]), edge_eq(s.x[0], s.y[0], s.x[1], s.y[1])};
}

// words[block * 4 + wave] = the ballot of the wave's big faces, bsum[block] = their number; block = slot * gridDim.x + blockIdx.x
__global__ __launch_bounds__(RS_THREADS) void raster_faces_kernel(RasterMesh m, RasterViews v, unsigned long long* __restrict__ zbuf,
                                                                  unsigned long long* __restrict__ words, int* __restrict__ bsum)
{
    __shared__ int s_tot[RS_THREADS / 64];
    const int a = blockIdx.y;
    const int64_t f = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    const int view = v.view_ids ? v.view_ids[a] : a;
    bool big = false;
    FaceSetup s;
    if ((unsigned)view < (unsigned)v.M && f < m.T && face_setup(m, v, view, f, s) && s.xs <= s.xe && s.ys <= s.ye) {
        big = s.xe - s.xs + 1 > RS_BIG || s.ye - s.ys + 1 > RS_BIG;
        if (!big) {
            const FaceEdges g = face_edges(s);
            int64_t r0 = edge_at(g.e0, s.xs, s.ys), r1 = edge_at(g.e1, s.xs, s.ys), r2 = edge_at(g.e2, s.xs, s.ys);
            for (int y = s.ys; y <= s.ye; ++y) {
                int64_t e0 = r0, e1 = r1, e2 = r2;
                const int64_t row = ((int64_t)a * v.H + y) * v.W;                         // inside the z-buffer: a < slots, 0 <= y < H, 0 <= x < W
                for (int x = s.xs; x <= s.xe; ++x) {
                    if (((e0 + g.e0.bias) | (e1 + g.e1.bias) | (e2 + g.e2.bias)) >= 0) {
                        float t[3], z;
                        if (fragment(s, e1, e2, v.z_min, t, z)) depth_test(zbuf, row + x, z, (unsigned)f);
                    }
                    e0 += g.e0.ax; e1 += g.e1.ax; e2 += g.e2.ax;
                }
                r0 += g.e0.ay; r1 += g.e1.ay; r2 += g.e2.ay;
            }
        }
    }
    const unsigned long long word = __ballot(big);
    const int64_t block = (int64_t)a * gridDim.x + blockIdx.x;
    if ((threadIdx.x & 63) == 0) words[block * 4 + (threadIdx.x >> 6)] = word;
    const int total = mvs_block_sum<RS_THREADS>(__popcll(word), s_tot);
    if (threadIdx.x == 0) bsum[block] = total;
}

// ONE workgroup: boff = the exclusive prefix of bsum, total[0] = the number of big items.  nb <= 2^22 and an item number is an int32: nb + 1024 and the
// grand total (<= 256 nb) fit in an int.
__global__ __launch_bounds__(RS_SCAN_THREADS) void raster_big_scan_kernel(const int* __restrict__ bsum, int nb, int* __restrict__ boff, int* __restrict__ total)
{
    __shared__ int s_tot[RS_SCAN_THREADS / 64];
    const int all = mvs_block_scan_runs<RS_SCAN_THREADS>(nb, [&](int i) { return bsum[i]; }, [&](int i, int pre) { boff[i] = pre; }, s_tot);
    if (threadIdx.x == 0) total[0] = all;
}

// list[boff[block] + rank] = block * 256 + thread for the big items, in item order
__global__ __launch_bounds__(RS_THREADS) void raster_big_list_kernel(const unsigned long long* __restrict__ words, const int* __restrict__ boff,
                                                                     int* __restrict__ list)
{
    __shared__ int s_pop[RS_THREADS / 64];
    const int w = threadIdx.x >> 6;
    const unsigned long long word = words[(int64_t)blockIdx.x * 4 + w];
    if ((threadIdx.x & 63) == 0) s_pop[w] = __popcll(word);
    __syncthreads();
    if ((word >> (threadIdx.x & 63)) & 1ull) list[boff[blockIdx.x] + mvs_tile_rank(s_pop, w, word)] = (int)blockIdx.x * RS_THREADS + (int)threadIdx.x;
}

// a workgroup per listed item, striding over the list; its threads stride over the item's box.  nbx: raster_faces_kernel's gridDim.x
__global__ __launch_bounds__(RS_THREADS) void raster_big_faces_kernel(RasterMesh m, RasterViews v, int nbx, const int* __restrict__ list,
                                                                      const int* __restrict__ total, unsigned long long* __restrict__ zbuf)
{
    const int n = total[0];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int item = list[i];
        const int block = item >> 8, a = block / nbx;
        const int64_t f = (int64_t)(block - a * nbx) * RS_THREADS + (item & (RS_THREADS - 1));
        const int view = v.view_ids ? v.view_ids[a] : a;                                  // inside [0, M): the item passed raster_faces_kernel's test
        FaceSetup s;
        if (!((unsigned)view < (unsigned)v.M && face_setup(m, v, view, f, s) && s.xs <= s.xe && s.ys <= s.ye)) continue;
        const FaceEdges g = face_edges(s);
        const int bw = s.xe - s.xs + 1, cells = bw * (s.ye - s.ys + 1);                   // <= 2^30
        for (int c = threadIdx.x; c < cells; c += RS_THREADS) {
            const int dy = c / bw, x = s.xs + (c - dy * bw), y = s.ys + dy;
            const int64_t e0 = edge_at(g.e0, x, y), e1 = edge_at(g.e1, x, y), e2 = edge_at(g.e2, x, y);
            if (((e0 + g.e0.bias) | (e1 + g.e1.bias) | (e2 + g.e2.bias)) < 0) continue;
            float t[3], z;
            if (fragment(s, e1, e2, v.z_min, t, z)) depth_test(zbuf, ((int64_t)a * v.H + y) * v.W + x, z, (unsigned)f);
        }
    }
}

__global__ __launch_bounds__(RS_THREADS) void raster_resolve_kernel(RasterMesh m, RasterViews v, const unsigned long long* __restrict__ zbuf, int64_t pixels,
                                                                    unsigned background, float* __restrict__ depth, int* __restrict__ face,
                                                                    unsigned char* __restrict__ colors)
{
    const int64_t p = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (p >= pixels) return;
    const unsigned long long key = zbuf[p];
    float z = 0.0f;
    int f = -1;
    unsigned char rgb[3] = {(unsigned char)(background & 255u), (unsigned char)((background >> 8) & 255u), (unsigned char)((background >> 16) & 255u)};
    if (key != RS_EMPTY) {
        int x, y, a;
        mvs_unflatten3(p, v.W, v.H, x, y, a);
        const int view = v.view_ids ? v.view_ids[a] : a;
        FaceSetup s;
        if ((unsigned)view < (unsigned)v.M && face_setup(m, v, view, (int64_t)(unsigned)key, s)) {      // the winner's setup: the very statements that made it
            z = __uint_as_float((unsigned)(key >> 32));
            f = (int)(unsigned)key;
            if (colors) {
                const FaceEdges g = face_edges(s);
                float t[3], zz;
                fragment(s, edge_at(g.e1, x, y), edge_at(g.e2, x, y), v.z_min, t, zz);    // zz has z's bits
                const unsigned char* ca = m.colors + (int64_t)s.ia * 3;
                const unsigned char* cb = m.colors + (int64_t)s.ib * 3;
                const unsigned char* cc = m.colors + (int64_t)s.ic * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float c = floorf(((t[0] * (float)ca[k] + t[1] * (float)cb[k]) + t[2] * (float)cc[k]) * z + 0.5f);
                    rgb[k] = (unsigned char)(int)fminf(fmaxf(c, 0.0f), 255.0f);
                }
            }
        }
    }
    depth[p] = z;
    face[p] = f;
    if (colors) { colors[p * 3 + 0] = rgb[0]; colors[p * 3 + 1] = rgb[1]; colors[p * 3 + 2] = rgb[2]; }
}

// ---- the views a face owns pixels in
__global__ __launch_bounds__(RS_THREADS) void mesh_face_views_kernel(const int* __restrict__ face, int64_t pixels, int H, int W, const int* __restrict__ view_ids,
                                                                     int M, int64_t n_faces, const int64_t* __restrict__ mesh_count, int words,
                                                                     unsigned* __restrict__ seen)
{
    const int64_t p = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (p >= pixels) return;
    int x, y, a;
    mvs_unflatten3(p, W, H, x, y, a);
    const int view = view_ids ? view_ids[a] : a;
    if ((unsigned)view >= (unsigned)M) return;
    int64_t T = n_faces;
    if (mesh_count) T = min(T, max(mesh_count[1], (int64_t)0));
    const int f = face[p];
    if (f < 0 || f >= T) return;
    if (x > 0 && face[p - 1] == f) return;                                                // the pixel to the left ORs the same bit
    atomicOr(seen + (int64_t)f * words + (view >> 5), 1u << (view & 31));                 // inside seen: f < n_faces, view < M <= 32 words
}

__global__ __launch_bounds__(RS_THREADS) void mesh_face_view_count_kernel(const unsigned* __restrict__ seen, int64_t n_faces, int words, int* __restrict__ n)
{
    const int64_t f = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (f >= n_faces) return;
    int c = 0;
    for (int k = 0; k < words; ++k) c += __popc(seen[f * words + k]);
    n[f] = c;
}

// ---- a mesh cut down to the faces of a mask
struct FilterMesh {
    const float* vertices;             // [V][3]
    const float* ndc;                  // [V][3] or NULL
    const int64_t* vertex_edge;        // [V] or NULL
    const unsigned char* colors;       // [V][3] or NULL
    const int* faces;                  // [T][3]
    const unsigned char* keep;         // [T]: non-zero = kept
    const int64_t* mesh_count;
    int64_t V, T;
};

// fkeep[f] = 1 for a kept face below the mesh's count whose three vertex numbers are inside the mesh; its vertices are marked used
__global__ __launch_bounds__(RS_THREADS) void filter_mark_kernel(FilterMesh m, unsigned char* __restrict__ used, unsigned char* __restrict__ fkeep)
{
    const int64_t f = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (f >= m.T) return;
    int64_t V = m.V, T = m.T;
    if (m.mesh_count) { V = min(V, max(m.mesh_count[0], (int64_t)0)); T = min(T, max(m.mesh_count[1], (int64_t)0)); }
    bool k = f < T && m.keep[f] != 0;
    if (k) {
        const int ia = m.faces[f * 3 + 0], ib = m.faces[f * 3 + 1], ic = m.faces[f * 3 + 2];
        k = ia >= 0 && ib >= 0 && ic >= 0 && ia < V && ib < V && ic < V;
        if (k) { used[ia] = 1; used[ib] = 1; used[ic] = 1; }                              // plain stores of one value: any order
    }
    fkeep[f] = k ? 1 : 0;
}

// bsum[b] = the set flags of workgroup b's 256 rows
__global__ __launch_bounds__(RS_THREADS) void filter_count_kernel(const unsigned char* __restrict__ flag, int64_t n, int* __restrict__ bsum)
{
    __shared__ int s_tot[RS_THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    const int c = i < n && flag[i] != 0;
    const int total = mvs_block_sum<RS_THREADS>(mvs_wave_sum_down(c), s_tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// ONE workgroup: boff = the exclusive prefix of bsum, *count = the total.  nb <= 2^23: nb + 1024 and the total (< 2^31 rows) fit in an int.
__global__ __launch_bounds__(RS_SCAN_THREADS) void filter_scan_kernel(const int* __restrict__ bsum, int nb, int* __restrict__ boff, int64_t* __restrict__ count)
{
    __shared__ int s_tot[RS_SCAN_THREADS / 64];
    const int all = mvs_block_scan_runs<RS_SCAN_THREADS>(nb, [&](int i) { return bsum[i]; }, [&](int i, int pre) { boff[i] = pre; }, s_tot);
    if (threadIdx.x == 0) count[0] = all;
}

// remap[v] = the new number of vertex v, -1 when no kept face uses it; the rows below cap are written
__global__ __launch_bounds__(RS_THREADS) void filter_vertices_kernel(FilterMesh m, const unsigned char* __restrict__ used, const int* __restrict__ boff,
                                                                     int64_t cap, int* __restrict__ remap, float* __restrict__ vertices,
                                                                     float* __restrict__ ndc, int64_t* __restrict__ vertex_edge,
                                                                     unsigned char* __restrict__ colors, int64_t* __restrict__ vertex_index)
{
    __shared__ int s_tot[RS_THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    const int flag = i < m.V && used[i] != 0;
    const int64_t row = (int64_t)boff[blockIdx.x] + mvs_block_exclusive<RS_THREADS>(flag, s_tot);
    if (i >= m.V) return;
    remap[i] = flag ? (int)row : -1;
    if (!flag || row >= cap) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        vertices[row * 3 + k] = m.vertices[i * 3 + k];
        if (m.ndc) ndc[row * 3 + k] = m.ndc[i * 3 + k];
        if (m.colors) colors[row * 3 + k] = m.colors[i * 3 + k];
    }
    if (m.vertex_edge) vertex_edge[row] = m.vertex_edge[i];
    vertex_index[row] = i;
}

__global__ __launch_bounds__(RS_THREADS) void filter_faces_kernel(FilterMesh m, const unsigned char* __restrict__ fkeep, const int* __restrict__ boff,
                                                                  const int* __restrict__ remap, int64_t cap, int* __restrict__ faces,
                                                                  int64_t* __restrict__ face_index)
{
    __shared__ int s_tot[RS_THREADS / 64];
    const int64_t f = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    const int flag = f < m.T && fkeep[f] != 0;
    const int64_t row = (int64_t)boff[blockIdx.x] + mvs_block_exclusive<RS_THREADS>(flag, s_tot);
    if (!flag || row >= cap) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) faces[row * 3 + k] = remap[m.faces[f * 3 + k]];            // a kept face's vertex numbers are inside the mesh and used
    face_index[row] = f;
}

inline bool rows_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }

// the shapes of the rasteriser: slots views of H x W pixels, nbx workgroups of faces per view
struct RasterShape {
    int slots, nbx;
    int64_t nb, pixels;
};
inline int raster_shape(int64_t n_faces, const int* view_ids, int n_views, int M, int H, int W, RasterShape* r)
{
    if (n_faces < 0 || M < 1 || H < 1 || W < 1 || (view_ids && n_views < 1)) return MVSNERF_EINVAL;
    const int slots = view_ids ? n_views : M;
    if (!rows_ok(n_faces) || slots > RS_MAX_VIEWS || M >= (1 << 22) || H > RS_MAX_IMAGE || W > RS_MAX_IMAGE) return MVSNERF_EUNSUPPORTED;
    r->slots = slots;
    r->nbx = (int)((n_faces + RS_THREADS - 1) / RS_THREADS);                              // <= 2^23
    r->nb = (int64_t)r->nbx * slots;
    r->pixels = (int64_t)slots * H * W;                                                   // < 2^46
    if (r->nb > RS_MAX_BLOCKS || (r->pixels + RS_THREADS - 1) / RS_THREADS >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    return MVSNERF_OK;
}

}  // namespace

// workspace: zbuf uint64 [slots H W] | words uint64 [4 nb] | bsum int32 [nb] | boff int32 [nb] | total int32 [2] | list int32 [256 nb]
extern "C" size_t mvsnerf_mesh_raster_workspace_bytes(int64_t n_faces, int n_views, int H, int W)
{
    RasterShape r;
    if (raster_shape(n_faces, nullptr, 0, n_views, H, W, &r) != MVSNERF_OK) return 0;
    return (size_t)r.pixels * 8 + (size_t)r.nb * (32 + 4 + 4 + 4 * RS_THREADS) + 8;
}

extern "C" int mvsnerf_mesh_raster_fwd(const float* vertices, int64_t n_vertices, const int* faces, int64_t n_faces, const unsigned char* colors,
                                       const int64_t* mesh_count, const float* w2c, const float* K, const int* view_ids, int n_views, int M, int H, int W,
                                       int cull, float z_min, unsigned background, float* depth, int* face, unsigned char* out_colors, void* workspace,
                                       void* stream)
{
    if (!w2c || !K || !depth || !face || !workspace || n_vertices < 0 || (n_vertices > 0 && !vertices) || (n_faces > 0 && !faces)) return MVSNERF_EINVAL;
    if ((colors != nullptr) != (out_colors != nullptr) || cull < -1 || cull > 1) return MVSNERF_EINVAL;
    RasterShape r;
    const int rc = raster_shape(n_faces, view_ids, n_views, M, H, W, &r);
    if (rc != MVSNERF_OK) return rc;
    if (!rows_ok(n_vertices) || !(isfinite(z_min) && z_min >= 0.0f)) return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(vertices, 4) || mvs_misaligned(faces, 4) || mvs_misaligned(mesh_count, 8) || mvs_misaligned(w2c, 4) || mvs_misaligned(K, 4) ||
        mvs_misaligned(view_ids, 4) || mvs_misaligned(depth, 4) || mvs_misaligned(face, 4) || mvs_misaligned(workspace, 8))
        return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* zbuf = static_cast<unsigned long long*>(workspace);
    unsigned long long* words = zbuf + r.pixels;
    int* bsum = reinterpret_cast<int*>(words + 4 * r.nb);
    int* boff = bsum + r.nb;
    int* total = boff + r.nb;
    int* list = total + 2;
    const RasterMesh m{vertices, faces, colors, mesh_count, n_vertices, n_faces};
    const RasterViews v{w2c, K, view_ids, r.slots, M, H, W, cull, z_min};
    hipError_t e = hipMemsetAsync(zbuf, 0xff, (size_t)r.pixels * 8, st);
    if (e != hipSuccess) return (int)e;
    if (r.nb > 0) {
        raster_faces_kernel<<<dim3((unsigned)r.nbx, (unsigned)r.slots), RS_THREADS, 0, st>>>(m, v, zbuf, words, bsum);
        MVS_LAUNCH_CHECK();
        raster_big_scan_kernel<<<1, RS_SCAN_THREADS, 0, st>>>(bsum, (int)r.nb, boff, total);
        MVS_LAUNCH_CHECK();
        raster_big_list_kernel<<<(unsigned)r.nb, RS_THREADS, 0, st>>>(words, boff, list);
        MVS_LAUNCH_CHECK();
        const int64_t items = r.nb * RS_THREADS;
        raster_big_faces_kernel<<<(unsigned)(items < RS_BIG_GRID ? items : RS_BIG_GRID), RS_THREADS, 0, st>>>(m, v, r.nbx, list, total, zbuf);
        MVS_LAUNCH_CHECK();
    }
    raster_resolve_kernel<<<mvs_cdiv(r.pixels, RS_THREADS), RS_THREADS, 0, st>>>(m, v, zbuf, r.pixels, background, depth, face, out_colors);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_mesh_face_views_fwd(const int* face, int n_maps, int H, int W, const int* view_ids, int M, int64_t n_faces, const int64_t* mesh_count,
                                           int* seen, int* n, void* stream)
{
    if (!face || n_maps < 1 || H < 1 || W < 1 || M < 1 || n_faces < 0 || (n_faces > 0 && (!seen || !n))) return MVSNERF_EINVAL;
    if (!view_ids && n_maps != M) return MVSNERF_EINVAL;
    const int64_t pixels = (int64_t)n_maps * H * W;
    if (!rows_ok(n_faces) || n_maps > RS_MAX_VIEWS || M >= (1 << 22) || H > RS_MAX_IMAGE || W > RS_MAX_IMAGE ||
        (pixels + RS_THREADS - 1) / RS_THREADS >= ((int64_t)1 << 31))
        return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(face, 4) || mvs_misaligned(view_ids, 4) || mvs_misaligned(mesh_count, 8) || mvs_misaligned(seen, 4) || mvs_misaligned(n, 4))
        return MVSNERF_EALIGN;
    if (n_faces == 0) return MVSNERF_OK;
    hipStream_t st = (hipStream_t)stream;
    const int words = (M + 31) / 32;
    hipError_t e = hipMemsetAsync(seen, 0, (size_t)n_faces * words * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    mesh_face_views_kernel<<<mvs_cdiv(pixels, RS_THREADS), RS_THREADS, 0, st>>>(face, pixels, H, W, view_ids, M, n_faces, mesh_count, words,
                                                                              reinterpret_cast<unsigned*>(seen));
    MVS_LAUNCH_CHECK();
    mesh_face_view_count_kernel<<<mvs_cdiv(n_faces, RS_THREADS), RS_THREADS, 0, st>>>(reinterpret_cast<const unsigned*>(seen), n_faces, words, n);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// workspace: remap int32 [V] | bsum, boff int32 [nbv] each | bsum, boff int32 [nbf] each | used uint8 [V] | fkeep uint8 [T]
extern "C" size_t mvsnerf_mesh_filter_workspace_bytes(int64_t n_vertices, int64_t n_faces)
{
    if (!rows_ok(n_vertices) || !rows_ok(n_faces)) return 0;
    const int64_t nbv = (n_vertices + RS_THREADS - 1) / RS_THREADS, nbf = (n_faces + RS_THREADS - 1) / RS_THREADS;
    return (size_t)(n_vertices + 2 * nbv + 2 * nbf) * sizeof(int) + (size_t)(n_vertices + n_faces) + 8;
}

extern "C" int mvsnerf_mesh_filter_fwd(const float* vertices, const float* ndc, const int64_t* vertex_edge, const unsigned char* colors, int64_t n_vertices,
                                       const int* faces, int64_t n_faces, const int64_t* mesh_count, const unsigned char* keep, int64_t cap_vertices,
                                       int64_t cap_faces, float* out_vertices, float* out_ndc, int64_t* out_vertex_edge, unsigned char* out_colors,
                                       int64_t* vertex_index, int* out_faces, int64_t* face_index, int64_t* count, void* workspace, void* stream)
{
    if (!count || !workspace || n_vertices < 0 || n_faces < 0 || cap_vertices < 0 || cap_faces < 0) return MVSNERF_EINVAL;
    if ((n_vertices > 0 && !vertices) || (n_faces > 0 && (!faces || !keep))) return MVSNERF_EINVAL;
    if (cap_vertices > 0 && (!out_vertices || !vertex_index || (ndc && !out_ndc) || (vertex_edge && !out_vertex_edge) || (colors && !out_colors))) return MVSNERF_EINVAL;
    if (cap_faces > 0 && (!out_faces || !face_index)) return MVSNERF_EINVAL;
    if (!rows_ok(n_vertices) || !rows_ok(n_faces) || !rows_ok(cap_vertices) || !rows_ok(cap_faces)) return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(vertices, 4) || mvs_misaligned(ndc, 4) || mvs_misaligned(vertex_edge, 8) || mvs_misaligned(faces, 4) || mvs_misaligned(mesh_count, 8) ||
        mvs_misaligned(out_vertices, 4) || mvs_misaligned(out_ndc, 4) || mvs_misaligned(out_vertex_edge, 8) || mvs_misaligned(vertex_index, 8) ||
        mvs_misaligned(out_faces, 4) || mvs_misaligned(face_index, 8) || mvs_misaligned(count, 8) || mvs_misaligned(workspace, 4))
        return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int nbv = (int)((n_vertices + RS_THREADS - 1) / RS_THREADS), nbf = (int)((n_faces + RS_THREADS - 1) / RS_THREADS);      // <= 2^23
    int* remap = static_cast<int*>(workspace);
    int* bsum_v = remap + n_vertices;
    int* boff_v = bsum_v + nbv;
    int* bsum_f = boff_v + nbv;
    int* boff_f = bsum_f + nbf;
    unsigned char* used = reinterpret_cast<unsigned char*>(boff_f + nbf);
    unsigned char* fkeep = used + n_vertices;
    const FilterMesh m{vertices, ndc, vertex_edge, colors, faces, keep, mesh_count, n_vertices, n_faces};
    if (n_vertices > 0) {
        hipError_t e = hipMemsetAsync(used, 0, (size_t)n_vertices, st);
        if (e != hipSuccess) return (int)e;
    }
    if (nbf > 0) {
        filter_mark_kernel<<<(unsigned)nbf, RS_THREADS, 0, st>>>(m, used, fkeep);
        MVS_LAUNCH_CHECK();
        filter_count_kernel<<<(unsigned)nbf, RS_THREADS, 0, st>>>(fkeep, n_faces, bsum_f);
        MVS_LAUNCH_CHECK();
    }
    if (nbv > 0) {
        filter_count_kernel<<<(unsigned)nbv, RS_THREADS, 0, st>>>(used, n_vertices, bsum_v);
        MVS_LAUNCH_CHECK();
    }
    filter_scan_kernel<<<1, RS_SCAN_THREADS, 0, st>>>(bsum_v, nbv, boff_v, count);
    MVS_LAUNCH_CHECK();
    filter_scan_kernel<<<1, RS_SCAN_THREADS, 0, st>>>(bsum_f, nbf, boff_f, count + 1);
    MVS_LAUNCH_CHECK();
    if (cap_vertices == 0 && cap_faces == 0) return MVSNERF_OK;                           // the counts alone: a caller sizing its outputs
    if (nbv > 0) {
        filter_vertices_kernel<<<(unsigned)nbv, RS_THREADS, 0, st>>>(m, used, boff_v, cap_vertices, remap, out_vertices, out_ndc, out_vertex_edge, out_colors,
                                                                    vertex_index);
        MVS_LAUNCH_CHECK();
    }
    if (nbf > 0 && cap_faces > 0) {
        filter_faces_kernel<<<(unsigned)nbf, RS_THREADS, 0, st>>>(m, fkeep, boff_f, remap, cap_faces, out_faces, face_index);
        MVS_LAUNCH_CHECK();
    }
    return MVSNERF_OK;
}
