// A (D,H,W) scalar field (a scene's node density) -> a triangle mesh of its level set: marching tetrahedra over the Kuhn (Freudenthal)
// split of every grid cell.  No counterpart in the reference.  Node (i,j,k) = field[k][j][i], flat index n = (k H + j) W + i, inside iff field >= level
// (a NaN is outside).  A node OWNS the up to 7 edges to the node at +(dx,dy,dz), e = 0..6: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1); an
// edge carries a vertex iff exactly one end is inside, at t = (level - s0) / (s1 - s0) from the owner (0.5 when an end is not finite); vertices are
// ordered by n * 8 + e.  A cell has 6 tetrahedra, one per permutation (a,b,c) of the axes in lexicographic order: v0 = origin, v1 = v0 + e_a,
// v2 = v1 + e_b, v3 = v2 + e_c; all 6 edges of a tetrahedron are owned edges of v0, v1 or v2.  Faces are ordered by cell, tetrahedron, triangle.
//
// mesh_classify_kernel   one thread per node: the 8 corners of its cell (neighbouring threads run along W) -> the 7-bit owned-edge mask (1 byte) and the
//                        workgroup's numbers of vertices (mask bits) and faces (0..12 per cell).
// mesh_scan_kernel       ONE workgroup of 1024: exclusive offsets of both arrays of workgroup counts and the two totals -> count[2] (int64): the scan
//                        of scan_dev.h with the vertex and the face count of a workgroup carried in the two halves of one 64-bit word - one pass for both.
// mesh_vertices_kernel   in-workgroup scan of the mask popcounts + the workgroup's offset -> vbase[node] (int32, every node); rows < capacity of
//                        vertices, ndc and vertex_edge.
// mesh_faces_kernel      (a launch of its own: it reads vbase and mask of nodes of other workgroups) in-workgroup scan of the cells' face counts + the
//                        offset; the case of each tetrahedron comes from MT_CASE; the vertex of edge e of node m is vbase[m] + popcount(mask[m] & ((1 << e) - 1)).
// mesh_dirs_kernel, mesh_rgb_u8_kernel   rows vertex - origin; bytes trunc(clamp(rgb, 0, 1) * 255) of the first three of four floats (frames.hip's rule).
// valid (optional, a byte per node, non-zero = valid): an owned edge carries a vertex only if both its ends are valid, a tetrahedron emits faces only if its
// four corners are valid.  The field is still read at invalid nodes; nothing that touches them survives.  The same as the unmasked extraction with every
// vertex on an edge with an invalid end and every face using such a vertex dropped, and the rest renumbered.
// No atomics: the order is what the scans produce, two runs give the same bytes.  Rows >= capacity are never written.
// Arithmetic: fp32, every operation rounded on its own (no contraction), IEEE division - what numpy does on float32 arrays.
#include "common.h"
#include "scan_dev.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int MT_THREADS = 256, MT_SCAN_THREADS = 1024;
constexpr int64_t MT_MAX_NODES = (int64_t)1 << 27;       // 7 vertices per node and 12 faces per cell stay inside int32

// The triangles of a POSITIVELY oriented tetrahedron (det(v1-v0, v2-v0, v3-v0) > 0: the permutations xyz, yzx, zxy) by its inside corners (bit c: corner
// v_c).  A nibble per triangle vertex, lowest first: the tetrahedron's edge 0..5 = v0v1 v0v2 v0v3 v1v2 v1v3 v2v3.  One inside (or outside) corner: the
// triangle on its three edges; two: the quad on the four edges between the pairs, split along the edge from the lower inside corner to the lower outside
// one.  The normal points to the outside corners.  A negatively oriented tetrahedron (xzy, yxz, zyx) swaps the second and third vertex of each triangle.
__constant__ unsigned MT_CASE[16] = {0x000000, 0x000210, 0x000340, 0x341421, 0x000531, 0x530250, 0x150540, 0x000542,
                                     0x000452, 0x450510, 0x520350, 0x000351, 0x241431, 0x000430, 0x000120, 0x000000};

// the owned edge towards the cell corner with code c = dx | dy << 1 | dz << 2 (c = 1..7)
__host__ __device__ constexpr int edge_of(int c) { return c == 1 ? 0 : c == 2 ? 1 : c == 4 ? 2 : c == 3 ? 3 : c == 5 ? 4 : c == 6 ? 5 : 6; }
// the axes (a, b, c) of tetrahedron p, lexicographic
__host__ __device__ constexpr int perm_axis(int p, int k)
{
    const int a = p >> 1;
    const int lo = a == 0 ? 1 : 0, hi = a == 2 ? 1 : 2;         // the two other axes, ascending
    const int b = (p & 1) ? hi : lo, c = (p & 1) ? lo : hi;
    return k == 0 ? a : k == 1 ? b : c;
}
__host__ __device__ constexpr bool perm_odd(int p) { return p == 1 || p == 2 || p == 5; }     // xzy, yxz, zyx
// corner code of v_k of tetrahedron p
__host__ __device__ constexpr int tet_corner(int p, int k)
{
    return k == 0 ? 0 : k == 1 ? (1 << perm_axis(p, 0)) : k == 2 ? ((1 << perm_axis(p, 0)) | (1 << perm_axis(p, 1))) : 7;
}
// edge l = 0..5 of tetrahedron p as (owner corner code) << 3 | owned edge
__host__ __device__ constexpr int tet_edge(int p, int l)
{
    const int lo = l < 3 ? 0 : l < 5 ? 1 : 2, hi = l < 3 ? l + 1 : l < 5 ? l - 1 : 3;
    return (tet_corner(p, lo) << 3) | edge_of(tet_corner(p, hi) ^ tet_corner(p, lo));
}
// the six (owner, edge) codes of tetrahedron p, 6 bits each
__host__ __device__ constexpr uint64_t tet_edges(int p)
{
    uint64_t w = 0;
    for (int l = 0; l < 6; ++l) w |= (uint64_t)tet_edge(p, l) << (6 * l);
    return w;
}

struct MeshGrid {
    const float* field;                // [D][H][W]
    int D, H, W, HW, N;                // N = D H W <= 2^27
    float level;
    const unsigned char* valid;        // [D][H][W] or NULL: a node with a zero byte carries no vertex and no face (the mask)
};

__device__ __forceinline__ int corner_offset(const MeshGrid& g, int c) { return (c & 1) + ((c >> 1) & 1) * g.W + (c >> 2) * g.HW; }

// bits 0..7: corner c of the cell at node n is inside; bits 8..15: corner c is in the grid; bits 16..23: corner c is valid (every corner in the grid
// without a mask).  Reads nothing outside the field.
__device__ __forceinline__ unsigned cell_corners(const MeshGrid& g, int n, int i, int j, int k)
{
    const bool hx = i + 1 < g.W, hy = j + 1 < g.H, hz = k + 1 < g.D;
    unsigned bits = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const bool in_grid = (!(c & 1) || hx) && (!(c & 2) || hy) && (!(c & 4) || hz);
        if (in_grid) {
            const float s = g.field[n + corner_offset(g, c)];
            const unsigned ok = (!g.valid || g.valid[n + corner_offset(g, c)] != 0) ? 0x10000u : 0u;
            bits |= (ok | 0x100u | (s >= g.level ? 1u : 0u)) << c;
        }
    }
    return bits;
}

__device__ __forceinline__ unsigned owned_edges(unsigned corners)
{
    const unsigned own = corners & 1u;
    unsigned mask = 0u;
    if (!((corners >> 16) & 1u)) return mask;                            // an invalid owner
#pragma unroll
    for (int c = 1; c < 8; ++c)
        if (((corners >> (16 + c)) & 1u) && ((corners >> c) & 1u) != own) mask |= 1u << edge_of(c);     // (valid implies in the grid)
    return mask;
}

// 0 (no face) for a tetrahedron with an invalid corner: every triangle of every case touches all four corners
__device__ __forceinline__ unsigned tet_case(unsigned corners, int p)
{
    const unsigned need = 0x10000u | (0x10000u << tet_corner(p, 1)) | (0x10000u << tet_corner(p, 2)) | 0x800000u;
    if ((corners & need) != need) return 0u;
    return (corners & 1u) | (((corners >> tet_corner(p, 1)) & 1u) << 1) | (((corners >> tet_corner(p, 2)) & 1u) << 2) | (((corners >> 7) & 1u) << 3);
}
__device__ __forceinline__ int case_triangles(unsigned cs)
{
    const int pc = __popc(cs);
    return (pc & 3) ? (pc == 2 ? 2 : 1) : 0;
}
// faces of the cell: 0 when the cell is not whole (its far corner is outside the grid)
__device__ __forceinline__ int cell_faces(unsigned corners)
{
    if (!((corners >> 15) & 1u)) return 0;
    int f = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p) f += case_triangles(tet_case(corners, p));
    return f;
}

__global__ __launch_bounds__(MT_THREADS) void mesh_classify_kernel(MeshGrid g, unsigned char* __restrict__ mask, int* __restrict__ vcount,
                                                                   int* __restrict__ fcount)
{
    __shared__ int s_v[MT_THREADS / 64], s_f[MT_THREADS / 64];
    const int n = blockIdx.x * MT_THREADS + threadIdx.x;                 // < 2^27 + 256
    int nv = 0, nf = 0;
    if (n < g.N) {
        int i, j, k;
        mvs_unflatten3(n, g.W, g.H, i, j, k);
        const unsigned corners = cell_corners(g, n, i, j, k);
        const unsigned m = owned_edges(corners);
        mask[n] = (unsigned char)m;
        nv = __popc(m);
        nf = cell_faces(corners);
    }
    nv = mvs_wave_sum_down(nv);
    nf = mvs_wave_sum_down(nf);
    if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = nf;
    nv = mvs_block_sum<MT_THREADS>(nv, s_v);                             // (its barrier covers s_f too)
    if (threadIdx.x == 0) {
        vcount[blockIdx.x] = nv;
        fcount[blockIdx.x] = mvs_waves_total<MT_THREADS>(s_f);
    }
}

// counts = [vcount[nb] | fcount[nb]], offsets = [voffset[nb] | foffset[nb]]
__global__ __launch_bounds__(MT_SCAN_THREADS) void mesh_scan_kernel(const int* __restrict__ counts, int nb, int* __restrict__ offsets,
                                                                    int64_t* __restrict__ count)
{
    typedef unsigned long long u64;
    __shared__ u64 s_tot[MT_SCAN_THREADS / 64];
    // both sums in one word, faces above vertices: the vertex total is < 7 * 2^27 < 2^32, so nothing carries over, and the face total < 12 * 2^27 < 2^31.
    // nb <= 2^19, so the run arithmetic stays below 2^19 + 2^10
    const u64 total = mvs_block_scan_runs<MT_SCAN_THREADS>(
        nb, [&](int i) { return (u64)(unsigned)counts[i] | ((u64)(unsigned)counts[nb + i] << 32); },
        [&](int i, u64 pre) { offsets[i] = (int)(unsigned)pre; offsets[nb + i] = (int)(unsigned)(pre >> 32); }, s_tot);
    if (threadIdx.x == 0) {
        count[0] = (int64_t)(total & 0xffffffffull);
        count[1] = (int64_t)(total >> 32);
    }
}

struct MeshMap {
    const float* positions;            // [D][H][W][3] or NULL
    int box;                           // 1: lo + ndc * size
    float lo[3], size[3];
};

__global__ __launch_bounds__(MT_THREADS) void mesh_vertices_kernel(MeshGrid g, MeshMap map, const unsigned char* __restrict__ mask,
                                                                   const int* __restrict__ voffset, int64_t capacity, int* __restrict__ vbase,
                                                                   float* __restrict__ vertices, float* __restrict__ ndc,
                                                                   int64_t* __restrict__ vertex_edge)
{
    __shared__ int s_tot[MT_THREADS / 64];
    const int n = blockIdx.x * MT_THREADS + threadIdx.x;
    const unsigned m = n < g.N ? mask[n] : 0u;
    const int base = voffset[blockIdx.x] + mvs_block_exclusive<MT_THREADS>((int)__popc(m), s_tot);
    if (n >= g.N) return;
    vbase[n] = base;
    if (!m || base >= capacity) return;
    int i, j, k;
    mvs_unflatten3(n, g.W, g.H, i, j, k);
    const float s0 = g.field[n];
    const float fi = (float)i, fj = (float)j, fk = (float)k;
    const float wx = (float)(g.W - 1), wy = (float)(g.H - 1), wz = (float)(g.D - 1);
    int64_t row = base;
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        if (!((m >> e) & 1u)) continue;
        if (row >= capacity) return;                                     // the caller's rows and no others
        const int c = e == 0 ? 1 : e == 1 ? 2 : e == 2 ? 4 : e == 3 ? 3 : e == 4 ? 5 : e == 5 ? 6 : 7;      // edge_of(c) == e
        const int up = n + corner_offset(g, c);                          // in the grid: the mask has no bit for an edge that leaves it
        const float s1 = g.field[up];
        const float t = (isfinite(s0) && isfinite(s1)) ? (g.level - s0) / (s1 - s0) : 0.5f;
        const float gx = (c & 1) ? fi + t : fi, gy = (c & 2) ? fj + t : fj, gz = (c & 4) ? fk + t : fk;
        const float nx = gx / wx, ny = gy / wy, nz = gz / wz;
        float x = gx, y = gy, z = gz;
        if (map.box) {
            x = map.lo[0] + nx * map.size[0]; y = map.lo[1] + ny * map.size[1]; z = map.lo[2] + nz * map.size[2];
        } else if (map.positions) {
            const float* p0 = map.positions + (int64_t)n * 3;
            const float* p1 = map.positions + (int64_t)up * 3;
            x = p0[0] + t * (p1[0] - p0[0]); y = p0[1] + t * (p1[1] - p0[1]); z = p0[2] + t * (p1[2] - p0[2]);
        }
        vertices[row * 3 + 0] = x; vertices[row * 3 + 1] = y; vertices[row * 3 + 2] = z;
        ndc[row * 3 + 0] = nx; ndc[row * 3 + 1] = ny; ndc[row * 3 + 2] = nz;
        vertex_edge[row] = (int64_t)n * 8 + e;
        ++row;
    }
}

__global__ __launch_bounds__(MT_THREADS) void mesh_faces_kernel(MeshGrid g, const unsigned char* __restrict__ mask, const int* __restrict__ vbase,
                                                                const int* __restrict__ foffset, int64_t capacity, int* __restrict__ faces)
{
    __shared__ int s_tot[MT_THREADS / 64];
    const int n = blockIdx.x * MT_THREADS + threadIdx.x;
    unsigned corners = 0u;
    if (n < g.N) {
        int i, j, k;
        mvs_unflatten3(n, g.W, g.H, i, j, k);
        corners = cell_corners(g, n, i, j, k);
    }
    const int nf = cell_faces(corners);
    const int base = foffset[blockIdx.x] + mvs_block_exclusive<MT_THREADS>(nf, s_tot);
    if (!nf || base >= capacity) return;
    int64_t row = base;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const unsigned cs = tet_case(corners, p);
        const int nt = case_triangles(cs);
        if (!nt) continue;
        const unsigned code = MT_CASE[cs];
        const uint64_t edges = tet_edges(p);                             // a constant once the loop is unrolled
        for (int tri = 0; tri < nt; ++tri) {
            if (row >= capacity) return;                                 // the caller's rows and no others
            int v[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int l = (int)(code >> (4 * (3 * tri + q))) & 7;    // 0..5: MT_CASE holds no other value in a used nibble
                const int oe = (int)(edges >> (6 * l)) & 63;
                const int m = n + corner_offset(g, oe >> 3);             // a corner of a whole cell: in the grid
                v[q] = vbase[m] + __popc((unsigned)mask[m] & ((1u << (oe & 7)) - 1u));
            }
            faces[row * 3 + 0] = v[0];
            faces[row * 3 + 1] = perm_odd(p) ? v[2] : v[1];
            faces[row * 3 + 2] = perm_odd(p) ? v[1] : v[2];
            ++row;
        }
    }
}

__global__ __launch_bounds__(256) void mesh_dirs_kernel(const float* __restrict__ vertices, const float* __restrict__ origin, int64_t n3,
                                                        float* __restrict__ dirs)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n3) return;
    dirs[t] = vertices[t] - origin[t % 3];
}

__global__ __launch_bounds__(256) void mesh_rgb_u8_kernel(const float* __restrict__ rgba, int64_t n, unsigned char* __restrict__ rgb)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const float4 c = reinterpret_cast<const float4*>(rgba)[t];
    const float v[3] = {c.x, c.y, c.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[t * 3 + k] = (unsigned char)(int)(fminf(fmaxf(v[k], 0.f), 1.f) * 255.f);      // NaN -> 0
}

inline int64_t mesh_blocks(int64_t n) { return (n + MT_THREADS - 1) / MT_THREADS; }

// D, H, W >= 2 and D H W <= 2^27
inline bool mesh_nodes(int D, int H, int W, int64_t* n)
{
    if (D < 2 || H < 2 || W < 2) return false;
    const int64_t HW = (int64_t)H * W;                                   // < 2^62
    if (HW > MT_MAX_NODES) return false;
    *n = (int64_t)D * HW;                                                // < 2^58
    return *n <= MT_MAX_NODES;
}

}  // namespace

// workspace: vbase int32 [N] | vcount, fcount, voffset, foffset int32 [nb] each | mask uint8 [N]
extern "C" size_t mvsnerf_mesh_workspace_bytes(int D, int H, int W)
{
    int64_t n;
    if (!mesh_nodes(D, H, W, &n)) return 0;
    return (size_t)n * 5 + (size_t)mesh_blocks(n) * 4 * sizeof(int);
}

extern "C" int mvsnerf_mesh_extract_masked_fwd(const float* field, const unsigned char* valid, int D, int H, int W, float level, const float* positions,
                                               const float* box, int64_t cap_vertices, int64_t cap_faces, float* vertices, float* ndc, int64_t* vertex_edge,
                                               int* faces, int64_t* count, void* workspace, void* stream)
{
    if (!field || !count || !workspace || cap_vertices < 0 || cap_faces < 0) return MVSNERF_EINVAL;
    if (cap_vertices > 0 && (!vertices || !ndc || !vertex_edge)) return MVSNERF_EINVAL;
    if (cap_faces > 0 && !faces) return MVSNERF_EINVAL;
    int64_t n;
    if (!mesh_nodes(D, H, W, &n) || !isfinite(level) || (positions && box)) return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(field, 4) || mvs_misaligned(positions, 4) || mvs_misaligned(vertices, 4) || mvs_misaligned(ndc, 4) || mvs_misaligned(vertex_edge, 8) ||
        mvs_misaligned(faces, 4) || mvs_misaligned(count, 8) || mvs_misaligned(workspace, 4))
        return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = mesh_blocks(n);                                   // <= 2^19
    int* vbase = static_cast<int*>(workspace);
    int* counts = vbase + n;                                             // vcount | fcount
    int* offsets = counts + 2 * nb;                                      // voffset | foffset
    unsigned char* mask = reinterpret_cast<unsigned char*>(offsets + 2 * nb);
    const MeshGrid g{field, D, H, W, H * W, (int)n, level, valid};
    mesh_classify_kernel<<<(unsigned)nb, MT_THREADS, 0, st>>>(g, mask, counts, counts + nb);
    MVS_LAUNCH_CHECK();
    mesh_scan_kernel<<<1, MT_SCAN_THREADS, 0, st>>>(counts, (int)nb, offsets, count);
    MVS_LAUNCH_CHECK();
    if (cap_vertices == 0 && cap_faces == 0) return MVSNERF_OK;          // the counts alone: a caller sizing its outputs
    MeshMap map{positions, box ? 1 : 0, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    if (box)
        for (int k = 0; k < 3; ++k) { map.lo[k] = box[k]; map.size[k] = box[3 + k] - box[k]; }
    mesh_vertices_kernel<<<(unsigned)nb, MT_THREADS, 0, st>>>(g, map, mask, offsets, cap_vertices, vbase, vertices, ndc, vertex_edge);   // (vbase: the faces need it)
    MVS_LAUNCH_CHECK();
    if (cap_faces == 0) return MVSNERF_OK;
    mesh_faces_kernel<<<(unsigned)nb, MT_THREADS, 0, st>>>(g, mask, vbase, offsets + nb, cap_faces, faces);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_mesh_extract_fwd(const float* field, int D, int H, int W, float level, const float* positions, const float* box,
                                        int64_t cap_vertices, int64_t cap_faces, float* vertices, float* ndc, int64_t* vertex_edge, int* faces,
                                        int64_t* count, void* workspace, void* stream)
{
    return mvsnerf_mesh_extract_masked_fwd(field, nullptr, D, H, W, level, positions, box, cap_vertices, cap_faces, vertices, ndc, vertex_edge, faces, count,
                                           workspace, stream);
}

extern "C" int mvsnerf_mesh_dirs_fwd(const float* vertices, const float* origin, int64_t n, float* dirs, void* stream)
{
    if (n < 0 || !origin || (n > 0 && (!vertices || !dirs))) return MVSNERF_EINVAL;
    if (n >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(vertices, 4) || mvs_misaligned(origin, 4) || mvs_misaligned(dirs, 4)) return MVSNERF_EALIGN;
    if (n == 0) return MVSNERF_OK;
    mesh_dirs_kernel<<<mvs_cdiv(n * 3, 256), 256, 0, (hipStream_t)stream>>>(vertices, origin, n * 3, dirs);      // < 2^25 workgroups
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_mesh_rgb_u8_fwd(const float* rgba, int64_t n, unsigned char* rgb, void* stream)
{
    if (n < 0 || (n > 0 && (!rgba || !rgb))) return MVSNERF_EINVAL;
    if (n >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(rgba, 16)) return MVSNERF_EALIGN;
    if (n == 0) return MVSNERF_OK;
    mesh_rgb_u8_kernel<<<mvs_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(rgba, n, rgb);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
