// The depth maps of a scene's views -> a truncated signed distance volume (Curless-Levoy / KinectFusion) on a (D,H,W) grid of nodes over a world box, and
// the colours of a mesh's vertices from that volume.  No counterpart in the reference.  Conventions are the bank's (scene_rays.hip) and the
// mesher's (mesh.hip): node (i,j,k) = [k][j][i], flat index n = (k H + j) W + i, at X = lo + ((i,j,k) / (W-1, H-1, D-1)) * (hi - lo) - mesh.hip's box= mapping,
// operation for operation, so a mesh vertex and a TSDF node share one frame.
//
// tsdf_integrate_kernel   one thread per node, consecutive threads along W (neighbouring lanes tap neighbouring pixels); a workgroup owns a 32 x 4 x 2 brick
//                         of nodes, whose taps stay in a compact patch of every image, and skips a view whose frustum the brick's eight corners all miss on
//                         the same side (brick_misses; the verdict is a ballot, so the branch is wave-uniform).  The loop over the views runs inside the
//                         kernel and a view's 12 + 4 camera floats are read at wave-uniform addresses (scalar loads, scalar registers).  Per view m of
//                         the list, in the list's order, each step only if the one before held:
//                           1. q = w2c_m X (depth_fusion.hip's to_camera), q.z > z_min
//                           2. u = fx q.x / q.z + cx, v = fy q.y / q.z + cy; the NEAREST pixel x = floor(u + 0.5), y = floor(v + 0.5), with
//                              0 <= u + 0.5 < W_img and 0 <= v + 0.5 < H_img (a NaN fails here)
//                           3. d = depth[m][y][x] usable: finite, > 0, valid != 0, alpha != 0 (depth_fusion.hip's rule)
//                           4. sdf = d - q.z >= -trunc (further behind the surface: occluded, skipped)
//                           5. tsum += min(sdf / trunc, 1), wsum += 1
//                           6. if sdf <= trunc: csum[0:3] += images[m][y][x][0:3], cw += 1 (integers)
//                         tsdf = tsum / wsum (+1 where wsum == 0), weight = wsum, colors = ((2 csum + cw) / (2 cw), 255) or four zero bytes where cw == 0, in
//                         ONE 32-bit store.  A view id outside [0, M) is skipped and reads nothing.
// tsdf_vertex_colors_kernel   one thread per vertex row below min(count[0], rows): the two ends of the grid edge vertex_edge names (node * 8 + e, mesh.hip's
//                         owned edges), t = (0 - f0) / (f1 - f0) on f = -tsdf (0.5 when an end is not finite: the mesher's rule), byte = clamp(floor(c0 +
//                         t (c1 - c0) + 0.5), 0, 255) per channel; one end with a colour (alpha 255): that end's; neither, or a key outside the grid: 0.
// No atomics, no LDS: two runs give the same bytes.  Arithmetic: fp32, every operation rounded on its own (no contraction), IEEE division.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int TS_THREADS = 256;
constexpr int64_t TS_MAX_NODES = (int64_t)1 << 27;       // the mesher's bound: the volume is made for it

struct TsdfViews {
    const float* depth;                // [M][H][W]
    const unsigned char* valid;        // [M][H][W] or NULL
    const uchar4* images;              // [M][H][W] RGBA
    const float* w2c;                  // [M][3][4]
    const float* K;                    // [M][3][3]
    const int* view_ids;               // [n_views] or NULL: every view, ascending
    int n_views, alpha, M, H, W;       // alpha: 1 = a pixel with alpha 0 is a hole
};

struct TsdfGrid {
    int D, H, W, N;                    // N = D H W <= 2^27
    float lo[3], size[3];              // size = hi - lo
    float trunc, z_min;
};

struct TsdfSums {
    float tsum;
    int wsum, csum[3], cw;
};

__device__ __forceinline__ void node_position(const TsdfGrid& g, int i, int j, int k, float X[3])
{
    const float nx = (float)i / (float)(g.W - 1), ny = (float)j / (float)(g.H - 1), nz = (float)k / (float)(g.D - 1);
    X[0] = g.lo[0] + nx * g.size[0]; X[1] = g.lo[1] + ny * g.size[1]; X[2] = g.lo[2] + nz * g.size[2];
}

__device__ __forceinline__ void to_camera(const float* __restrict__ w2c, const float P[3], float q[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = ((w2c[k * 4 + 0] * P[0] + w2c[k * 4 + 1] * P[1]) + w2c[k * 4 + 2] * P[2]) + w2c[k * 4 + 3];
}

// steps 1..6 of view m (inside [0, M)) for the node at X
__device__ __forceinline__ void integrate_view(const TsdfViews& v, const TsdfGrid& g, int m, const float X[3], TsdfSums& s)
{
    const float* K = v.K + (int64_t)m * 9;
    float q[3];
    to_camera(v.w2c + (int64_t)m * 12, X, q);
    if (!(q[2] > g.z_min)) return;
    const float up = (K[0] * q[0] / q[2] + K[2]) + 0.5f, vp = (K[4] * q[1] / q[2] + K[5]) + 0.5f;
    if (!(up >= 0.0f && up < (float)v.W && vp >= 0.0f && vp < (float)v.H)) return;     // a NaN or an infinity fails here
    const int x = (int)floorf(up), y = (int)floorf(vp);                                // 0 <= x <= W - 1, 0 <= y <= H - 1: W, H <= 2^24 are exact floats
    const int64_t t = ((int64_t)m * v.H + y) * v.W + x;                                // inside the inputs
    const float d = v.depth[t];
    bool ok = isfinite(d) && d > 0.0f;
    if (v.valid) ok = ok && v.valid[t] != 0;
    uchar4 c = make_uchar4(0, 0, 0, 255);
    if (ok) c = v.images[t];
    if (v.alpha) ok = ok && c.w != 0;
    if (!ok) return;
    const float sdf = d - q[2];
    if (!(sdf >= -g.trunc)) return;
    s.tsum += fminf(sdf / g.trunc, 1.0f);
    s.wsum += 1;
    if (sdf <= g.trunc) {
        s.csum[0] += c.x; s.csum[1] += c.y; s.csum[2] += c.z;
        s.cw += 1;
    }
}

__device__ __forceinline__ void store_node(const TsdfSums& s, int n, float* __restrict__ tsdf, int* __restrict__ weight, unsigned* __restrict__ colors)
{
    tsdf[n] = s.wsum ? s.tsum / (float)s.wsum : 1.0f;
    weight[n] = s.wsum;
    unsigned word = 0u;
    if (s.cw) {
        const unsigned den = 2u * (unsigned)s.cw;                                      // 2 csum + cw <= 511 n_views < 2^31: the entry takes fewer than 2^22 views
        word = (2u * (unsigned)s.csum[0] + (unsigned)s.cw) / den | ((2u * (unsigned)s.csum[1] + (unsigned)s.cw) / den) << 8 |
               ((2u * (unsigned)s.csum[2] + (unsigned)s.cw) / den) << 16 | 0xff000000u;
    }
    colors[n] = word;                                                                  // R | G << 8 | B << 16 | A << 24: the bytes R G B A
}

constexpr int TS_BW = 32, TS_BH = 4, TS_BD = 2;           // a workgroup's brick of nodes: 32 along W, so half a wave shares a row; 32 x 4 x 2 = TS_THREADS

// true when no node of the brick [i0,i1] x [j0,j1] x [k0,k1] can pass steps 1 and 2 of view m: its eight corners all lie behind z_min, or all on the outer
// side of ONE border of the image, stated as a half space through the camera centre (fx q.x + (cx + 0.5) q.z < 0 is u + 0.5 < 0 for q.z > 0), which is
// convex, so it holds for every node between the corners.  tau keeps fp32 rounding from deciding: 1e-4 of the magnitude of the terms of q (a thousand
// roundings), so a node that the exact test excludes by that much is excluded by the kernel's own fp32 arithmetic too.  A NaN culls nothing.
__device__ __forceinline__ bool brick_misses(const TsdfViews& v, const TsdfGrid& g, int m, int i0, int i1, int j0, int j1, int k0, int k1)
{
    const float* w = v.w2c + (int64_t)m * 12;
    const float* K = v.K + (int64_t)m * 9;
    float q[8][3], s = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float X[3];
        node_position(g, (c & 1) ? i1 : i0, (c & 2) ? j1 : j0, (c & 4) ? k1 : k0, X);
        to_camera(w, X, q[c]);
        float mag = 0.0f;
#pragma unroll
        for (int r = 0; r < 3; ++r) mag += fabsf(w[r * 4 + 0] * X[0]) + fabsf(w[r * 4 + 1] * X[1]) + fabsf(w[r * 4 + 2] * X[2]) + fabsf(w[r * 4 + 3]);
        s = fmaxf(s, mag);
    }
    const float tau = 1e-4f * s;
    const float tx = tau * (fabsf(K[0]) + fabsf(K[2]) + (float)v.W + 1.0f), ty = tau * (fabsf(K[4]) + fabsf(K[5]) + (float)v.H + 1.0f);
    bool behind = true, left = true, right = true, above = true, below = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float ax = K[0] * q[c][0], ay = K[4] * q[c][1], z = q[c][2];
        behind = behind && z < g.z_min - tau;
        left = left && ax + (K[2] + 0.5f) * z < -tx;
        right = right && ax + (K[2] + 0.5f - (float)v.W) * z > tx;
        above = above && ay + (K[5] + 0.5f) * z < -ty;
        below = below && ay + (K[5] + 0.5f - (float)v.H) * z > ty;
    }
    return behind || left || right || above || below;
}

// A workgroup owns a 32 x 4 x 2 brick of nodes (bricks (bx, by, .)) and skips a view whose frustum its brick misses; 64 views are tested at once, one per
// lane, and the ballot of the survivors drives the wave-uniform loop over the views, ascending.
__global__ __launch_bounds__(TS_THREADS) void tsdf_integrate_kernel(TsdfViews v, TsdfGrid g, int bx, int by, float* __restrict__ tsdf,
                                                                    int* __restrict__ weight, unsigned* __restrict__ colors)
{
    int bi, bj, bk;
    mvs_unflatten3(blockIdx.x, bx, by, bi, bj, bk);
    const int i0 = bi * TS_BW, j0 = bj * TS_BH, k0 = bk * TS_BD;
    const int i1 = min(i0 + TS_BW, g.W) - 1, j1 = min(j0 + TS_BH, g.H) - 1, k1 = min(k0 + TS_BD, g.D) - 1;
    const int i = i0 + (threadIdx.x & (TS_BW - 1)), j = j0 + ((threadIdx.x / TS_BW) & (TS_BH - 1)), k = k0 + threadIdx.x / (TS_BW * TS_BH);
    const bool in_grid = i <= i1 && j <= j1 && k <= k1;                                 // (a lane outside the grid still votes below)
    const int lane = threadIdx.x & 63;
    float X[3];
    node_position(g, i, j, k, X);
    TsdfSums s{0.0f, 0, {0, 0, 0}, 0};
    for (int a0 = 0; a0 < v.n_views; a0 += 64) {
        bool live = false;
        if (a0 + lane < v.n_views) {
            const int m = v.view_ids ? v.view_ids[a0 + lane] : a0 + lane;
            live = (unsigned)m < (unsigned)v.M && !brick_misses(v, g, m, i0, i1, j0, j1, k0, k1);
        }
        unsigned long long todo = __ballot(live);                                       // wave-uniform: the views this brick can see
        while (todo) {
            const int a = a0 + __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int m = v.view_ids ? v.view_ids[a] : a;                               // a scalar load: inside [0, M), the ballot holds no other
            if (in_grid) integrate_view(v, g, m, X, s);
        }
    }
    if (in_grid) store_node(s, (k * g.H + j) * g.W + i, tsdf, weight, colors);          // < 2^27
}

__global__ __launch_bounds__(256) void tsdf_vertex_colors_kernel(const float* __restrict__ tsdf, const uchar4* __restrict__ node_colors, int D, int H, int W,
                                                                 const int64_t* __restrict__ vertex_edge, const int64_t* __restrict__ count, int64_t rows,
                                                                 unsigned char* __restrict__ colors)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t live = count[0] < rows ? count[0] : rows;
    if (r >= live) return;
    const int64_t key = vertex_edge[r];
    const int64_t N = (int64_t)D * H * W;
    const int e = (int)(key & 7);
    const int64_t n = key >> 3;
    unsigned char out[3] = {0, 0, 0};
    if (key >= 0 && n < N && e < 7) {
        int i, j, k;
        mvs_unflatten3(n, W, H, i, j, k);
        const int c = e == 0 ? 1 : e == 1 ? 2 : e == 2 ? 4 : e == 3 ? 3 : e == 4 ? 5 : e == 5 ? 6 : 7;       // mesh.hip's owned edges: dx | dy << 1 | dz << 2
        const int i1 = i + (c & 1), j1 = j + ((c >> 1) & 1), k1 = k + (c >> 2);
        if (i1 < W && j1 < H && k1 < D) {
            const int64_t up = ((int64_t)k1 * H + j1) * W + i1;
            const uchar4 c0 = node_colors[n], c1 = node_colors[up];
            const bool h0 = c0.w == 255, h1 = c1.w == 255;
            if (h0 && h1) {
                const float f0 = -tsdf[n], f1 = -tsdf[up];
                const float t = (isfinite(f0) && isfinite(f1)) ? (0.0f - f0) / (f1 - f0) : 0.5f;
                const unsigned char a[3] = {c0.x, c0.y, c0.z}, b[3] = {c1.x, c1.y, c1.z};
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float x = floorf(((float)a[q] + t * ((float)b[q] - (float)a[q])) + 0.5f);
                    out[q] = (unsigned char)(int)fminf(fmaxf(x, 0.0f), 255.0f);        // NaN -> 0
                }
            } else if (h0 || h1) {
                const uchar4 u = h0 ? c0 : c1;
                out[0] = u.x; out[1] = u.y; out[2] = u.z;
            }
        }
    }
    colors[r * 3 + 0] = out[0]; colors[r * 3 + 1] = out[1]; colors[r * 3 + 2] = out[2];
}

// D, H, W >= 2 and D H W <= 2^27
inline bool tsdf_nodes(int D, int H, int W, int64_t* n)
{
    if (D < 2 || H < 2 || W < 2) return false;
    const int64_t HW = (int64_t)H * W;                                   // < 2^62
    if (HW > TS_MAX_NODES) return false;
    *n = (int64_t)D * HW;                                                // < 2^58
    return *n <= TS_MAX_NODES;
}

}  // namespace

extern "C" int mvsnerf_tsdf_integrate_fwd(const float* depth, const unsigned char* valid, const unsigned char* images_rgba, int alpha, const float* w2c,
                                          const float* K, const int* view_ids, int n_views, int M, int H_img, int W_img, const float* box, int D, int H, int W,
                                          float trunc, float z_min, float* tsdf, int* weight, unsigned char* colors, void* stream)
{
    if (!depth || !images_rgba || !w2c || !K || !box || !tsdf || !weight || !colors) return MVSNERF_EINVAL;
    int64_t n;
    if (!tsdf_nodes(D, H, W, &n) || !(isfinite(trunc) && trunc > 0.0f) || !(isfinite(z_min) && z_min >= 0.0f)) return MVSNERF_EUNSUPPORTED;
    if (M < 1 || M >= (1 << 22) || H_img < 1 || W_img < 1 || H_img > (1 << 24) || W_img > (1 << 24) || (view_ids && (n_views < 1 || n_views >= (1 << 22)))) return MVSNERF_EUNSUPPORTED;
    for (int k = 0; k < 6; ++k)
        if (!isfinite(box[k])) return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(depth, 4) || mvs_misaligned(images_rgba, 4) || mvs_misaligned(w2c, 4) || mvs_misaligned(K, 4) || mvs_misaligned(view_ids, 4) || mvs_misaligned(tsdf, 4) ||
        mvs_misaligned(weight, 4) || mvs_misaligned(colors, 4))
        return MVSNERF_EALIGN;
    const TsdfViews v{depth, valid, reinterpret_cast<const uchar4*>(images_rgba), w2c, K, view_ids, view_ids ? n_views : M, alpha ? 1 : 0, M, H_img, W_img};
    TsdfGrid g{D, H, W, (int)n, {box[0], box[1], box[2]}, {box[3] - box[0], box[4] - box[1], box[5] - box[2]}, trunc, z_min};
    const int bx = (int)mvs_cdiv(W, TS_BW), by = (int)mvs_cdiv(H, TS_BH), bz = (int)mvs_cdiv(D, TS_BD);        // at most one brick per node: <= 2^27
    tsdf_integrate_kernel<<<(unsigned)((int64_t)bx * by * bz), TS_THREADS, 0, (hipStream_t)stream>>>(v, g, bx, by, tsdf, weight,
                                                                                                  reinterpret_cast<unsigned*>(colors));
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_tsdf_vertex_colors_fwd(const float* tsdf, const unsigned char* node_colors, int D, int H, int W, const int64_t* vertex_edge,
                                              const int64_t* count, int64_t rows, unsigned char* colors, void* stream)
{
    if (!tsdf || !node_colors || !count || rows < 0 || (rows > 0 && (!vertex_edge || !colors))) return MVSNERF_EINVAL;
    int64_t n;
    if (!tsdf_nodes(D, H, W, &n) || rows >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    if (mvs_misaligned(tsdf, 4) || mvs_misaligned(node_colors, 4) || mvs_misaligned(vertex_edge, 8) || mvs_misaligned(count, 8)) return MVSNERF_EALIGN;
    if (rows == 0) return MVSNERF_OK;
    tsdf_vertex_colors_kernel<<<mvs_cdiv(rows, 256), 256, 0, (hipStream_t)stream>>>(tsdf, reinterpret_cast<const uchar4*>(node_colors), D, H, W, vertex_edge,
                                                                                   count, rows, colors);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
