// The depth maps of a scene's M views -> a coloured point cloud: the cross-view geometric-consistency filter of the MVSNet line of work
// (reproject every pixel into its source views and back, keep it where enough views agree, average the agreeing depths) and the stable compaction of the
// kept pixels.  No counterpart in the reference, which stops at depth maps.  Conventions are the bank's (scene_rays.hip, scene_ray_row): pixel centres at
// integer coordinates, camera direction ((x - cx) / fx, (y - cy) / fy, 1), a depth z the parameter of o + d z with that unnormalised d (camera-space z).
//
// depth_consistency_kernel   one thread per reference pixel, a workgroup inside ONE view r: r, its source ids and the cameras of the <= 33 views involved
//                      are workgroup-uniform (scalar loads, scalar registers); the four depth taps per source are the only irregular traffic.  A depth
//                      is INVALID when it is not finite, <= 0, masked by `valid`, or its pixel has alpha 0 in the bank; an invalid pixel gives
//                      seen = fused = mask = 0 and an invalid tap makes its pair inconsistent (a hole never bleeds into a neighbour).  Per source j:
//                      P = o_r + d_r z -> (u, v) in view s -> z_s bilinear at x0 = min(floor u, W - 2), y0 = min(floor v, H - 2) -> back through view s
//                      into view r as (x', y', z'); consistent iff z' > 0, |(x' - x, y' - y)| < pix_thr, |z' - z| / z < rel_thr.  seen bit j, fused =
//                      (z + sum z') / (1 + popcount), mask = popcount >= min_views.  Every output element is written; no LDS, no atomics.
//                      A source id outside [0, M) (-1 is the padding) or equal to r is skipped: no id makes the kernel read outside the inputs.
// cloud_count_kernel   a workgroup owns PC_TILE = 1024 consecutive pixels, four rounds of 256; each wave ballots its mask bytes and counts the bits, the
//                      four waves' counts meet in LDS -> one count per workgroup.
// cloud_scan_kernel    ONE workgroup: exclusive scan of the workgroup counts (scan_dev.h) and the total -> *count (int64).  One level: fewer than 2^21
//                      workgroup counts.
// cloud_write_kernel   ballots the mask bytes again; a kept pixel's slot is the workgroup's offset + the bits of the words in front of its own (through
//                      LDS) + mbcnt of its own word: slot order = flat-ray-index order (view-major, then row-major), the order of torch.nonzero, and every
//                      run gives the same bytes.  A slot >= capacity is not written.  (sparse.hip's live_* kernels are the pattern.)
#include "common.h"
#include "scan_dev.h"
#include <math.h>

namespace {

constexpr int DC_THREADS = 256;
constexpr int PC_THREADS = 256, PC_ROUNDS = 4, PC_TILE = PC_THREADS * PC_ROUNDS, PC_WORDS = PC_TILE / 64;
constexpr int PC_SCAN_THREADS = 256;

inline int64_t cloud_blocks(int64_t n) { return (n + PC_TILE - 1) / PC_TILE; }

struct FusionViews {
    const float* depth;                // [M][H][W]
    const unsigned char* valid;        // [M][H][W] or NULL
    const unsigned char* images;       // [M][H][W][4] or NULL (no alpha test)
    const float* c2w;                  // [M][3][4]
    const float* w2c;                  // [M][3][4]
    const float* K;                    // [M][3][3]
    int M, H, W;
};

// i: a flat pixel index inside the inputs
__device__ __forceinline__ bool depth_usable(const FusionViews& v, int64_t i, float& z)
{
    z = v.depth[i];
    bool ok = isfinite(z) && z > 0.0f;
    if (v.valid) ok = ok && v.valid[i] != 0;
    if (v.images) ok = ok && v.images[i * 4 + 3] != 0;
    return ok;
}

// pixel (px, py) at camera depth z of the view with pose c2w and intrinsics K -> world
__device__ __forceinline__ void lift(const float* __restrict__ c2w, const float* __restrict__ K, float px, float py, float z, float P[3])
{
    const float dx = (px - K[2]) / K[0], dy = (py - K[5]) / K[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float d = (dx * c2w[k * 4 + 0] + dy * c2w[k * 4 + 1]) + c2w[k * 4 + 2];
        P[k] = c2w[k * 4 + 3] + d * z;
    }
}

// world -> camera point q of the view with w2c; the image position is (fx q.x / q.z + cx, fy q.y / q.z + cy)
__device__ __forceinline__ void to_camera(const float* __restrict__ w2c, const float P[3], float q[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = ((w2c[k * 4 + 0] * P[0] + w2c[k * 4 + 1] * P[1]) + w2c[k * 4 + 2] * P[2]) + w2c[k * 4 + 3];
}

__global__ __launch_bounds__(DC_THREADS) void depth_consistency_kernel(FusionViews v, const int* __restrict__ src_ids, int n_src, int tiles, float pix_thr,
                                                                        float rel_thr, int min_views, unsigned* __restrict__ seen,
                                                                        float* __restrict__ fused, unsigned char* __restrict__ mask)
{
    const int r = (int)(blockIdx.x / (unsigned)tiles);                                  // workgroup-uniform: the view, its sources, their cameras
    const int64_t p = (int64_t)(blockIdx.x - (unsigned)r * (unsigned)tiles) * DC_THREADS + threadIdx.x;
    const int64_t HW = (int64_t)v.H * v.W;                                              // < 2^31
    if (p >= HW) return;
    const int y = (int)((unsigned)p / (unsigned)v.W), x = (int)((unsigned)p - (unsigned)y * (unsigned)v.W);
    const int64_t i = (int64_t)r * HW + p;
    float z;
    if (!depth_usable(v, i, z)) {
        seen[i] = 0u; fused[i] = 0.0f; mask[i] = 0;
        return;
    }
    const float* c2w_r = v.c2w + (int64_t)r * 12;
    const float* w2c_r = v.w2c + (int64_t)r * 12;
    const float* K_r = v.K + (int64_t)r * 9;
    float P[3];
    lift(c2w_r, K_r, (float)x, (float)y, z, P);
    unsigned bits = 0u;
    float sum = z;
    for (int j = 0; j < n_src; ++j) {
        const int s = src_ids[(int64_t)r * n_src + j];
        if ((unsigned)s >= (unsigned)v.M || s == r) continue;                           // -1 padding; nothing is read for an id outside the views
        const float* K_s = v.K + (int64_t)s * 9;
        float q[3];
        to_camera(v.w2c + (int64_t)s * 12, P, q);
        if (!(q[2] > 0.0f)) continue;
        const float u = K_s[0] * q[0] / q[2] + K_s[2], w = K_s[4] * q[1] / q[2] + K_s[5];
        if (!(u >= 0.0f && u <= (float)(v.W - 1) && w >= 0.0f && w <= (float)(v.H - 1))) continue;      // a NaN or an infinity fails here
        const int x0 = min((int)floorf(u), v.W - 2), y0 = min((int)floorf(w), v.H - 2);  // 0 <= x0 <= W - 2, 0 <= y0 <= H - 2: four taps inside view s
        const float ax = u - (float)x0, ay = w - (float)y0;
        const int64_t t = (int64_t)s * HW + (int64_t)y0 * v.W + x0;                     // t + W + 1 < (s + 1) HW
        float z00, z01, z10, z11;
        const bool ok = depth_usable(v, t, z00) & depth_usable(v, t + 1, z01) & depth_usable(v, t + v.W, z10) & depth_usable(v, t + v.W + 1, z11);
        if (!ok) continue;
        const float zs = (z00 * (1.0f - ax) + z01 * ax) * (1.0f - ay) + (z10 * (1.0f - ax) + z11 * ax) * ay;
        float Q[3], b[3];
        lift(v.c2w + (int64_t)s * 12, K_s, u, w, zs, Q);
        to_camera(w2c_r, Q, b);
        if (!(b[2] > 0.0f)) continue;
        const float ex = (K_r[0] * b[0] / b[2] + K_r[2]) - (float)x, ey = (K_r[4] * b[1] / b[2] + K_r[5]) - (float)y;
        if (sqrtf(ex * ex + ey * ey) < pix_thr && fabsf(b[2] - z) / z < rel_thr) {
            bits |= 1u << j;
            sum += b[2];
        }
    }
    const int n = __popc(bits);
    seen[i] = bits;
    fused[i] = sum / (float)(1 + n);
    mask[i] = n >= min_views ? 1 : 0;
}

__global__ __launch_bounds__(PC_THREADS) void cloud_count_kernel(const unsigned char* __restrict__ mask, int64_t n, int* __restrict__ counts)
{
    __shared__ int s_cnt[PC_THREADS / 64];
    int c = 0;                                                           // the wave's count, in every lane of it
#pragma unroll
    for (int r = 0; r < PC_ROUNDS; ++r) {
        const int64_t t = (int64_t)blockIdx.x * PC_TILE + r * PC_THREADS + threadIdx.x;
        const bool keep = t < n && mask[t] != 0;
        c += __popcll(__ballot(keep));
    }
    const int total = mvs_block_sum<PC_THREADS>(c, s_cnt);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_SCAN_THREADS) void cloud_scan_kernel(const int* __restrict__ counts, int nb, int* __restrict__ offsets,
                                                                     int64_t* __restrict__ count)
{
    __shared__ int s_tot[PC_SCAN_THREADS / 64];
    // nb <= 2^21, so the run arithmetic stays far inside 32 bits; the total is < 2^31 (one bit per pixel)
    const int total = mvs_block_scan_runs<PC_SCAN_THREADS>(nb, [&](int i) { return counts[i]; }, [&](int i, int pre) { offsets[i] = pre; }, s_tot);
    if (threadIdx.x == 0) *count = total;
}

__global__ __launch_bounds__(PC_THREADS) void cloud_write_kernel(FusionViews v, const float* __restrict__ fused, const unsigned* __restrict__ seen,
                                                                 const unsigned char* __restrict__ mask, int64_t n, const int* __restrict__ offsets,
                                                                 int64_t capacity, float* __restrict__ points, unsigned char* __restrict__ colors,
                                                                 unsigned char* __restrict__ n_views, int64_t* __restrict__ index)
{
    __shared__ int s_pop[PC_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long m[PC_ROUNDS];
#pragma unroll
    for (int r = 0; r < PC_ROUNDS; ++r) {
        const int64_t t = (int64_t)blockIdx.x * PC_TILE + r * PC_THREADS + threadIdx.x;
        m[r] = __ballot(t < n && mask[t] != 0);
        if (lane == 0) s_pop[r * (PC_THREADS / 64) + wave] = __popcll(m[r]);
    }
    __syncthreads();
    const int64_t base = offsets[blockIdx.x];
#pragma unroll
    for (int r = 0; r < PC_ROUNDS; ++r) {
        if (!((m[r] >> lane) & 1ull)) continue;
        const int w = r * (PC_THREADS / 64) + wave;
        const int64_t j = base + mvs_tile_rank(s_pop, w, m[r]);
        if (j < 0 || j >= capacity) continue;                            // the caller's rows and no others
        const int64_t t = (int64_t)blockIdx.x * PC_TILE + r * PC_THREADS + threadIdx.x;         // < n: the ballot sets no bit past the end
        int x, y, view;
        mvs_unflatten3(t, v.W, v.H, x, y, view);
        float P[3];
        lift(v.c2w + (int64_t)view * 12, v.K + (int64_t)view * 9, (float)x, (float)y, fused[t], P);
        points[j * 3 + 0] = P[0]; points[j * 3 + 1] = P[1]; points[j * 3 + 2] = P[2];
        const uchar4 c = reinterpret_cast<const uchar4*>(v.images)[t];
        colors[j * 3 + 0] = c.x; colors[j * 3 + 1] = c.y; colors[j * 3 + 2] = c.z;
        n_views[j] = (unsigned char)__popc(seen[t]);
        index[j] = t;
    }
}

// M, H, W of both entries: sizes < 1 are MVSNERF_EINVAL, H or W < 2 (no bilinear cell) and M H W >= 2^31 MVSNERF_EUNSUPPORTED
int fusion_sizes(int M, int H, int W, int64_t* n)
{
    if (M < 1 || H < 1 || W < 1) return MVSNERF_EINVAL;
    if (H < 2 || W < 2) return MVSNERF_EUNSUPPORTED;
    const int64_t HW = (int64_t)H * W;                                   // < 2^62
    if (HW >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    *n = (int64_t)M * HW;                                                // < 2^62
    if (*n >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    return MVSNERF_OK;
}

}  // namespace

extern "C" int mvsnerf_depth_consistency_fwd(const float* depth, const unsigned char* valid, const unsigned char* images_rgba, const float* c2w,
                                             const float* w2c, const float* K, const int* src_ids, int M, int H, int W, int n_src, float pix_thr,
                                             float rel_thr, int min_views, unsigned* seen, float* fused, unsigned char* mask, void* stream)
{
    if (!depth || !c2w || !w2c || !K || !src_ids || !seen || !fused || !mask) return MVSNERF_EINVAL;
    if (n_src < 1 || n_src > 32 || min_views < 0 || !(isfinite(pix_thr) && pix_thr > 0.0f) || !(isfinite(rel_thr) && rel_thr > 0.0f)) return MVSNERF_EINVAL;
    int64_t n;
    if (int rc = fusion_sizes(M, H, W, &n)) return rc;
    if (mvs_misaligned(depth, 4) || mvs_misaligned(images_rgba, 4) || mvs_misaligned(c2w, 4) || mvs_misaligned(w2c, 4) || mvs_misaligned(K, 4) || mvs_misaligned(src_ids, 4) ||
        mvs_misaligned(seen, 4) || mvs_misaligned(fused, 4))
        return MVSNERF_EALIGN;
    const int tiles = (int)(((int64_t)H * W + DC_THREADS - 1) / DC_THREADS);
    const FusionViews v{depth, valid, images_rgba, c2w, w2c, K, M, H, W};
    depth_consistency_kernel<<<(unsigned)((int64_t)M * tiles), DC_THREADS, 0, (hipStream_t)stream>>>(v, src_ids, n_src, tiles, pix_thr, rel_thr, min_views,
                                                                                                    seen, fused, mask);      // M tiles <= M H W < 2^31
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" size_t mvsnerf_point_cloud_workspace_bytes(int64_t n_pixels)
{
    if (n_pixels < 1 || n_pixels >= ((int64_t)1 << 31)) return 0;
    return (size_t)cloud_blocks(n_pixels) * 2 * sizeof(int);
}

extern "C" int mvsnerf_point_cloud_fwd(const unsigned char* images_rgba, const float* c2w, const float* K, int M, int H, int W, const float* fused,
                                       const unsigned* seen, const unsigned char* mask, int64_t capacity, float* points, unsigned char* colors,
                                       unsigned char* n_views, int64_t* index, int64_t* count, void* workspace, void* stream)
{
    if (!mask || !count || !workspace || capacity < 0) return MVSNERF_EINVAL;
    if (capacity > 0 && (!images_rgba || !c2w || !K || !fused || !seen || !points || !colors || !n_views || !index)) return MVSNERF_EINVAL;
    int64_t n;
    if (int rc = fusion_sizes(M, H, W, &n)) return rc;
    if (mvs_misaligned(images_rgba, 4) || mvs_misaligned(c2w, 4) || mvs_misaligned(K, 4) || mvs_misaligned(fused, 4) || mvs_misaligned(seen, 4) || mvs_misaligned(points, 4) ||
        mvs_misaligned(index, 8) || mvs_misaligned(count, 8) || mvs_misaligned(workspace, 4))
        return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = cloud_blocks(n);
    int* counts = static_cast<int*>(workspace);
    int* offsets = counts + nb;
    cloud_count_kernel<<<(unsigned)nb, PC_THREADS, 0, st>>>(mask, n, counts);
    MVS_LAUNCH_CHECK();
    cloud_scan_kernel<<<1, PC_SCAN_THREADS, 0, st>>>(counts, (int)nb, offsets, count);
    MVS_LAUNCH_CHECK();
    if (capacity == 0) return MVSNERF_OK;                                // the count alone: a caller sizing its outputs
    const FusionViews v{nullptr, nullptr, images_rgba, c2w, nullptr, K, M, H, W};
    cloud_write_kernel<<<(unsigned)nb, PC_THREADS, 0, st>>>(v, fused, seen, mask, n, offsets, capacity, points, colors, n_views, index);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
