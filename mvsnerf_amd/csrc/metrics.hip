// Evaluation record of K finished frames (the protocol of the reference's renderer.ipynb, cells 8 and 16; mvsnerf_amd/evaluate.py states it on the host):
// squared-error sums over all pixels / the centre crop / the DTU mask, the SSIM sum per channel over the valid region
// (skimage 0.19 structural_similarity defaults: uniform window, sample covariance) and the depth errors, one row of MVSNERF_METRICS_ROW doubles per frame.
//
// frame_metrics_tile_kernel   one workgroup per (frame, 16 x 32 tile of window origins).  It stages rows ty0 .. ty0 + 16 + WIN - 2 and columns
//                             tx0 .. tx0 + 32 + WIN - 2 of both images (HWC, as they lie in memory) in LDS, then per channel:
//                               rows     for every staged row and window origin: sum and CENTRED second moments of the WIN values to its right
//                               columns  WIN such row records combine into the window's mean and centred moments (the pairwise update of
//                                        Chan et al.: M2 = sum_r m2_r + WIN * sum_r (mean_r - mean)^2), the SSIM value is formed in registers
//                             Every value has the tile's first pixel subtracted on the way out of LDS, so a constant image gives sums, moments and
//                             variances of exactly 0; the moments are never a difference of raw fp32 sums.  The tile's own 16 x 32 pixels give the
//                             squared-error and depth sums (fp32 per pixel and channel, double from there on).  Reduction: shuffle tree per wave, the
//                             four waves in order; one partial row per tile.  No atomics.
// frame_metrics_sum_kernel    one workgroup per frame: entry e of the row = the tiles' entries, lane l of 16 taking tiles l, l + 16, ... in order,
//                             then a fixed shuffle tree over the 16 lanes, all in double.  The order depends on H, W and WIN only: frame k of a batch has
//                             the bits of the same frame alone.
#include "common.h"
#include "scan_dev.h"

#pragma clang fp contract(off)      // pred == gt must give bit-equal x / y / xy moments and a quotient of exactly 1: every fused product below is an explicit fmaf

namespace {

constexpr int MT_H = 16, MT_W = 32, MT_THREADS = 256;
constexpr int ROW = MVSNERF_METRICS_ROW;
// row entries
enum { R_SSE = 0, R_N, R_SSE_CROP, R_N_CROP, R_SSE_MASK, R_N_MASK, R_SSIM0, R_SSIM1, R_SSIM2, R_N_SSIM, R_ABS, R_ACC0, R_ACC1, R_ACC2, R_N_DEPTH };
static_assert(R_N_DEPTH + 1 == ROW, "row layout");

struct MetricsParams {
    const float* pred; const float* gt; const float* depth_pred; const float* depth_gt;
    int H, W, tiles_x, tiles_y;
    float C1, C2;
    double gt_scale, thr0, thr1, thr2;
    double* partial;
};

template <int WIN>
__global__ __launch_bounds__(MT_THREADS) void frame_metrics_tile_kernel(MetricsParams P)
{
    constexpr int SH = MT_H + WIN - 1, SW = MT_W + WIN - 1, SWC = 3 * SW;
    __shared__ float s_img[2][SH][SWC];              // raw values, channels interleaved as in memory (lanes 3 floats apart: no bank conflict)
    __shared__ float s_row[5][SH][MT_W];             // per staged row and window origin: sum x, sum y, centred xx, yy, xy
    __shared__ double s_red[MT_THREADS / 64][ROW];

    const int tid = threadIdx.x;
    const int tiles = P.tiles_x * P.tiles_y;
    const int k = blockIdx.x / tiles, t = blockIdx.x - k * tiles;
    const int tyi = t / P.tiles_x, txi = t - tyi * P.tiles_x;
    const int ty0 = tyi * MT_H, tx0 = txi * MT_W;
    const int H = P.H, W = P.W;
    const size_t frame = (size_t)k * H * W;
    const float* __restrict__ pred = P.pred + frame * 3;
    const float* __restrict__ gt = P.gt + frame * 3;

    // ---- stage: rows of 3 * SW contiguous floats; outside the image: 0 (only windows that are not counted read them)
    for (int idx = tid; idx < SH * SWC; idx += MT_THREADS) {
        const int r = idx / SWC, cc = idx - r * SWC;
        const int gy = ty0 + r, gx = tx0 + cc / 3;
        float a = 0.f, b = 0.f;
        if (gy < H && gx < W) {
            const size_t o = ((size_t)gy * W + tx0) * 3 + cc;
            a = pred[o]; b = gt[o];
        }
        s_img[0][r][cc] = a; s_img[1][r][cc] = b;
    }
    __syncthreads();

    double acc[ROW];
#pragma unroll
    for (int e = 0; e < ROW; ++e) acc[e] = 0.0;

    // ---- the tile's own pixels: squared error (all / centre crop / DTU mask) and depth errors
    const int hc = H / 10, wc = W / 10;
    const bool has_crop = hc > 0 && wc > 0;
    for (int p = tid; p < MT_H * MT_W; p += MT_THREADS) {
        const int py = p / MT_W, px = p - py * MT_W;
        const int gy = ty0 + py, gx = tx0 + px;
        if (gy >= H || gx >= W) continue;
        double e = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = s_img[0][py][3 * px + c] - s_img[1][py][3 * px + c];
            e += (double)(d * d);
        }
        acc[R_SSE] += e; acc[R_N] += 1.0;
        if (has_crop && gy >= hc && gy < H - hc && gx >= wc && gx < W - wc) { acc[R_SSE_CROP] += e; acc[R_N_CROP] += 1.0; }
        if (P.depth_gt) {
            const size_t o = frame + (size_t)gy * W + gx;
            const float dg = P.depth_gt[o];
            if (dg != 0.f) { acc[R_SSE_MASK] += e; acc[R_N_MASK] += 1.0; }
            if (dg > 0.f) {
                const double err = fabs((double)P.depth_pred[o] - (double)dg * P.gt_scale);
                acc[R_ABS] += err; acc[R_N_DEPTH] += 1.0;
                if (err < P.thr0) acc[R_ACC0] += 1.0;
                if (err < P.thr1) acc[R_ACC1] += 1.0;
                if (err < P.thr2) acc[R_ACC2] += 1.0;
            }
        }
    }

    // ---- SSIM, one channel at a time
    constexpr float inv_w = 1.0f / WIN, inv_n = 1.0f / (WIN * WIN), inv_nm1 = 1.0f / (WIN * WIN - 1);
    const int n_valid_y = H - WIN + 1, n_valid_x = W - WIN + 1;          // window origins 0 .. n_valid - 1
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        const float ox = s_img[0][0][c], oy = s_img[1][0][c];            // the tile's first pixel (always inside the image)
        for (int idx = tid; idx < SH * MT_W; idx += MT_THREADS) {
            const int r = idx / MT_W, j = idx - r * MT_W;
            float x[WIN], y[WIN], sx = 0.f, sy = 0.f;
#pragma unroll
            for (int i = 0; i < WIN; ++i) {
                x[i] = s_img[0][r][3 * (j + i) + c] - ox; y[i] = s_img[1][r][3 * (j + i) + c] - oy;
                sx += x[i]; sy += y[i];
            }
            const float mx = sx * inv_w, my = sy * inv_w;
            float xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
            for (int i = 0; i < WIN; ++i) {
                const float dx = x[i] - mx, dy = y[i] - my;
                xx = fmaf(dx, dx, xx); yy = fmaf(dy, dy, yy); xy = fmaf(dx, dy, xy);
            }
            s_row[0][r][j] = sx; s_row[1][r][j] = sy; s_row[2][r][j] = xx; s_row[3][r][j] = yy; s_row[4][r][j] = xy;
        }
        __syncthreads();
        double ssim = 0.0;
        for (int p = tid; p < MT_H * MT_W; p += MT_THREADS) {
            const int i0 = p / MT_W, j = p - i0 * MT_W;
            if (ty0 + i0 >= n_valid_y || tx0 + j >= n_valid_x) continue;
            float rx[WIN], ry[WIN], sx = 0.f, sy = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
            for (int r = 0; r < WIN; ++r) {
                rx[r] = s_row[0][i0 + r][j]; ry[r] = s_row[1][i0 + r][j];
                sx += rx[r]; sy += ry[r];
                xx += s_row[2][i0 + r][j]; yy += s_row[3][i0 + r][j]; xy += s_row[4][i0 + r][j];
            }
            const float mx = sx * inv_n, my = sy * inv_n;
            float bx = 0.f, by = 0.f, bxy = 0.f;                          // between-row part: sum_r (mean_r - mean)^2
#pragma unroll
            for (int r = 0; r < WIN; ++r) {
                const float dx = rx[r] * inv_w - mx, dy = ry[r] * inv_w - my;
                bx = fmaf(dx, dx, bx); by = fmaf(dy, dy, by); bxy = fmaf(dx, dy, bxy);
            }
            const float vx = fmaf((float)WIN, bx, xx) * inv_nm1, vy = fmaf((float)WIN, by, yy) * inv_nm1, vxy = fmaf((float)WIN, bxy, xy) * inv_nm1;
            const float ux = ox + mx, uy = oy + my;
            const float num = (2.f * ux * uy + P.C1) * (2.f * vxy + P.C2);
            const float den = (ux * ux + uy * uy + P.C1) * (vx + vy + P.C2);
            ssim += (double)(num / den);
            if (c == 0) acc[R_N_SSIM] += 1.0;
        }
        if (c == 0) acc[R_SSIM0] = ssim; else if (c == 1) acc[R_SSIM1] = ssim; else acc[R_SSIM2] = ssim;      // (no runtime index into acc[])
        __syncthreads();
    }

    // ---- fixed-order reduction: shuffle tree inside each wave, then the four waves in order
#pragma unroll
    for (int e = 0; e < ROW; ++e) acc[e] = mvs_wave_sum_down(acc[e]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int e = 0; e < ROW; ++e) s_red[tid >> 6][e] = acc[e];
    }
    __syncthreads();
    if (tid < ROW) {
        double v = s_red[0][tid];
        for (int w = 1; w < MT_THREADS / 64; ++w) v += s_red[w][tid];
        P.partial[(size_t)blockIdx.x * ROW + tid] = v;
    }
}

__global__ __launch_bounds__(256) void frame_metrics_sum_kernel(const double* __restrict__ partial, int tiles, double* __restrict__ out)
{
    const int e = threadIdx.x >> 4, l = threadIdx.x & 15;
    const double* p = partial + (size_t)blockIdx.x * tiles * ROW;
    double v = 0.0;
    if (e < ROW)
        for (int t = l; t < tiles; t += 16) v += p[(size_t)t * ROW + e];
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_down(v, off, 16);
    if (e < ROW && l == 0) out[(size_t)blockIdx.x * ROW + e] = v;
}

inline int64_t metrics_tiles(int H, int W) { return (int64_t)mvs_cdiv(H, MT_H) * mvs_cdiv(W, MT_W); }
inline bool metrics_win_ok(int win) { return win >= 3 && win <= 11 && (win & 1); }

}  // namespace

extern "C" size_t mvsnerf_frame_metrics_workspace_bytes(int K, int H, int W, int win_size)
{
    if (K < 1 || H < 1 || W < 1 || !metrics_win_ok(win_size) || H < win_size || W < win_size) return 0;
    return (size_t)K * (size_t)metrics_tiles(H, W) * ROW * sizeof(double);
}

extern "C" int mvsnerf_frame_metrics_fwd(const float* pred, const float* gt, const float* depth_pred, const float* depth_gt, int K, int H, int W,
                                         int win_size, double data_range, double K1, double K2, double gt_scale, const double* thresholds,
                                         double* out, void* workspace, void* stream)
{
    if (!pred || !gt || !out || !workspace || !thresholds || K < 1 || H < 1 || W < 1 || !metrics_win_ok(win_size)) return MVSNERF_EINVAL;
    if ((depth_pred == nullptr) != (depth_gt == nullptr)) return MVSNERF_EINVAL;
    if (H < win_size || W < win_size) return MVSNERF_EUNSUPPORTED;
    const int64_t tiles = metrics_tiles(H, W);
    if ((int64_t)K * tiles >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    auto mis = [](const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (mis(pred, 4) || mis(gt, 4) || mis(depth_pred, 4) || mis(depth_gt, 4) || mis(out, 8) || mis(workspace, 8)) return MVSNERF_EALIGN;

    MetricsParams P;
    P.pred = pred; P.gt = gt; P.depth_pred = depth_pred; P.depth_gt = depth_gt;
    P.H = H; P.W = W; P.tiles_x = (int)mvs_cdiv(W, MT_W); P.tiles_y = (int)mvs_cdiv(H, MT_H);
    P.C1 = (float)((K1 * data_range) * (K1 * data_range)); P.C2 = (float)((K2 * data_range) * (K2 * data_range));
    P.gt_scale = gt_scale; P.thr0 = thresholds[0]; P.thr1 = thresholds[1]; P.thr2 = thresholds[2];
    P.partial = static_cast<double*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(K * tiles);
    switch (win_size) {
        case 3:  frame_metrics_tile_kernel<3><<<grid, MT_THREADS, 0, st>>>(P); break;
        case 5:  frame_metrics_tile_kernel<5><<<grid, MT_THREADS, 0, st>>>(P); break;
        case 7:  frame_metrics_tile_kernel<7><<<grid, MT_THREADS, 0, st>>>(P); break;
        case 9:  frame_metrics_tile_kernel<9><<<grid, MT_THREADS, 0, st>>>(P); break;
        default: frame_metrics_tile_kernel<11><<<grid, MT_THREADS, 0, st>>>(P); break;
    }
    MVS_LAUNCH_CHECK();
    frame_metrics_sum_kernel<<<K, 256, 0, st>>>(P.partial, (int)tiles, out);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
