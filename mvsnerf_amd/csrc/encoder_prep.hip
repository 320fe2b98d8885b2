// Scene-encode preparation: the layout and resize helpers in front of the plane sweep, the depth hypotheses, and the stand-alone homo_warp.
//
// Layouts (all fp32, channel-last so that a voxel's channels are one contiguous vector):
//   source features   feat[v][y][x][32]          (NCHW from the 2-D FeatureNet is transposed once)
//   source thumbnails img[v][y][x][4]            (rgb + pad)
// The plane sweep itself: planesweep.hip (forward), planesweep_bwd.hip (backward).
#include "common.h"

__global__ __launch_bounds__(256) void nchw_to_nhwc_pad_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                               int N, int C, int64_t HW, int Cpad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over N*HW*Cpad
    if (i >= (int64_t)N * HW * Cpad) return;
    const int c = (int)(i % Cpad);
    const int64_t r = i / Cpad;
    const int64_t n = r / HW, p = r - n * HW;
    dst[i] = c < C ? src[(n * C + c) * HW + p] : 0.0f;
}

extern "C" int mvsnerf_nchw_to_nhwc(const float* src, float* dst, int N, int C, int H, int W, int Cpad, void* stream)
{
    if (!src || !dst || N < 1 || C < 1 || H < 1 || W < 1 || Cpad < C) return MVSNERF_EINVAL;
    const int64_t tot = (int64_t)N * H * W * Cpad;
    nchw_to_nhwc_pad_kernel<<<mvs_cdiv(tot, 256), 256, 0, (hipStream_t)stream>>>(src, dst, N, C, (int64_t)H * W, Cpad);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// F.interpolate(mode='bilinear', align_corners=False) (models.py:859).  Both resize kernels form every output value through the two helpers
// below, with every operation spelled out and nothing left to contract: the channel-last form holds the BITS of the planar one
// (tests/test_gpu_sweep_edges.py).  Left to the compiler, the same source expression was contracted differently in the two kernels and even
// per channel inside one of them (green took fma(hy, top, ly * bot), red and blue fma(ly, bot, hy * top)): last-bit differences between
// entries that claim the same operations.  The arithmetic kept is the one red and blue had: the source coordinate in one rounding,
// fma(scale, o + 0.5, -0.5), top = fma(lx, p01, hx * p00), bottom = fma(hx, p10, lx * p11), value = fma(ly, bottom, hy * top).
__device__ __forceinline__ void resize_axis(int o, int n_in, int n_out, int& i0, int& i1, float& l, float& h)
{
#pragma clang fp contract(off)
    const float scale = (float)n_in / (float)n_out;                          // area_pixel_compute_scale
    float f = fmaf(scale, (float)o + 0.5f, -0.5f); if (f < 0.f) f = 0.f;
    i0 = (int)f;
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l = f - (float)i0; h = 1.f - l;
}
__device__ __forceinline__ float resize_blend(const float* __restrict__ p, int Wi, int y0, int y1, int x0, int x1, float ly, float hy, float lx, float hx)
{
#pragma clang fp contract(off)
    const float top = fmaf(lx, p[(int64_t)y0 * Wi + x1], hx * p[(int64_t)y0 * Wi + x0]);
    const float bot = fmaf(hx, p[(int64_t)y1 * Wi + x0], lx * p[(int64_t)y1 * Wi + x1]);
    return fmaf(ly, bot, hy * top);
}

// planes [NC][Hi][Wi] -> [NC][Ho][Wo]
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                              int NC, int Hi, int Wi, int Ho, int Wo)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)NC * Ho * Wo) return;
    const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho);
    const int64_t n = i / ((int64_t)Wo * Ho);
    int y0, y1, x0, x1;
    float ly, hy, lx, hx;
    resize_axis(y, Hi, Ho, y0, y1, ly, hy);
    resize_axis(x, Wi, Wo, x0, x1, lx, hx);
    dst[i] = resize_blend(src + n * Hi * Wi, Wi, y0, y1, x0, x1, ly, hy, lx, hx);
}

// the same interpolation of N three-channel images written channel-last with a zero fourth channel ([N][Ho][Wo][4]: what the plane sweep reads): one launch
// instead of resize + mvsnerf_nchw_to_nhwc, the same operations per value
__global__ __launch_bounds__(256) void resize_bilinear_nhwc4_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int Hi, int Wi, int Ho, int Wo)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * Ho * Wo) return;
    int x, y, n;
    mvs_unflatten3(i, Wo, Ho, x, y, n);
    int y0, y1, x0, x1;
    float ly, hy, lx, hx;
    resize_axis(y, Hi, Ho, y0, y1, ly, hy);
    resize_axis(x, Wi, Wo, x0, x1, lx, hx);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = resize_blend(src + ((int64_t)n * 3 + c) * Hi * Wi, Wi, y0, y1, x0, x1, ly, hy, lx, hx);
    *reinterpret_cast<f32x4*>(dst + i * 4) = o;
}

extern "C" int mvsnerf_resize_bilinear_nhwc4(const float* src, float* dst, int N, int Hi, int Wi, int Ho, int Wo, void* stream)
{
    if (!src || !dst || N < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1) return MVSNERF_EINVAL;
    if (!mvs_aligned16(dst)) return MVSNERF_EALIGN;
    resize_bilinear_nhwc4_kernel<<<mvs_cdiv((int64_t)N * Ho * Wo, 256), 256, 0, (hipStream_t)stream>>>(src, dst, N, Hi, Wi, Ho, Wo);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_resize_bilinear(const float* src, float* dst, int NC, int Hi, int Wi, int Ho, int Wo, void* stream)
{
    if (!src || !dst || NC < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1) return MVSNERF_EINVAL;
    resize_bilinear_kernel<<<mvs_cdiv((int64_t)NC * Ho * Wo, 256), 256, 0, (hipStream_t)stream>>>(src, dst, NC, Hi, Wi, Ho, Wo);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// depth hypotheses of MVSNet.forward (models.py:903-906, linear in depth): depth[i] = near * (1 - t[i]) + far * t[i], every operation rounded to fp32 on its own like the
// four ATen kernels it replaces (t = torch.linspace(0, 1, D), cached by the caller; near_far = the two floats on the device: no host synchronisation)
__global__ __launch_bounds__(256) void depth_values_kernel(const float* __restrict__ t, const float* __restrict__ near_far, int D, float* __restrict__ out)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D) return;
    const float near = near_far[0], far = near_far[1];
    const float a = 1.0f - t[i];
    const float b = near * a;
    const float c = far * t[i];
    out[i] = b + c;
}

extern "C" int mvsnerf_depth_values(const float* t, const float* near_far, int D, float* out, void* stream)
{
    if (!t || !near_far || !out || D < 1) return MVSNERF_EINVAL;
    depth_values_kernel<<<mvs_cdiv(D, 256), 256, 0, (hipStream_t)stream>>>(t, near_far, D, out);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// stand-alone homo_warp (utils.py:580-630): one source view, NCHW in, (C,D,Hp,Wp) out + grid (D,Hp*Wp,2)
// A sample coordinate that is not finite gives NaN here (0 * NaN in the blend), as in the CPU reference - on purpose, unlike the plane sweep and its backward
// kernels, which give such a view four zero weights (planesweep.hip header).  Every load is guarded by its tap's in-image test.
__global__ __launch_bounds__(256) void homo_warp_kernel(const float* __restrict__ src, const float* __restrict__ P, const float* __restrict__ depth,
                                                        const float* __restrict__ grid_in, int C, int H, int W, int D, int pad,
                                                        float* __restrict__ out, float* __restrict__ grid_out)
{
#pragma clang fp contract(off)
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const int64_t nvox = (int64_t)D * Hp * Wp;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvox) return;
    float gx, gy;
    if (grid_in) { gx = grid_in[i * 2]; gy = grid_in[i * 2 + 1]; }
    else {
        const int x = (int)(i % Wp), y = (int)((i / Wp) % Hp), d = (int)(i / ((int64_t)Wp * Hp));
        const float u = (float)(x - pad), v = (float)(y - pad), dep = depth[d];
        const float p0 = fmaf(P[2], 1.0f, fmaf(P[1], v, P[0] * u)) + P[3] / dep;
        const float p1 = fmaf(P[6], 1.0f, fmaf(P[5], v, P[4] * u)) + P[7] / dep;
        const float p2 = fmaf(P[10], 1.0f, fmaf(P[9], v, P[8] * u)) + P[11] / dep;
        gx = (p0 / p2) / ((float)(W - 1) / 2.0f) - 1.0f;
        gy = (p1 / p2) / ((float)(H - 1) / 2.0f) - 1.0f;
    }
    if (grid_out) { grid_out[i * 2] = gx; grid_out[i * 2 + 1] = gy; }
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
    const float fx = floorf(ix), fy = floorf(iy);
    const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix, wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
    const bool x0in = fx >= 0.f && fx <= (float)(W - 1), x1in = fx + 1.f >= 0.f && fx + 1.f <= (float)(W - 1);
    const bool y0in = fy >= 0.f && fy <= (float)(H - 1), y1in = fy + 1.f >= 0.f && fy + 1.f <= (float)(H - 1);
    const int x0 = (int)fx, y0 = (int)fy;
    for (int c = 0; c < C; ++c) {
        const float* pl = src + (int64_t)c * H * W;
        // the CPU reference's chain fma(se, w_se, fma(sw, w_sw, fma(ne, w_ne, nw * w_nw))) with 0 for a tap outside the image
        const float nw = (x0in && y0in) ? pl[(int64_t)y0 * W + x0] : 0.f, ne = (x1in && y0in) ? pl[(int64_t)y0 * W + x0 + 1] : 0.f;
        const float sw = (x0in && y1in) ? pl[(int64_t)(y0 + 1) * W + x0] : 0.f, se = (x1in && y1in) ? pl[(int64_t)(y0 + 1) * W + x0 + 1] : 0.f;
        out[(int64_t)c * nvox + i] = fmaf(se, wx1 * wy1, fmaf(sw, wx0 * wy1, fmaf(ne, wx1 * wy0, nw * (wx0 * wy0))));
    }
}

extern "C" int mvsnerf_homo_warp_fwd(const float* src_nchw, const float* proj, const float* depth, const float* grid_in,
                                     int C, int H, int W, int D, int pad, float* warped, float* grid_out, void* stream)
{
    if (!src_nchw || !warped || C < 1 || H < 2 || W < 2 || D < 1 || pad < 0) return MVSNERF_EINVAL;
    if (!grid_in && (!proj || !depth)) return MVSNERF_EINVAL;
    const int64_t nvox = (int64_t)D * (H + 2 * pad) * (W + 2 * pad);
    homo_warp_kernel<<<mvs_cdiv(nvox, 256), 256, 0, (hipStream_t)stream>>>(src_nchw, proj, depth, grid_in, C, H, W, D, pad, warped, grid_out);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
