// 8-bit video frames of a camera path (the reference's renderer_video.ipynb: clamp * 255 -> uint8 of the colours, visualize_depth_numpy of the depths,
// utils.py:30-45, both cropped and put side by side), on the device, so that a render loop never hands a frame to the host.
//
// depth_range_part_kernel    grid-stride pass over x0 = nan_to_num(depth): per workgroup min{x0 : x0 > 0} and max x0 (shuffle tree, the four waves through LDS),
//                            one pair per workgroup into the workspace.
// depth_range_final_kernel   one wave over the pairs -> out2.  min and max commute and never round: any order gives the same bits, no atomics needed.
// frame_u8_kernel            a thread owns 4 consecutive output BYTES at a 4-byte-aligned address and stores them as one dword; the bytes in front of the
//                            first aligned address and behind the last one (frame k of a (K,H',Wout,3) tensor starts anywhere) are single byte stores of
//                            the first / last thread.  It walks (row, column, channel) of its bytes with one division pair at the start; a depth pixel's table
//                            index is computed once per pixel.  The colour table (768 bytes) is staged in LDS.
// Arithmetic: fp32, every operation rounded on its own (no contraction), IEEE division - what numpy does on float32 arrays.
#include "common.h"
#include "scan_dev.h"
#include <float.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int DR_THREADS = 256, DR_MAX_BLOCKS = 1024;
constexpr int FR_THREADS = 256;

__device__ __forceinline__ float nan_to_num_f(float x)
{
    if (x != x) return 0.f;
    if (x > FLT_MAX) return FLT_MAX;
    if (x < -FLT_MAX) return -FLT_MAX;
    return x;
}

__global__ __launch_bounds__(DR_THREADS) void depth_range_part_kernel(const float* __restrict__ depth, int64_t n, float* __restrict__ part)
{
    __shared__ float s_lo[DR_THREADS / 64], s_hi[DR_THREADS / 64];
    float lo = INFINITY, hi = -FLT_MAX;                      // x0 >= -FLT_MAX always; no positive element leaves lo = +inf
    for (int64_t i = (int64_t)blockIdx.x * DR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * DR_THREADS) {
        const float x = nan_to_num_f(depth[i]);
        if (x > 0.f) lo = fminf(lo, x);
        hi = fmaxf(hi, x);
    }
    lo = mvs_wave_min_down(lo); hi = mvs_wave_max_down(hi);
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < DR_THREADS / 64; ++w) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); }
        part[2 * blockIdx.x] = lo; part[2 * blockIdx.x + 1] = hi;
    }
}

__global__ __launch_bounds__(64) void depth_range_final_kernel(const float* __restrict__ part, int nparts, float* __restrict__ out2)
{
    float lo = INFINITY, hi = -FLT_MAX;
    for (int i = threadIdx.x; i < nparts; i += 64) { lo = fminf(lo, part[2 * i]); hi = fmaxf(hi, part[2 * i + 1]); }
    lo = mvs_wave_min_down(lo); hi = mvs_wave_max_down(hi);
    if (threadIdx.x == 0) { out2[0] = lo; out2[1] = hi; }
}

inline int depth_range_blocks(int64_t n) { const int64_t b = (n + DR_THREADS * 4 - 1) / (DR_THREADS * 4); return (int)(b < 1 ? 1 : (b > DR_MAX_BLOCKS ? DR_MAX_BLOCKS : b)); }

struct FrameParams {
    const float* rgb; const float* depth; const float* minmax; const unsigned char* lut;
    int W, crop_h, crop_w;                  // source row length and the crop
    int Wc, Wout;                           // cropped panel width, output pixels per row
    int color_panel, depth_panel;
    unsigned char* out; int head; int64_t total, nquads;      // head: bytes in front of the first 4-byte-aligned address; total bytes; whole dwords behind the head
};

// byte (0..255) of a colour value: clamp to [0,1] (NaN -> 0), * 255, truncate
__device__ __forceinline__ unsigned color_byte(float r)
{
    const float c = fminf(fmaxf(r, 0.f), 1.f);
    return (unsigned)(int)(c * 255.f);
}

// table index of a depth: trunc(255 * (x0 - mi) / ((ma - mi) + 1e-8f)) saturated to [0,255], NaN -> 0
__device__ __forceinline__ int depth_index(float d, float mi, float den)
{
    const float x0 = nan_to_num_f(d);
    const float t = (x0 - mi) / den;
    const float v = 255.f * t;
    return (int)fminf(fmaxf(v, 0.f), 255.f);
}

__global__ __launch_bounds__(FR_THREADS) void frame_u8_kernel(FrameParams P)
{
    __shared__ unsigned char s_lut[768];
    float mi = 0.f, den = 1.f;
    if (P.depth_panel) {
        for (int i = threadIdx.x; i < 768; i += FR_THREADS) s_lut[i] = P.lut[i];
        mi = P.minmax[0];
        den = (P.minmax[1] - mi) + 1e-8f;
        __syncthreads();
    }
    // work items: 0 = the head bytes, 1 .. nquads = aligned dwords, nquads + 1 = the tail bytes
    const int64_t item = (int64_t)blockIdx.x * FR_THREADS + threadIdx.x;
    if (item > P.nquads + 1) return;
    int64_t b0; int nb;
    if (item == 0) { b0 = 0; nb = P.head; }
    else if (item <= P.nquads) { b0 = P.head + (item - 1) * 4; nb = 4; }
    else { b0 = P.head + P.nquads * 4; nb = (int)(P.total - b0); }
    if (nb <= 0) return;

    const int64_t p0 = b0 / 3;
    int c = (int)(b0 - p0 * 3);
    int y = (int)(p0 / P.Wout), xo = (int)(p0 - (int64_t)y * P.Wout);
    int idx = -1;                                           // table index of the current depth pixel; -1: not computed yet
    unsigned word = 0;
    for (int j = 0; j < nb; ++j) {
        const bool in_depth = P.depth_panel && (!P.color_panel || xo >= P.Wc);
        const int x = (in_depth && P.color_panel) ? xo - P.Wc : xo;
        const int64_t src = (int64_t)(y + P.crop_h) * P.W + (x + P.crop_w);
        unsigned v;
        if (in_depth) {
            if (idx < 0) idx = depth_index(P.depth[src], mi, den);
            v = s_lut[idx * 3 + c];
        } else {
            v = color_byte(P.rgb[src * 3 + c]);
        }
        word |= v << (8 * j);
        if (++c == 3) { c = 0; idx = -1; if (++xo == P.Wout) { xo = 0; ++y; } }
    }
    if (nb == 4 && item != 0 && item <= P.nquads) {
        *reinterpret_cast<unsigned*>(P.out + b0) = word;       // 4-byte aligned by construction
    } else {
        for (int j = 0; j < nb; ++j) P.out[b0 + j] = (unsigned char)(word >> (8 * j));
    }
}

}  // namespace

extern "C" size_t mvsnerf_depth_range_workspace_floats(int64_t n)
{
    return n < 1 ? 0 : (size_t)2 * depth_range_blocks(n);
}

extern "C" int mvsnerf_depth_range_fwd(const float* depth, int64_t n, float* out2, float* workspace, void* stream)
{
    if (!depth || !out2 || !workspace || n < 1) return MVSNERF_EINVAL;
    auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; };
    if (mis(depth) || mis(out2) || mis(workspace)) return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = depth_range_blocks(n);
    depth_range_part_kernel<<<blocks, DR_THREADS, 0, st>>>(depth, n, workspace);
    MVS_LAUNCH_CHECK();
    depth_range_final_kernel<<<1, 64, 0, st>>>(workspace, blocks, out2);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_frame_u8_fwd(const float* rgb, const float* depth, int H, int W, const float* minmax, const unsigned char* lut,
                                    int crop_h, int crop_w, int depth_panel, unsigned char* out, void* stream)
{
    if (!out || H < 1 || W < 1 || crop_h < 0 || crop_w < 0 || (depth_panel != 0 && depth_panel != 1)) return MVSNERF_EINVAL;
    if (!rgb && !depth_panel) return MVSNERF_EINVAL;                             // nothing to write
    if (depth_panel && (!depth || !minmax || !lut)) return MVSNERF_EINVAL;
    if (2 * (int64_t)crop_h >= H || 2 * (int64_t)crop_w >= W) return MVSNERF_EINVAL;
    auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; };
    if (mis(rgb) || (depth_panel && (mis(depth) || mis(minmax)))) return MVSNERF_EALIGN;
    if ((int64_t)H * W >= ((int64_t)1 << 28)) return MVSNERF_EUNSUPPORTED;        // pixel and byte counts stay far inside 32 / 63 bits

    FrameParams P;
    P.rgb = rgb; P.depth = depth; P.minmax = minmax; P.lut = lut;
    P.W = W; P.crop_h = crop_h; P.crop_w = crop_w;
    P.Wc = W - 2 * crop_w;
    P.color_panel = rgb ? 1 : 0; P.depth_panel = depth_panel;
    P.Wout = P.Wc * (P.color_panel + depth_panel);
    P.out = out;
    P.total = (int64_t)(H - 2 * crop_h) * P.Wout * 3;
    int head = (int)((4 - (reinterpret_cast<uintptr_t>(out) & 3u)) & 3u);
    if (head > P.total) head = (int)P.total;
    P.head = head;
    P.nquads = (P.total - head) / 4;
    const int64_t items = P.nquads + 2;
    frame_u8_kernel<<<mvs_cdiv(items, FR_THREADS), FR_THREADS, 0, (hipStream_t)stream>>>(P);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
