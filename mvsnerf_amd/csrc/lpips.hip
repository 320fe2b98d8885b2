// LPIPS-VGG (Zhang et al. 2018; the `lpips.LPIPS(net='vgg')` the reference's renderer.ipynb reports per held-out view): the VGG-16 trunk and the five
// 1x1 heads on channel-last fp32 activations act[n][y][x][C].  DESIGN.md 4l.
//
// lpips_conv3x3_kernel     conv3x3 + bias + ReLU, stride 1, zero padding 1, Cin in {64,128,256,512}, Cout a multiple of 64, as an implicit GEMM on
//                          v_mfma_f32_32x32x2_f32 (exact fp32: per chunk of 16 input channels one fmaf chain over tap and channel, the chunk sums added in order).  One workgroup = 4 rows x 32
//                          columns of pixels x 64 output channels; wave w owns row w: A = 32 pixels (lane & 31) x 2 input channels (lane >> 5), B = 2 input
//                          channels x 32 output channels, two accumulator tiles (output channels 0-31, 32-63 of the workgroup's 64).  Per chunk of 16 input
//                          channels the 6 x 34 halo tile is staged once in LDS ([pixel][18 floats]: a stride of 2 mod 4 floats puts the 32 pixels of an 8-byte
//                          operand read on 32 different bank pairs) and serves all nine taps; the chunk's weights (9 taps x 16 x 64, packed in fragment order
//                          by lpips_pack_kernel: a lane's 8-byte read is its B value of two consecutive k-steps) are a linear copy.  The next chunk's global
//                          loads are issued before the current chunk's MFMAs and stored after them.  Pixels outside the image are zero in LDS and never
//                          stored; a tile never crosses a row end, an image end or the next image of the batch (tiles are counted per image).
// lpips_conv1_kernel       conv1_1 (3 -> 64) on the VALU: lane = pixel, wave = 16 output channels (weights by scalar loads).  Its loader applies LPIPS's
//                          scaling layer ((2x - 1) - shift_c) / scale_c to a [0,1] input INSIDE the image only: a padding tap contributes 0.
// lpips_pool_kernel        maxpool 2x2 / 2, floor mode (an odd last row / column is dropped), NaN propagating as torch's.
// lpips_head_kernel        one tap layer: per pixel n = sqrt(sum_c f^2) + 1e-10 for both maps, d = sum_c lin_c (f0_c / n0 - f1_c / n1)^2, everything past the
//                          loads in double; one wave per pixel, 64 pixels per workgroup, one partial per workgroup.  lpips_head_sum_kernel adds a frame's
//                          partials in a fixed order and divides by the pixel count.  No atomics: two calls give equal bits, frame k of a batch the bits of
//                          the frame alone.
#include "common.h"
#include "scan_dev.h"

namespace {

constexpr int LT_H = 4, LT_W = 32, LT_N = 64, LKC = 16, L_THREADS = 256;
constexpr int LHALO_W = LT_W + 2, LHALO = (LT_H + 2) * LHALO_W;        // 204 staged pixels
constexpr int LPIX = LKC + 2;                                          // floats per staged pixel
constexpr int LW_STAGE = 9 * (LKC / 4) * 2 * 64 * 2;                   // floats of one (64 output channels, 16 input channels) weight stage
constexpr int LIN_ITEMS = LHALO * (LKC / 4);                           // float4 loads of one input stage
constexpr int LIN_PT = (LIN_ITEMS + L_THREADS - 1) / L_THREADS;        // 4 per thread
constexpr int LW_PT = LW_STAGE / 4 / L_THREADS;                        // 9 per thread
static_assert(LW_STAGE == 9 << 10 && LW_STAGE % (4 * L_THREADS) == 0, "weight stage layout");

__global__ __launch_bounds__(256) void lpips_pack_kernel(const float* __restrict__ w, const float* __restrict__ b, int Cin, int Cout, float* __restrict__ packed)
{
    const int64_t total = (int64_t)Cin * Cout * 9;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < Cout) packed[total + p] = b[p];
    if (p >= total) return;
    if (Cin == 3) {                                   // conv1_1: [ci * 9 + tap][cout]
        const int co = (int)(p % Cout), k = (int)(p / Cout);
        packed[p] = w[(size_t)co * 27 + k];
        return;
    }
    // [cout / 64][chunk][tap][q][j][lane][e]: the value lane (r, h) feeds to k-step 2q + e of accumulator tile j
    const int e = (int)(p & 1), lane = (int)(p >> 1) & 63, j = (int)(p >> 7) & 1, q = (int)(p >> 8) & 3;
    const int64_t s = p >> 10;
    const int tap = (int)(s % 9);
    const int64_t rest = s / 9;
    const int nchunks = Cin / LKC;
    const int chunk = (int)(rest % nchunks), nt = (int)(rest / nchunks);
    const int co = nt * LT_N + 32 * j + (lane & 31), ci = chunk * LKC + 4 * q + 2 * (lane >> 5) + e;
    packed[p] = w[((size_t)co * Cin + ci) * 9 + tap];
}

__global__ __launch_bounds__(L_THREADS) void lpips_conv3x3_kernel(const float* __restrict__ in, const float* __restrict__ wp, float* __restrict__ out,
                                                                  int H, int W, int Cin, int Cout, int tiles_x, int tiles_y)
{
    __shared__ __attribute__((aligned(16))) float s_in[LHALO * LPIX];
    __shared__ __attribute__((aligned(16))) float s_w[LW_STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int NT = Cout / LT_N, nchunks = Cin / LKC;
    int b = blockIdx.x;
    const int nt = b % NT; b /= NT;
    const int txi = b % tiles_x; b /= tiles_x;
    const int tyi = b % tiles_y;
    const int n = b / tiles_y;
    const int y0 = tyi * LT_H, x0 = txi * LT_W;
    const float* __restrict__ img = in + (size_t)n * H * W * Cin;
    const f32x4* __restrict__ wsrc = reinterpret_cast<const f32x4*>(wp) + (size_t)nt * nchunks * (LW_STAGE / 4);
    const float* __restrict__ bias = wp + (size_t)Cin * Cout * 9;

    int in_off[LIN_PT], lds_off[LIN_PT];              // this thread's halo items: source element (-1: outside the image) and LDS float offset (-1: no item)
#pragma unroll
    for (int i = 0; i < LIN_PT; ++i) {
        const int item = tid + L_THREADS * i, pix = item >> 2, cg = item & 3;
        const int hy = pix / LHALO_W, hx = pix - hy * LHALO_W;
        const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
        lds_off[i] = item < LIN_ITEMS ? pix * LPIX + 4 * cg : -1;
        in_off[i] = (item < LIN_ITEMS && gy >= 0 && gy < H && gx >= 0 && gx < W) ? (gy * W + gx) * Cin + 4 * cg : -1;
    }
    f32x4 rin[LIN_PT], rw[LW_PT];
#define LPIPS_LOAD_STAGE(c)                                                                                                              \
    do {                                                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < LIN_PT; ++i) {                                                                             \
            rin[i] = f32x4{0.f, 0.f, 0.f, 0.f};                                                                                          \
            if (in_off[i] >= 0) rin[i] = *reinterpret_cast<const f32x4*>(img + in_off[i] + (c) * LKC);                                   \
        }                                                                                                                                \
        _Pragma("unroll") for (int i = 0; i < LW_PT; ++i) rw[i] = wsrc[(size_t)(c) * (LW_STAGE / 4) + tid + L_THREADS * i];              \
    } while (0)

    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
    const float* a_base = s_in + (wave * LHALO_W + r) * LPIX + 2 * h;
    const float2* b_base = reinterpret_cast<const float2*>(s_w) + lane;

    LPIPS_LOAD_STAGE(0);
#pragma unroll 1
    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();                              // the previous chunk's reads are done
#pragma unroll
        for (int i = 0; i < LIN_PT; ++i)
            if (lds_off[i] >= 0) {
                *reinterpret_cast<float2*>(s_in + lds_off[i]) = make_float2(rin[i].x, rin[i].y);
                *reinterpret_cast<float2*>(s_in + lds_off[i] + 2) = make_float2(rin[i].z, rin[i].w);
            }
#pragma unroll
        for (int i = 0; i < LW_PT; ++i) reinterpret_cast<f32x4*>(s_w)[tid + L_THREADS * i] = rw[i];
        __syncthreads();
        if (c + 1 < nchunks) LPIPS_LOAD_STAGE(c + 1);
        f32x16 t0, t1;                                // the chunk's 144 terms start from 0: short chains, then one addition per chunk (accuracy)
#pragma unroll
        for (int i = 0; i < 16; ++i) { t0[i] = 0.f; t1[i] = 0.f; }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ty = tap / 3, tx = tap - 3 * ty;
#pragma unroll
            for (int q = 0; q < LKC / 4; ++q) {
                const float2 a = *reinterpret_cast<const float2*>(a_base + (ty * LHALO_W + tx) * LPIX + 4 * q);
                const float2 b0 = b_base[((tap * 4 + q) * 2 + 0) * 64], b1 = b_base[((tap * 4 + q) * 2 + 1) * 64];
                t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, t0, 0, 0, 0);
                t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, t1, 0, 0, 0);
                t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, t0, 0, 0, 0);
                t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, t1, 0, 0, 0);
            }
        }
        acc0 += t0; acc1 += t1;
    }

#undef LPIPS_LOAD_STAGE
    // epilogue: register i of lane (r, h) is pixel (i & 3) + 8 (i >> 2) + 4 h of the wave's row, output channel r (+ 32 for acc1)
    const int y = y0 + wave;
    if (y >= H) return;
    const int co = nt * LT_N + r;
    const float bias0 = bias[co], bias1 = bias[co + 32];
    float* __restrict__ orow = out + ((size_t)n * H + y) * W * Cout + co;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int x = x0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (x < W) {
            orow[(size_t)x * Cout] = fmaxf(acc0[i] + bias0, 0.f);
            orow[(size_t)x * Cout + 32] = fmaxf(acc1[i] + bias1, 0.f);
        }
    }
}

__global__ __launch_bounds__(256) void lpips_conv1_kernel(const float* __restrict__ in, const float* __restrict__ wp, float* __restrict__ out,
                                                          int N, int H, int W)
{
    const int g = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));          // 16 output channels per wave: weight addresses are wave-uniform
    const int64_t npix = (int64_t)N * H * W;
    const int64_t p = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    if (p >= npix) return;
    const int x = (int)(p % W);
    const int64_t t = p / W;
    const int y = (int)(t % H);
    const float* __restrict__ img = in + (t / H) * (int64_t)H * W * 3;
    const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
    float v[27];                                                                    // [c][ky][kx]: the scaled input, 0 where the tap is padding
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int gy = y + ky - 1, gx = x + kx - 1;
            const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                v[c * 9 + ky * 3 + kx] = ok ? ((2.f * img[((size_t)gy * W + gx) * 3 + c] - 1.f) - shift[c]) / scale[c] : 0.f;
        }
    const float* __restrict__ wg = wp + g * 16;
    float acc[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) acc[o] = 0.f;
#pragma unroll
    for (int k = 0; k < 27; ++k)
#pragma unroll
        for (int o = 0; o < 16; ++o) acc[o] = fmaf(v[k], wg[k * 64 + o], acc[o]);
    const float* __restrict__ bias = wp + 27 * 64 + g * 16;
    float4* __restrict__ o4 = reinterpret_cast<float4*>(out + (size_t)p * 64 + g * 16);
#pragma unroll
    for (int o = 0; o < 4; ++o)
        o4[o] = make_float4(fmaxf(acc[4 * o] + bias[4 * o], 0.f), fmaxf(acc[4 * o + 1] + bias[4 * o + 1], 0.f),
                            fmaxf(acc[4 * o + 2] + bias[4 * o + 2], 0.f), fmaxf(acc[4 * o + 3] + bias[4 * o + 3], 0.f));
}

__device__ __forceinline__ float pool_max(float m, float v) { return (v > m || v != v) ? v : m; }

__global__ __launch_bounds__(256) void lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t total4, int H, int W, int C4)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int Ho = H >> 1, Wo = W >> 1;
    const int c = (int)(i % C4);
    int64_t t = i / C4;
    const int xo = (int)(t % Wo); t /= Wo;
    const int yo = (int)(t % Ho);
    const int64_t n = t / Ho;
    const float4* __restrict__ src = reinterpret_cast<const float4*>(in) + ((n * H + 2 * yo) * W + 2 * xo) * C4 + c;
    const float4 a = src[0], b = src[C4], d = src[(int64_t)W * C4], e = src[(int64_t)W * C4 + C4];
    float4 m;
    m.x = pool_max(pool_max(pool_max(a.x, b.x), d.x), e.x);
    m.y = pool_max(pool_max(pool_max(a.y, b.y), d.y), e.y);
    m.z = pool_max(pool_max(pool_max(a.z, b.z), d.z), e.z);
    m.w = pool_max(pool_max(pool_max(a.w, b.w), d.w), e.w);
    reinterpret_cast<float4*>(out)[i] = m;
}

constexpr int HP_PIX = 64;             // pixels per head workgroup (4 waves x 16)

__device__ __forceinline__ double wave_sum_all(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);      // a + b on both sides of every exchange: all lanes hold the same bits
    return v;
}

template <int CPL>                     // channels per lane: C = 64 CPL
__global__ __launch_bounds__(256) void lpips_head_kernel(const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ lin,
                                                         int npix, int nblk, double* __restrict__ partial)
{
    __shared__ double s_red[4];
    constexpr int C = 64 * CPL;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x / nblk, blk = blockIdx.x - k * nblk;
    const float* __restrict__ p0 = f0 + (size_t)k * npix * C;
    const float* __restrict__ p1 = f1 + (size_t)k * npix * C;
    float l[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) l[j] = lin[lane + 64 * j];
    double sum = 0.0;
#pragma unroll 1
    for (int i = 0; i < HP_PIX / 4; ++i) {
        const int p = blk * HP_PIX + 4 * i + wave;                             // wave-uniform
        if (p >= npix) break;
        float a[CPL], b[CPL];
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            a[j] = p0[(size_t)p * C + lane + 64 * j]; b[j] = p1[(size_t)p * C + lane + 64 * j];
            s0 += (double)a[j] * (double)a[j]; s1 += (double)b[j] * (double)b[j];
        }
        const double n0 = sqrt(wave_sum_all(s0)) + 1e-10, n1 = sqrt(wave_sum_all(s1)) + 1e-10;
        double d = 0.0;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const double u = (double)a[j] / n0 - (double)b[j] / n1;
            d += (double)l[j] * u * u;
        }
        sum += wave_sum_all(d);
    }
    if (lane == 0) s_red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

__global__ __launch_bounds__(64) void lpips_head_sum_kernel(const double* __restrict__ partial, int nblk, int npix, double* __restrict__ layer_out,
                                                            double* __restrict__ total, int accumulate)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    double v = 0.0;
    for (int t = lane; t < nblk; t += 64) v += partial[(size_t)k * nblk + t];
    v = mvs_wave_sum_down(v);
    if (lane == 0) {
        v /= (double)npix;
        if (layer_out) layer_out[k] = v;
        if (total) total[k] = accumulate ? total[k] + v : v;
    }
}

inline bool lpips_width_ok(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }
inline bool lpips_conv_ok(int Cin, int Cout) { return (Cin == 3 && Cout == 64) || (lpips_width_ok(Cin) && lpips_width_ok(Cout)); }
inline bool lpips_mis(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

extern "C" size_t mvsnerf_lpips_conv_packed_floats(int Cin, int Cout)
{
    return lpips_conv_ok(Cin, Cout) ? (size_t)Cin * Cout * 9 + Cout : 0;
}

extern "C" int mvsnerf_lpips_conv_pack(const float* w, const float* b, int Cin, int Cout, float* packed, void* stream)
{
    if (!w || !b || !packed || Cin < 1 || Cout < 1) return MVSNERF_EINVAL;
    if (!lpips_conv_ok(Cin, Cout)) return MVSNERF_EUNSUPPORTED;
    if (lpips_mis(w, 4) || lpips_mis(b, 4) || lpips_mis(packed, 16)) return MVSNERF_EALIGN;
    lpips_pack_kernel<<<mvs_cdiv((int64_t)Cin * Cout * 9, 256), 256, 0, (hipStream_t)stream>>>(w, b, Cin, Cout, packed);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_lpips_conv_fwd(const float* in, const float* packed, int N, int H, int W, int Cin, int Cout, float* out, void* stream)
{
    if (!in || !packed || !out || N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return MVSNERF_EINVAL;
    if (!lpips_conv_ok(Cin, Cout)) return MVSNERF_EUNSUPPORTED;
    const int Cmax = Cin > Cout ? Cin : Cout;
    if ((int64_t)H * W * Cmax >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;          // a frame's element offsets are 32-bit in the kernels
    if (lpips_mis(packed, 16) || lpips_mis(out, 16) || lpips_mis(in, Cin == 3 ? 4 : 16)) return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (Cin == 3) {
        const int64_t blocks = ((int64_t)N * H * W + 63) / 64;
        if (blocks >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
        lpips_conv1_kernel<<<(unsigned)blocks, 256, 0, st>>>(in, packed, out, N, H, W);
    } else {
        const int tiles_x = (int)mvs_cdiv(W, LT_W), tiles_y = (int)mvs_cdiv(H, LT_H);
        const int64_t blocks = (int64_t)N * tiles_x * tiles_y * (Cout / LT_N);
        if (blocks >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
        lpips_conv3x3_kernel<<<(unsigned)blocks, L_THREADS, 0, st>>>(in, packed, out, H, W, Cin, Cout, tiles_x, tiles_y);
    }
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_lpips_pool_fwd(const float* in, int N, int H, int W, int C, float* out, void* stream)
{
    if (!in || !out || N < 1 || H < 1 || W < 1 || C < 1) return MVSNERF_EINVAL;
    if (!lpips_width_ok(C) || H < 2 || W < 2) return MVSNERF_EUNSUPPORTED;
    if (lpips_mis(in, 16) || lpips_mis(out, 16)) return MVSNERF_EALIGN;
    const int64_t total4 = (int64_t)N * (H / 2) * (W / 2) * (C / 4);
    if ((total4 + 255) / 256 >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    lpips_pool_kernel<<<(unsigned)((total4 + 255) / 256), 256, 0, (hipStream_t)stream>>>(in, out, total4, H, W, C / 4);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" size_t mvsnerf_lpips_head_workspace_bytes(int K, int h, int w, int C)
{
    if (K < 1 || h < 1 || w < 1 || !lpips_width_ok(C) || (int64_t)h * w >= ((int64_t)1 << 31)) return 0;
    return (size_t)K * (size_t)(((int64_t)h * w + HP_PIX - 1) / HP_PIX) * sizeof(double);
}

extern "C" int mvsnerf_lpips_head_fwd(const float* f0, const float* f1, const float* lin, int K, int h, int w, int C, double* layer_out, double* total,
                                      int accumulate, void* workspace, void* stream)
{
    if (!f0 || !f1 || !lin || !workspace || (!layer_out && !total) || K < 1 || h < 1 || w < 1 || C < 1) return MVSNERF_EINVAL;
    if (!lpips_width_ok(C) || (int64_t)h * w >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    const int npix = h * w, nblk = (npix + HP_PIX - 1) / HP_PIX;
    if ((int64_t)K * nblk >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    if (lpips_mis(f0, 4) || lpips_mis(f1, 4) || lpips_mis(lin, 4) || lpips_mis(layer_out, 8) || lpips_mis(total, 8) || lpips_mis(workspace, 8)) return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    double* partial = static_cast<double*>(workspace);
    const unsigned grid = (unsigned)(K * nblk);
    switch (C) {
        case 64:  lpips_head_kernel<1><<<grid, 256, 0, st>>>(f0, f1, lin, npix, nblk, partial); break;
        case 128: lpips_head_kernel<2><<<grid, 256, 0, st>>>(f0, f1, lin, npix, nblk, partial); break;
        case 256: lpips_head_kernel<4><<<grid, 256, 0, st>>>(f0, f1, lin, npix, nblk, partial); break;
        default:  lpips_head_kernel<8><<<grid, 256, 0, st>>>(f0, f1, lin, npix, nblk, partial); break;
    }
    MVS_LAUNCH_CHECK();
    lpips_head_sum_kernel<<<K, 64, 0, st>>>(partial, nblk, npix, layer_out, total, accumulate);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
