// Pillow's 8-bit resampler on the bank's images: Image.resize(size, LANCZOS | BILINEAR) of the reference's per-scene datasets
// (data/dtu_ft.py:108,163, data/blender.py:66,133, data/llff.py:241,344; BILINEAR: data/dtu.py:160), byte for byte.  Pillow's resampler
// (src/libImaging/Resample.c) is integer arithmetic on 22-bit fixed-point coefficients, so there is no tolerance: tests/resample_refs.py is the
// restatement, pinned to Pillow's own outputs.
//   resample_h_kernel   src [M*Hin][Win] -> dst [M*Hin][Wout]     (first, over all input rows, and only if the width changes)
//   resample_v_kernel   src [M][Hin][W]  -> dst [M][Hout][W]      (second, and only if the height changes)
//   copy_u8_kernel      equal sizes: Pillow returns a copy
// Images: uint8 [M][H][W][4], one 32-bit load per pixel.  One output pixel per thread: acc = 2^21 + sum_x src[xmin + x] * kk[x] in int32 per channel,
// byte = clamp(acc >> 22, 0, 255).  An image with alpha is resampled premultiplied, as Pillow does (Image.resize converts RGBA -> RGBa -> RGBA around
// the resize; Convert.c rgbA2rgba, rgba2rgbA): the conversions are per pixel, fused into the first pass's load and the last pass's store.
// Tables per axis, built by the host (ops._resample_tables): win [n_out][2] = (xmin, n), kk [n_out][ksize] int32.  They are caller input, so every
// thread checks its own window before any load (xmin >= 0, 0 <= n <= ksize, xmin + n <= n_in); a bad window gives an all-zero pixel and reads nothing.
// No LDS: the threads of a wave read one contiguous span of a row per tap (horizontal) or one contiguous row segment (vertical); the taps' reuse is the
// vector cache's.  No atomics, no inline assembly; two runs give the same bytes.
#include "common.h"

// rgbA2rgba (Pillow's MULDIV255): c' = ((t >> 8) + t) >> 8 with t = c * a + 128
__device__ __forceinline__ unsigned premul255(unsigned c, unsigned a)
{
    const unsigned t = c * a + 128u;
    return ((t >> 8) + t) >> 8;
}

// One output pixel: src points at the window's first pixel candidate (index 0 of the axis), stride in pixels along the axis.
// ALPHA: four channels, premultiplied on load in the FIRST pass and divided by alpha again on the LAST pass's store; else three channels, alpha 255.
template <bool ALPHA, bool FIRST, bool LAST>
__device__ __forceinline__ uchar4 resample_pixel(const uchar4* __restrict__ src, int64_t stride, int n_in, const int* __restrict__ win,
                                                 const int* __restrict__ kk, int ks)
{
    const int xmin = win[0], n = win[1];
    if (xmin < 0 || n < 0 || n > ks || xmin > n_in - n) return uchar4{0, 0, 0, 0};      // (n <= ks bounds n, so n_in - n cannot overflow)
    // unsigned accumulators: the low 32 bits of Pillow's int32 sums, and no undefined overflow whatever a caller's coefficients are
    unsigned a0 = 1u << 21, a1 = 1u << 21, a2 = 1u << 21, a3 = 1u << 21;
    src += (int64_t)xmin * stride;
    for (int x = 0; x < n; ++x) {
        const uchar4 p = src[(int64_t)x * stride];
        const unsigned k = (unsigned)kk[x];
        unsigned c0 = p.x, c1 = p.y, c2 = p.z;
        if (ALPHA && FIRST) { c0 = premul255(c0, p.w); c1 = premul255(c1, p.w); c2 = premul255(c2, p.w); }
        a0 += c0 * k; a1 += c1 * k; a2 += c2 * k;
        if (ALPHA) a3 += (unsigned)p.w * k;
    }
    int r0 = min(max((int)a0 >> 22, 0), 255), r1 = min(max((int)a1 >> 22, 0), 255), r2 = min(max((int)a2 >> 22, 0), 255);
    int r3 = 255;
    if (ALPHA) {
        r3 = min(max((int)a3 >> 22, 0), 255);
        if (LAST && r3 != 0 && r3 != 255) {                                             // rgba2rgbA: CLIP8(255 * c / a), a copy at alpha 0 and 255
            r0 = min(255 * r0 / r3, 255); r1 = min(255 * r1 / r3, 255); r2 = min(255 * r2 / r3, 255);
        }
    }
    return uchar4{(unsigned char)r0, (unsigned char)r1, (unsigned char)r2, (unsigned char)r3};
}

// t = row * Wout + xx over the M * Hin rows of all images
template <bool ALPHA, bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void resample_h_kernel(const uchar4* __restrict__ src, uchar4* __restrict__ dst, int64_t total, int Win, int Wout,
                                                         const int* __restrict__ win, const int* __restrict__ kk, int ks)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t row = t / Wout;
    const int xx = (int)(t - row * Wout);
    dst[t] = resample_pixel<ALPHA, FIRST, LAST>(src + row * Win, 1, Win, win + 2 * xx, kk + (int64_t)xx * ks, ks);
}

// t = (m * Hout + yy) * W + x: a wave reads and writes contiguous pixels of a row
template <bool ALPHA, bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void resample_v_kernel(const uchar4* __restrict__ src, uchar4* __restrict__ dst, int64_t total, int Hin, int Hout, int W,
                                                         const int* __restrict__ win, const int* __restrict__ kk, int ks)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t r = t / W, m = r / Hout;
    const int x = (int)(t - r * W), yy = (int)(r - m * Hout);
    dst[t] = resample_pixel<ALPHA, FIRST, LAST>(src + m * Hin * W + x, W, Hin, win + 2 * yy, kk + (int64_t)yy * ks, ks);
}

template <bool ALPHA>
__global__ __launch_bounds__(256) void copy_u8_kernel(const uchar4* __restrict__ src, uchar4* __restrict__ dst, int64_t total)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    uchar4 p = src[t];
    if (!ALPHA) p.w = 255;
    dst[t] = p;
}

static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

static const int64_t kMaxImagePixels = 0x7fffffff;          // per image and pass: Hin*Win, Hin*Wout, Hout*Wout
static const int64_t kMaxPassPixels = (int64_t)1 << 38;     // per pass over all M images: its 256-thread workgroups must fit the grid
static const int kMaxKsize = 65535;                         // (a Lanczos reduction by more than 10 000)

// sizes >= 1 and inside the limits: MVSNERF_OK and the pixel counts of the horizontal pass's and the whole call's output
static int resample_sizes(int M, int Hin, int Win, int Hout, int Wout, int64_t* n_mid, int64_t* n_dst)
{
    if (M < 1 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1) return MVSNERF_EINVAL;
    const int64_t src = (int64_t)Hin * Win, mid = (int64_t)Hin * Wout, dst = (int64_t)Hout * Wout;
    if (src > kMaxImagePixels || mid > kMaxImagePixels || dst > kMaxImagePixels) return MVSNERF_EUNSUPPORTED;
    if (mid > kMaxPassPixels / M || dst > kMaxPassPixels / M || src > kMaxPassPixels / M) return MVSNERF_EUNSUPPORTED;
    *n_mid = mid * M;
    *n_dst = dst * M;
    return MVSNERF_OK;
}

extern "C" size_t mvsnerf_resample_u8_workspace_bytes(int M, int Hin, int Win, int Hout, int Wout)
{
    int64_t n_mid, n_dst;
    if (resample_sizes(M, Hin, Win, Hout, Wout, &n_mid, &n_dst) != MVSNERF_OK) return 0;
    return (Win != Wout && Hin != Hout) ? (size_t)n_mid * 4 : 0;
}

template <bool ALPHA, bool FIRST, bool LAST>
static void launch_h(const uchar4* src, uchar4* dst, int64_t total, int Win, int Wout, const int* win, const int* kk, int ks, hipStream_t st)
{
    resample_h_kernel<ALPHA, FIRST, LAST><<<mvs_cdiv(total, 256), 256, 0, st>>>(src, dst, total, Win, Wout, win, kk, ks);
}

template <bool ALPHA, bool FIRST, bool LAST>
static void launch_v(const uchar4* src, uchar4* dst, int64_t total, int Hin, int Hout, int W, const int* win, const int* kk, int ks, hipStream_t st)
{
    resample_v_kernel<ALPHA, FIRST, LAST><<<mvs_cdiv(total, 256), 256, 0, st>>>(src, dst, total, Hin, Hout, W, win, kk, ks);
}

extern "C" int mvsnerf_resample_u8_fwd(const unsigned char* src, int M, int Hin, int Win, unsigned char* dst, int Hout, int Wout, const int* xwin,
                                       const int* xkk, int xks, const int* ywin, const int* ykk, int yks, int alpha_mode, void* workspace, void* stream)
{
    int64_t n_mid, n_dst;
    if (!src || !dst || (alpha_mode != 0 && alpha_mode != 1)) return MVSNERF_EINVAL;
    if (int rc = resample_sizes(M, Hin, Win, Hout, Wout, &n_mid, &n_dst)) return rc;
    const bool horiz = Win != Wout, vert = Hin != Hout;
    if (horiz && (!xwin || !xkk || xks < 1)) return MVSNERF_EINVAL;
    if (vert && (!ywin || !ykk || yks < 1)) return MVSNERF_EINVAL;
    if (horiz && vert && !workspace) return MVSNERF_EINVAL;
    if (!aligned4(src) || !aligned4(dst) || (horiz && vert && !aligned4(workspace))) return MVSNERF_EALIGN;
    if ((horiz && (!aligned4(xwin) || !aligned4(xkk))) || (vert && (!aligned4(ywin) || !aligned4(ykk)))) return MVSNERF_EALIGN;
    if ((horiz && xks > kMaxKsize) || (vert && yks > kMaxKsize)) return MVSNERF_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const uchar4* s = reinterpret_cast<const uchar4*>(src);
    uchar4* d = reinterpret_cast<uchar4*>(dst);
    uchar4* w = reinterpret_cast<uchar4*>(workspace);
    const bool alpha = alpha_mode == 1;
    if (!horiz && !vert) {
        if (alpha) copy_u8_kernel<true><<<mvs_cdiv(n_dst, 256), 256, 0, st>>>(s, d, n_dst);
        else copy_u8_kernel<false><<<mvs_cdiv(n_dst, 256), 256, 0, st>>>(s, d, n_dst);
    } else if (horiz && !vert) {
        if (alpha) launch_h<true, true, true>(s, d, n_dst, Win, Wout, xwin, xkk, xks, st);
        else launch_h<false, true, true>(s, d, n_dst, Win, Wout, xwin, xkk, xks, st);
    } else if (!horiz) {
        if (alpha) launch_v<true, true, true>(s, d, n_dst, Hin, Hout, Wout, ywin, ykk, yks, st);
        else launch_v<false, true, true>(s, d, n_dst, Hin, Hout, Wout, ywin, ykk, yks, st);
    } else {
        if (alpha) launch_h<true, true, false>(s, w, n_mid, Win, Wout, xwin, xkk, xks, st);
        else launch_h<false, true, false>(s, w, n_mid, Win, Wout, xwin, xkk, xks, st);
        MVS_LAUNCH_CHECK();
        if (alpha) launch_v<true, false, true>(w, d, n_dst, Hin, Hout, Wout, ywin, ykk, yks, st);
        else launch_v<false, false, true>(w, d, n_dst, Hin, Hout, Wout, ywin, ykk, yks, st);
    }
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
