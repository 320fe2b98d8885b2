// Train-mode InPlaceABN of the lazily-activated tensors (conv3d.hip header): batch statistics -> per-channel (scale, shift), the
// materialising apply-and-add epilogues, and the backward.
#include "common.h"
#include "act.h"
#include "conv.h"

// ---------------------------------------------------------------------------------------------
// InPlaceABN in train mode: batch statistics over all voxels of a channel-last tensor x[n][C].
// Stage 1: per-block partial (sum, sum of squares) per channel, fp32, deterministic order.
// Stage 2: one block combines the partials in fp64 and emits
//     scale = (|w|+eps) / sqrt(var_biased + eps),  shift = b - mean*scale
// and updates running_mean / running_var (momentum, unbiased variance) like F.batch_norm does.
// ---------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void abn_partial_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ part, const int* __restrict__ run_if = nullptr)
{
    if (run_if && *run_if == 0) return;                          // fp32 half of a guarded sequence (mvsnerf_sweep_conv0_guarded_fwd)
    // thread t handles channel group (t % (C/4)) of voxels t / (C/4) + k*stride  -> float4 loads, fully coalesced
    constexpr int G = C / 4;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)gridDim.x * blockDim.x;
    const int g = (int)(t % G);
    f32x4 s = {0, 0, 0, 0}, q = {0, 0, 0, 0};
    for (int64_t v = t / G; v < n; v += total / G) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + v * C + g * 4);
        s += a; q += a * a;
    }
    // block reduce: threads with equal g (stride G in threadIdx since 256 % G == 0)
    __shared__ float sh[256 * 8];
#pragma unroll
    for (int k = 0; k < 4; ++k) { sh[threadIdx.x * 8 + k] = s[k]; sh[threadIdx.x * 8 + 4 + k] = q[k]; }
    __syncthreads();
    if (threadIdx.x < C * 2) {
        const int c = threadIdx.x % C, which = threadIdx.x / C;     // which: 0 sum, 1 sumsq
        const int gg = c / 4, k = c % 4;
        float acc = 0.f;
        for (int j = gg; j < 256; j += G) acc += sh[j * 8 + which * 4 + k];
        part[abn_part_at(which, c, C, blockIdx.x, gridDim.x)] = acc;
    }
}

__global__ __launch_bounds__(1024) void abn_finalize_kernel(const float* __restrict__ part, int nblocks, int C, int64_t n,
                                    const float* __restrict__ weight, const float* __restrict__ bias,
                                    float* __restrict__ running_mean, float* __restrict__ running_var,
                                    float momentum, float eps, float* __restrict__ scale, float* __restrict__ shift,
                                    float* __restrict__ mean_out, float* __restrict__ invstd_out)
{
    // one workgroup of 1024 threads per channel: thread t adds the partials of slots t, t+1024, ... - two contiguous runs of the
    // channel-major partial array (abn_part_at), four independent loads in flight per run (a full-resolution layer has ~9 k slots: three
    // rounds; 256 threads needed nine, each a round trip to L2) - then a shuffle tree inside the wave and the 16 wave sums in a fixed
    // order (deterministic), fp64 throughout
    const int c = blockIdx.x, t = threadIdx.x;
    const float* ps = part + abn_part_at(0, c, C, 0, nblocks);
    const float* pq = part + abn_part_at(1, c, C, 0, nblocks);
    double s = 0.0, q = 0.0;
    int b = t;
    for (; b + 3072 < nblocks; b += 4096) {
        const float s0 = ps[b], s1 = ps[b + 1024], s2 = ps[b + 2048], s3 = ps[b + 3072];
        const float q0 = pq[b], q1 = pq[b + 1024], q2 = pq[b + 2048], q3 = pq[b + 3072];
        s += ((double)s0 + (double)s1) + ((double)s2 + (double)s3);
        q += ((double)q0 + (double)q1) + ((double)q2 + (double)q3);
    }
    {   // the (up to three) remaining rounds: all loads first
        float sv[3] = {0.f, 0.f, 0.f}, qv[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (b + k * 1024 < nblocks) { sv[k] = ps[b + k * 1024]; qv[k] = pq[b + k * 1024]; }
        s += ((double)sv[0] + (double)sv[1]) + (double)sv[2];
        q += ((double)qv[0] + (double)qv[1]) + (double)qv[2];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { s += __shfl_xor(s, d); q += __shfl_xor(q, d); }
    __shared__ double rs[16], rq[16];
    if ((t & 63) == 0) { rs[t >> 6] = s; rq[t >> 6] = q; }
    __syncthreads();
    if (t != 0) return;
    s = 0.0; q = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { s += rs[w]; q += rq[w]; }
    const double mean = s / (double)n;
    double var = q / (double)n - mean * mean;
    if (var < 0.0) var = 0.0;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float gamma = fabsf(weight[c]) + eps;                    // InPlaceABN: |weight| + eps
    const float sc = gamma * invstd;
    scale[c] = sc;
    shift[c] = bias[c] - (float)mean * sc;
    if (mean_out) { mean_out[c] = (float)mean; invstd_out[c] = invstd; }
    if (running_mean) {
        running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * (float)mean;
        const double unb = n > 1 ? var * (double)n / (double)(n - 1) : var;
        running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)unb;
    }
}

int mvs_abn_partial(const float* x, int64_t n, int C, int slots, float* part, const int* run_if, hipStream_t st)
{
    switch (C) {
        case 8:  abn_partial_kernel<8><<<slots, 256, 0, st>>>(x, n, part, run_if); break;
        case 16: abn_partial_kernel<16><<<slots, 256, 0, st>>>(x, n, part, run_if); break;
        case 32: abn_partial_kernel<32><<<slots, 256, 0, st>>>(x, n, part, run_if); break;
        case 64: abn_partial_kernel<64><<<slots, 256, 0, st>>>(x, n, part, run_if); break;
        default: return MVSNERF_EUNSUPPORTED;
    }
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// (Measured and dropped: folding this kernel into abn_partial_kernel through a "last workgroup finalizes" ticket.  With an agent-scope
// release fence per workgroup the 5 us partial kernel took 60 us (one L2 write-back per workgroup); with write-through partial stores and
// a parallel read by the last workgroup 20 us - the last workgroup reads nb x 2C partials that no cache holds, alone, after everybody
// else has left.  Two small launches, 5 + 5.5 us, are faster.)
extern "C" size_t mvsnerf_abn_workspace_floats(int C) { return (size_t)1024 * 2 * C + 2 * C; }

extern "C" int mvsnerf_abn_stats(const float* x, int64_t n_vox, int C, const float* weight, const float* bias,
                                 float* running_mean, float* running_var, float momentum, float eps,
                                 float* scale, float* shift, float* mean_out, float* invstd_out, float* workspace, void* stream)
{
    if (!x || !weight || !bias || !scale || !shift || !workspace || n_vox < 1) return MVSNERF_EINVAL;
    if ((running_mean == nullptr) != (running_var == nullptr)) return MVSNERF_EINVAL;
    if (!mvs_aligned16(x)) return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    int nb = (int)((n_vox * (C / 4) + 255) / 256);
    if (nb > 1024) nb = 1024;
    if (const int rc = mvs_abn_partial(x, n_vox, C, nb, workspace, nullptr, st)) return rc;
    abn_finalize_kernel<<<C, 1024, 0, st>>>(workspace, nb, C, n_vox, weight, bias, running_mean, running_var, momentum, eps, scale, shift, mean_out, invstd_out);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// stage 2 alone, for producers that leave the per-workgroup sums themselves (part[({sum, sum of squares} * C + c) * n_blocks + b], b < n_blocks)
extern "C" int mvsnerf_abn_finalize(const float* part, int n_blocks, int C, int64_t n_vox, const float* weight, const float* bias,
                                    float* running_mean, float* running_var, float momentum, float eps,
                                    float* scale, float* shift, float* mean_out, float* invstd_out, void* stream)
{
    if (!part || n_blocks < 1 || C < 1 || n_vox < 1 || !weight || !bias || !scale || !shift) return MVSNERF_EINVAL;
    if ((running_mean == nullptr) != (running_var == nullptr)) return MVSNERF_EINVAL;
    abn_finalize_kernel<<<C, 1024, 0, (hipStream_t)stream>>>(part, n_blocks, C, n_vox, weight, bias, running_mean, running_var, momentum, eps, scale, shift,
                                                            mean_out, invstd_out);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// out = leaky(x1*scale1+shift1) [+ leaky(x2*scale2+shift2)]  (materialises an activated tensor, e.g. the final
// 8-channel neural volume  conv0 + conv11(x), models.py:766)
__global__ __launch_bounds__(256) void abn_apply_add_kernel(ActSrc a, ActSrc b, int64_t n4, int C, float* __restrict__ out)
{
    // a thread keeps its channel group for the whole grid-stride walk (the stride is a multiple of C/4), so the per-channel
    // (scale, shift) are loaded once and no 64-bit modulo sits on the streaming path (the first version did one per float4
    // and ran at 1.7 TB/s)
    const int g4 = C >> 2;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;          // multiple of 256, hence of g4 (C in {8,16,32,64})
    const int c = (int)(t0 % g4) * 4;
    f32x4 sa, ha, sb = {0, 0, 0, 0}, hb = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) { sa[k] = a.scale[c + k]; ha[k] = a.shift[c + k]; if (b.x) { sb[k] = b.scale[c + k]; hb[k] = b.shift[c + k]; } }
    for (int64_t i = t0; i < n4; i += stride) {
        f32x4 v = *reinterpret_cast<const f32x4*>(a.x + i * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = act_apply(v[k], sa[k], ha[k]);
        if (b.x) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(b.x + i * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] += act_apply(t[k], sb[k], hb[k]);
        }
        *reinterpret_cast<f32x4*>(out + i * 4) = v;
    }
}

extern "C" int mvsnerf_abn_apply_add(const float* x1, const float* scale1, const float* shift1,
                                     const float* x2, const float* scale2, const float* shift2,
                                     int64_t n_vox, int C, float* out, void* stream)
{
    if (!x1 || !scale1 || !shift1 || !out || n_vox < 1 || (C & 3) || (1024 % C)) return MVSNERF_EINVAL;
    if (x2 && (!scale2 || !shift2)) return MVSNERF_EINVAL;
    if (!mvs_aligned16(x1) || !mvs_aligned16(out) || (x2 && !mvs_aligned16(x2))) return MVSNERF_EALIGN;
    const ActSrc a{x1, scale1, shift1}, b{x2, scale2, shift2};
    const int64_t n4 = n_vox * C / 4;
    const unsigned nblk = mvs_cdiv(n4, 256) < 8192u ? mvs_cdiv(n4, 256) : 8192u;       // <= 32 workgroups per CU, grid-stride beyond
    abn_apply_add_kernel<<<nblk, 256, 0, (hipStream_t)stream>>>(a, b, n4, C, out);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// The 8-channel sum of two lazily-activated tensors, written DEPTH-FASTEST: a, b [D][H][W][8] -> out[H][W][D][8] (MVSNERF_VOL_HWDC, the
// layout the ray march reads best: sample_dev.h).  A workgroup owns a tile of 32 depth planes x 16 x-columns of one row y: it reads 32
// runs of 512 B (along x), applies leaky(x * scale + shift) to both operands, adds, parks the tile in LDS and writes 16 runs of 1 KB (along
// depth): 82 us at config 2, what the channel-last epilogue takes for the same 450 MB (78 us); a 32 x 32 tile (34 KB of LDS, four
// workgroups per CU instead of nine) took 101 us.  Both sides of the transpose are contiguous; nothing else differs from abn_apply_add_kernel (same operation order per element).
__global__ __launch_bounds__(256) void abn_apply_add_hwdc_kernel(ActSrc a, ActSrc b, int D, int H, int W, float* __restrict__ out)
{
    constexpr int TZ = 32, TX = 16, ROW = TX * 8 + 8;             // LDS row of a depth plane: 128 floats + 8 pad (spreads the column reads over the banks)
    __shared__ __attribute__((aligned(16))) float tile[TZ * ROW];
    const int nbx = (W + TX - 1) / TX, nbz = (D + TZ - 1) / TZ;
    const int bx = blockIdx.x % nbx, bz = (blockIdx.x / nbx) % nbz, y = blockIdx.x / (nbx * nbz);
    const int x0 = bx * TX, z0 = bz * TZ;
    const int tid = threadIdx.x;
    const int c4 = (tid & 1) * 4;                                  // this thread's channel quad, in both phases
    f32x4 sa, ha, sb = {0, 0, 0, 0}, hb = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) { sa[k] = a.scale[c4 + k]; ha[k] = a.shift[c4 + k]; if (b.x) { sb[k] = b.scale[c4 + k]; hb[k] = b.shift[c4 + k]; } }
    // phase 1: float4 number f of the tile = (plane f / 32, column (f % 32) / 2, quad f % 2): consecutive threads read consecutive 16 bytes
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int f = tid + 256 * r, zi = f >> 5, xi = (f & 31) >> 1;
        const int z = z0 + zi, x = x0 + xi;
        if (z < D && x < W) {
            const int64_t at = ((((int64_t)z * H + y) * W + x) << 3) + c4;
            f32x4 v = *reinterpret_cast<const f32x4*>(a.x + at);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = act_apply(v[k], sa[k], ha[k]);
            if (b.x) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(b.x + at);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] += act_apply(t[k], sb[k], hb[k]);
            }
            *reinterpret_cast<f32x4*>(tile + zi * ROW + xi * 8 + c4) = v;
        }
    }
    __syncthreads();
    // phase 2: float4 number f = (column f / 64, plane (f % 64) / 2, quad f % 2): consecutive threads write consecutive 16 bytes of a column's run
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int f = tid + 256 * r, xi = f >> 6, zi = (f & 63) >> 1;
        const int z = z0 + zi, x = x0 + xi;
        if (z < D && x < W)
            *reinterpret_cast<f32x4*>(out + (((((int64_t)y * W + x) * D + z) << 3) + c4)) = *reinterpret_cast<const f32x4*>(tile + zi * ROW + xi * 8 + c4);
    }
}

extern "C" int mvsnerf_abn_apply_add_hwdc(const float* x1, const float* scale1, const float* shift1,
                                          const float* x2, const float* scale2, const float* shift2,
                                          int D, int H, int W, float* out, void* stream)
{
    if (!x1 || !scale1 || !shift1 || !out || D < 1 || H < 1 || W < 1) return MVSNERF_EINVAL;
    if (x2 && (!scale2 || !shift2)) return MVSNERF_EINVAL;
    if (!mvs_aligned16(x1) || !mvs_aligned16(out) || (x2 && !mvs_aligned16(x2))) return MVSNERF_EALIGN;
    const ActSrc a{x1, scale1, shift1}, b{x2, scale2, shift2};
    const int64_t nblk = (int64_t)((W + 15) / 16) * ((D + 31) / 32) * H;
    if (nblk >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    abn_apply_add_hwdc_kernel<<<(unsigned)nblk, 256, 0, (hipStream_t)stream>>>(a, b, D, H, W, out);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// ---- train-mode InPlaceABN backward (generalizable training, train_mvs_nerf_pl.py:104-168).  y = leaky(g*xhat + b), xhat = (x-mean)*invstd, g = |w|+eps.
//   gp = gy * leaky'(pre);  S1 = sum gp;  S2 = sum gp*xhat
//   gx = g*invstd * (gp - S1/n - xhat*S2/n);   d b = S1;  d w = sign(w) * S2
// gy may be the sum of two upstream tensors (U-Net skips fan out).
template <int C>
__global__ __launch_bounds__(256) void abn_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd,
                                                             const float* __restrict__ g1, const float* __restrict__ g2, int64_t n, float* __restrict__ part)
{
    constexpr int G = C / 4;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)gridDim.x * blockDim.x;
    const int g = (int)(t % G);
    f32x4 sc, sh, mu, is;
#pragma unroll
    for (int k = 0; k < 4; ++k) { sc[k] = scale[g * 4 + k]; sh[k] = shift[g * 4 + k]; mu[k] = mean[g * 4 + k]; is[k] = invstd[g * 4 + k]; }
    f32x4 s = {0, 0, 0, 0}, q = {0, 0, 0, 0};
    for (int64_t v = t / G; v < n; v += total / G) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + v * C + g * 4);
        f32x4 gy = *reinterpret_cast<const f32x4*>(g1 + v * C + g * 4);
        if (g2) gy += *reinterpret_cast<const f32x4*>(g2 + v * C + g * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float pre = fmaf(a[k], sc[k], sh[k]);
            const float gp = pre > 0.f ? gy[k] : 0.01f * gy[k];
            s[k] += gp;
            q[k] += gp * ((a[k] - mu[k]) * is[k]);
        }
    }
    __shared__ float shm[256 * 8];
#pragma unroll
    for (int k = 0; k < 4; ++k) { shm[threadIdx.x * 8 + k] = s[k]; shm[threadIdx.x * 8 + 4 + k] = q[k]; }
    __syncthreads();
    if (threadIdx.x < C * 2) {
        const int c = threadIdx.x % C, which = threadIdx.x / C;
        const int gg = c / 4, k = c % 4;
        float acc = 0.f;
        for (int j = gg; j < 256; j += G) acc += shm[j * 8 + which * 4 + k];
        part[abn_part_at(which, c, C, blockIdx.x, gridDim.x)] = acc;
    }
}

__global__ __launch_bounds__(64) void abn_bwd_finalize_kernel(const float* __restrict__ part, int nblocks, int C, int64_t n,
                                                             const float* __restrict__ weight, float* __restrict__ m1, float* __restrict__ m2,
                                                             float* __restrict__ g_weight, float* __restrict__ g_bias)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    const float* ps = part + abn_part_at(0, c, C, 0, nblocks);
    const float* pq = part + abn_part_at(1, c, C, 0, nblocks);
    double s = 0.0, q = 0.0;
    int b = lane;
    for (; b + 192 < nblocks; b += 256) {                              // contiguous runs (channel-major partials), four loads in flight
        const float s0 = ps[b], s1 = ps[b + 64], s2 = ps[b + 128], s3 = ps[b + 192];
        const float q0 = pq[b], q1 = pq[b + 64], q2 = pq[b + 128], q3 = pq[b + 192];
        s += ((double)s0 + (double)s1) + ((double)s2 + (double)s3);
        q += ((double)q0 + (double)q1) + ((double)q2 + (double)q3);
    }
    for (; b < nblocks; b += 64) { s += (double)ps[b]; q += (double)pq[b]; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { s += __shfl_xor(s, d); q += __shfl_xor(q, d); }
    if (lane != 0) return;
    m1[c] = (float)(s / (double)n);
    m2[c] = (float)(q / (double)n);
    g_bias[c] = (float)s;
    g_weight[c] = weight[c] < 0.f ? -(float)q : (float)q;          // d|w|/dw
}

template <int C>
__global__ __launch_bounds__(256) void abn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ g1, const float* __restrict__ g2,
                                                           const float* __restrict__ m1, const float* __restrict__ m2, int64_t n4, float* __restrict__ gx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)((i * 4) % C);
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + i * 4);
    f32x4 gy = *reinterpret_cast<const f32x4*>(g1 + i * 4);
    if (g2) gy += *reinterpret_cast<const f32x4*>(g2 + i * 4);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float pre = fmaf(a[k], scale[c + k], shift[c + k]);
        const float gp = pre > 0.f ? gy[k] : 0.01f * gy[k];
        const float xh = (a[k] - mean[c + k]) * invstd[c + k];
        o[k] = scale[c + k] * (gp - m1[c + k] - xh * m2[c + k]);
    }
    *reinterpret_cast<f32x4*>(gx + i * 4) = o;
}

extern "C" int mvsnerf_abn_bwd(const float* x, int64_t n_vox, int C, const float* weight, const float* scale, const float* shift,
                               const float* mean, const float* invstd, const float* g1, const float* g2,
                               float* gx, float* g_weight, float* g_bias, float* workspace, void* stream)
{
    if (!x || !weight || !scale || !shift || !mean || !invstd || !g1 || !gx || !g_weight || !g_bias || !workspace || n_vox < 1) return MVSNERF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int nb = (int)((n_vox * (C / 4) + 255) / 256);
    if (nb > 1024) nb = 1024;
    float* m1 = workspace + (size_t)1024 * 2 * C;       // workspace: mvsnerf_abn_workspace_floats(C) + 2*C
    float* m2 = m1 + C;
    const int64_t n4 = n_vox * C / 4;
#define MVS_ABNB(CC)                                                                                                            \
    abn_bwd_partial_kernel<CC><<<nb, 256, 0, st>>>(x, scale, shift, mean, invstd, g1, g2, n_vox, workspace);                        \
    abn_bwd_finalize_kernel<<<CC, 64, 0, st>>>(workspace, nb, CC, n_vox, weight, m1, m2, g_weight, g_bias);                         \
    abn_bwd_apply_kernel<CC><<<mvs_cdiv(n4, 256), 256, 0, st>>>(x, scale, shift, mean, invstd, g1, g2, m1, m2, n4, gx)
    switch (C) {
        case 8:  MVS_ABNB(8); break;
        case 16: MVS_ABNB(16); break;
        case 32: MVS_ABNB(32); break;
        case 64: MVS_ABNB(64); break;
        default: return MVSNERF_EUNSUPPORTED;
    }
#undef MVS_ABNB
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
