// Weight gradients of CostRegNet's convolutions: the VALU row kernel (the shapes without a matrix-core kernel in wgrad_mfma.hip), the
// multi-job reduction of the partial results a training step leaves (kernels: act.h), and the entries of conv0's blocked weight gradient
// (kernel: conv_mfma.hip).
#include "common.h"
#include "act.h"
#include "conv.h"

// ---- weight gradient of a k3 convolution (stride S, padding 1):
//   gW[a][b][tap] = sum_o G[o][a] * X[o*S - 1 + tap][b]
// G lives on the conv's OUTPUT grid (A channels), X on its INPUT grid (B channels).  For Conv3d G = grad of the raw
// output and X = the (lazily activated) input; for ConvTranspose3d the roles swap (G = activated coarse input,
// X = grad of the fine raw output) and the result is already in ConvTranspose3d's (Cin,Cout,27) layout.
// Organisation: a lane owns one (dz,dy) tap row x 4 consecutive input channels (one 16-byte vector of X) and
// accumulates all 3 dx taps x 4 channels x 8 `a` channels = 96 sums in registers while it walks ONE output row along x.
// Walking along x the three dx taps slide over the same X vectors, so a step costs one new 16-byte X load (two for
// stride 2) and one 32-byte G load per 96 FMAs (the pair-per-thread predecessor did one 4-byte load per 8 FMAs and
// ran at 7.5 TFLOP/s).  npr = 9*ceil(B/4) lanes cover one output row; a 256-thread workgroup carries R = 256/npr rows
// at a time and grid-strides over row groups; every (workgroup,row slot) leaves one partial that stage 2 reduces.
__device__ __forceinline__ f32x4 wg_load_x(const ActSrc& x1, const ActSrc& x2, const float* p1, const float* p2, int ix, int Wi, int ldx, bool row_ok,
                                           const f32x4& s1, const f32x4& h1, const f32x4& s2, const f32x4& h2)
{
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row_ok && (unsigned)ix < (unsigned)Wi) {
        v = *reinterpret_cast<const f32x4*>(p1 + (int64_t)ix * ldx);
        if (x1.scale) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = act_apply(v[k], s1[k], h1[k]);
        }
        if (x2.x) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p2 + (int64_t)ix * ldx);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] += act_apply(t[k], s2[k], h2[k]);
        }
    }
    return v;
}

struct G8 { f32x4 lo, hi; };

__device__ __forceinline__ G8 wg_load_g(const ActSrc& g1, const ActSrc& g2, const float* p1, const float* p2, int ox, int Wo, int A, int a0, bool live)
{
    G8 g{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (live && ox < Wo) {
        g.lo = *reinterpret_cast<const f32x4*>(p1 + (int64_t)ox * A);
        g.hi = *reinterpret_cast<const f32x4*>(p1 + (int64_t)ox * A + 4);
        if (g1.scale) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { g.lo[k] = act_apply(g.lo[k], g1.scale[a0 + k], g1.shift[a0 + k]); g.hi[k] = act_apply(g.hi[k], g1.scale[a0 + 4 + k], g1.shift[a0 + 4 + k]); }
        }
        if (g2.x) {
            const f32x4 tl = *reinterpret_cast<const f32x4*>(p2 + (int64_t)ox * A), th = *reinterpret_cast<const f32x4*>(p2 + (int64_t)ox * A + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) { g.lo[k] += act_apply(tl[k], g2.scale[a0 + k], g2.shift[a0 + k]); g.hi[k] += act_apply(th[k], g2.scale[a0 + 4 + k], g2.shift[a0 + 4 + k]); }
        }
    }
    return g;
}

// Built without packed fp32 instructions: with them the compiler broadcasts w[k] through `v_pk_fma_f32 ... op_sel:[0,1,0]` (the high half of src1 feeding
// the low result), the one packed form that returns wrong values in lanes 48-63 while the fp16x3 conv0 runs on another stream
// (profiles/r05_pk_fma_opsel_reproducer.txt).  csrc/check_isa.sh fails the build if that form shows up in any code object of the library.
#if defined(__HIP_DEVICE_COMPILE__)
#define MVS_NO_PACKED_FP32 __attribute__((target("no-packed-fp32-ops")))
#else
#define MVS_NO_PACKED_FP32                                  // the host pass does not know the device feature
#endif
template <int S>
__global__ __launch_bounds__(256) MVS_NO_PACKED_FP32 void conv3d_wgrad_rows_kernel(ActSrc g1, ActSrc g2, int A, ActSrc x1, ActSrc x2, int B, int ldx,
                                                               int Do, int Ho, int Wo, int Di, int Hi, int Wi, int nb4, int R,
                                                               float* __restrict__ partial)
{
    const int a0 = blockIdx.y * 8;
    const int npr = nb4 * 9;
    const int r = threadIdx.x / npr, it = threadIdx.x - r * npr;
    const bool active = r < R;
    const int b4 = it % nb4, dyz = it / nb4;
    const int dy = dyz % 3 - 1, dz = dyz / 3 - 1;
    const int c0 = b4 * 4;
    f32x4 s1 = {1, 1, 1, 1}, h1 = {0, 0, 0, 0}, s2 = s1, h2 = h1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + k < B ? c0 + k : B - 1;
        if (x1.scale) { s1[k] = x1.scale[c]; h1[k] = x1.shift[c]; }
        if (x2.x) { s2[k] = x2.scale[c]; h2[k] = x2.shift[c]; }
    }
    float acc[3][4][8];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int a = 0; a < 8; ++a) acc[d][k][a] = 0.f;
    const int nrows = Do * Ho;
    for (int grp = blockIdx.x; grp * R < nrows; grp += gridDim.x) {
        const int row = grp * R + r;
        const bool live = active && row < nrows;
        const int oz = live ? row / Ho : 0, oy = live ? row - oz * Ho : 0;
        const int zi = oz * S + dz, yi = oy * S + dy;
        const bool row_ok = live && (unsigned)zi < (unsigned)Di && (unsigned)yi < (unsigned)Hi;
        const int64_t xoff = row_ok ? (((int64_t)zi * Hi + yi) * Wi) * ldx + c0 : 0;
        const float* px1 = x1.x + xoff;
        const float* px2 = x2.x ? x2.x + xoff : nullptr;
        const int64_t goff = live ? ((int64_t)row * Wo) * A + a0 : 0;
        const float* pg1 = g1.x + goff;
        const float* pg2 = g2.x ? g2.x + goff : nullptr;
#define MVS_LX(ix) wg_load_x(x1, x2, px1, px2, (ix), Wi, ldx, row_ok, s1, h1, s2, h2)
#define MVS_LG(ox) wg_load_g(g1, g2, pg1, pg2, (ox), Wo, A, a0, live)
        f32x4 w0 = MVS_LX(-1), w1 = MVS_LX(0), w2 = MVS_LX(1);
        G8 gc = MVS_LG(0);
#pragma unroll 3                                            // three steps per trip: the sliding window (w0 <- w1 <- w2) renames instead of moving 20 registers per step
        for (int ox = 0; ox < Wo; ++ox) {
            // next step's operands are requested before this step's 96 FMAs
            const G8 gn = MVS_LG(ox + 1);
            f32x4 n1, n2;
            if (S == 1) { n2 = MVS_LX(ox + 2); }
            else        { n1 = MVS_LX(2 * ox + 2); n2 = MVS_LX(2 * ox + 3); }
            const float gv[8] = {gc.lo[0], gc.lo[1], gc.lo[2], gc.lo[3], gc.hi[0], gc.hi[1], gc.hi[2], gc.hi[3]};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int a = 0; a < 8; ++a) {
                    acc[0][k][a] = fmaf(gv[a], w0[k], acc[0][k][a]);
                    acc[1][k][a] = fmaf(gv[a], w1[k], acc[1][k][a]);
                    acc[2][k][a] = fmaf(gv[a], w2[k], acc[2][k][a]);
                }
            if (S == 1) { w0 = w1; w1 = w2; w2 = n2; }
            else        { w0 = w2; w1 = n1; w2 = n2; }
            gc = gn;
        }
#undef MVS_LX
#undef MVS_LG
    }
    if (!active) return;
    // partial[(blockIdx.x*R + r)][a][b][tap], tap = (dz*3 + dy)*3 + dx
    float* po = partial + ((int64_t)(blockIdx.x * R + r) * A + a0) * B * 27;
    const int tap0 = ((dz + 1) * 3 + (dy + 1)) * 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (c0 + k >= B) continue;
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int d = 0; d < 3; ++d) po[((int64_t)a * B + c0 + k) * 27 + tap0 + d] = acc[d][k][a];
    }
}

// number of partial results the workspace is sized for
static int wgrad3d_part_cap(int A, int B)
{
    const int64_t n_out = (int64_t)A * B * 27, by_mem = ((int64_t)16 << 20) / n_out;
    return (int)(by_mem < 2048 ? 2048 : (by_mem > 16384 ? 16384 : by_mem));
}

extern "C" size_t mvsnerf_conv3d_wgrad_workspace_floats(int A, int B) { return (size_t)(wgrad3d_part_cap(A, B) + MVS_RED_SLICES) * A * B * 27; }

extern "C" int mvsnerf_conv3d_wgrad(const float* g1, const float* g1_scale, const float* g1_shift,
                                    const float* g2, const float* g2_scale, const float* g2_shift, int A,
                                    const float* x1, const float* x1_scale, const float* x1_shift,
                                    const float* x2, const float* x2_scale, const float* x2_shift, int B, int ldx,
                                    int Do, int Ho, int Wo, int Di, int Hi, int Wi, int stride,
                                    float* gw, float* workspace, void* stream)
{
    if (!g1 || !x1 || !workspace || A < 8 || (A & 7) || B < 1 || ldx < B || (ldx & 3)) return MVSNERF_EINVAL;
    if (stride != 1 && stride != 2) return MVSNERF_EUNSUPPORTED;
    if (!mvs_aligned16(g1) || !mvs_aligned16(x1) || (g2 && !mvs_aligned16(g2)) || (x2 && !mvs_aligned16(x2))) return MVSNERF_EALIGN;
    const int nb4 = (B + 3) / 4, npr = nb4 * 9;
    if (npr > 256 || (nb4 * 4 > ldx)) return MVSNERF_EUNSUPPORTED;
    const ActSrc G1{g1, g1_scale, g1_shift}, G2{g2, g2_scale, g2_shift}, X1{x1, x1_scale, x1_shift}, X2{x2, x2_scale, x2_shift};
    if (!x2) {                                             // 16 / 32 / 64 `a` channels: matrix cores (wgrad_mfma.hip)
        const int cap = wgrad3d_part_cap(A, B);
        const int rc = mvs_conv3d_wgrad_mfma4(G1, G2, A, X1, X2, B, ldx, Do, Ho, Wo, Di, Hi, Wi, stride, workspace, cap, (hipStream_t)stream);
        if (rc != MVSNERF_EUNSUPPORTED) {
            if (rc != MVSNERF_OK || !gw) return rc;
            const int64_t n_out = (int64_t)A * B * 27;
            mvs_partial_sum(workspace, mvs_conv3d_wgrad_mfma4_parts(A, B, Do, Ho, Wo, stride, cap), n_out, workspace + (size_t)cap * n_out, gw,
                            (hipStream_t)stream);
            MVS_LAUNCH_CHECK();
            return MVSNERF_OK;
        }
    }
    const int R = 256 / npr;
    const int nrows = Do * Ho, ngroups = (nrows + R - 1) / R;
    const int cap = wgrad3d_part_cap(A, B) / R;
    const int nwg = ngroups < cap ? ngroups : cap;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(nwg, A / 8);
    if (stride == 1) conv3d_wgrad_rows_kernel<1><<<grid, 256, 0, st>>>(G1, G2, A, X1, X2, B, ldx, Do, Ho, Wo, Di, Hi, Wi, nb4, R, workspace);
    else             conv3d_wgrad_rows_kernel<2><<<grid, 256, 0, st>>>(G1, G2, A, X1, X2, B, ldx, Do, Ho, Wo, Di, Hi, Wi, nb4, R, workspace);
    MVS_LAUNCH_CHECK();
    if (!gw) return MVSNERF_OK;                            // partials left in `workspace` for mvsnerf_partial_sum_multi
    const int64_t n_out = (int64_t)A * B * 27;
    mvs_partial_sum(workspace, nwg * R, n_out, workspace + (size_t)wgrad3d_part_cap(A, B) * n_out, gw, st);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// number of partial results mvsnerf_conv3d_wgrad leaves at the start of its workspace (rows of A*B*27 floats)
extern "C" int mvsnerf_conv3d_wgrad_parts(int A, int B, int Do, int Ho, int Wo, int stride, int two_x_sources)
{
    if (A < 8 || B < 1) return 0;
    if (!two_x_sources) {
        const int n = mvs_conv3d_wgrad_mfma4_parts(A, B, Do, Ho, Wo, stride, wgrad3d_part_cap(A, B));
        if (n > 0) return n;
    }
    const int npr = ((B + 3) / 4) * 9;
    if (npr > 256) return 0;
    const int R = 256 / npr, ngroups = (Do * Ho + R - 1) / R, cap = wgrad3d_part_cap(A, B) / R;
    return (ngroups < cap ? ngroups : cap) * R;
}

// dst_j[i] = sum_p partial_j[p][i] for n_jobs independent reductions in two launches (host arrays, copied into the kernel arguments).
// scratch: mvsnerf_partial_sum_multi_scratch_floats(sum of n_out) floats.
extern "C" size_t mvsnerf_partial_sum_multi_scratch_floats(int64_t total_n_out) { return (size_t)MVS_RED_SLICES * (size_t)total_n_out; }

extern "C" int mvsnerf_partial_sum_multi(int n_jobs, const float* const* partial, const int* n_part, const int64_t* n_out, float* const* dst,
                                         float* scratch, void* stream)
{
    if (n_jobs < 1 || n_jobs > MVS_PSUM_JOBS || !partial || !n_part || !n_out || !dst || !scratch) return MVSNERF_EINVAL;
    PsumJobs J;
    J.n = n_jobs;
    J.vec4 = 0;
    int b1 = 0, b2 = 0;
    size_t off = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (!partial[j] || !dst[j] || n_part[j] < 1 || n_out[j] < 1) return MVSNERF_EINVAL;
        // scratch + off stays 16-byte aligned as long as every job before this one was a vector job (slices * n_out multiples of 4)
        const bool vec4 = (n_out[j] & 3) == 0 && mvs_aligned16(partial[j]) && mvs_aligned16(dst[j]) && mvs_aligned16(scratch + off);
        if (vec4) J.vec4 |= 1u << j;
        const int gx = mvs_psum_gx(n_out[j], vec4);
        const int chunk = n_part[j] <= MVS_RED_SLICES ? n_part[j] : (n_part[j] + MVS_RED_SLICES - 1) / MVS_RED_SLICES;
        const int slices = (n_part[j] + chunk - 1) / chunk;
        J.partial[j] = partial[j]; J.dst[j] = dst[j]; J.scratch[j] = scratch + off; J.n_out[j] = n_out[j];
        J.n_part[j] = n_part[j]; J.chunk[j] = chunk; J.slices[j] = slices;
        J.blk1[j] = b1; J.blk2[j] = b2;
        b1 += gx * slices;
        b2 += slices > 1 ? gx : 0;
        off += (size_t)slices * (size_t)n_out[j];
    }
    J.blk1[n_jobs] = b1; J.blk2[n_jobs] = b2;
    hipStream_t st = (hipStream_t)stream;
    mvs_partial_sum_multi_kernel<1><<<b1, 256, 0, st>>>(J);
    MVS_LAUNCH_CHECK();
    if (b2 > 0) {
        // stage 2 walks only the jobs that have slices: give the others an empty block range
        mvs_partial_sum_multi_kernel<2><<<b2, 256, 0, st>>>(J);
        MVS_LAUNCH_CHECK();
    }
    return MVSNERF_OK;
}

// conv0's weight gradient with the cost volume in channel blocks of four (what mvsnerf_planesweep_costvar_blocked_fwd writes): matrix
// cores, conv_mfma.hip.  g: gradient of conv0's raw output, channel-last [D][H][W][8].  gw: (8, Cin_real, 3,3,3).  workspace:
// mvsnerf_conv3d_wgrad_workspace_floats(8, Cin_real) floats.  Deterministic (fixed partial-sum order).
extern "C" int mvsnerf_conv3d_c8_blocked_wgrad_parts(int Cin, int Cin_real, int D, int H, int W)
{
    return mvs_conv3d_c8_wgrad4_parts(Cin, D, H, W, wgrad3d_part_cap(8, Cin_real));
}

extern "C" int mvsnerf_conv3d_c8_blocked_wgrad(const float* x_blocked, int Cin, int Cin_real, int D, int H, int W, const float* g, float* gw,
                                               float* workspace, void* stream)
{
    if (!x_blocked || !g || !workspace || D < 1 || H < 1 || W < 1 || Cin < 4 || (Cin & 3) || Cin_real < 1 || Cin_real > Cin || Cin_real <= Cin - 4)
        return MVSNERF_EINVAL;
    if (!mvs_aligned16(x_blocked) || !mvs_aligned16(g)) return MVSNERF_EALIGN;
    if ((int64_t)D * H * W * 8 >= (int64_t)1 << 31) return MVSNERF_EUNSUPPORTED;
    return mvs_conv3d_c8_wgrad4(x_blocked, Cin, Cin_real, D, H, W, g, gw, workspace, wgrad3d_part_cap(8, Cin_real), (hipStream_t)stream);
}
