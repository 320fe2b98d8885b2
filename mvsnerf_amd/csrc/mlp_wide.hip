// Fused Embedder + Renderer_ours / Renderer_linear MLP at netwidth 256 for gfx950, no-grad forward only (reference models.py:145-222, 464-538
// with W = 256: the constructor default and the width of the authors' v2 network, run_batch.py:34).
//
// The 128-wide tile of mlp.hip with the counts of mlp_wide_layout.h: one workgroup = 4 waves = 128 points, each wave owns 32 points for the
// whole network, every layer transposed on v_mfma_f32_32x32x2_f32 with the weights as A operand from LDS and the activations as B operand
// straight from the previous layer's accumulator registers.  464 384 MAC per point at F = 20 (1.85x the 128-wide network's matrix work per
// output, 3.7x per point).
// Registers: 128 accumulators + 128 previous activations + the 128 values of pts_bias(feat), which every layer's epilogue multiplies or adds,
// are 384 per lane, so the kernel runs at one wave per SIMD (the unified 512-entry VGPR/AGPR file) = one workgroup per CU.  The positional
// encoding's operands are evaluated again for layer 5 (the skip connection) instead of being held across layers 1..4.
// LDS: a 256 x 256 layer is 256 KB, so the weights stream through two 64 KB buffers in 31 slabs (pts_bias, layer 0, 4 x 4 for layers 1..4,
// 1 + 4 for layer 5, 4 for feature_linear, 3 for views_linears.0; a sigma-only launch stops after 23): while the MFMAs of slab i run, slab i + 1
// arrives by LDS-DMA, its 16 pieces per wave spread under the k-steps (SlabUnder, mlp_fp32_dev.h); one barrier per slab.  Two buffers and the
// vector block are 139 KB of the CU's 160.
// feature_linear is not folded into views_linears.0 here (mlp_layout.h does that for the 128-wide no-grad kernels); it is 14 % of the matrix work.
#include "common.h"
#include "mlp_wide_layout.h"
#include "mlp_fp32_dev.h"

using namespace mlpw;
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------ pack
struct WidePackArgs {
    const float* w[11];
    const float* b[11];
    int F;
    float add;      // V_ADD
};
// order of w/b: 0..5 pts_linears, 6 pts_bias, 7 feature_linear, 8 alpha_linear, 9 views_linears.0, 10 rgb_linear

__device__ inline void pack_segment_wide(float* __restrict__ dst, const float* __restrict__ W, int ld, int col_off,
                                         int kmap, int steps, int nb, int F, int tid, int nthreads)
{
    const int total = steps * nb * 64;
    for (int i = tid; i < total; i += nthreads) {
        const int j = i & 3;
        const int lane = (i >> 2) & 63;
        const int rest = i >> 8;               // t4*nb + b
        const int b = rest % nb, t = (rest / nb) * 4 + j;
        const int col = kmap_col(kmap, t, lane >> 5, F);
        const int row = b * 32 + (lane & 31);
        dst[i] = col < 0 ? 0.0f : W[(size_t)row * ld + col_off + col];
    }
}

__global__ __launch_bounds__(256) void mlp_pack_wide_kernel(WidePackArgs a, float* __restrict__ packed)
{
    const Layout L = layout(a.F);
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    pack_segment_wide(packed + L.biasw, a.w[6], a.F, 0, K_FEAT, L.fsteps, NB, a.F, tid, nt);
    pack_segment_wide(packed + L.l0, a.w[0], PE_DIM, 0, K_PE, PE_STEPS, NB, a.F, tid, nt);
    for (int i = 0; i < 4; ++i)
        pack_segment_wide(packed + L.l1 + i * seg_floats(ACT_STEPS, NB), a.w[1 + i], WIDTH, 0, K_ACT, ACT_STEPS, NB, a.F, tid, nt);
    pack_segment_wide(packed + L.l5a, a.w[5], WIDTH + PE_DIM, 0, K_PE, PE_STEPS, NB, a.F, tid, nt);        // cat([pts, h]) models.py:205
    pack_segment_wide(packed + L.l5b, a.w[5], WIDTH + PE_DIM, PE_DIM, K_ACT, ACT_STEPS, NB, a.F, tid, nt);
    pack_segment_wide(packed + L.feat, a.w[7], WIDTH, 0, K_ACT, ACT_STEPS, NB, a.F, tid, nt);
    pack_segment_wide(packed + L.views, a.w[9], WIDTH + 3, 0, K_VIEWS, VIEW_STEPS, VIEW_NB, a.F, tid, nt);
    float* v = packed + L.vec;
    for (int i = tid; i < V_TOTAL; i += nt) {
        float x = 0.0f;
        if (i < V_VIEWS) {                       // eight [2][128] bias vectors
            const int which = i >> 8, h = (i >> 7) & 1, q = i & 127;
            const float* src = which == 0 ? a.b[6] : which <= 6 ? a.b[which - 1] : a.b[7];
            x = src[act_n(q, h)];
        } else if (i < V_WA) {                   // views bias [2][64]
            const int k = i - V_VIEWS;
            x = a.b[9][act_n(k & 63, k >> 6)];
        } else if (i < V_BA) {                   // alpha weight [2][128]
            const int k = i - V_WA;
            x = a.w[8][act_n(k & 127, k >> 7)];
        } else if (i < V_WR) {
            x = (i == V_BA) ? a.b[8][0] : (i == V_ADD) ? a.add : 0.0f;
        } else if (i < V_BR) {                   // rgb weight [3][2][64]
            const int k = i - V_WR, c = k >> 7, h = (k >> 6) & 1, q = k & 63;
            x = a.w[10][c * (WIDTH / 2) + act_n(q, h)];
        } else {
            const int c = i - V_BR;
            x = c < 3 ? a.b[10][c] : 0.0f;
        }
        v[i] = x;
    }
}

static bool wide_shape_ok(int F, int width) { return width == WIDTH && F >= MIN_F && F <= MAX_F && !(F & 1); }

extern "C" size_t mvsnerf_mlp_wide_packed_floats(int F, int width)
{
    return wide_shape_ok(F, width) ? layout(F).total : 0;
}

extern "C" int mvsnerf_mlp_pack_wide(const float* const w[11], const float* const b[11], int F, int width, int variant, float* packed, void* stream)
{
    if (!w || !b || !packed || (variant != 0 && variant != 1)) return MVSNERF_EINVAL;
    if (!wide_shape_ok(F, width)) return MVSNERF_EUNSUPPORTED;
    if (!mvs_aligned16(packed)) return MVSNERF_EALIGN;
    WidePackArgs a;
    for (int i = 0; i < 11; ++i) {
        if (!w[i] || !b[i]) return MVSNERF_EINVAL;
        a.w[i] = w[i]; a.b[i] = b[i];
    }
    a.F = F;
    a.add = variant ? 1.0f : 0.0f;
    mlp_pack_wide_kernel<<<256, 256, 0, (hipStream_t)stream>>>(a, packed);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// ------------------------------------------------------------------------------------------ compute
constexpr int WIDE_LDS_FLOATS = 2 * SLAB_FLOATS + V_TOTAL;      // 142 368 bytes

// h = relu(acc * bias) (v0) or relu(acc + bias) (v2, `add`: wave-uniform) over the 128 registers of a 256-wide layer
__device__ __forceinline__ void activate_wide(const f32x16 (&acc)[1][NB], const float (&bias)[ACT_STEPS], float (&h)[ACT_STEPS], bool add)
{
    if (add) {
#pragma unroll
        for (int q = 0; q < ACT_STEPS; q += 2) {
            const f32x2 m2 = f32x2{acc[0][q >> 4][q & 15], acc[0][q >> 4][(q & 15) + 1]} + f32x2{bias[q], bias[q + 1]};   // v_pk_add_f32
            h[q] = fmaxf(m2[0], 0.0f); h[q + 1] = fmaxf(m2[1], 0.0f);
            if ((q & 15) == 14) __builtin_amdgcn_sched_barrier(0);
        }
    } else {
#pragma unroll
        for (int q = 0; q < ACT_STEPS; q += 2) {
            const f32x2 m2 = f32x2{acc[0][q >> 4][q & 15], acc[0][q >> 4][(q & 15) + 1]} * f32x2{bias[q], bias[q + 1]};   // v_pk_mul_f32
            h[q] = fmaxf(m2[0], 0.0f); h[q + 1] = fmaxf(m2[1], 0.0f);
            if ((q & 15) == 14) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// One workgroup = one tile of 128 points.  ALPHA_ONLY: forward_alpha - raw[P][1], stops after layer 5; on a v2 buffer the value is written
// without the ReLU (models.py:507), the full forward keeps it (models.py:525).  ADD: the buffer's variant (V_ADD) as a compile-time constant -
// with both epilogues in one instruction stream the register allocator keeps 22 to 40 values in scratch, with one it keeps none; the kernel
// below reads the flag and runs the matching instantiation.
template <bool ALPHA_ONLY, bool ADD>
__device__ __forceinline__ void mlp_fwd_wide_tile(
    const float* __restrict__ packed, int F, const float* __restrict__ ndc, int ndc_stride,
    const float* __restrict__ feat, int feat_stride, const float* __restrict__ dirs, int dirs_stride,
    int64_t P, int S, float* __restrict__ raw, const int wave, const unsigned tile)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* buf0 = lds;
    float* buf1 = lds + SLAB_FLOATS;
    float* vec = lds + 2 * SLAB_FLOATS;
    constexpr int G = 1;
    constexpr int SL = SLAB_FLOATS;
    constexpr bool add = ADD;
    using Next = SlabUnder<SL>;
    const Layout L = layout(F);
    // The lane number, from the hardware anew (v_mbcnt; volatile, so no copy of it is kept): every phase below - start, a layer, the heads - asks
    // again and derives its LDS addresses, its lane half and its point's index from the answer.  What the thread index would otherwise keep alive
    // through all GEMMs (itself, the half, two LDS base addresses, a 64-bit point index) is five registers more than the 384 above leave.
    // Tail lanes read point P - 1 and store nothing.
    auto lane_now = []() {
        int l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return l;
    };
    auto point_raw = [&](int lane) { return ((int64_t)tile * 4 + wave) * 32 + (lane & 31); };
    auto point = [&](int lane) { const int64_t r = point_raw(lane); return r < P ? r : P - 1; };
    float bias[ACT_STEPS], h[ACT_STEPS];
    auto hq0 = [&](int g, int t) { return h[t]; };
    auto hq1 = [&](int g, int t) { return h[32 + t]; };
    auto hq2 = [&](int g, int t) { return h[64 + t]; };
    auto hq3 = [&](int g, int t) { return h[96 + t]; };
    // The slab to fetch next.  From layer 1 on the segments are contiguous and whole slabs (mlp_wide_layout.h), so the kernel walks one pointer.
    // It passes through an empty asm at every step: handed `packed + constant` sources, the compiler forms the piece addresses of many slabs
    // ahead of time and parks them - 170 scalar registers - in lanes of vector registers, which the 384 above leave no room for either.
    const float* nxt = packed + L.l1;
    auto take = [&]() {
        const float* r = nxt;
        nxt += SL;
        asm volatile("" : "+s"(nxt));
        return r;
    };

  {
    const int lane = lane_now(), half = lane >> 5;
    const int64_t p = point(lane);

    slab_dma(buf0, packed + L.biasw, (int)seg_floats(L.fsteps, NB), wave, lane);           // slab 0: pts_bias
    slab_dma_c<SL>(buf1, packed + L.l0, wave, lane);                                       // slab 1: layer 0
    for (int i = wave * 64 + lane; i < V_TOTAL; i += 256) vec[i] = packed[L.vec + i];
    const float px = ndc[p * ndc_stride + 0], py = ndc[p * ndc_stride + 1], pz = ndc[p * ndc_stride + 2];
    float fv[MAX_F / 2];
    {
        const float* fp = feat + p * feat_stride + half * (F / 2);
#pragma unroll
        for (int i = 0; i < MAX_F / 2; ++i) fv[i] = i < F / 2 ? fp[i] : 0.0f;
    }
    auto pe = [&](int g, int t) { return pe_operand(t, half, px, py, pz); };
    // ---- slab 0: bias = pts_bias(feat)
    slab_sync();
    {
        f32x16 acc[G][NB];
        init_acc<NB, G>(acc, vec + V_BIASG + half * ACT_STEPS);
        auto fb = [&](int g, int t) { return fv[t]; };
        switch (L.fsteps) {
            case 4:  gemm_stage<1, NB, G>(buf0, acc, lane, fb); break;
            case 8:  gemm_stage<2, NB, G>(buf0, acc, lane, fb); break;
            case 12: gemm_stage<3, NB, G>(buf0, acc, lane, fb); break;
            case 16: gemm_stage<4, NB, G>(buf0, acc, lane, fb); break;
            default: gemm_stage<5, NB, G>(buf0, acc, lane, fb); break;
        }
#pragma unroll
        for (int q = 0; q < ACT_STEPS; ++q) bias[q] = acc[0][q >> 4][q & 15];
    }
    // ---- slab 1: layer 0 on the positional encoding
    slab_sync();
    {
        f32x16 acc[G][NB];
        init_acc<NB, G>(acc, vec + V_L0 + half * ACT_STEPS);
        gemm_stage<PE_STEPS / 4, NB, G>(buf1, acc, lane, pe, Next{buf0, take(), wave, lane});
        activate_wide(acc, bias, h, add);
    }
  }
    // ---- layers 1..4: four slabs each (buf0, buf1, buf0, buf1)
#pragma unroll 1
    for (int layer = 1; layer <= 4; ++layer) {
        const int lane = lane_now(), half = lane >> 5;
        f32x16 acc[G][NB];
        slab_sync();
        init_acc<NB, G>(acc, vec + V_L0 + WIDTH * layer + half * ACT_STEPS);
        gemm_stage<8, NB, G>(buf0, acc, lane, hq0, Next{buf1, take(), wave, lane});
        slab_sync();
        gemm_stage<8, NB, G>(buf1, acc, lane, hq1, Next{buf0, take(), wave, lane});
        slab_sync();
        gemm_stage<8, NB, G>(buf0, acc, lane, hq2, Next{buf1, take(), wave, lane});
        slab_sync();
        // next slab: the first quarter of the next layer, or - behind layer 4 - the positional-encoding part of layer 5
        gemm_stage<8, NB, G>(buf1, acc, lane, hq3, Next{buf0, take(), wave, lane});
        activate_wide(acc, bias, h, add);
    }
    // ---- layer 5 on cat([pts, h4]): the encoding's slab (buf0), then four (buf1, buf0, buf1, buf0)
    float sigma;
    {
        // the coordinates again, from memory: the 30 sin/cos are evaluated a second time here instead of 32 operands (or the coordinates) being
        // held across layers 1..4, for which the 384 registers above leave no room
        const int lane = lane_now(), half = lane >> 5;
        const int64_t p5 = point(lane);
        const float qx = ndc[p5 * ndc_stride + 0], qy = ndc[p5 * ndc_stride + 1], qz = ndc[p5 * ndc_stride + 2];
        auto pe5 = [&](int g, int t) { return pe_operand(t, half, qx, qy, qz); };
        f32x16 acc[G][NB];
        slab_sync();
        init_acc<NB, G>(acc, vec + V_L0 + WIDTH * 5 + half * ACT_STEPS);
        gemm_stage<PE_STEPS / 4, NB, G>(buf0, acc, lane, pe5, Next{buf1, take(), wave, lane});
        slab_sync();
        gemm_stage<8, NB, G>(buf1, acc, lane, hq0, Next{buf0, take(), wave, lane});
        slab_sync();
        gemm_stage<8, NB, G>(buf0, acc, lane, hq1, Next{buf1, take(), wave, lane});
        slab_sync();
        gemm_stage<8, NB, G>(buf1, acc, lane, hq2, Next{buf0, take(), wave, lane});
        slab_sync();
        if constexpr (ALPHA_ONLY) gemm_stage<8, NB, G>(buf0, acc, lane, hq3);
        else gemm_stage<8, NB, G>(buf0, acc, lane, hq3, Next{buf1, take(), wave, lane});
        activate_wide(acc, bias, h, add);
        // alpha_linear: a 256-term dot product, 128 terms per lane half
        const float* wa = vec + V_WA + half * ACT_STEPS;
        float part = 0.0f;
#pragma unroll
        for (int q = 0; q < ACT_STEPS; ++q) part = fmaf(wa[q], h[q], part);
        part += __shfl_xor(part, 32);
        sigma = part + vec[V_BA];
        if (!(ALPHA_ONLY && add)) sigma = fmaxf(sigma, 0.0f);
    }
    if constexpr (ALPHA_ONLY) {
        const int lane = lane_now();
        const int64_t q_raw = point_raw(lane);
        if (q_raw < P && lane < 32) raw[q_raw] = sigma;
        return;
    }
    // ---- feature_linear: four slabs (buf1, buf0, buf1, buf0), no activation
    {
        const int lane = lane_now(), half = lane >> 5;
        f32x16 acc[G][NB];
        slab_sync();
        init_acc<NB, G>(acc, vec + V_FEAT + half * ACT_STEPS);
        gemm_stage<8, NB, G>(buf1, acc, lane, hq0, Next{buf0, take(), wave, lane});
        slab_sync();
        gemm_stage<8, NB, G>(buf0, acc, lane, hq1, Next{buf1, take(), wave, lane});
        slab_sync();
        gemm_stage<8, NB, G>(buf1, acc, lane, hq2, Next{buf0, take(), wave, lane});
        slab_sync();
        gemm_stage<8, NB, G>(buf0, acc, lane, hq3, Next{buf1, take(), wave, lane});
#pragma unroll
        for (int q = 0; q < ACT_STEPS; ++q) h[q] = acc[0][q >> 4][q & 15];
    }
    // ---- views_linears.0 on cat([feature, dir]) + the rgb head: 64 + 64 + 4 k-steps of 4 blocks (buf1, buf0, buf1)
    {
        const int lane = lane_now(), half = lane >> 5;
        const int64_t q_raw = point_raw(lane);
        const bool q_live = q_raw < P;
        const int64_t ray = (q_live ? q_raw : P - 1) / S;
        const float d0 = dirs[ray * dirs_stride + 0], d1 = dirs[ray * dirs_stride + 1], d2 = dirs[ray * dirs_stride + 2];
        constexpr int TAIL = (int)seg_floats(VIEW_STEPS, VIEW_NB) - 2 * SL;               // the last 4 k-steps: 4 KB
        f32x16 acc[G][VIEW_NB];
        slab_sync();
        init_acc<VIEW_NB, G>(acc, vec + V_VIEWS + half * 64);
        gemm_stage<16, VIEW_NB, G>(buf1, acc, lane, [&](int g, int t) { return h[t]; }, Next{buf0, take(), wave, lane});
        slab_sync();
        gemm_stage<16, VIEW_NB, G>(buf0, acc, lane, [&](int g, int t) { return h[64 + t]; }, SlabUnder<TAIL>{buf1, take(), wave, lane});
        slab_sync();
        gemm_stage<1, VIEW_NB, G>(buf1, acc, lane, [&](int g, int t) { return t == 0 ? (half ? d1 : d0) : t == 1 ? (half ? 0.0f : d2) : 0.0f; });
        // rgb_linear: three 128-term dot products, 64 terms per lane half
        float rgb[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* wr = vec + V_WR + c * 128 + half * 64;
            float part = 0.0f;
#pragma unroll
            for (int q = 0; q < 64; ++q) part = fmaf(wr[q], fmaxf(acc[0][q >> 4][q & 15], 0.0f), part);
            part += __shfl_xor(part, 32);
            const float x = part + vec[V_BR + c];
            rgb[c] = 1.0f / (1.0f + expf(-x));
        }
        if (q_live && half == 0) *reinterpret_cast<f32x4*>(raw + q_raw * 4) = f32x4{rgb[0], rgb[1], rgb[2], sigma};
    }
}

// The packed buffer names its variant (V_ADD, mlp_wide_layout.h): one scalar load, a workgroup-uniform branch
template <bool ALPHA_ONLY>
__global__ __launch_bounds__(256, 1) void mlp_fwd_wide_kernel(
    const float* __restrict__ packed, int F, const float* __restrict__ ndc, int ndc_stride,
    const float* __restrict__ feat, int feat_stride, const float* __restrict__ dirs, int dirs_stride,
    int64_t P, int S, float* __restrict__ raw)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (packed[layout(F).vec + V_ADD] != 0.0f) mlp_fwd_wide_tile<ALPHA_ONLY, true>(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, P, S, raw, wave, blockIdx.x);
    else mlp_fwd_wide_tile<ALPHA_ONLY, false>(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, P, S, raw, wave, blockIdx.x);
}

// Counted launch: the rows form (S = 1, dense strides) on the first n = min(max(*count, 0), cap) rows, n read on the device.  A
// grid for the capacity; a workgroup whose tile starts at or behind row n returns before any other global load, the others run the tile with
// P = n: the plain kernel's bits at N = n, no row >= n written.  (The tile walk is the DEV probe -DMVS_COUNTED_WALK, never defined in the product
// build: DESIGN.md 4i.)
template <bool ALPHA_ONLY>
__global__ __launch_bounds__(256, 1) void mlp_fwd_wide_counted_kernel(
    const float* __restrict__ packed, int F, const float* __restrict__ ndc, const float* __restrict__ feat, const float* __restrict__ dirs,
    int cap, const int* __restrict__ count, float* __restrict__ raw)
{
    const int n = mvs_counted_rows(count, cap);
#if defined(MVS_COUNTED_WALK)
    const unsigned n_tiles = ((unsigned)n + 127u) / 128u;
    if (blockIdx.x >= n_tiles) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool add = packed[layout(F).vec + V_ADD] != 0.0f;
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (add) mlp_fwd_wide_tile<ALPHA_ONLY, true>(packed, F, ndc, 3, feat, F, dirs, 3, n, 1, raw, wave, tile);
        else mlp_fwd_wide_tile<ALPHA_ONLY, false>(packed, F, ndc, 3, feat, F, dirs, 3, n, 1, raw, wave, tile);
        __syncthreads();
    }
#else
    if (blockIdx.x * 128u >= (unsigned)n) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (packed[layout(F).vec + V_ADD] != 0.0f) mlp_fwd_wide_tile<ALPHA_ONLY, true>(packed, F, ndc, 3, feat, F, dirs, 3, n, 1, raw, wave, blockIdx.x);
    else mlp_fwd_wide_tile<ALPHA_ONLY, false>(packed, F, ndc, 3, feat, F, dirs, 3, n, 1, raw, wave, blockIdx.x);
#endif
}

template <bool AO>
static int launch_mlp_wide_counted(const float* packed, int F, const float* ndc, const float* feat, const float* dirs, int cap, const int* count,
                                   float* raw, hipStream_t st)
{
    const size_t lds_bytes = WIDE_LDS_FLOATS * sizeof(float);
    static unsigned long long lds_cap_set = 0;          // per-device bit mask (common.h)
    if (int rc_ = mvs_raise_lds_cap(reinterpret_cast<const void*>(mlp_fwd_wide_counted_kernel<AO>), (int)lds_bytes, &lds_cap_set)) return rc_;
    unsigned grid = mvs_cdiv(cap, 128);
#if defined(MVS_COUNTED_WALK)
    if (grid > 256u) grid = 256u;
#endif
    mlp_fwd_wide_counted_kernel<AO><<<grid, 256, lds_bytes, st>>>(packed, F, ndc, feat, dirs, cap, count, raw);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

template <bool AO>
static int launch_mlp_wide(const float* packed, int F, const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                           const float* dirs, int dirs_stride, int64_t P, int S, float* raw, hipStream_t st)
{
    const size_t lds_bytes = WIDE_LDS_FLOATS * sizeof(float);
    static unsigned long long lds_cap_set = 0;          // per-device bit mask (common.h)
    if (int rc_ = mvs_raise_lds_cap(reinterpret_cast<const void*>(mlp_fwd_wide_kernel<AO>), (int)lds_bytes, &lds_cap_set)) return rc_;
    mlp_fwd_wide_kernel<AO><<<mvs_cdiv(P, 128), 256, lds_bytes, st>>>(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, P, S, raw);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_mlp_fwd_wide(const float* packed, int F, int width, const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                                    const float* dirs, int dirs_stride, int64_t N, int S, int alpha_only, float* raw, void* stream)
{
    if (!packed || !ndc || !feat || !raw || N < 0 || S < 1 || feat_stride < F || ndc_stride < 3) return MVSNERF_EINVAL;
    if (!alpha_only && (dirs_stride < 3 || !dirs)) return MVSNERF_EINVAL;
    if (!wide_shape_ok(F, width)) return MVSNERF_EUNSUPPORTED;
    if (!mvs_aligned16(packed) || !mvs_aligned16(raw)) return MVSNERF_EALIGN;
    const int64_t P = N * S;
    if (P == 0) return MVSNERF_OK;
    if (P > (int64_t)0x7fffffff * 128) return MVSNERF_EUNSUPPORTED;        // one workgroup per 128 points
    hipStream_t st = (hipStream_t)stream;
    if (alpha_only) return launch_mlp_wide<true>(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, P, S, raw, st);
    return launch_mlp_wide<false>(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, P, S, raw, st);
}

extern "C" int mvsnerf_mlp_fwd_wide_counted(const float* packed, int F, int width, const float* ndc, const float* feat, const float* dirs,
                                            int64_t cap, const int* count, int alpha_only, float* raw, void* stream)
{
    if (!packed || !ndc || !feat || !raw || (!alpha_only && !dirs)) return MVSNERF_EINVAL;
    if (int rc = mvs_counted_args(count, cap)) return rc;
    if (!wide_shape_ok(F, width)) return MVSNERF_EUNSUPPORTED;
    if (!mvs_aligned16(packed) || !mvs_aligned16(raw)) return MVSNERF_EALIGN;
    if (cap == 0) return MVSNERF_OK;
    hipStream_t st = (hipStream_t)stream;
    if (alpha_only) return launch_mlp_wide_counted<true>(packed, F, ndc, feat, dirs, (int)cap, count, raw, st);
    return launch_mlp_wide_counted<false>(packed, F, ndc, feat, dirs, (int)cap, count, raw, st);
}
