// Fused Embedder + Renderer_ours MLP for gfx950 (models.py:17-51, 145-222; renderer.py:42-63).
//
// One workgroup = 4 waves = 128 points; each wave owns 32 points for the whole network.  Every layer
// is computed transposed on v_mfma_f32_32x32x2_f32 (exact fp32 fma chains, 157 TFLOP/s peak) with the
// weights as A operand streamed through a 64 KB LDS buffer and the activations as B operand straight
// from the previous layer's accumulator registers (see mlp_layout.h) - the 86-wide input and all
// 128-wide activations of the reference (~1.5 GB of ATen traffic per 1024x128 batch) never exist in
// memory.  MFMA-bound: 251 392 FLOP per point (the reference network's count; 1 976 MFMAs per wave of 32 points) against 12 B + 4*F B read
// and 16 B written.  With a folded buffer (mvsnerf_mlp_pack_fold, mlp_layout.h) the no-grad kernels run feature_linear and views_linears.0 as one
// affine map: 1 720 MFMAs per wave, 218 624 FLOP per point issued for the same result.
// Renderer_linear (net_type v2, models.py:464-538) is the same network with h = relu(p + bias) for relu(p * bias) and an un-clamped forward_alpha:
// a buffer whose V_ADD is 1.0f (mvsnerf_mlp_pack_fold_variant, mlp_layout.h) selects it in every kernel of this file, the matrix work is identical.
#include "common.h"
#include "mlp_layout.h"
#include "lds_dma.h"
#include "mlp_fp32_dev.h"
#include "sample_dev.h"
#include "composite_wave.h"
#include "march.h"

using namespace mlp;
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------ pack
struct PackArgs {
    const float* w[11];
    const float* b[11];
    int F;
    float add;      // V_ADD: 0.0f = h = relu(p * bias) (Renderer_ours), 1.0f = h = relu(p + bias) (Renderer_linear)
};
// order of w/b: 0..5 pts_linears, 6 pts_bias, 7 feature_linear, 8 alpha_linear, 9 views_linears.0, 10 rgb_linear

__device__ inline void pack_segment(float* __restrict__ dst, const float* __restrict__ W, int ld, int col_off,
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

// FOLD: the fold tail of mlp_layout.h behind the standard buffer and V_FOLD = 1.  One thread per tail element, a sequential double chain over
// j = 0..127 (products of two fp32 values are exact in double, so this is `acc = acc + a*b` in float64, j ascending), rounded to fp32 once.
template <bool FOLD>
__global__ __launch_bounds__(256) void mlp_pack_kernel(PackArgs a, float* __restrict__ packed)
{
    const Layout L = layout(a.F);
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    pack_segment(packed + L.biasw, a.w[6], a.F, 0, K_FEAT, L.fsteps, 4, a.F, tid, nt);
    pack_segment(packed + L.l0, a.w[0], PE_DIM, 0, K_PE, PE_STEPS, 4, a.F, tid, nt);
    pack_segment(packed + L.l1, a.w[1], WIDTH, 0, K_ACT, ACT_STEPS, 4, a.F, tid, nt);
    pack_segment(packed + L.l2, a.w[2], WIDTH, 0, K_ACT, ACT_STEPS, 4, a.F, tid, nt);
    pack_segment(packed + L.l3, a.w[3], WIDTH, 0, K_ACT, ACT_STEPS, 4, a.F, tid, nt);
    pack_segment(packed + L.l4, a.w[4], WIDTH, 0, K_ACT, ACT_STEPS, 4, a.F, tid, nt);
    pack_segment(packed + L.l5a, a.w[5], WIDTH + PE_DIM, 0, K_PE, PE_STEPS, 4, a.F, tid, nt);        // cat([pts, h]) models.py:205
    pack_segment(packed + L.l5b, a.w[5], WIDTH + PE_DIM, PE_DIM, K_ACT, ACT_STEPS, 4, a.F, tid, nt);
    pack_segment(packed + L.feat, a.w[7], WIDTH, 0, K_ACT, ACT_STEPS, 4, a.F, tid, nt);
    pack_segment(packed + L.views, a.w[9], WIDTH + 3, 0, K_VIEWS, VIEW_STEPS, 2, a.F, tid, nt);
    float* v = packed + L.vec;
    for (int i = tid; i < V_TOTAL; i += nt) {
        float x = 0.0f;
        if (i < V_VIEWS) {                       // eight [2][64] bias vectors
            const int which = i >> 7, h = (i >> 6) & 1, q = i & 63;
            const float* src = which == 0 ? a.b[6] : which <= 6 ? a.b[which - 1] : a.b[7];
            x = src[act_n(q, h)];
        } else if (i < V_WA) {                   // views bias [2][32]
            const int k = i - V_VIEWS;
            x = a.b[9][act_n(k & 31, k >> 5)];
        } else if (i < V_BA) {                   // alpha weight [2][64]
            const int k = i - V_WA;
            x = a.w[8][act_n(k & 63, k >> 6)];
        } else if (i < V_WR) {
            x = (i == V_BA) ? a.b[8][0] : (FOLD && i == V_FOLD) ? 1.0f : (i == V_ADD) ? a.add : 0.0f;
        } else if (i < V_BR) {                   // rgb weight [3][2][32]
            const int k = i - V_WR, c = k >> 6, h = (k >> 5) & 1, q = k & 31;
            x = a.w[10][c * 64 + act_n(q, h)];
        } else {
            const int c = i - V_BR;
            x = c < 3 ? a.b[10][c] : 0.0f;
        }
        v[i] = x;
    }
    if constexpr (FOLD) {
        const float* Wv = a.w[9];
        const float* Wf = a.w[7];
        float* fw = packed + fold_views_off(a.F);
        float* fb = packed + fold_bias_off(a.F);
        constexpr int total = (int)seg_floats(VIEW_STEPS, 2);
        for (int i = tid; i < total + 64; i += nt) {
            if (i < total) {                     // as pack_segment(.., K_VIEWS, VIEW_STEPS, 2, ..) on [W' | Wv[:, 128:131]]
                const int lane = (i >> 2) & 63, rest = i >> 8;
                const int t = (rest >> 1) * 4 + (i & 3);
                const int col = kmap_col(K_VIEWS, t, lane >> 5, a.F);
                const float* wrow = Wv + (size_t)((rest & 1) * 32 + (lane & 31)) * (WIDTH + 3);
                float x = 0.0f;
                if (col >= WIDTH) {
                    x = wrow[col];
                } else if (col >= 0) {
                    double acc = 0.0;
                    for (int j = 0; j < WIDTH; ++j) acc = acc + (double)wrow[j] * (double)Wf[j * WIDTH + col];
                    x = (float)acc;
                }
                fw[i] = x;
            } else {
                const int k = i - total, n = act_n(k & 31, k >> 5);
                double acc = (double)a.b[9][n];
                for (int j = 0; j < WIDTH; ++j) acc = acc + (double)Wv[(size_t)n * (WIDTH + 3) + j] * (double)a.b[7][j];
                fb[k] = (float)acc;
            }
        }
    }
}

static size_t off16(int F) { return (layout(F).total + 3) & ~(size_t)3; }

extern "C" size_t mvsnerf_mlp_packed_floats(int F)
{
    if (F < 2 || F > MAX_F || (F & 1)) return 0;
    return off16(F);
}

extern "C" size_t mvsnerf_mlp_packed_fold_floats(int F)
{
    if (F < 2 || F > MAX_F || (F & 1)) return 0;
    return fold_total(F);
}

template <bool FOLD>
static int mlp_pack_impl(const float* const w[11], const float* const b[11], int F, float* packed, void* stream, float add = 0.0f)
{
    if (!w || !b || !packed) return MVSNERF_EINVAL;
    if (F < 2 || F > MAX_F || (F & 1)) return MVSNERF_EUNSUPPORTED;
    if (!mvs_aligned16(packed)) return MVSNERF_EALIGN;
    PackArgs a;
    for (int i = 0; i < 11; ++i) {
        if (!w[i] || !b[i]) return MVSNERF_EINVAL;
        a.w[i] = w[i]; a.b[i] = b[i];
    }
    a.F = F;
    a.add = add;
    mlp_pack_kernel<FOLD><<<64, 256, 0, (hipStream_t)stream>>>(a, packed);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_mlp_pack(const float* const w[11], const float* const b[11], int F, float* packed, void* stream)
{
    return mlp_pack_impl<false>(w, b, F, packed, stream);
}

extern "C" int mvsnerf_mlp_pack_fold(const float* const w[11], const float* const b[11], int F, float* packed, void* stream)
{
    return mlp_pack_impl<true>(w, b, F, packed, stream);
}

// The folded buffer of a given network variant: 0 = Renderer_ours (what the two entries above write), 1 = Renderer_linear (V_ADD = 1.0f,
// mlp_layout.h).  Same size and, but for that one float, the same bits as mvsnerf_mlp_pack_fold.
extern "C" int mvsnerf_mlp_pack_fold_variant(const float* const w[11], const float* const b[11], int F, int variant, float* packed, void* stream)
{
    if (variant != 0 && variant != 1) return MVSNERF_EINVAL;
    return mlp_pack_impl<true>(w, b, F, packed, stream, variant ? 1.0f : 0.0f);
}

// ------------------------------------------------------------------------------------------ compute
constexpr int WBUF_FLOATS = 16384;                      // 64 KB weight stage
constexpr int LDS_FLOATS = WBUF_FLOATS + V_TOTAL;       // + fragment-ordered vectors (5.5 KB)

__device__ __forceinline__ void stage_weights(float* __restrict__ wbuf, const float* __restrict__ src, int n_floats, int tid)
{
    // 256 threads x float4, fully coalesced; n_floats is a multiple of 1024
    const f32x4* s = reinterpret_cast<const f32x4*>(src);
    f32x4* d = reinterpret_cast<f32x4*>(wbuf);
    const int n4 = n_floats >> 2;
#pragma unroll 4
    for (int i = tid; i < n4; i += 256) d[i] = s[i];
}

// ------------------------------------------------------------------------------------------ pipelined forward
// Measured on MI355X: 0.237 ms per 1024x128 batch = 139 TFLOP/s = 88 % of the 157.3 TFLOP/s fp32-MFMA peak; PMC:
// matrix pipes busy 85 % of the kernel's duration (folded: 1 720 MFMAs per wave, 83-85 % busy).  What the rest is: DESIGN.md section 4, "Where the fp32 tile's
// idle matrix-pipe time is" - stretches of a wave's own stream without an MFMA that the partner wave of its SIMD is not there to fill (layer boundaries, the
// start, the lone tail of the two-round grid), and the wave's own VALU instructions, ~5 cycles each wherever they stand: the positional encoding is evaluated once
// per point, shared between the two lanes that hold it (pe_all), and stays in registers across the layer loop.  Negative results kept out of the code: (i) staggering /
// prioritising the two co-resident workgroups of a CU: no change; (ii) reading A fragments straight from L2 (no LDS stage, no
// barriers): 114 TFLOP/s; (iii) 64 points per wave at one wave per SIMD: 114 TFLOP/s.
// Same arithmetic as mlp_fwd_kernel<.., G=1, ..>, different weight logistics: the packed weights are cut into 16 slabs (folded: 14 - feature_linear's two are not
// fetched, the folded views segment takes the place of the plain one)
// of <= 34 KB (half a 128x128 layer = 32 k-steps) that alternate between two LDS buffers.  While the MFMAs of slab i
// run, slab i+1 arrives by LDS-DMA (global_load_lds_dwordx4: no VGPRs, no ds_write pass); one barrier per slab.
constexpr int SLAB_FLOATS = 8704;                        // 34 KB = 34 k-steps x 4 blocks x 64 lanes (views: 68 x 2)
constexpr int PIPE_LDS_FLOATS = 2 * SLAB_FLOATS + V_TOTAL;

// What the one-launch ray march (raymarch_fused_kernel below) adds to a tile: the lookups that produce its input rows, the view direction
// and the compositing.  The volume is depth-fastest (MVSNERF_VOL_HWDC) and every offset fits 32 bits (gather_fits_32bit).
struct RaymarchTileArgs {
    const float* vol; int D, H, W;
    const float* img; int V, IH, IW;            // [V][IH][IW][4]
    const float* w2c; const float* Kmat;        // [V][4][4], [V][3][3]; view 0 is the reference view
    const float* pts; const float* rays_dir;    // [P][3], [N][3]
    float* feat; float* dirs_out;               // input_feat [P][F], dirs_tmp [N][3]
    const float* z; int64_t N; int rays_per_tile;
    CompositeOut o;
};

// Prologue of a tile: the arithmetic of gather_fused_kernel<true, true> (sample.hip) for the tile's 128 samples - quad per sample, two passes
// of 64 samples over the 256 threads, every load of both passes issued before the first is consumed.  The rows go to `stage` (128 x F
// floats of LDS), from which the MLP lanes take their features and the tile's block of `feat` is written (tile_rows_out).
__device__ __forceinline__ void tile_lookups(const unsigned tile, const RaymarchTileArgs& a, const float* __restrict__ ndc, int64_t P, int F,
                                             float* __restrict__ stage)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x, q = tid & 3;
    int r[2];
    bool live[2];
    unsigned p[2];
    ZfastTaps zt[2];
    ColorTap ct[2][2];
    f32x3 tap[2][2][4];
    f32x3 nn[2], pp[2];
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        r[ps] = ps * 64 + (tid >> 2);
        const int64_t p_raw = (int64_t)tile * 128 + r[ps];
        live[ps] = p_raw < P;
        p[ps] = (unsigned)(live[ps] ? p_raw : P - 1);
        nn[ps] = f32x3{ndc[p[ps] * 3 + 0], ndc[p[ps] * 3 + 1], ndc[p[ps] * 3 + 2]};
        pp[ps] = *reinterpret_cast<const f32x3*>(a.pts + p[ps] * 3);              // one 12-byte load
    }
    // this lane's views q and q + 4 (the second one only when V > 4: a uniform branch) are the same in both passes: their matrices travel with
    // the coordinates.  A lane without a view of its own projects into view V - 1 and does not store: the taps are issued without a
    // divergent branch, whose join would make the compiler wait for them there.
    const bool two = a.V > 4;
    const int vk[2] = {q < a.V ? q : a.V - 1, q + 4 < a.V ? q + 4 : a.V - 1};
    float Mv[2][12], Kv[2][9];
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (k == 0 || two) {
#pragma unroll
            for (int i = 0; i < 12; ++i) Mv[k][i] = a.w2c[vk[k] * 16 + i];
#pragma unroll
            for (int i = 0; i < 9; ++i) Kv[k][i] = a.Kmat[vk[k] * 9 + i];
        }
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) zt[ps] = zfast_taps<true>(a.vol, a.D, a.H, a.W, nn[ps][0], nn[ps][1], nn[ps][2], q);
#pragma unroll
    for (int ps = 0; ps < 2; ++ps)
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (k == 0 || two) {
                ct[ps][k] = color_project(pp[ps][0], pp[ps][1], pp[ps][2], Mv[k], Kv[k], a.IW, a.IH);
                color_taps_nhwc4<true, f32x3>(a.img, vk[k], a.IH, a.IW, ct[ps][k], tap[ps][k]);
            }
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        float* srow = stage + r[ps] * F;
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if ((k == 0 || two) && q + 4 * k < a.V) *reinterpret_cast<f32x4*>(srow + 8 + 16 * k + 4 * q) = color_row(ct[ps][k], tap[ps][k]);
        const f32x4 acc = zfast_fold_y0_lane(zt[ps]);                             // valid in the y0 lanes
        if (q < 2) *reinterpret_cast<f32x4*>(srow + q * 4) = acc;
    }
}

// The staged rows of the tile's live samples to input_feat, where they form one contiguous block: 16-byte stores issued after the barrier, so
// that they complete under the first GEMM instead of in front of it.
__device__ __forceinline__ void tile_rows_out(const unsigned tile, float* __restrict__ feat, const float* __restrict__ stage, int64_t P, int F)
{
    const int64_t row0 = (int64_t)tile * 128;
    const int n4 = (int)(P - row0 < 128 ? P - row0 : 128) * (F / 4);
    f32x4* dst = reinterpret_cast<f32x4*>(feat + row0 * F);
    const f32x4* src = reinterpret_cast<const f32x4*>(stage);
    for (int i = threadIdx.x; i < n4; i += 256) dst[i] = src[i];
}

// One tile = 128 points = one workgroup's work; `tile` is the workgroup index in the plain kernel and the loop variable of the predicated one below.
// FUSED (with `fa`): the one-launch ray march - `feat` and `dirs` are not read, the tile produces them; NR > 0: it also composites its rays.
template <bool ALPHA_ONLY, bool SAVE, bool FUSED = false, int NR = 0>
__device__ __forceinline__ void mlp_fwd_pipe_tile(
    const unsigned tile, const float* __restrict__ packed, int F, const float* __restrict__ ndc, int ndc_stride,
    const float* __restrict__ feat, int feat_stride, const float* __restrict__ dirs, int dirs_stride,
    int64_t P, int S, float* __restrict__ raw, float* __restrict__ saved, long long* __restrict__ census, const RaymarchTileArgs* fa = nullptr)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    long long t_start = 0, c_start = 0;
    if (census) { t_start = wall_clock64(); c_start = __builtin_amdgcn_s_memtime(); }
    int stamp_i = 4;
    auto stamp = [&]() { if (census && threadIdx.x == 0 && stamp_i < 16) census[tile * 16 + stamp_i] = wall_clock64(); ++stamp_i; };
    float* buf0 = lds;
    float* buf1 = lds + SLAB_FLOATS;
    float* vec = lds + 2 * SLAB_FLOATS;
    constexpr int G = 1;
    const Layout L = layout(F);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int64_t p_raw = ((int64_t)tile * 4 + wave) * 32 + (lane & 31);
    const bool live = p_raw < P;
    const int64_t p = live ? p_raw : P - 1;
    float* sv = nullptr;
    if (SAVE) sv = saved + ((int64_t)tile * 4 + wave) * (SLOTS_SAVED * 64) + lane;
    auto save = [&](int slot, float v) { if (SAVE) sv[slot * 64] = v; };
    constexpr int HALF = (int)(ACT_STEPS / 2) * 4 * 64;                   // floats of half a 128x128 layer

    // FUSED: the fragment-ordered vectors are loaded first, all at once (their LDS stores wait until after the lookups), so that no wait for
    // them also waits for the weight DMA issued behind them
    constexpr int VEC_PER_THREAD = (V_TOTAL + 255) / 256;
    float vec_pre[VEC_PER_THREAD];
    if constexpr (FUSED) {
#pragma unroll
        for (int k = 0; k < VEC_PER_THREAD; ++k) vec_pre[k] = tid + 256 * k < V_TOTAL ? packed[L.vec + tid + 256 * k] : 0.0f;
    }
    slab_dma(buf0, packed + L.biasw, (int)seg_floats(L.fsteps, 4), wave, lane);          // slab 0
    // FUSED: the lookups' rows are staged behind slab 0 when they fit there (F <= 28), else in buf1, whose slab then waits for them to be read
    const bool l0_first = !FUSED || seg_floats(L.fsteps, 4) + 128 * (size_t)F <= SLAB_FLOATS;
    float* stage = l0_first ? buf0 + seg_floats(L.fsteps, 4) : buf1;
    if (l0_first) slab_dma_c<(int)seg_floats(PE_STEPS, 4)>(buf1, packed + L.l0, wave, lane);   // slab 1 (buf1 is free at tile start)
    if constexpr (FUSED) {
        tile_lookups(tile, *fa, ndc, P, F, stage);
#pragma unroll
        for (int k = 0; k < VEC_PER_THREAD; ++k)
            if (tid + 256 * k < V_TOTAL) vec[tid + 256 * k] = vec_pre[k];
    } else {
        for (int i = tid; i < V_TOTAL; i += 256) vec[i] = packed[L.vec + i];
    }
    const float px = ndc[p * ndc_stride + 0], py = ndc[p * ndc_stride + 1], pz = ndc[p * ndc_stride + 2];
    float fv[MAX_F / 2];
    if constexpr (FUSED) {
        slab_sync();                                                                        // slab 0 and the stage are in LDS
        const float* fp = stage + (wave * 32 + (lane & 31)) * F + half * (F / 2);
#pragma unroll
        for (int i = 0; i < MAX_F / 2; ++i) fv[i] = i < F / 2 ? fp[i] : 0.0f;
        tile_rows_out(tile, fa->feat, stage, P, F);
        if (!l0_first) {
            __syncthreads();                                                                // every wave has its features out of buf1
            slab_dma_c<(int)seg_floats(PE_STEPS, 4)>(buf1, packed + L.l0, wave, lane);
        }
    } else {
        const float* fp = feat + p * feat_stride + half * (F / 2);
#pragma unroll
        for (int i = 0; i < MAX_F / 2; ++i) fv[i] = i < F / 2 ? fp[i] : 0.0f;
    }
    float bias[64], h[64], pe_e[PE_STEPS];
    auto pe = [&](int g, int t) { return pe_e[t]; };
    auto hlo = [&](int g, int t) { return h[t]; };
    auto hhi = [&](int g, int t) { return h[32 + t]; };

    // ---- slab 0: bias = pts_bias(feat)
    if constexpr (!FUSED) slab_sync();
    // A folded buffer (V_FOLD, mlp_layout.h) describes itself: every fp32 no-grad kernel handed it makes the same, wave-uniform choice,
    // read from the LDS copy of the vector block.  The training forward ignores the flag (the backward consumes S_FE), the sigma-only
    // launch never reaches the tail.  The folded bias takes the LDS place of V_VIEWS, which a folded tile does not read (one LDS-DMA
    // dword per lane of wave 0; the slab barriers below cover it).
    constexpr bool MAY_FOLD = !ALPHA_ONLY && !SAVE;
    bool fold = false;
    if constexpr (MAY_FOLD) {
        fold = __builtin_amdgcn_readfirstlane(__float_as_int(vec[V_FOLD])) != 0;
        if (fold && wave == 0) lds_dma_dword(packed + fold_bias_off(F), lds_byte_addr(vec + V_VIEWS), lane * 4);
    }
    // Additive network (V_ADD, mlp_layout.h: Renderer_linear, h = relu(p + bias)): the same kind of self-description, read by every form of
    // this tile - the training forward included, its backward reads the same flag.  Wave-uniform; the multiplicative branch below is the
    // code this kernel always had.
    const bool add = __builtin_amdgcn_readfirstlane(__float_as_int(vec[V_ADD])) != 0;
    stamp();                                                                                // [4] startup done
    {
        f32x16 acc[G][4];
        init_acc<4, G>(acc, vec + V_BIASG + half * 64);
        auto fb = [&](int g, int t) { return fv[t]; };
        switch (L.fsteps) {
            case 4:  gemm_stage<1, 4, G>(buf0, acc, lane, fb); break;
            case 8:  gemm_stage<2, 4, G>(buf0, acc, lane, fb); break;
            case 12: gemm_stage<3, 4, G>(buf0, acc, lane, fb); break;
            case 16: gemm_stage<4, 4, G>(buf0, acc, lane, fb); break;
            default: gemm_stage<5, 4, G>(buf0, acc, lane, fb); break;
        }
#pragma unroll
        for (int q = 0; q < 64; ++q) { bias[q] = acc[0][q >> 4][q & 15]; save(S_BM + q, bias[q]); }
        if (SAVE) {
#pragma unroll
            for (int t = 0; t < 16; ++t) save(S_FV + t, fv[t]);
            if (F > 32) {                          // kernel argument: uniform.  Feature operands 16..19 (zero from F/2 on) go to S_FV_HI (mlp_layout.h)
#pragma unroll
                for (int t = 16; t < MAX_F / 2; ++t) save(S_FV_HI + t - 16, fv[t]);
            }
        }
    }
    stamp();                                                                                // [5] bias gemm done
    // The 32 positional-encoding operands, evaluated once per point (pe_all, mlp_fp32_dev.h) in front of layer 0: its GEMM, layer 5's and the
    // training forward's activation store read these registers.  The lane half is made opaque to the compiler, so that nothing of the encoding
    // is hoisted above the bias GEMM and carried (in the predicated kernel: spilled) across it.  Under the one-launch tile's lookups instead,
    // between the issue of the taps and their use, the 330 instructions cost the same (profiles/pe_packed_summary.txt).
    {
        int half_o = half;
        asm("" : "+v"(half_o));
        pe_all(half_o, px, py, pz, pe_e);
    }
    if (SAVE) {
#pragma unroll
        for (int t = 0; t < PE_STEPS; ++t) save(S_E + t, pe_e[t]);
    }
    // ---- slab 1: layer 0
    slab_sync();
    // FUSED: the rays' directions, wanted by the views GEMM, fetched here - where h is not live yet - by LDS-DMA into the 2 KB of buf0 that no
    // slab from here on reaches (none is longer than HALF in buf0; the staged rows were last read in front of the barrier above): they hold no
    // register meanwhile.  Lane (m, half) fetches component `half` of point m's ray, then component 2: [3][32] (+ 32 unused) per wave.
    float* rdir_lds = buf0 + HALF + wave * 128;
    if constexpr (FUSED) {
        const unsigned ray_of_p = (unsigned)p / (unsigned)S;                                // every offset fits 32 bits
        lds_dma_dword(fa->rays_dir, lds_byte_addr(rdir_lds), (ray_of_p * 3 + half) * 4);
        lds_dma_dword(fa->rays_dir, lds_byte_addr(rdir_lds + 64), (ray_of_p * 3 + 2) * 4);
    }
    {
        f32x16 acc[G][4];
        init_acc<4, G>(acc, vec + V_L0 + half * 64);
        gemm_stage<PE_STEPS / 4, 4, G>(buf1, acc, lane, pe, SlabUnder<HALF>{buf0, packed + L.l1, wave, lane});        // slab 2
        if (add) {
#pragma unroll
            for (int q = 0; q < 64; q += 2) {
                const f32x2 m2 = f32x2{acc[0][q >> 4][q & 15], acc[0][q >> 4][(q & 15) + 1]} + f32x2{bias[q], bias[q + 1]};   // v_pk_add_f32
                h[q] = fmaxf(m2[0], 0.0f); h[q + 1] = fmaxf(m2[1], 0.0f);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 64; q += 2) {
                const f32x2 m2 = f32x2{acc[0][q >> 4][q & 15], acc[0][q >> 4][(q & 15) + 1]} * f32x2{bias[q], bias[q + 1]};   // v_pk_mul_f32
                h[q] = fmaxf(m2[0], 0.0f); h[q + 1] = fmaxf(m2[1], 0.0f);
            }
        }
        if constexpr (SAVE) {
#pragma unroll
            for (int q = 0; q < 64; ++q) save(S_H + q, h[q]);
        }
    }
    stamp();                                                                                // [6] layer 0 done
    // ---- layers 1..4: two slabs each (buf0 then buf1)
#pragma unroll 1
    for (int layer = 1; layer <= 4; ++layer) {
        const float* wl = packed + L.l1 + (size_t)(layer - 1) * seg_floats(ACT_STEPS, 4);
        f32x16 acc[G][4];
        slab_sync();
        init_acc<4, G>(acc, vec + V_L0 + 128 * layer + half * 64);
        gemm_stage<8, 4, G>(buf0, acc, lane, hlo, SlabUnder<HALF>{buf1, wl + HALF, wave, lane});
        slab_sync();
        // next slab: first half of the next layer, or the positional-encoding part of layer 5
        gemm_stage<8, 4, G>(buf1, acc, lane, hhi, SlabUnder<HALF>{buf0, layer < 4 ? wl + 2 * HALF : packed + L.l5a, wave, lane});
        if (add) {
#pragma unroll
            for (int q = 0; q < 64; q += 2) {
                const f32x2 m2 = f32x2{acc[0][q >> 4][q & 15], acc[0][q >> 4][(q & 15) + 1]} + f32x2{bias[q], bias[q + 1]};   // v_pk_add_f32
                h[q] = fmaxf(m2[0], 0.0f); h[q + 1] = fmaxf(m2[1], 0.0f);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 64; q += 2) {
                const f32x2 m2 = f32x2{acc[0][q >> 4][q & 15], acc[0][q >> 4][(q & 15) + 1]} * f32x2{bias[q], bias[q + 1]};   // v_pk_mul_f32
                h[q] = fmaxf(m2[0], 0.0f); h[q + 1] = fmaxf(m2[1], 0.0f);
            }
        }
        if constexpr (SAVE) {
#pragma unroll
            for (int q = 0; q < 64; ++q) save(S_H + layer * 64 + q, h[q]);
        }
        stamp();                                                                            // [7..10] layers 1..4 done
    }
    // ---- layer 5 on cat([pts, h4]): slabs 10 (buf0), 11 (buf1), 12 (buf0)
    float sigma;
    {
        f32x16 acc[G][4];
        slab_sync();
        init_acc<4, G>(acc, vec + V_L0 + 128 * 5 + half * 64);
        gemm_stage<PE_STEPS / 4, 4, G>(buf0, acc, lane, pe, SlabUnder<HALF>{buf1, packed + L.l5b, wave, lane});
        slab_sync();
        gemm_stage<8, 4, G>(buf1, acc, lane, hlo, SlabUnder<HALF>{buf0, packed + L.l5b + HALF, wave, lane});
        slab_sync();
        // next slab: the first half of feature_linear, or - folded - the folded views segment, which fills the buffer (SLAB_FLOATS).  One
        // branch-free DMA of that size serves both (an unfolded tile moves 2 KB of feature_linear's second half it does not read).
        if constexpr (SAVE) gemm_stage<8, 4, G>(buf0, acc, lane, hhi, SlabUnder<HALF>{buf1, packed + L.feat, wave, lane});
        else if constexpr (!ALPHA_ONLY) gemm_stage<8, 4, G>(buf0, acc, lane, hhi, SlabUnder<(int)seg_floats(VIEW_STEPS, 2)>{buf1, packed + (fold ? fold_views_off(F) : L.feat), wave, lane});
        else gemm_stage<8, 4, G>(buf0, acc, lane, hhi);
        if (add) {
#pragma unroll
            for (int q = 0; q < 64; q += 2) {
                const f32x2 m2 = f32x2{acc[0][q >> 4][q & 15], acc[0][q >> 4][(q & 15) + 1]} + f32x2{bias[q], bias[q + 1]};   // v_pk_add_f32
                h[q] = fmaxf(m2[0], 0.0f); h[q + 1] = fmaxf(m2[1], 0.0f);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 64; q += 2) {
                const f32x2 m2 = f32x2{acc[0][q >> 4][q & 15], acc[0][q >> 4][(q & 15) + 1]} * f32x2{bias[q], bias[q + 1]};   // v_pk_mul_f32
                h[q] = fmaxf(m2[0], 0.0f); h[q + 1] = fmaxf(m2[1], 0.0f);
            }
        }
        if constexpr (SAVE) {
#pragma unroll
            for (int q = 0; q < 64; ++q) save(S_H + 5 * 64 + q, h[q]);
        }
        const float* wa = vec + V_WA + half * 64;
        float part = 0.0f;
#pragma unroll
        for (int q = 0; q < 64; ++q) part = fmaf(wa[q], h[q], part);
        part += __shfl_xor(part, 32);
        sigma = part + vec[V_BA];
        // Renderer_linear.forward_alpha returns alpha_linear(h) without the ReLU (its forward keeps it): only a sigma-only launch on an
        // additive buffer writes the un-clamped value
        if (!(ALPHA_ONLY && add)) sigma = fmaxf(sigma, 0.0f);
    }
    stamp();                                                                                // [11] layer 5 + sigma head done
    if (ALPHA_ONLY) {
        if (live && half == 0) raw[p_raw] = sigma;
        return;
    }
    // ---- feature_linear: slabs 13 (buf1), 14 (buf0).  Folded: skipped, the views GEMM below takes h5 and the folded segment already on its way
    if (!fold) {
        f32x16 acc[G][4];
        slab_sync();
        init_acc<4, G>(acc, vec + V_FEAT + half * 64);
        gemm_stage<8, 4, G>(buf1, acc, lane, hlo, SlabUnder<HALF>{buf0, packed + L.feat + HALF, wave, lane});
        slab_sync();
        gemm_stage<8, 4, G>(buf0, acc, lane, hhi, SlabUnder<(int)seg_floats(VIEW_STEPS, 2)>{buf1, packed + L.views, wave, lane});
#pragma unroll
        for (int q = 0; q < 64; ++q) { h[q] = acc[0][q >> 4][q & 15]; save(S_FE + q, h[q]); }
    }
    stamp();                                                                                // [12] feature_linear done
    // ---- views_linears[0] + rgb head: slab 15 (buf1; folded: slab 13)
    {
        // the point's index again, from the lane number: opaque to the compiler, so that the 64-bit values of the prologue are not carried in
        // registers (or spilled) through every GEMM for the few uses below
        int lane_o = lane;
        asm("" : "+v"(lane_o));
        const int64_t p_raw = ((int64_t)tile * 4 + wave) * 32 + (lane_o & 31);
        const bool live = p_raw < P;
        const int64_t p = live ? p_raw : P - 1;
        // compositing in the tile: its 128 z values are one contiguous block, loaded here so that they land under the views GEMM
        float z_pre = 0.0f;
        if constexpr (FUSED && NR > 0)
            if (tid < 128 && (int64_t)tile * 128 + tid < P) z_pre = fa->z[(int64_t)tile * 128 + tid];
        float d0, d1, d2;
        if constexpr (FUSED) {
            // the ray's view direction in registers: with S > 128 a ray spans tiles, so dirs_tmp is written (by the tile holding the ray's
            // first sample) and never read back
            const int64_t ray = (unsigned)p / (unsigned)S;
            const float rdir[3] = {rdir_lds[lane & 31], rdir_lds[32 + (lane & 31)], rdir_lds[64 + (lane & 31)]};
            float rot[11];
#pragma unroll
            for (int i = 0; i < 11; ++i) rot[i] = fa->w2c[i];
            float d[3];
            dir_feature_of(rdir, rot, 1, d);
            d0 = d[0]; d1 = d[1]; d2 = d[2];
            if (live && half == 0 && p_raw == ray * S) { fa->dirs_out[ray * 3 + 0] = d0; fa->dirs_out[ray * 3 + 1] = d1; fa->dirs_out[ray * 3 + 2] = d2; }
        } else {
            const int64_t ray = p / S; d0 = dirs[ray * dirs_stride + 0]; d1 = dirs[ray * dirs_stride + 1]; d2 = dirs[ray * dirs_stride + 2];
        }
        f32x16 acc[G][2];
        slab_sync();
        init_acc<2, G>(acc, vec + V_VIEWS + half * 32);
        gemm_stage<VIEW_STEPS / 4, 2, G>(buf1, acc, lane, [&](int g, int t) {
            return t < ACT_STEPS ? h[t < ACT_STEPS ? t : 0] : t == ACT_STEPS ? (half ? d1 : d0) : t == ACT_STEPS + 1 ? (half ? 0.0f : d2) : 0.0f;
        });
        if (SAVE) {
#pragma unroll
            for (int q = 0; q < 32; ++q) save(S_HV + q, fmaxf(acc[0][q >> 4][q & 15], 0.0f));
            save(S_DR + 0, half ? d1 : d0);
            save(S_DR + 1, half ? 0.0f : d2);
        }
        float rgb[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* wr = vec + V_WR + c * 64 + half * 32;
            float part = 0.0f;
#pragma unroll
            for (int q = 0; q < 32; ++q) part = fmaf(wr[q], fmaxf(acc[0][q >> 4][q & 15], 0.0f), part);
            part += __shfl_xor(part, 32);
            const float x = part + vec[V_BR + c];
            rgb[c] = 1.0f / (1.0f + expf(-x));
        }
        if (live && half == 0) *reinterpret_cast<f32x4*>(raw + p_raw * 4) = f32x4{rgb[0], rgb[1], rgb[2], sigma};
        if constexpr (FUSED && NR > 0) {
            // the tile holds whole rays (128 % S == 0): raw and z staged in buf0 (free since the barrier in front of the views GEMM), then
            // composite_kernel<NR>'s lane ownership - wave w composites the tile's rays w, w + 4, ...
            if (half == 0) reinterpret_cast<f32x4*>(buf0)[wave * 32 + (lane_o & 31)] = f32x4{rgb[0], rgb[1], rgb[2], sigma};
            float* zs = buf0 + 4 * 128;
            if (tid < 128) zs[tid] = z_pre;
            __syncthreads();
            const f32x4* rs = reinterpret_cast<const f32x4*>(buf0);
            for (int rl = wave; rl < fa->rays_per_tile; rl += 4) {
                const int64_t ray = (int64_t)tile * fa->rays_per_tile + rl;
                if (ray >= fa->N) break;                                                    // wave-uniform
                f32x4 rv[NR];
#pragma unroll
                for (int i = 0; i < NR; ++i) {
                    const int s = lane * NR + i;
                    rv[i] = s < S ? rs[rl * S + s] : f32x4{0, 0, 0, 0};
                }
                composite_wave<NR>(rv, zs + rl * S, ray, S, lane, fa->o);
            }
        }
    }
    if (census && tid == 0) {
        census[tile * 16 + 0] = t_start;
        census[tile * 16 + 1] = wall_clock64();
        census[tile * 16 + 2] = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));      // HW_REG_HW_ID
        census[tile * 16 + 3] = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));     // HW_REG_XCC_ID
        census[tile * 16 + 13] = __builtin_amdgcn_s_memtime() - c_start;                      // shader-clock ticks of this workgroup
    }
}

template <bool ALPHA_ONLY, bool SAVE>
__global__ __launch_bounds__(256, 2) void mlp_fwd_pipe_kernel(
    const float* __restrict__ packed, int F, const float* __restrict__ ndc, int ndc_stride,
    const float* __restrict__ feat, int feat_stride, const float* __restrict__ dirs, int dirs_stride,
    int64_t P, int S, float* __restrict__ raw, float* __restrict__ saved, long long* __restrict__ census)
{
    mlp_fwd_pipe_tile<ALPHA_ONLY, SAVE>(blockIdx.x, packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, P, S, raw, saved, census);
}

// Second half of a guarded 16-bit sequence (include/mvsnerf_hip.h): launched behind the fp16x3 kernel, does its work only when that kernel
// reported a value outside fp16's range.  A small persistent grid that walks the tiles: when the guard is clear - the usual case - a few
// hundred workgroups leave at once (the plain kernel's 1024 early exits, each waiting for its 69 KB of LDS, cost ~3 us of every batch);
// when it is set, the same per-tile code runs and the results are the plain kernel's bits.
template <bool ALPHA_ONLY>
__global__ __launch_bounds__(256, 2) void mlp_fwd_pipe_if_kernel(
    const float* __restrict__ packed, int F, const float* __restrict__ ndc, int ndc_stride,
    const float* __restrict__ feat, int feat_stride, const float* __restrict__ dirs, int dirs_stride,
    int64_t P, int S, float* __restrict__ raw, const int* __restrict__ run_if)
{
    if (*run_if == 0) return;
    const unsigned n_tiles = (unsigned)((P + 127) / 128);
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        mlp_fwd_pipe_tile<ALPHA_ONLY, false>(tile, packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, P, S, raw, nullptr, nullptr);
        __syncthreads();                                       // the next tile's first slabs overwrite what the last GEMMs of this one read
    }
}

// Counted launch: the rows form (S = 1: every compact row of ops.live_samples has its own direction row, dense 3 / F / 3 strides)
// on the first n = min(max(*count, 0), cap) rows, n read on the device.  The same tile walk: the grid is sized by the capacity, a workgroup
// walks the ceil(n / 128) tiles the count leaves and one without a tile returns before any other global load (n = 0: all of them).  Each tile is
// mlp_fwd_pipe_tile with P = n - the plain kernel's bits at N = n, and no row >= n is written.  run_if (may be NULL): the guard word of a
// counted guarded sequence, as in mlp_fwd_pipe_if_kernel.
template <bool ALPHA_ONLY>
__global__ __launch_bounds__(256, 2) void mlp_fwd_pipe_counted_kernel(
    const float* __restrict__ packed, int F, const float* __restrict__ ndc, const float* __restrict__ feat, const float* __restrict__ dirs,
    int cap, const int* __restrict__ count, float* __restrict__ raw, const int* __restrict__ run_if)
{
    if (run_if && *run_if == 0) return;
    const int n = mvs_counted_rows(count, cap);
    const unsigned n_tiles = ((unsigned)n + 127u) / 128u;
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        mlp_fwd_pipe_tile<ALPHA_ONLY, false>(tile, packed, F, ndc, 3, feat, F, dirs, 3, n, 1, raw, nullptr, nullptr);
        __syncthreads();                                       // as above: the next tile's first slabs overwrite what this one's last GEMMs read
    }
}

template <bool AO>
static int launch_mlp_pipe_counted(const float* packed, int F, const float* ndc, const float* feat, const float* dirs, int cap, const int* count,
                                   float* raw, const int* run_if, hipStream_t st)
{
    const size_t lds_bytes = PIPE_LDS_FLOATS * sizeof(float);
    static unsigned long long cap_set = 0;
    if (int rc_ = mvs_raise_lds_cap(reinterpret_cast<const void*>(mlp_fwd_pipe_counted_kernel<AO>), (int)lds_bytes, &cap_set)) return rc_;
    const unsigned n_tiles = mvs_cdiv(cap, 128);
    mlp_fwd_pipe_counted_kernel<AO><<<n_tiles < 512u ? n_tiles : 512u, 256, lds_bytes, st>>>(packed, F, ndc, feat, dirs, cap, count, raw, run_if);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

int mvs_mlp_fwd_counted(const float* packed, int F, const float* ndc, const float* feat, const float* dirs, int64_t cap, const int* count,
                        int alpha_only, float* raw, const int* run_if, void* stream)
{
    if (!packed || !ndc || !feat || !raw || (!alpha_only && !dirs)) return MVSNERF_EINVAL;
    if (int rc = mvs_counted_args(count, cap)) return rc;
    if (F < 2 || F > MAX_F || (F & 1)) return MVSNERF_EUNSUPPORTED;
    if (!mvs_aligned16(packed) || !mvs_aligned16(raw)) return MVSNERF_EALIGN;
    if (cap == 0) return MVSNERF_OK;
    if (alpha_only) return launch_mlp_pipe_counted<true>(packed, F, ndc, feat, dirs, (int)cap, count, raw, run_if, (hipStream_t)stream);
    return launch_mlp_pipe_counted<false>(packed, F, ndc, feat, dirs, (int)cap, count, raw, run_if, (hipStream_t)stream);
}

extern "C" int mvsnerf_mlp_fwd_counted(const float* packed, int F, const float* ndc, const float* feat, const float* dirs, int64_t cap,
                                       const int* count, int alpha_only, float* raw, void* stream)
{
    return mvs_mlp_fwd_counted(packed, F, ndc, feat, dirs, cap, count, alpha_only, raw, nullptr, stream);
}

template <bool AO, bool SAVE>
static int launch_mlp_pipe(const float* packed, int F, const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                           const float* dirs, int dirs_stride, int64_t P, int S, float* raw, hipStream_t st, float* saved = nullptr, long long* census = nullptr,
                           const int* run_if = nullptr)
{
    const size_t lds_bytes = PIPE_LDS_FLOATS * sizeof(float);
    if (run_if) {                                       // predicated on a guard word: persistent grid (never with an activation store or a census)
        if constexpr (!SAVE) {
            static unsigned long long cap_if = 0;
            if (int rc_ = mvs_raise_lds_cap(reinterpret_cast<const void*>(mlp_fwd_pipe_if_kernel<AO>), (int)lds_bytes, &cap_if)) return rc_;
            const unsigned n_tiles = mvs_cdiv(P, 128);
            mlp_fwd_pipe_if_kernel<AO><<<n_tiles < 512u ? n_tiles : 512u, 256, lds_bytes, st>>>(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, P, S, raw, run_if);
            MVS_LAUNCH_CHECK();
            return MVSNERF_OK;
        } else {
            return MVSNERF_EINVAL;
        }
    }
    static unsigned long long lds_cap_set = 0;          // per-device bit mask (common.h)
    if (int rc_ = mvs_raise_lds_cap(reinterpret_cast<const void*>(mlp_fwd_pipe_kernel<AO, SAVE>), (int)lds_bytes, &lds_cap_set)) return rc_;
    mlp_fwd_pipe_kernel<AO, SAVE><<<mvs_cdiv(P, 128), 256, lds_bytes, st>>>(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, P, S, raw, saved, census);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// ------------------------------------------------------------------------------------------ one-launch ray march
// mvsnerf_raymarch_fwd's fp32 path in one launch (raymarch.hip): lookups -> MLP -> compositing per 128-sample tile, the same bits as
// mvsnerf_gather_fwd -> mvsnerf_mlp_fwd -> mvsnerf_composite_fwd.  Measured at config 2: 247.5 us against 255 us for the three launches; the two
// workgroups of a CU start their tiles together (two rounds of 512), so the lookups are not hidden behind the partner's GEMMs, they are made
// one round trip deep (tile_lookups).  NR > 0: the tile composites its rays itself (128 % S == 0, NR = ceil(S / 64)).
template <int NR>
__global__ __launch_bounds__(256, 2) void raymarch_fused_kernel(const float* __restrict__ packed, int F, const float* __restrict__ ndc, int64_t P, int S,
                                                                float* __restrict__ raw, RaymarchTileArgs fa)
{
    mlp_fwd_pipe_tile<false, false, true, NR>(blockIdx.x, packed, F, ndc, 3, nullptr, F, nullptr, 3, P, S, raw, nullptr, nullptr, &fa);
}

// mvs_raymarch_fused_applies / mvs_raymarch_fused_fwd (march.h): a batch they do not take - invalid arguments, a DHWC volume, a shape whose
// offsets need 64 bits, another MLP - goes through the launch sequence of march_batch (raymarch.hip), with that sequence's own error codes.
bool mvs_raymarch_fused_applies(const MarchBatch& b)
{
    if (b.packed_bf16 || b.packed_split || b.guard) return false;
    const int F = 8 + 4 * b.V;
    if (b.vol_layout != MVSNERF_VOL_HWDC || !b.vol || !b.imgs_nhwc4 || !b.w2c || !b.K || !b.packed || !b.pts || !b.ndc || !b.z || !b.rays_dir ||
        !b.feat || !b.dirs || !b.raw) return false;
    if (b.D < 1 || b.H < 1 || b.W < 1 || b.V < 1 || F > MAX_F || b.IH < 2 || b.IW < 2 || b.N < 1 || b.S < 1) return false;
    if (!mvs_aligned16(b.feat) || !mvs_aligned16(b.vol) || !mvs_aligned16(b.imgs_nhwc4) || !mvs_aligned16(b.packed) || !mvs_aligned16(b.raw)) return false;
    return gather_fits_32bit(b.D, b.H, b.W, b.V, b.IH, b.IW, b.N * b.S, F);
}

int mvs_raymarch_fused_fwd(const MarchBatch& b, hipStream_t st)
{
    const int F = 8 + 4 * b.V, S = b.S;
    const int64_t P = b.N * S;
    const RaymarchTileArgs fa{b.vol, b.D, b.H, b.W, b.imgs_nhwc4, b.V, b.IH, b.IW, b.w2c, b.K, b.pts, b.rays_dir, b.feat, b.dirs, b.z, b.N,
                              128 % S == 0 ? 128 / S : 0, CompositeOut{b.rgb_map, b.disp, b.acc, b.weights, b.depth, b.alpha, b.white_bkgd, nullptr}};
    const size_t lds_bytes = PIPE_LDS_FLOATS * sizeof(float);
    const unsigned grid = mvs_cdiv(P, 128);
    static unsigned long long cap[3] = {0, 0, 0};
#define MVS_FUSED(NR_)                                                                                                                 \
    do {                                                                                                                               \
        if (int rc_ = mvs_raise_lds_cap(reinterpret_cast<const void*>(raymarch_fused_kernel<NR_>), (int)lds_bytes, &cap[NR_])) return rc_; \
        raymarch_fused_kernel<NR_><<<grid, 256, lds_bytes, st>>>(b.packed, F, b.ndc, P, S, b.raw, fa);                               \
    } while (0)
    if (fa.rays_per_tile == 0) MVS_FUSED(0);
    else if (S <= 64) MVS_FUSED(1);
    else MVS_FUSED(2);
#undef MVS_FUSED
    MVS_LAUNCH_CHECK();
    if (fa.rays_per_tile == 0)                      // a tile holds pieces of rays: the compositing is a launch of its own
        return mvs_composite_fwd(b.raw, b.z, b.N, S, b.white_bkgd, b.rgb_map, b.disp, b.acc, b.weights, b.depth, b.alpha, nullptr, st);
    return MVSNERF_OK;
}

static int mlp_fwd_checked(const float* packed, int F, const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                           const float* dirs, int dirs_stride, int64_t N, int S, int alpha_only, float* raw, void* stream, long long* census,
                           const int* run_if = nullptr)
{
    if (!packed || !ndc || !feat || !raw || N < 0 || S < 1 || feat_stride < F || ndc_stride < 3) return MVSNERF_EINVAL;
    if (!alpha_only && dirs_stride < 3) return MVSNERF_EINVAL;
    if (!alpha_only && !dirs) return MVSNERF_EINVAL;
    if (F < 2 || F > MAX_F || (F & 1)) return MVSNERF_EUNSUPPORTED;
    if (!mvs_aligned16(packed) || !mvs_aligned16(raw)) return MVSNERF_EALIGN;
    const int64_t P = N * S;
    if (P == 0) return MVSNERF_OK;
    hipStream_t st = (hipStream_t)stream;
    if (alpha_only) return launch_mlp_pipe<true, false>(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, P, S, raw, st, nullptr, census, run_if);
    return launch_mlp_pipe<false, false>(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, P, S, raw, st, nullptr, census, run_if);
}

int mvs_mlp_fwd_if(const float* packed, int F, const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                   const float* dirs, int dirs_stride, int64_t N, int S, int alpha_only, float* raw, const int* run_if, void* stream)
{
    return mlp_fwd_checked(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, N, S, alpha_only, raw, stream, nullptr, run_if);
}

extern "C" int mvsnerf_mlp_fwd(const float* packed, int F, const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                               const float* dirs, int dirs_stride, int64_t N, int S, int alpha_only, float* raw, void* stream)
{
    return mlp_fwd_checked(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, N, S, alpha_only, raw, stream, nullptr);
}

// The same launch with a per-workgroup timing record (stateless diagnostics for bench.py's sustained-clock figure): census =
// (N*S + 127) / 128 rows of 16 int64 {start, end (100 MHz wall clock), HW_ID, XCC_ID, phase stamps [4..12], shader-clock ticks [13]}.
extern "C" int mvsnerf_mlp_fwd_census(const float* packed, int F, const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                                      const float* dirs, int dirs_stride, int64_t N, int S, int alpha_only, float* raw, long long* census, void* stream)
{
    if (!census) return MVSNERF_EINVAL;
    return mlp_fwd_checked(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, N, S, alpha_only, raw, stream, census);
}

// Training forward: identical arithmetic to mvsnerf_mlp_fwd (32 points per wave) + the activation store the
// backward pass consumes (mvsnerf_mlp_saved_floats(N*S) floats, slot format of mlp_layout.h).
extern "C" int mvsnerf_mlp_fwd_train(const float* packed, int F, const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                                     const float* dirs, int dirs_stride, int64_t N, int S, float* raw, float* saved, void* stream)
{
    if (!packed || !ndc || !feat || !dirs || !raw || !saved || N < 0 || S < 1 || feat_stride < F || ndc_stride < 3 || dirs_stride < 3) return MVSNERF_EINVAL;
    if (F < 2 || F > MAX_F || (F & 1)) return MVSNERF_EUNSUPPORTED;
    if (!mvs_aligned16(packed) || !mvs_aligned16(raw) || !mvs_aligned16(saved)) return MVSNERF_EALIGN;
    const int64_t P = N * S;
    if (P == 0) return MVSNERF_OK;
    return launch_mlp_pipe<false, true>(packed, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, P, S, raw, (hipStream_t)stream, saved);
}

// ------------------------------------------------------------------------------------------ positional-encoding operands (test entry)
// The tile's 32 B operands of both lane halves, as the two routines of mlp_fp32_dev.h produce them: one wave per 32 points, lane (m, half)
// writes out[p][t][half] for its point p = 32 * block + m.  VARIANT 0: pe_operand per k-step (the per-lane evaluation mlp_wide.hip runs);
// VARIANT 1: pe_all, what mlp_fwd_pipe_tile runs.
template <int VARIANT>
__global__ __launch_bounds__(64) void pe_operands_kernel(const float* __restrict__ ndc, float* __restrict__ out)
{
    const int lane = threadIdx.x, half = lane >> 5;
    const int64_t p = (int64_t)blockIdx.x * 32 + (lane & 31);
    const float px = ndc[p * 3 + 0], py = ndc[p * 3 + 1], pz = ndc[p * 3 + 2];
    float e[PE_STEPS];
    if constexpr (VARIANT == 0) {
#pragma unroll
        for (int t = 0; t < PE_STEPS; ++t) e[t] = pe_operand(t, half, px, py, pz);
    } else {
        pe_all(half, px, py, pz, e);
    }
#pragma unroll
    for (int t = 0; t < PE_STEPS; ++t) out[(p * PE_STEPS + t) * 2 + half] = e[t];
}

extern "C" int mvsnerf_pe_operands_fwd(const float* ndc, int64_t P, int variant, float* out, void* stream)
{
    if (!ndc || !out || P < 0 || (P & 31) || P / 32 > 0x7fffffff || (variant != 0 && variant != 1)) return MVSNERF_EINVAL;
    if (P == 0) return MVSNERF_OK;
    if (variant == 0) pe_operands_kernel<0><<<(unsigned)(P / 32), 64, 0, (hipStream_t)stream>>>(ndc, out);
    else pe_operands_kernel<1><<<(unsigned)(P / 32), 64, 0, (hipStream_t)stream>>>(ndc, out);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
