// Device pieces shared by the fp32 MLP tiles (mlp.hip: netwidth 128; mlp_wide.hip: netwidth 256): the k-step loop on v_mfma_f32_32x32x2_f32, the
// accumulator initialisation from a fragment-ordered bias, the positional encoding's sin/cos and the weight-slab logistics (LDS-DMA pieces and
// the one barrier per slab).  Both kernels evaluate the same arithmetic with these, so a point's encoding has the same bits in either.
#pragma once
#include "common.h"
#include "lds_dma.h"

// acc[g][b] += W_frag(t, b) * bfn(g, t) for t in [0, 4*STEPS4); G = 32-point groups per wave
// (one A fragment read from LDS feeds G MFMAs).
struct NoHook {
    static constexpr int STEPS = 0;
    __device__ __forceinline__ void operator()(int) const {}
};

// `under(i)` issues piece i of what the hook spreads under this GEMM, i < HOOK::STEPS: the pipelined kernel's DMA of the next slab (SlabUnder below).
// A wave issues in order: eight pieces back to back are a stretch of its stream without an MFMA, one piece between two k-steps sits behind the MFMA
// in flight.  The pieces go behind k-steps 0, 1, 2 of every group of four; k-step 3 keeps none, the compiler requests the next group's A fragments
// around its MFMAs and a piece there would put the LDS latency behind the piece instead of under the MFMAs (measured, CHANGELOG.md).  Eight pieces
// are out after k-step 9, nine after k-step 10.  sched_barrier(0) pins each piece between its two k-steps: nothing crosses, the inline asm included
// (a barrier with a mask lets it through).
template <int STEPS4, int NBLK, int G, typename BFN, typename HOOK = NoHook>
__device__ __forceinline__ void gemm_stage(const float* __restrict__ w, f32x16 (&acc)[G][NBLK], int lane, BFN bfn, HOOK under = HOOK())
{
    static_assert(HOOK::STEPS <= 3 * STEPS4, "the hook's pieces must fit under the GEMM's k-steps");
#pragma unroll
    for (int t4 = 0; t4 < STEPS4; ++t4) {
        f32x4 a[NBLK];
#pragma unroll
        for (int b = 0; b < NBLK; ++b)
            a[b] = *reinterpret_cast<const f32x4*>(w + ((t4 * NBLK + b) * 64 + lane) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float bv[G];
#pragma unroll
            for (int g = 0; g < G; ++g) bv[g] = bfn(g, t4 * 4 + j);
#pragma unroll
            for (int b = 0; b < NBLK; ++b)
#pragma unroll
                for (int g = 0; g < G; ++g)
                    acc[g][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[b][j], bv[g], acc[g][b], 0, 0, 0);
            if (j < 3 && t4 * 3 + j < HOOK::STEPS) {
                __builtin_amdgcn_sched_barrier(0);
                under(t4 * 3 + j);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

template <int NBLK, int G>
__device__ __forceinline__ void init_acc(f32x16 (&acc)[G][NBLK], const float* __restrict__ vec_h)
{
    // vec_h points at this lane-half's [NBLK*16] bias fragment (LDS broadcast reads)
#pragma unroll
    for (int b = 0; b < NBLK; ++b)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(vec_h + b * 16 + r4 * 4);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                acc[g][b][r4 * 4 + 0] = v[0]; acc[g][b][r4 * 4 + 1] = v[1]; acc[g][b][r4 * 4 + 2] = v[2]; acc[g][b][r4 * 4 + 3] = v[3];
            }
        }
}

// sin or cos of x for the positional encoding (x = ndc * 2^f, f <= 9, ndc in [0,1] inside the volume): Cody-Waite
// reduction by pi/2 in three fma steps (k*C1 is exact for |k| < 2^16, i.e. |x| < 1e5), cephes minimax polynomials on
// [-pi/4, pi/4], quadrant select.  cos(x) = sin(x + pi/2) is a quadrant shift, so every lane evaluates one polynomial
// pair and picks.  Branch-free on purpose (a branch here would cut the unrolled MFMA stream into basic blocks).
// Max abs error 7.6e-8 on |x| <= 1600 (numpy float32 sin: 6.6e-8).  Arguments are clamped to +-65536, i.e. samples
// more than 128 volume-widths outside the frustum (where the encoding is physically meaningless anyway).
__device__ __forceinline__ float pe_sin_or_cos(float x, int want_cos)
{
    x = fminf(fmaxf(x, -65536.0f), 65536.0f);
    const float k = rintf(x * 0.63661977236758134f);
    float r = fmaf(k, -1.5703125f, x);
    r = fmaf(k, -4.837512969970703125e-4f, r);
    r = fmaf(k, -7.54978995489188e-8f, r);
    const float r2 = r * r;
    const float sp = fmaf(fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f), r2, -1.6666654611e-1f);
    const float sn = fmaf(sp * r2, r, r);
    const float cp = fmaf(fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f), r2, 4.166664568298827e-2f);
    const float cs = fmaf(cp * r2, r2, fmaf(-0.5f, r2, 1.0f));
    const int q = (int)k + want_cos;
    const float v = (q & 1) ? cs : sn;
    return (q & 2) ? -v : v;
}

// positional-encoding B operand of k-step t for this lane (point coords px,py,pz; half)
__device__ __forceinline__ float pe_operand(int t, int half, float px, float py, float pz)
{
    if (t == 0) return half ? py : px;
    if (t == 1) return half ? 0.0f : pz;
    const int j = t - 2, f = j / 3, c = j - 3 * f;
    const float x = (c == 0 ? px : c == 1 ? py : pz) * (float)(1 << f);   // exact, as x*2^f in models.py:49
    return pe_sin_or_cos(x, half);
}

__device__ __forceinline__ void slab_dma(float* __restrict__ dst, const float* __restrict__ src, int n_floats, int wave, int lane)
{
    lds_dma<4>(dst, src, n_floats >> 8, wave, lane);     // 1 KB per wave-instruction, scalar base + one lane offset (lds_dma.h)
}
template <int N_FLOATS>
__device__ __forceinline__ void slab_dma_c(float* __restrict__ dst, const float* __restrict__ src, int wave, int lane)
{
    lds_dma_c<4, N_FLOATS / 256>(dst, src, wave, lane);
}

// The same slab as slab_dma_c<N_FLOATS>, as a gemm_stage hook: this wave's share goes out piece by piece under the first k-steps of the GEMM that runs
// meanwhile (8 pieces for half a layer, 9 in waves 0 and 1 for the views segment), the rest of the GEMM - 21 k-steps or more - covers the fetch.
template <int N_FLOATS>
struct SlabUnder {
    static constexpr int STEPS = lds_dma_steps(4, N_FLOATS / 256);
    float* dst; const float* src; int wave, lane;
    __device__ __forceinline__ void operator()(int k) const { lds_dma_piece<4, N_FLOATS / 256>(dst, src, wave, lane, k); }
};

__device__ __forceinline__ void slab_sync()
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's DMA pieces (and earlier stores) have landed
    __syncthreads();                                      // ... everybody's have, and everybody left the other buffer
}
