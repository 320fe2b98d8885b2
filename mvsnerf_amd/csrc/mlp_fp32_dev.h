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

// The same encoding, evaluated once per point instead of once per lane: pe_operand above makes lane (m, half 0) and lane (m, half 1) reduce the
// same 30 angles and evaluate both polynomials on each, to keep sin in one lane and cos in the other.  Here a lane evaluates 15 of the angles -
// half 0 the even frequencies f = 2m, half 1 the odd ones f = 2m + 1 - keeps both values and trades one of each pair with its partner lane.
//
// pe_sincos2: pe_sin_or_cos's operations in its order on two angles at once.  The multiplies and fmas are written on float2 (v_pk_mul_f32,
// v_pk_fma_f32: the IEEE operation per component, so the bits are pe_sin_or_cos's); clamp, rintf and the quadrant select have no packed form and
// stay per component.  sin takes quadrant k, cos quadrant k + 1 of the same (sn, cs); the sign is an xor of the sign bit, which is what the
// negation of pe_sin_or_cos does to every input.
typedef float pe_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void pe_sincos2(pe_f32x2 x, pe_f32x2& s, pe_f32x2& c)
{
    x[0] = fminf(fmaxf(x[0], -65536.0f), 65536.0f);
    x[1] = fminf(fmaxf(x[1], -65536.0f), 65536.0f);
    const pe_f32x2 kx = x * pe_f32x2{0.63661977236758134f, 0.63661977236758134f};
    const pe_f32x2 k = {rintf(kx[0]), rintf(kx[1])};
    auto fma2 = [](pe_f32x2 a, pe_f32x2 b, pe_f32x2 d) { return __builtin_elementwise_fma(a, b, d); };
    auto all = [](float v) { return pe_f32x2{v, v}; };
    pe_f32x2 r = fma2(k, all(-1.5703125f), x);
    r = fma2(k, all(-4.837512969970703125e-4f), r);
    r = fma2(k, all(-7.54978995489188e-8f), r);
    const pe_f32x2 r2 = r * r;
    const pe_f32x2 sp = fma2(fma2(all(-1.9515295891e-4f), r2, all(8.3321608736e-3f)), r2, all(-1.6666654611e-1f));
    const pe_f32x2 sn = fma2(sp * r2, r, r);
    const pe_f32x2 cp = fma2(fma2(all(2.443315711809948e-5f), r2, all(-1.388731625493765e-3f)), r2, all(4.166664568298827e-2f));
    const pe_f32x2 cs = fma2(cp * r2, r2, fma2(all(-0.5f), r2, all(1.0f)));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const unsigned q = (unsigned)(int)k[i];
        const bool odd = q & 1u;
        s[i] = __uint_as_float(__float_as_uint(odd ? cs[i] : sn[i]) ^ ((q & 2u) << 30));
        c[i] = __uint_as_float(__float_as_uint(odd ? sn[i] : cs[i]) ^ (((q + 1u) & 2u) << 30));
    }
}

// All 32 positional-encoding B operands of this lane: e[t] has the bits of pe_operand(t, half, px, py, pz).  The angle of (f, c) is coord_c * 2^f
// as there (the same multiplication; the scale is selected by lane half).  Lane (m, half) evaluates (f = 2m' + half, c) for m' = 0..4, c = 0..2;
// its sin values are sv, its cos values cv.  Operand t = 2 + 3f + c wants sin in half 0 and cos in half 1: for an even f half 0 has its own sin
// and half 1 needs half 0's cos, for the odd f above it half 1 has its own cos and half 0 needs half 1's sin.  v_permlane32_swap(sv, cv) exchanges
// lanes 32-63 of sv with lanes 0-31 of cv, which is exactly that trade: afterwards sv is operand (2m', c) and cv operand (2m' + 1, c) in every
// lane - one VALU instruction per two operands.
__device__ __forceinline__ void pe_all(int half, float px, float py, float pz, float (&e)[32])
{
    e[0] = half ? py : px;
    e[1] = half ? 0.0f : pz;
    const float co[3] = {px, py, pz};
    float x[16], sv[16], cv[16];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        const float scale = half ? (float)(2 << (2 * m)) : (float)(1 << (2 * m));
#pragma unroll
        for (int c = 0; c < 3; ++c) x[3 * m + c] = co[c] * scale;
    }
    x[15] = x[14];                                        // 15 angles, eight pairs
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        pe_f32x2 s2, c2;
        pe_sincos2(pe_f32x2{x[i], x[i + 1]}, s2, c2);
        sv[i] = s2[0]; sv[i + 1] = s2[1]; cv[i] = c2[0]; cv[i + 1] = c2[1];
    }
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(sv[3 * m + c]), __float_as_uint(cv[3 * m + c]), false, false);
            e[2 + 6 * m + c] = __uint_as_float(sw[0]);
            e[5 + 6 * m + c] = __uint_as_float(sw[1]);
        }
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
