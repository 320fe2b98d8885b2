// Deterministic count -> scan -> write: the integer scans, totals and ballot ranks that the compacting kernels share (sparse.hip,
// depth_fusion.hip, mesh.hip, cloud_metrics.hip), and the __shfl_down trees of the wave reductions.  Device only.  No atomics: a kernel that places
// its rows at base + prefix + rank with these gives the same bytes on every run.
//
// Contract:
//   - a workgroup is THREADS = a multiple of 64 threads in x, wave = threadIdx.x >> 6, and EVERY thread of it calls the mvs_block_* helpers
//     (each holds exactly one __syncthreads(); LDS the caller wrote before the call is visible after it);
//   - s_tot / s is THREADS / 64 words of the caller's LDS, one per wave, and holds the waves' totals after the call;
//   - mvs_block_scan_runs: nb + THREADS fits in an int and the grand total fits in T.  Each caller derives its own bound at the call site;
//   - integer code and pure shuffles only.  The mvs_wave_*_down trees may carry a float or a double, but they add one operation per step (nothing
//     to contract), so the caller's `fp contract` and vectorizer settings cannot change their bits.  No float helper belongs here: the translation
//     units differ in `#pragma clang fp contract` and in -fno-slp-vectorize, and a shared projection (to_camera, lift, depth_usable) would tie their
//     bits together for no gain.  They stay in their files on purpose.
#pragma once
#include "common.h"

// inclusive sum over the 64 lanes of a wave
template <typename T>
__device__ __forceinline__ T mvs_wave_inclusive(T v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// exclusive prefix of v over the workgroup
template <int THREADS, typename T>
__device__ __forceinline__ T mvs_block_exclusive(T v, T* s_tot)
{
    static_assert(THREADS % 64 == 0 && THREADS <= 1024, "whole waves");
    const int wave = threadIdx.x >> 6;
    const T incl = mvs_wave_inclusive(v);
    if ((threadIdx.x & 63) == 63) s_tot[wave] = incl;
    __syncthreads();
    T pre = incl - v;
    for (int w = 0; w < wave; ++w) pre += s_tot[w];
    return pre;
}

// the sum of the waves' words
template <int THREADS, typename T>
__device__ __forceinline__ T mvs_waves_total(const T* s)
{
    T total = s[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) total += s[w];
    return total;
}

// v: a wave's sum, valid in its lane 0 -> the workgroup's sum, in every thread
template <int THREADS>
__device__ __forceinline__ int mvs_block_sum(int v, int* s)
{
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return mvs_waves_total<THREADS>(s);
}

// ONE workgroup scans nb entries: thread t owns the run [min(t c, nb), min(t c + c, nb)), c = ceil(nb / THREADS).  load(i) returns entry i,
// store(i, prefix) takes its exclusive prefix; returns the grand total.  load and store may name the same array: a run is read whole before the
// barrier, and behind it entry i is read again before store(i, .).
template <int THREADS, typename T, typename Load, typename Store>
__device__ __forceinline__ T mvs_block_scan_runs(int nb, Load load, Store store, T* s_tot)
{
    const int c = (nb + THREADS - 1) / THREADS;
    const int b = min((int)threadIdx.x * c, nb), e = min(b + c, nb);
    T sum = 0;
    for (int i = b; i < e; ++i) sum += load(i);
    T run = mvs_block_exclusive<THREADS>(sum, s_tot);
    for (int i = b; i < e; ++i) {
        const T t = load(i);
        store(i, run);
        run += t;
    }
    return mvs_waves_total<THREADS>(s_tot);
}

// __shfl_down trees, off = 32 .. 1: the result is valid in lane 0
template <typename T>
__device__ __forceinline__ T mvs_wave_sum_down(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ T mvs_wave_min_down(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_down(v, off, 64));      // (float: fminf)
    return v;
}
template <typename T>
__device__ __forceinline__ T mvs_wave_max_down(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_down(v, off, 64));      // (float: fmaxf)
    return v;
}

// the set bits of ballot word m below the calling lane
__device__ __forceinline__ int mvs_ballot_rank(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
// rank inside a tile of ballot words: s_pop[k] = popcount of word k, m = word w (the calling wave's own)
__device__ __forceinline__ int mvs_tile_rank(const int* s_pop, int w, unsigned long long m)
{
    int pre = 0;
    for (int k = 0; k < w; ++k) pre += s_pop[k];
    return pre + mvs_ballot_rank(m);
}
