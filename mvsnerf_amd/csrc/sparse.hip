// Empty-space skipping for the render of a fine-tuned scene: which of the P = N*S samples of a ray batch can contribute at all, their stable
// compaction, and the way back to dense rows.  No counterpart in the reference (its renderer queries every sample).
//
// A sample is LIVE iff one of its NDC coordinates is non-finite, or some in-grid corner of its trilinear cell in the (D,H,W) density volume holds
// a value v with !(v <= thr) (a NaN voxel is live).  The cell is density_cell.h's: floor of ((x*2-1 + 1) / 2) * (W-1), ... - what density_lookup
// (importance.hip) forms.  The trilinear density is a convex combination of the in-grid corners and zeros, so for thr >= 0 a dead sample's density
// is <= thr.
//
// live_count_kernel    a workgroup owns LS_TILE = 1024 consecutive samples, four rounds of 256; each wave ballots its 64 predicates, stores the
//                      ballot word (16 words per workgroup) and counts its bits; the four waves' counts meet in LDS -> one count per workgroup.
// live_scan_kernel     ONE workgroup: exclusive scan of the workgroup counts (scan_dev.h) and the total -> *count.
// live_write_kernel    reads the ballot words back (the predicate is evaluated once): a live lane's slot is the workgroup's offset + the bits of
//                      the words in front of its own (through LDS) + mbcnt of its own word.  Slot order = sample order: idx is ascending, the
//                      order of torch.nonzero, and every run gives the same bytes.  Nothing is placed with an atomic and no workgroup waits on
//                      another (three launches in stream order instead).
// expand_rows_kernel   dst[idx[j]] = src[j], every other row zero, every row written once: a workgroup owns ER_TILE consecutive rows of dst, finds
//                      the first j with idx[j] >= its first row by one binary search (idx is ascending), and marks its rows' j in LDS.  An idx
//                      entry can only ever select a row of the workgroup's own tile, whatever the buffer holds.
// compact_rows_kernel  the inverse, for the backward of a training step that skips empty space: dst[j] = src[idx[j]] for j < count, every other row of
//                      dst zero, every row written once.  A thread owns a row (C == 4: one 16-byte load and store) or an element (other C); idx[j] is
//                      range-checked against [0, P) before the load, so a stale or foreign idx gives zero rows, never a read outside src.  The stores
//                      are consecutive; the loads follow the ascending idx (a gather: 16 of every 64-byte line at a live fraction of 1/4).
//
// Early ray termination marches a ray batch in segments of stop_every samples and runs the compaction on one segment at a time:
// live_count_range_kernel / live_write_range_kernel   the RANGE = true instantiations of the count and write tiles, over the window s0 <= s < s1 of
//                      every ray: element t of the N * (s1 - s0) window elements is sample s0 + t % (s1 - s0) of ray t / (s1 - s0), so ascending t is
//                      ascending n * S + s.  A sample is selected iff !(ray_T[n] < eps) (ray_T given) and its cell is live (density given).  The scan
//                      kernel is shared as it is.
// ray_transmittance_kernel   ray_T[n] *= the product over the window of ((1 - alpha) + 1e-10f), ascending s, every product rounded: four lanes own a
//                      ray, lane q reads sigma of rows s0 + 4 i + q, so one load of a wave touches sixteen 64-byte lines of raw, each of them whole;
//                      the four factors meet by shuffle and every lane of the quad runs the same serial chain.
// scatter_rows_kernel  dst[idx[j]] = src[j] for j < count and nothing else written: expand_rows without the zero fill (the host fills raw once, every
//                      segment scatters into it).  idx[j] is range-checked against [0, P) before the store.
#include "common.h"
#include "composite_wave.h"
#include "density_cell.h"
#include "scan_dev.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int LS_THREADS = 256, LS_ROUNDS = 4, LS_TILE = LS_THREADS * LS_ROUNDS, LS_WORDS = LS_TILE / 64;
constexpr int SCAN_THREADS = 256;
constexpr int ER_THREADS = 256, ER_TILE = 1024, ER_MAX_C = 64;

inline int64_t live_blocks(int64_t P) { return (P + LS_TILE - 1) / LS_TILE; }

__device__ __forceinline__ bool sample_live(const float* __restrict__ density, int D, int H, int W, float thr, float x, float y, float z)
{
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return true;
    const DensityCell c = density_cell(D, H, W, x, y, z);
    bool live = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float cx = c.fx + (float)(k & 1), cy = c.fy + (float)((k >> 1) & 1), cz = c.fz + (float)(k >> 2);
        if (density_corner_in_grid(D, H, W, cx, cy, cz)) {
            const float v = density[density_corner_index(H, W, cx, cy, cz)];
            live = live || !(v <= thr);
        }
    }
    return live;
}

// The window of a ray batch that the RANGE = true tiles walk (the RANGE = false ones never read it): samples s0 .. s0 + G - 1 of every ray.
struct LiveRange {
    unsigned S, s0, G;
    const float* ray_T;     // NULL: every ray is alive
    float eps;
};

// element t of the N * G window elements -> its ray and its flat sample index n * S + s (32-bit divisions: N * S < 2^31)
__device__ __forceinline__ int64_t range_sample(const LiveRange& w, int64_t t, unsigned& ray)
{
    ray = (unsigned)t / w.G;
    return (int64_t)ray * w.S + w.s0 + ((unsigned)t - ray * w.G);
}

template <bool RANGE>
__device__ __forceinline__ void live_count_tile(const float* __restrict__ density, int D, int H, int W, float thr, const float* __restrict__ ndc, int64_t P,
                                                const LiveRange& w, unsigned long long* __restrict__ masks, int* __restrict__ counts)
{
    __shared__ int s_cnt[LS_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n = 0;                                                          // the wave's count, in every lane of it
#pragma unroll
    for (int r = 0; r < LS_ROUNDS; ++r) {
        const int64_t t = (int64_t)blockIdx.x * LS_TILE + r * LS_THREADS + threadIdx.x;
        bool live = false;
        if (RANGE) {
            if (t < P) {
                unsigned ray;
                const int64_t f = range_sample(w, t, ray);
                live = true;
                if (w.ray_T) live = !(w.ray_T[ray] < w.eps);                // a NaN transmittance never stops its ray
                if (live && density) live = sample_live(density, D, H, W, thr, ndc[f * 3 + 0], ndc[f * 3 + 1], ndc[f * 3 + 2]);
            }
        } else {
            if (t < P) live = sample_live(density, D, H, W, thr, ndc[t * 3 + 0], ndc[t * 3 + 1], ndc[t * 3 + 2]);
        }
        const unsigned long long m = __ballot(live);
        if (lane == 0) masks[(int64_t)blockIdx.x * LS_WORDS + r * (LS_THREADS / 64) + wave] = m;      // all 16 words, the tail's zeros too
        n += __popcll(m);
    }
    const int total = mvs_block_sum<LS_THREADS>(n, s_cnt);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(LS_THREADS) void live_count_kernel(const float* __restrict__ density, int D, int H, int W, float thr,
                                                                const float* __restrict__ ndc, int64_t P,
                                                                unsigned long long* __restrict__ masks, int* __restrict__ counts)
{
    live_count_tile<false>(density, D, H, W, thr, ndc, P, LiveRange{}, masks, counts);
}

__global__ __launch_bounds__(LS_THREADS) void live_count_range_kernel(const float* __restrict__ density, int D, int H, int W, float thr,
                                                                      const float* __restrict__ ndc, int64_t P, LiveRange w,
                                                                      unsigned long long* __restrict__ masks, int* __restrict__ counts)
{
    live_count_tile<true>(density, D, H, W, thr, ndc, P, w, masks, counts);
}

__global__ __launch_bounds__(SCAN_THREADS) void live_scan_kernel(const int* __restrict__ counts, int nb, int* __restrict__ offsets, int* __restrict__ count)
{
    __shared__ int s_tot[SCAN_THREADS / 64];
    // nb < 2^21 + 1, so the run arithmetic stays far inside 32 bits; the total is <= P < 2^31
    const int total = mvs_block_scan_runs<SCAN_THREADS>(nb, [&](int i) { return counts[i]; }, [&](int i, int pre) { offsets[i] = pre; }, s_tot);
    if (threadIdx.x == 0) *count = total;
}

template <bool RANGE>
__device__ __forceinline__ void live_write_tile(const unsigned long long* __restrict__ masks, const int* __restrict__ offsets,
                                                const float* __restrict__ ndc, const float* __restrict__ pts,
                                                const float* __restrict__ rays_dir, int64_t P, unsigned S, const LiveRange& rw,
                                                int* __restrict__ idx, float* __restrict__ ndc_c, float* __restrict__ pts_c,
                                                float* __restrict__ dir_c)
{
    __shared__ unsigned long long s_mask[LS_WORDS];
    __shared__ int s_pop[LS_WORDS];
    if (threadIdx.x < LS_WORDS) {
        const unsigned long long m = masks[(int64_t)blockIdx.x * LS_WORDS + threadIdx.x];
        s_mask[threadIdx.x] = m;
        s_pop[threadIdx.x] = __popcll(m);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int base = offsets[blockIdx.x];
#pragma unroll
    for (int r = 0; r < LS_ROUNDS; ++r) {
        const int w = r * (LS_THREADS / 64) + wave;
        const unsigned long long m = s_mask[w];
        if (!((m >> lane) & 1ull)) continue;
        const int64_t j = (int64_t)base + mvs_tile_rank(s_pop, w, m);   // < count <= P: inside every output
        int64_t t = (int64_t)blockIdx.x * LS_TILE + r * LS_THREADS + threadIdx.x;             // < P: the count pass sets no bit past the end
        if (t >= P || j >= P) continue;
        unsigned ray = 0;
        if (RANGE) t = range_sample(rw, t, ray);                        // the window element -> its sample: t < N * S from here on
        idx[j] = (int)t;
        ndc_c[j * 3 + 0] = ndc[t * 3 + 0]; ndc_c[j * 3 + 1] = ndc[t * 3 + 1]; ndc_c[j * 3 + 2] = ndc[t * 3 + 2];
        if (pts) { pts_c[j * 3 + 0] = pts[t * 3 + 0]; pts_c[j * 3 + 1] = pts[t * 3 + 1]; pts_c[j * 3 + 2] = pts[t * 3 + 2]; }
        if (rays_dir) {
            const int64_t n = RANGE ? ray : (unsigned)t / S;            // P < 2^31: one 32-bit division
            dir_c[j * 3 + 0] = rays_dir[n * 3 + 0]; dir_c[j * 3 + 1] = rays_dir[n * 3 + 1]; dir_c[j * 3 + 2] = rays_dir[n * 3 + 2];
        }
    }
}

__global__ __launch_bounds__(LS_THREADS) void live_write_kernel(const unsigned long long* __restrict__ masks, const int* __restrict__ offsets,
                                                                const float* __restrict__ ndc, const float* __restrict__ pts,
                                                                const float* __restrict__ rays_dir, int64_t P, unsigned S,
                                                                int* __restrict__ idx, float* __restrict__ ndc_c, float* __restrict__ pts_c,
                                                                float* __restrict__ dir_c)
{
    live_write_tile<false>(masks, offsets, ndc, pts, rays_dir, P, S, LiveRange{}, idx, ndc_c, pts_c, dir_c);
}

__global__ __launch_bounds__(LS_THREADS) void live_write_range_kernel(const unsigned long long* __restrict__ masks, const int* __restrict__ offsets,
                                                                      const float* __restrict__ ndc, const float* __restrict__ pts,
                                                                      const float* __restrict__ rays_dir, int64_t P, LiveRange w,
                                                                      int* __restrict__ idx, float* __restrict__ ndc_c, float* __restrict__ pts_c,
                                                                      float* __restrict__ dir_c)
{
    live_write_tile<true>(masks, offsets, ndc, pts, rays_dir, P, w.S, w, idx, ndc_c, pts_c, dir_c);
}

template <bool VEC4>
__global__ __launch_bounds__(ER_THREADS) void expand_rows_kernel(const float* __restrict__ src, const int* __restrict__ idx, const int* __restrict__ count,
                                                                 int64_t src_rows, int64_t P, int C, float* __restrict__ dst)
{
    __shared__ int s_j[ER_TILE];
    const int64_t row0 = (int64_t)blockIdx.x * ER_TILE;
    const int rows = (int)(P - row0 < ER_TILE ? P - row0 : ER_TILE);
    for (int r = threadIdx.x; r < ER_TILE; r += ER_THREADS) s_j[r] = -1;
    int64_t n = *count;
    n = n < 0 ? 0 : (n > src_rows ? src_rows : n);                      // never past what src and idx hold
    // first j with idx[j] >= row0 (every thread runs the same search: uniform loads)
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if ((int64_t)idx[mid] < row0) lo = mid + 1; else hi = mid; }
    __syncthreads();
    // at most `rows` entries of an ascending idx fall into this tile
    for (int k = threadIdx.x; k < rows; k += ER_THREADS) {
        const int64_t j = lo + k;
        if (j >= n) break;
        const int64_t r = (int64_t)idx[j] - row0;
        if (r >= 0 && r < rows) s_j[r] = (int)j;
    }
    __syncthreads();
    if (VEC4) {
        for (int r = threadIdx.x; r < rows; r += ER_THREADS) {
            const int j = s_j[r];
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j >= 0) v = reinterpret_cast<const f32x4*>(src)[j];
            reinterpret_cast<f32x4*>(dst)[row0 + r] = v;
        }
    } else {
        const int total = rows * C;                                     // C <= ER_MAX_C: far inside 32 bits
        for (int e = threadIdx.x; e < total; e += ER_THREADS) {
            const int r = e / C, c = e - r * C;
            const int j = s_j[r];
            dst[row0 * C + e] = j >= 0 ? src[(int64_t)j * C + c] : 0.f;
        }
    }
}

template <bool VEC4>
__global__ __launch_bounds__(ER_THREADS) void compact_rows_kernel(const float* __restrict__ src, const int* __restrict__ idx, const int* __restrict__ count,
                                                                  int64_t P, int64_t dst_rows, int C, float* __restrict__ dst)
{
    int64_t n = *count;
    n = n < 0 ? 0 : (n > dst_rows ? dst_rows : n);                      // never past what dst and idx hold
    const int64_t t = (int64_t)blockIdx.x * ER_THREADS + threadIdx.x;
    if (VEC4) {
        if (t >= dst_rows) return;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t < n) {
            const int64_t r = idx[t];
            if (r >= 0 && r < P) v = reinterpret_cast<const f32x4*>(src)[r];
        }
        reinterpret_cast<f32x4*>(dst)[t] = v;
    } else {
        if (t >= dst_rows * C) return;
        const int64_t j = t / C;
        const int c = (int)(t - j * C);
        float v = 0.f;
        if (j < n) {
            const int64_t r = idx[j];
            if (r >= 0 && r < P) v = src[r * C + c];
        }
        dst[t] = v;
    }
}

constexpr int RT_THREADS = 256, RT_RAYS = RT_THREADS / 4;

// ray_T[n] *= prod_{s0 <= s < s1} ((1 - alpha_s) + 1e-10f): the running transmittance of compositing (composite_wave.h: raw2alpha, transmittance_step),
// ascending s, every product rounded.  Lanes 4 r .. 4 r + 3 of a wave own ray r of its sixteen; in round i lane q reads sigma of row s0 + 4 i + q - the
// quad one 64-byte line of raw when the window starts on one.  The four factors travel by shuffle (the round count is uniform, so every lane of the
// wave executes them) and each lane of the quad multiplies them in, in order: all four hold the same bits, lane q == 0 stores them.
__global__ __launch_bounds__(RT_THREADS) void ray_transmittance_kernel(const float* __restrict__ raw, int64_t N, int S, int s0, int s1, float* __restrict__ ray_T)
{
    const int q = threadIdx.x & 3, lane0 = threadIdx.x & 60;
    const int64_t n = (int64_t)blockIdx.x * RT_RAYS + (threadIdx.x >> 2);
    const bool have = n < N;
    const f32x4* __restrict__ row = reinterpret_cast<const f32x4*>(raw) + (have ? n : 0) * S;
    float T = have ? ray_T[n] : 1.0f;
    for (int b = s0; b < s1; b += 4) {
        const int s = b + q;
        float f = 1.0f;
        if (have && s < s1) f = transmittance_step(raw2alpha(row[s][3]));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float fk = __shfl(f, lane0 + k, 64);
            if (b + k < s1) T *= fk;
        }
    }
    if (have && q == 0) ray_T[n] = T;
}

template <bool VEC4>
__global__ __launch_bounds__(ER_THREADS) void scatter_rows_kernel(const float* __restrict__ src, const int* __restrict__ idx, const int* __restrict__ count,
                                                                  int64_t src_rows, int64_t P, int C, float* __restrict__ dst)
{
    int64_t n = *count;
    n = n < 0 ? 0 : (n > src_rows ? src_rows : n);                      // never past what src and idx hold
    const int64_t t = (int64_t)blockIdx.x * ER_THREADS + threadIdx.x;
    if (VEC4) {
        if (t >= n) return;
        const int64_t r = idx[t];
        if (r >= 0 && r < P) reinterpret_cast<f32x4*>(dst)[r] = reinterpret_cast<const f32x4*>(src)[t];
    } else {
        if (t >= n * C) return;
        const int64_t j = t / C;
        const int c = (int)(t - j * C);
        const int64_t r = idx[j];
        if (r >= 0 && r < P) dst[r * C + c] = src[t];
    }
}

}  // namespace

extern "C" size_t mvsnerf_live_samples_workspace_bytes(int64_t P)
{
    if (P < 1 || P >= ((int64_t)1 << 31)) return 0;
    const size_t nb = (size_t)live_blocks(P);
    return nb * LS_WORDS * sizeof(unsigned long long) + nb * 2 * sizeof(int);
}

extern "C" int mvsnerf_live_samples_fwd(const float* density, int D, int H, int W, float thr, const float* ndc, const float* pts, const float* rays_dir,
                                        int64_t N, int S, int* count, int* idx, float* ndc_c, float* pts_c, float* dir_c, void* workspace, void* stream)
{
    if (!density || !count || D < 1 || H < 1 || W < 1 || N < 0 || S < 1 || thr != thr) return MVSNERF_EINVAL;
    if ((pts && !pts_c) || (rays_dir && !dir_c)) return MVSNERF_EINVAL;
    if (N > (((int64_t)1 << 31) - 1) / S) return MVSNERF_EUNSUPPORTED;                  // P >= 2^31: idx is int32
    const int64_t P = N * (int64_t)S;
    hipStream_t st = (hipStream_t)stream;
    auto mis = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (mis(density, 4) || mis(ndc, 4) || mis(pts, 4) || mis(rays_dir, 4) || mis(count, 4) || mis(idx, 4) || mis(ndc_c, 4) || mis(pts_c, 4) || mis(dir_c, 4) ||
        mis(workspace, 8))
        return MVSNERF_EALIGN;
    if (P == 0) {
        hipError_t e = hipMemsetAsync(count, 0, sizeof(int), st);
        return e == hipSuccess ? MVSNERF_OK : (int)e;
    }
    if (!ndc || !idx || !ndc_c || !workspace) return MVSNERF_EINVAL;
    const int64_t nb = live_blocks(P);
    unsigned long long* masks = static_cast<unsigned long long*>(workspace);
    int* counts = reinterpret_cast<int*>(masks + nb * LS_WORDS);
    int* offsets = counts + nb;
    live_count_kernel<<<(unsigned)nb, LS_THREADS, 0, st>>>(density, D, H, W, thr, ndc, P, masks, counts);
    MVS_LAUNCH_CHECK();
    live_scan_kernel<<<1, SCAN_THREADS, 0, st>>>(counts, (int)nb, offsets, count);
    MVS_LAUNCH_CHECK();
    live_write_kernel<<<(unsigned)nb, LS_THREADS, 0, st>>>(masks, offsets, ndc, pts, rays_dir, P, (unsigned)S, idx, ndc_c, pts_c, dir_c);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_expand_rows_fwd(const float* src, const int* idx, const int* count, int64_t src_rows, int64_t P, int C, float* dst, void* stream)
{
    if (!count || !dst || src_rows < 0 || P < 0 || C < 1 || src_rows > P) return MVSNERF_EINVAL;
    if (src_rows > 0 && (!src || !idx)) return MVSNERF_EINVAL;
    if (C > ER_MAX_C || P >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; };
    if (mis(src) || mis(idx) || mis(count) || mis(dst)) return MVSNERF_EALIGN;
    if (P == 0) return MVSNERF_OK;
    const unsigned grid = mvs_cdiv(P, ER_TILE);
    hipStream_t st = (hipStream_t)stream;
    if (C == 4 && mvs_aligned16(src) && mvs_aligned16(dst))
        expand_rows_kernel<true><<<grid, ER_THREADS, 0, st>>>(src, idx, count, src_rows, P, C, dst);
    else
        expand_rows_kernel<false><<<grid, ER_THREADS, 0, st>>>(src, idx, count, src_rows, P, C, dst);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_compact_rows_fwd(const float* src, const int* idx, const int* count, int64_t P, int64_t dst_rows, int C, float* dst, void* stream)
{
    if (!count || !dst || P < 0 || dst_rows < 0 || C < 1 || dst_rows > P) return MVSNERF_EINVAL;
    if (dst_rows > 0 && (!src || !idx)) return MVSNERF_EINVAL;
    if (C > ER_MAX_C || P >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; };
    if (mis(src) || mis(idx) || mis(count) || mis(dst)) return MVSNERF_EALIGN;
    if (dst_rows == 0) return MVSNERF_OK;
    hipStream_t st = (hipStream_t)stream;
    if (C == 4 && mvs_aligned16(src) && mvs_aligned16(dst))
        compact_rows_kernel<true><<<mvs_cdiv(dst_rows, ER_THREADS), ER_THREADS, 0, st>>>(src, idx, count, P, dst_rows, C, dst);
    else
        compact_rows_kernel<false><<<mvs_cdiv(dst_rows * C, ER_THREADS), ER_THREADS, 0, st>>>(src, idx, count, P, dst_rows, C, dst);     // fewer than 2^37 elements: the grid fits 32 bits
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// ---- early ray termination.  These three entries answer a misaligned pointer with MVSNERF_EINVAL, like a NULL one.
extern "C" size_t mvsnerf_live_samples_range_workspace_bytes(int64_t N, int G)
{
    if (N < 1 || G < 1 || N > (((int64_t)1 << 31) - 1) / G) return 0;
    return mvsnerf_live_samples_workspace_bytes(N * (int64_t)G);
}

extern "C" int mvsnerf_live_samples_range_fwd(const float* density, int D, int H, int W, float thr, const float* ndc, const float* pts, const float* rays_dir,
                                              int64_t N, int S, int s0, int s1, const float* ray_T, float eps, int* count, int* idx, float* ndc_c,
                                              float* pts_c, float* dir_c, void* workspace, void* stream)
{
    if (!count || N < 0 || S < 1 || s0 < 0 || s1 > S || s0 >= s1 || eps != eps) return MVSNERF_EINVAL;
    if (density && (D < 1 || H < 1 || W < 1 || thr != thr)) return MVSNERF_EINVAL;
    if ((pts && !pts_c) || (rays_dir && !dir_c)) return MVSNERF_EINVAL;
    auto mis = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (mis(density, 4) || mis(ndc, 4) || mis(pts, 4) || mis(rays_dir, 4) || mis(ray_T, 4) || mis(count, 4) || mis(idx, 4) || mis(ndc_c, 4) || mis(pts_c, 4) ||
        mis(dir_c, 4) || mis(workspace, 8))
        return MVSNERF_EINVAL;
    if (N > (((int64_t)1 << 31) - 1) / S) return MVSNERF_EUNSUPPORTED;                  // N * S >= 2^31: idx is int32
    const int G = s1 - s0;
    const int64_t P = N * (int64_t)G;                                                   // the window elements
    hipStream_t st = (hipStream_t)stream;
    if (P == 0) {
        hipError_t e = hipMemsetAsync(count, 0, sizeof(int), st);
        return e == hipSuccess ? MVSNERF_OK : (int)e;
    }
    if (!ndc || !idx || !ndc_c || !workspace) return MVSNERF_EINVAL;
    const int64_t nb = live_blocks(P);
    unsigned long long* masks = static_cast<unsigned long long*>(workspace);
    int* counts = reinterpret_cast<int*>(masks + nb * LS_WORDS);
    int* offsets = counts + nb;
    const LiveRange w = {(unsigned)S, (unsigned)s0, (unsigned)G, ray_T, eps};
    live_count_range_kernel<<<(unsigned)nb, LS_THREADS, 0, st>>>(density, D, H, W, thr, ndc, P, w, masks, counts);
    MVS_LAUNCH_CHECK();
    live_scan_kernel<<<1, SCAN_THREADS, 0, st>>>(counts, (int)nb, offsets, count);
    MVS_LAUNCH_CHECK();
    live_write_range_kernel<<<(unsigned)nb, LS_THREADS, 0, st>>>(masks, offsets, ndc, pts, rays_dir, P, w, idx, ndc_c, pts_c, dir_c);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_ray_transmittance_fwd(const float* raw, int64_t N, int S, int s0, int s1, float* ray_T, void* stream)
{
    if (!raw || !ray_T || N < 0 || S < 1 || s0 < 0 || s1 > S || s0 >= s1) return MVSNERF_EINVAL;
    if (!mvs_aligned16(raw) || (reinterpret_cast<uintptr_t>(ray_T) & 3u)) return MVSNERF_EINVAL;
    if (N > (((int64_t)1 << 31) - 1) / S) return MVSNERF_EUNSUPPORTED;
    if (N == 0) return MVSNERF_OK;
    ray_transmittance_kernel<<<mvs_cdiv(N, RT_RAYS), RT_THREADS, 0, (hipStream_t)stream>>>(raw, N, S, s0, s1, ray_T);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_scatter_rows_fwd(const float* src, const int* idx, const int* count, int64_t src_rows, int64_t P, int C, float* dst, void* stream)
{
    if (!count || !dst || src_rows < 0 || P < 0 || C < 1 || src_rows > P) return MVSNERF_EINVAL;
    if (src_rows > 0 && (!src || !idx)) return MVSNERF_EINVAL;
    auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; };
    if (mis(src) || mis(idx) || mis(count) || mis(dst)) return MVSNERF_EINVAL;
    if (C > ER_MAX_C || P >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    if (src_rows == 0) return MVSNERF_OK;
    hipStream_t st = (hipStream_t)stream;
    if (C == 4 && mvs_aligned16(src) && mvs_aligned16(dst))
        scatter_rows_kernel<true><<<mvs_cdiv(src_rows, ER_THREADS), ER_THREADS, 0, st>>>(src, idx, count, src_rows, P, C, dst);
    else
        scatter_rows_kernel<false><<<mvs_cdiv(src_rows * C, ER_THREADS), ER_THREADS, 0, st>>>(src, idx, count, src_rows, P, C, dst);     // fewer than 2^37 elements: the grid fits 32 bits
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
