// Plane-sweep cost volume, backward: the per-voxel scatter kernel, the column form, and its deterministic (fixed-point) variant.
// Built with the default flags, unlike the forward sweep (planesweep.hip is built without the SLP vectorizer and checked for packed fp32
// instructions; these kernels never were).
#include "common.h"

// ---- plane-sweep backward: d cost[...variance channels] -> d feats (channel-last [V][H][W][32]).
// var_c = s2*inv - (s*inv)^2 with s = sum of warped values, so for every contributing value w:
//   d w = g_var * 2*inv*(w - s*inv).   Warped values are bilinear gathers => their gradient is a bilinear scatter
// (float atomics).  Masks/counts are step functions (no gradient); thumbnails carry no parameters.
// Both backward kernels ADD to g_feat (the caller hands in zeros), and give a view whose sample coordinate is not finite four zero weights, as the forward
// sweep does (planesweep.hip header): the three geometry blocks are the same code and must stay so.
template <int C>
__global__ __launch_bounds__(256) void planesweep_bwd_kernel(const float* __restrict__ feat, const float* __restrict__ proj, const float* __restrict__ depth,
                                                            int V, int H, int W, int D, int pad, const float* __restrict__ g_cost, int CP, int c_var,
                                                            float* __restrict__ g_feat)
{
    // Two phases per workgroup of 256 voxels.  (1) one thread per voxel: projection into every source view (7 divisions per view),
    // bilinear weights and tap indices -> LDS.  (2) one thread per (voxel, channel), 8 voxels per pass: the 32 lanes of a voxel read /
    // atomically update one contiguous 128-byte channel vector per tap (a per-voxel thread with a channel loop issues 4-byte atomics
    // 128 B apart: 10x slower; eight lanes x four channels per voxel: 4x the L2 atomic line visits, slower as well).  Phase 1 used to
    // be repeated by all 32 lanes of every voxel, and the kernel was bound by that arithmetic (2.3 ms).
    constexpr int VPB = 256;
    extern __shared__ __attribute__((aligned(16))) float geo[];    // [VPB][GS]: per source view {w_nw,w_ne,w_sw,w_se, t_nw,t_ne,t_sw,t_se}, then {1/count, ref pixel}
    const int GS = (V - 1) * 8 + 2;
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const int64_t nvox = (int64_t)D * Hp * Wp;
    const int64_t v0 = (int64_t)blockIdx.x * VPB;
    {
        const int64_t i = v0 + threadIdx.x;
        if (i < nvox) {
            float* o = geo + threadIdx.x * GS;
            const int x = (int)(i % Wp), y = (int)((i / Wp) % Hp), d = (int)(i / ((int64_t)Wp * Hp));
            const float u = (float)(x - pad), v = (float)(y - pad), dep = depth[d];
            const bool interior = x >= pad && x < W + pad && y >= pad && y < H + pad;
            float cnt = 1.0f;
            for (int vv = 1; vv < V; ++vv) {
                const float* P = proj + vv * 12;
                const float p0 = fmaf(P[2], 1.0f, fmaf(P[1], v, P[0] * u)) + P[3] / dep;
                const float p1 = fmaf(P[6], 1.0f, fmaf(P[5], v, P[4] * u)) + P[7] / dep;
                const float p2 = fmaf(P[10], 1.0f, fmaf(P[9], v, P[8] * u)) + P[11] / dep;
                const float gx = (p0 / p2) / ((float)(W - 1) / 2.0f) - 1.0f, gy = (p1 / p2) / ((float)(H - 1) / 2.0f) - 1.0f;
                cnt += (gx > -1.0f && gx < 1.0f && gy > -1.0f && gy < 1.0f) ? 1.0f : 0.0f;
                const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
                const float fx = floorf(ix), fy = floorf(iy);
                const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix, wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
                const bool x0in = fx >= 0.f && fx <= (float)(W - 1), x1in = fx + 1.f >= 0.f && fx + 1.f <= (float)(W - 1);
                const bool y0in = fy >= 0.f && fy <= (float)(H - 1), y1in = fy + 1.f >= 0.f && fy + 1.f <= (float)(H - 1);
                float* ov = o + (vv - 1) * 8;
                ov[0] = (x0in && y0in) ? wx0 * wy0 : 0.f; ov[1] = (x1in && y0in) ? wx1 * wy0 : 0.f;
                ov[2] = (x0in && y1in) ? wx0 * wy1 : 0.f; ov[3] = (x1in && y1in) ? wx1 * wy1 : 0.f;
                const bool any = (x0in || x1in) && (y0in || y1in);
                const int xa = any ? min(max((int)fx, 0), W - 1) : 0, xb = any ? min(max((int)fx + 1, 0), W - 1) : 0;
                const int ya = any ? min(max((int)fy, 0), H - 1) : 0, yb = any ? min(max((int)fy + 1, 0), H - 1) : 0;
                ov[4] = __int_as_float(ya * W + xa); ov[5] = __int_as_float(ya * W + xb);
                ov[6] = __int_as_float(yb * W + xa); ov[7] = __int_as_float(yb * W + xb);
            }
            o[(V - 1) * 8] = 1.0f / cnt;
            o[(V - 1) * 8 + 1] = __int_as_float(interior ? (y - pad) * W + (x - pad) : -1);
        }
    }
    __syncthreads();
    const int c = threadIdx.x & (C - 1);
    constexpr int MAXV = 8;
    for (int vl = threadIdx.x / C; vl < VPB; vl += 256 / C) {
        const int64_t i = v0 + vl;
        if (i >= nvox) break;
        const float* o = geo + vl * GS;
        const float inv = o[(V - 1) * 8];
        const int refpix = __float_as_int(o[(V - 1) * 8 + 1]);
        const float gv = g_cost[i * CP + c_var + c];
        const float ref = refpix >= 0 ? feat[(int64_t)refpix * C + c] : 0.f;
        float s = ref;
        float wv[MAXV];
        for (int vv = 1; vv < V; ++vv) {
            const float* ov = o + (vv - 1) * 8;
            const float* fb = feat + (int64_t)vv * H * W * C + c;
            wv[vv] = fmaf(fb[(int64_t)__float_as_int(ov[7]) * C], ov[3], fmaf(fb[(int64_t)__float_as_int(ov[6]) * C], ov[2],
                          fmaf(fb[(int64_t)__float_as_int(ov[5]) * C], ov[1], fb[(int64_t)__float_as_int(ov[4]) * C] * ov[0])));
            s += wv[vv];
        }
        const float k2 = gv * 2.0f * inv, mean = s * inv;
        if (refpix >= 0) atomicAdd(g_feat + (int64_t)refpix * C + c, k2 * (ref - mean));
        for (int vv = 1; vv < V; ++vv) {
            const float* ov = o + (vv - 1) * 8;
            float* gb = g_feat + (int64_t)vv * H * W * C + c;
            const float gw_ = k2 * (wv[vv] - mean);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ov[k] != 0.f) atomicAdd(gb + (int64_t)__float_as_int(ov[4 + k]) * C, gw_ * ov[k]);
        }
    }
}


// ---- helpers of the deterministic plane-sweep backward: largest magnitudes (float bits order like unsigned integers for x >= 0), the
// fixed-point scale every thread derives from them, and the conversion back
__global__ __launch_bounds__(256) void absmax_strided_kernel(const float* __restrict__ x, int64_t n_rows, int ld, int c0, int nc, unsigned* __restrict__ out)
{
    float m = 0.f;
    const int64_t n = n_rows * nc;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / nc;
        const float a = fabsf(x[r * ld + c0 + (int)(i - r * nc)]);
        if (a < __builtin_inff()) m = fmaxf(m, a);                    // the largest FINITE magnitude: an inf or NaN must not cost the finite sums their scale
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(out, __float_as_uint(m));
}
__device__ __forceinline__ float psw_fix_scale(const unsigned* mx)
{
    const float b = __uint_as_float(mx[0]) * __uint_as_float(mx[1]);
    if (!(b > 0.f) || !(b < 3.0e38f)) return 1.0f;
    int e;
    frexpf(b, &e);                                                    // b in [2^(e-1), 2^e)
    return ldexpf(1.0f, max(-120, min(120, 36 - e)));
}
__global__ __launch_bounds__(256) void psw_fix_to_float_kernel(const long long* __restrict__ fix, int64_t n, float* __restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float inv = 1.0f / psw_fix_scale(reinterpret_cast<const unsigned*>(fix + n));
    const long long v = fix[i];
    if (v != 0) dst[i] += (float)((double)v * (double)inv);
}

// ---- plane-sweep backward, column form.  A thread owns ONE channel of ONE voxel column (x, y) and walks the depth planes itself.  Along
// a column the sample point in a source view moves by the disparity step - a fraction of a pixel per plane for any rig the sweep is meant
// for (0.07 px at config 2) - so the four tap PIXELS stay the same for many consecutive planes; only the bilinear weights change.  The
// thread therefore keeps, per source view, the four tap values and four gradient accumulators in registers and touches memory only when
// the tap set changes: it sends the accumulators (one float atomic per tap with a non-zero sum) and gathers the new taps.  At config 2
// that is ~10 tap sets per column and view over 128 planes: the gathers and the atomics of the scatter kernel divided by ~13, no LDS
// atomics, no patch, and each gradient value of the cost volume is read exactly once (the tile form read it once per channel half too,
// but per plane it paid 36 gathers and 36 LDS atomics per thread).  What remains per plane and thread is one coalesced 4-byte load,
// the geometry from LDS and ~30 multiply-adds.  A rig whose taps move every plane degrades to the scatter kernel's traffic, not below it.
//   Workgroup = NV = 8 consecutive columns of one row x 32 channels.  Geometry (7 divisions per voxel and view) is computed once per
// voxel, DCH planes at a time: NV x NSRC x DCH items over the 256 threads -> LDS -> read back by the 32 channel lanes (broadcast reads).
// The reference view's gradient of a pixel has exactly one column contributing: register sum over all planes, one plain read-add-write.
// FIX (the deterministic variant, mvsnerf_planesweep_costvar_bwd_det): the source views' sums go to 64-bit FIXED-POINT accumulators - integer
// additions commute, so the result does not depend on the order in which the columns' atomics arrive (float atomics: last-bit differences
// from run to run).  fix = {int64 [NSRC][H][W][C] | float bits of max |g_cost|, max |feat|}: a contribution is rounded to a multiple of
// 2^-k with k = 36 - ceil(log2(max|g| * max|feat|)) (relative 2^-36 of the largest possible contribution: far below fp32's 2^-24) and
// 2^24.3 voxels x 4 |g| |feat| 2^k stay below 2^63.  The two maxima are those of the FINITE values, and a column sum that is inf or NaN (one such value in
// g_cost is enough) is added to the gradient by a float atomic instead: the elements the float-atomic variant makes non-finite are non-finite here.
template <int C, int NSRC, bool FIX>
__global__ __launch_bounds__(256) void planesweep_bwd_columns_kernel(const float* __restrict__ feat, const float* __restrict__ proj,
                                                                     const float* __restrict__ depth, int H, int W, int D, int pad,
                                                                     const float* __restrict__ g_cost, int CP, int c_var, float* __restrict__ g_feat,
                                                                     long long* __restrict__ fix)
{
    static_assert(C == 32, "one lane per channel, 8 columns per workgroup");
    constexpr int NV = 8, DCH = 16, GI = 12;                          // columns per workgroup, planes per geometry batch, floats per item
    // per (plane, column, source view): {w_nw,w_ne,w_sw,w_se | byte offset of the 4 tap pixels in a feature map | view counts (0/1), -, -, -}
    __shared__ __attribute__((aligned(16))) float geo[DCH * NV * NSRC * GI];
    const int tid = threadIdx.x;
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const int nbx = (Wp + NV - 1) / NV;
    const int y = blockIdx.x / nbx, x0 = (blockIdx.x - y * nbx) * NV;
    const float sx = (float)(W - 1) / 2.0f, sy = (float)(H - 1) / 2.0f;
    const int vl = tid >> 5, c = tid & 31, x = x0 + vl;
    const bool valid = x < Wp;
    const bool interior = valid && x >= pad && x < W + pad && y >= pad && y < H + pad;
    const int64_t refoff = interior ? ((int64_t)(y - pad) * W + (x - pad)) * C + c : 0;
    const float ref = interior ? feat[refoff] : 0.f;
    float racc = 0.f;
    int4 cur[NSRC];                                                   // tap set in the registers (byte offsets), -1: none yet
    float tap[NSRC][4], acc[NSRC][4];
#pragma unroll
    for (int vs = 0; vs < NSRC; ++vs) {
        cur[vs] = int4{-1, -1, -1, -1};
#pragma unroll
        for (int k = 0; k < 4; ++k) { tap[vs][k] = 0.f; acc[vs][k] = 0.f; }
    }
    float fix_scale = 1.0f;
    if (FIX) fix_scale = psw_fix_scale(reinterpret_cast<const unsigned*>(fix + (int64_t)NSRC * H * W * C));
    auto send = [&](int vs) {
        float* gview = g_feat + (int64_t)(vs + 1) * H * W * C + c;
        const int o[4] = {cur[vs].x, cur[vs].y, cur[vs].z, cur[vs].w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (acc[vs][k] != 0.f) {
                if (FIX) {
                    // a sum that is inf or NaN (or overflows under the scale) has no fixed-point value: (long long)rintf(NaN) is 0 and an inf saturates to a
                    // finite 2^63, so it goes to the gradient by the float atomic, as in the float-atomic entry, and the element ends non-finite
                    const float scaled = acc[vs][k] * fix_scale;
                    if ((__float_as_uint(scaled) & 0x7f800000u) == 0x7f800000u) atomicAdd(gview + (o[k] >> 2), acc[vs][k]);
                    else atomicAdd(reinterpret_cast<unsigned long long*>(fix + (int64_t)vs * H * W * C + c + (o[k] >> 2)), (unsigned long long)(long long)rintf(scaled));
                }
                else atomicAdd(gview + (o[k] >> 2), acc[vs][k]);
                acc[vs][k] = 0.f;
            }
    };
    const float* gcol = g_cost + ((int64_t)y * Wp + x) * CP + c_var + c;
    const int64_t gplane = (int64_t)Hp * Wp * CP;
    for (int d0 = 0; d0 < D; d0 += DCH) {
        // ---- geometry of DCH planes x NV columns x NSRC views
        for (int it = tid; it < DCH * NV * NSRC; it += 256) {
            const int dl = it / (NV * NSRC), r = it - dl * (NV * NSRC), pv = r / NSRC, vs = r - pv * NSRC;
            const int d = min(d0 + dl, D - 1), vx = x0 + pv;
            const bool pvalid = vx < Wp;
            const float u = (float)(vx - pad), v = (float)(y - pad), dep = depth[d];
            const float* P = proj + (vs + 1) * 12;
            const float p0 = fmaf(P[2], 1.0f, fmaf(P[1], v, P[0] * u)) + P[3] / dep;
            const float p1 = fmaf(P[6], 1.0f, fmaf(P[5], v, P[4] * u)) + P[7] / dep;
            const float p2 = fmaf(P[10], 1.0f, fmaf(P[9], v, P[8] * u)) + P[11] / dep;
            const float gx = (p0 / p2) / sx - 1.0f, gy = (p1 / p2) / sy - 1.0f;
            const bool inside = gx > -1.0f && gx < 1.0f && gy > -1.0f && gy < 1.0f;
            const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
            const float fxx = floorf(ix), fyy = floorf(iy);
            const float wx1 = ix - fxx, wx0 = (fxx + 1.0f) - ix, wy1 = iy - fyy, wy0 = (fyy + 1.0f) - iy;
            const bool x0in = fxx >= 0.f && fxx <= (float)(W - 1), x1in = fxx + 1.f >= 0.f && fxx + 1.f <= (float)(W - 1);
            const bool y0in = fyy >= 0.f && fyy <= (float)(H - 1), y1in = fyy + 1.f >= 0.f && fyy + 1.f <= (float)(H - 1);
            const bool any = pvalid && (x0in || x1in) && (y0in || y1in);
            const int xa = any ? min(max((int)fxx, 0), W - 1) : 0, xb = any ? min(max((int)fxx + 1, 0), W - 1) : 0;
            const int ya = any ? min(max((int)fyy, 0), H - 1) : 0, yb = any ? min(max((int)fyy + 1, 0), H - 1) : 0;
            float* ov = geo + it * GI;
            *reinterpret_cast<f32x4*>(ov) = f32x4{(any && x0in && y0in) ? wx0 * wy0 : 0.f, (any && x1in && y0in) ? wx1 * wy0 : 0.f,
                                                  (any && x0in && y1in) ? wx0 * wy1 : 0.f, (any && x1in && y1in) ? wx1 * wy1 : 0.f};
            *reinterpret_cast<int4*>(ov + 4) = int4{(ya * W + xa) * C * 4, (ya * W + xb) * C * 4, (yb * W + xa) * C * 4, (yb * W + xb) * C * 4};
            ov[8] = (pvalid && inside) ? 1.0f : 0.0f;
        }
        // this thread's DCH gradient values: all loads in flight before the first is used
        float gv[DCH];
#pragma unroll
        for (int dl = 0; dl < DCH; ++dl) gv[dl] = (valid && d0 + dl < D) ? gcol[(int64_t)(d0 + dl) * gplane] : 0.f;
        __syncthreads();
#pragma unroll 2
        for (int dl = 0; dl < DCH; ++dl) {
            const float* o = geo + (dl * NV + vl) * NSRC * GI;
            float cnt = 1.0f, s = ref, wv[NSRC];
            f32x4 wq[NSRC];
#pragma unroll
            for (int vs = 0; vs < NSRC; ++vs) {
                wq[vs] = *reinterpret_cast<const f32x4*>(o + vs * GI);
                const int4 gb = *reinterpret_cast<const int4*>(o + vs * GI + 4);
                cnt += o[vs * GI + 8];
                if ((gb.x != cur[vs].x) | (gb.w != cur[vs].w)) {   // new tap set (the nw and se offsets determine all four pixels): send, gather
                    send(vs);
                    cur[vs] = gb;
                    const char* fb = reinterpret_cast<const char*>(feat + (int64_t)(vs + 1) * H * W * C + c);
                    tap[vs][0] = *reinterpret_cast<const float*>(fb + gb.x); tap[vs][1] = *reinterpret_cast<const float*>(fb + gb.y);
                    tap[vs][2] = *reinterpret_cast<const float*>(fb + gb.z); tap[vs][3] = *reinterpret_cast<const float*>(fb + gb.w);
                }
                wv[vs] = fmaf(tap[vs][3], wq[vs][3], fmaf(tap[vs][2], wq[vs][2], fmaf(tap[vs][1], wq[vs][1], tap[vs][0] * wq[vs][0])));
                s += wv[vs];
            }
            const float inv = __builtin_amdgcn_rcpf(cnt);                // cnt = 1 .. V: v_rcp_f32 (<= 1 ulp) instead of the ten-instruction IEEE division, per plane and thread
            const float k2 = gv[dl] * 2.0f * inv, mean = s * inv;
            racc += k2 * (ref - mean);
#pragma unroll
            for (int vs = 0; vs < NSRC; ++vs) {
                const float gw_ = k2 * (wv[vs] - mean);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[vs][k] = fmaf(gw_, wq[vs][k], acc[vs][k]);
            }
        }
        __syncthreads();                                              // the next batch overwrites geo
    }
#pragma unroll
    for (int vs = 0; vs < NSRC; ++vs) send(vs);
    if (interior) g_feat[refoff] += racc;                             // the only contribution to this element of view 0
}


template <int NSRC>
static int planesweep_bwd_columns_launch(const float* feat, const float* proj, const float* depth, int H, int W, int D, int pad, const float* g_cost,
                                         int CP, int c_var, float* g_feat, long long* fix, hipStream_t st)
{
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const unsigned grid = (unsigned)(Hp * ((Wp + 7) / 8));
    if (!fix) {
        planesweep_bwd_columns_kernel<32, NSRC, false><<<grid, 256, 0, st>>>(feat, proj, depth, H, W, D, pad, g_cost, CP, c_var, g_feat, nullptr);
        MVS_LAUNCH_CHECK();
        return MVSNERF_OK;
    }
    const int64_t n = (int64_t)NSRC * H * W * 32;
    unsigned* mx = reinterpret_cast<unsigned*>(fix + n);
    absmax_strided_kernel<<<1024, 256, 0, st>>>(g_cost, (int64_t)D * Hp * Wp, CP, c_var, 32, mx);
    absmax_strided_kernel<<<256, 256, 0, st>>>(feat, (int64_t)(NSRC + 1) * H * W, 32, 0, 32, mx + 1);
    planesweep_bwd_columns_kernel<32, NSRC, true><<<grid, 256, 0, st>>>(feat, proj, depth, H, W, D, pad, g_cost, CP, c_var, g_feat, fix);
    psw_fix_to_float_kernel<<<mvs_cdiv(n, 256), 256, 0, st>>>(fix, n, g_feat + (int64_t)H * W * 32);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}


static int planesweep_costvar_bwd_impl(const float* feats_cl, const float* proj, const float* depth, int V, int C, int H, int W, int D, int pad,
                                       const float* g_cost, int CP, int with_img, float* g_feats_cl, long long* fix, void* stream)
{
    if (!feats_cl || !proj || !depth || !g_cost || !g_feats_cl || V < 1 || V > 8 || H < 2 || W < 2 || D < 1 || pad < 0) return MVSNERF_EINVAL;
    if (C != 32) return MVSNERF_EUNSUPPORTED;
    const int64_t nvox = (int64_t)D * (H + 2 * pad) * (W + 2 * pad);
    if (V >= 2) {                                           // column form; a single view has no taps to keep: the per-voxel scatter below
        hipStream_t st = (hipStream_t)stream;
        const int cv = with_img ? 3 * V : 0;
        switch (V - 1) {
#define MVS_PBC(N) case N: return planesweep_bwd_columns_launch<N>(feats_cl, proj, depth, H, W, D, pad, g_cost, CP, cv, g_feats_cl, fix, st)
            MVS_PBC(1); MVS_PBC(2); MVS_PBC(3); MVS_PBC(4); MVS_PBC(5); MVS_PBC(6); MVS_PBC(7);
#undef MVS_PBC
        }
    }
    const size_t lds = (size_t)256 * ((V - 1) * 8 + 2) * sizeof(float);
    planesweep_bwd_kernel<32><<<mvs_cdiv(nvox, 256), 256, lds, (hipStream_t)stream>>>(feats_cl, proj, depth, V, H, W, D, pad, g_cost, CP,
                                                                                    with_img ? 3 * V : 0, g_feats_cl);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_planesweep_costvar_bwd(const float* feats_cl, const float* proj, const float* depth, int V, int C, int H, int W, int D, int pad,
                                              const float* g_cost, int CP, int with_img, float* g_feats_cl, void* stream)
{
    return planesweep_costvar_bwd_impl(feats_cl, proj, depth, V, C, H, W, D, pad, g_cost, CP, with_img, g_feats_cl, nullptr, stream);
}

// int64 words of the deterministic variant's workspace (zeroed by the caller before every call)
extern "C" size_t mvsnerf_planesweep_costvar_bwd_det_workspace_words(int V, int C, int H, int W)
{
    return V >= 1 && C == 32 && H >= 1 && W >= 1 ? (size_t)(V > 1 ? V - 1 : 0) * H * W * C + 1 : 0;
}

extern "C" int mvsnerf_planesweep_costvar_bwd_det(const float* feats_cl, const float* proj, const float* depth, int V, int C, int H, int W, int D, int pad,
                                                  const float* g_cost, int CP, int with_img, float* g_feats_cl, void* workspace_zeroed, void* stream)
{
    if (!workspace_zeroed || ((uintptr_t)workspace_zeroed & 7)) return workspace_zeroed ? MVSNERF_EALIGN : MVSNERF_EINVAL;
    return planesweep_costvar_bwd_impl(feats_cl, proj, depth, V, C, H, W, D, pad, g_cost, CP, with_img, g_feats_cl,
                                       reinterpret_cast<long long*>(workspace_zeroed), stream);
}
