// A density volume the renderer can be held to: the node coordinates of a (D,H,W) volume in the renderer's own NDC frame (and the world
// positions they come from), and a grid-clipped maximum filter that widens the occupied region by r voxels.  No counterpart in the reference: its
// density volume (train_mvs_nerf_finetuning_pl.py:91-99) is queried at world positions, which is not what its renderer feeds the MLP.
//
// voxel_points_kernel  one thread per node (k,j,i) of planes [d0, d1): ndc = (i/(W-1), j/(H-1), k/(D-1)) by IEEE divisions (an axis of size 1 gives 0) -
//                      the coordinates at which density_cell.h's floor(((x*2-1 + 1) / 2) * (W-1)) lands on node i.  The world position inverts
//                      get_ndc_coordinate (utils.py:112-146; ray_points_kernel, importance.hip): pixel u = x * au + bu (the pad undone, then
//                      * (W_img - 1); au, bu formed on the host in double), depth z = near + z_ndc (far - near) (lindisp: the same in 1/z), then
//                      world = M (u z, v z, z) + t with M = R_c2w K^-1 formed on the host in double - nine multiply-adds here.
//                      The 256 rows of a workgroup meet in LDS (stride 3 dwords: no bank conflict) and leave as 192 dwordx4 stores when the output is
//                      16-byte aligned (a workgroup's first row is a multiple of 3072 bytes in), else as three coalesced dword stores per thread.
// max_dilate_axis_kernel  out[v] = max of in over [p - r, p + r] clipped to [0, L) along ONE axis (stride 1, W or H * W); a NaN in the window gives NaN.
//                      One thread per voxel, the loads of a wave are contiguous for every axis.  Three passes (W, H, D) through a caller-owned
//                      workspace make the (2r+1)^3 window: max is associative and the clipped box is the product of the clipped intervals.
// max_dilate_axis4_kernel  the same pass with four consecutive voxels of a row per thread and 16-byte accesses, taken when W % 4 == 0 and the three
//                      buffers are 16-byte aligned (every volume the encoder emits: W = W_img / 4 + 2 pad with pad a multiple of 4 or W_img of 16).
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int VP_THREADS = 256;

struct VoxelCam {
    float au, bu, av, bv;          // pixel = ndc * a + b
    float z0, dz;                  // z = z0 + z_ndc * dz  (lindisp: 1 / z)
    float m[9], t[3];              // world = m (u z, v z, z) + t
    int lindisp;
};

__device__ __forceinline__ float unit_coord(int i, int n) { return n > 1 ? __fdiv_rn((float)i, (float)(n - 1)) : 0.0f; }

__global__ __launch_bounds__(VP_THREADS) void voxel_points_kernel(int H, int W, int D, int d0, int64_t n, VoxelCam cam,
                                                                  float* __restrict__ ndc, float* __restrict__ pts, int vec4)
{
    __shared__ __attribute__((aligned(16))) float s_ndc[VP_THREADS * 3];
    __shared__ __attribute__((aligned(16))) float s_pts[VP_THREADS * 3];
    const int64_t row0 = (int64_t)blockIdx.x * VP_THREADS;
    const int64_t t = row0 + threadIdx.x;
    const int rows = (int)(n - row0 < VP_THREADS ? n - row0 : VP_THREADS);
    if (t < n) {
        int i, j, k;
        mvs_unflatten3(t, W, H, i, j, k);
        const float x = unit_coord(i, W), y = unit_coord(j, H), zn = unit_coord(k + d0, D);
        s_ndc[threadIdx.x * 3 + 0] = x; s_ndc[threadIdx.x * 3 + 1] = y; s_ndc[threadIdx.x * 3 + 2] = zn;
        if (pts) {
            const float u = fmaf(x, cam.au, cam.bu), v = fmaf(y, cam.av, cam.bv);
            float z = fmaf(zn, cam.dz, cam.z0);
            if (cam.lindisp) z = __fdiv_rn(1.0f, z);
            const float qx = u * z, qy = v * z;
            s_pts[threadIdx.x * 3 + 0] = fmaf(cam.m[2], z, fmaf(cam.m[1], qy, fmaf(cam.m[0], qx, cam.t[0])));
            s_pts[threadIdx.x * 3 + 1] = fmaf(cam.m[5], z, fmaf(cam.m[4], qy, fmaf(cam.m[3], qx, cam.t[1])));
            s_pts[threadIdx.x * 3 + 2] = fmaf(cam.m[8], z, fmaf(cam.m[7], qy, fmaf(cam.m[6], qx, cam.t[2])));
        }
    }
    __syncthreads();
    if (rows <= 0) return;
    const int total = rows * 3;                                          // <= 768 floats of this workgroup's rows, contiguous in the output
    if (vec4 && rows == VP_THREADS) {
        if (threadIdx.x < VP_THREADS * 3 / 4) {
            reinterpret_cast<f32x4*>(ndc + row0 * 3)[threadIdx.x] = reinterpret_cast<const f32x4*>(s_ndc)[threadIdx.x];
            if (pts) reinterpret_cast<f32x4*>(pts + row0 * 3)[threadIdx.x] = reinterpret_cast<const f32x4*>(s_pts)[threadIdx.x];
        }
    } else {
        for (int e = threadIdx.x; e < total; e += VP_THREADS) {
            ndc[row0 * 3 + e] = s_ndc[e];
            if (pts) pts[row0 * 3 + e] = s_pts[e];
        }
    }
}

__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }      // a NaN, once taken, stays: NaN > x and x > NaN are false

__global__ __launch_bounds__(256) void max_dilate_axis_kernel(const float* __restrict__ in, float* __restrict__ out, unsigned n, unsigned stride, unsigned L, int r)
{
    const unsigned v = blockIdx.x * 256u + threadIdx.x;                  // n < 2^31: 32-bit index arithmetic
    if (v >= n) return;
    const int p = (int)((v / stride) % L);
    float m = in[v];
    for (int o = 1; o <= r; ++o) {
        if (p - o >= 0) m = max_nan(m, in[v - (unsigned)o * stride]);
        if (p + o < (int)L) m = max_nan(m, in[v + (unsigned)o * stride]);
    }
    out[v] = m;
}

__device__ __forceinline__ f32x4 max_nan4(f32x4 m, f32x4 v)
{
    return f32x4{max_nan(m.x, v.x), max_nan(m.y, v.y), max_nan(m.z, v.z), max_nan(m.w, v.w)};
}

// The same pass for W % 4 == 0 and 16-byte aligned volumes: a thread owns four consecutive voxels of a row (one quad) and moves 16 bytes per access.
// n4 quads; along_w: L = quads per row, the window reaches into the two neighbouring quads of the row (r <= 2 < 4); else stride4 = quads between
// neighbours on the axis (W/4 or H*W/4) and L the axis length.  A neighbour outside the grid counts as -inf: the window always holds its own centre,
// so that value never comes out, and a NaN still does.
__global__ __launch_bounds__(256) void max_dilate_axis4_kernel(const f32x4* __restrict__ in, f32x4* __restrict__ out, unsigned n4, unsigned stride4, unsigned L, int r,
                                                               int along_w)
{
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n4) return;
    const f32x4 c = in[q];
    f32x4 m = c;
    if (along_w) {
        const unsigned pq = q % L;
        const float ninf = -INFINITY;
        f32x4 lo = {ninf, ninf, ninf, ninf}, hi = lo;
        if (pq > 0) lo = in[q - 1];
        if (pq + 1 < L) hi = in[q + 1];
        const float a[8] = {lo.z, lo.w, c.x, c.y, c.z, c.w, hi.x, hi.y};
        float o4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = a[e + 2];
#pragma unroll
            for (int o = 1; o <= 2; ++o)
                if (o <= r) v = max_nan(max_nan(v, a[e + 2 - o]), a[e + 2 + o]);
            o4[e] = v;
        }
        m = f32x4{o4[0], o4[1], o4[2], o4[3]};
    } else {
        const int p = (int)((q / stride4) % L);
        for (int o = 1; o <= r; ++o) {
            if (p - o >= 0) m = max_nan4(m, in[q - (unsigned)o * stride4]);
            if (p + o < (int)L) m = max_nan4(m, in[q + (unsigned)o * stride4]);
        }
    }
    out[q] = m;
}

// 3 x 3 inverse in double; false for a matrix that has none (or is not finite)
bool invert3(const double* a, double* inv)
{
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c0 + a[1] * c1 + a[2] * c2;
    if (!(det != 0.0) || !std::isfinite(det)) return false;
    const double s = 1.0 / det;
    inv[0] = c0 * s; inv[1] = (a[2] * a[7] - a[1] * a[8]) * s; inv[2] = (a[1] * a[5] - a[2] * a[4]) * s;
    inv[3] = c1 * s; inv[4] = (a[0] * a[8] - a[2] * a[6]) * s; inv[5] = (a[2] * a[3] - a[0] * a[5]) * s;
    inv[6] = c2 * s; inv[7] = (a[1] * a[6] - a[0] * a[7]) * s; inv[8] = (a[0] * a[4] - a[1] * a[3]) * s;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(inv[i])) return false;
    return true;
}

}  // namespace

extern "C" int mvsnerf_voxel_points_fwd(int D, int H, int W, int d0, int d1, const float* K_ref, const float* c2w_ref, const float* near_far,
                                        int W_img, int H_img, int pad, int lindisp, float* ndc, float* pts, void* stream)
{
    if (!ndc || D < 1 || H < 1 || W < 1 || d0 < 0 || d1 < d0 || d1 > D) return MVSNERF_EINVAL;
    if ((int64_t)D * H * W >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    VoxelCam cam = {};
    if (pts) {
        if (!K_ref || !c2w_ref || !near_far || W_img < 2 || H_img < 2 || pad < 0) return MVSNERF_EINVAL;
        double K[9], Kinv[9];
        for (int i = 0; i < 9; ++i) K[i] = K_ref[i];
        if (!invert3(K, Kinv)) return MVSNERF_EINVAL;
        const double near = near_far[0], far = near_far[1];
        if (!std::isfinite(near) || !std::isfinite(far) || (lindisp && (near == 0.0 || far == 0.0))) return MVSNERF_EINVAL;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c)
                cam.m[r * 3 + c] = (float)(c2w_ref[r * 4 + 0] * Kinv[c] + c2w_ref[r * 4 + 1] * Kinv[3 + c] + (double)c2w_ref[r * 4 + 2] * Kinv[6 + c]);
            cam.t[r] = c2w_ref[r * 4 + 3];
        }
        // x = q wf / (wf + 2 pad) + pad / (wf + 2 pad), q = u / (W_img - 1), wf = W_img / 4 (get_ndc_coordinate)  =>  u = x au + bu
        const double wf = W_img / 4.0, hf = H_img / 4.0;
        cam.au = (float)((wf + 2.0 * pad) / wf * (W_img - 1)); cam.bu = (float)(-(double)pad / wf * (W_img - 1));
        cam.av = (float)((hf + 2.0 * pad) / hf * (H_img - 1)); cam.bv = (float)(-(double)pad / hf * (H_img - 1));
        cam.z0 = (float)(lindisp ? 1.0 / near : near);
        cam.dz = (float)(lindisp ? 1.0 / far - 1.0 / near : far - near);
        cam.lindisp = lindisp ? 1 : 0;
    }
    auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; };
    if (mis(ndc) || mis(pts)) return MVSNERF_EALIGN;
    const int64_t n = (int64_t)(d1 - d0) * H * W;
    if (n == 0) return MVSNERF_OK;
    const int vec4 = mvs_aligned16(ndc) && (!pts || mvs_aligned16(pts));
    voxel_points_kernel<<<mvs_cdiv(n, VP_THREADS), VP_THREADS, 0, (hipStream_t)stream>>>(H, W, D, d0, n, cam, ndc, pts, vec4);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_max_dilate3d_fwd(const float* in, int D, int H, int W, int r, float* out, float* workspace, void* stream)
{
    if (!in || !out || D < 1 || H < 1 || W < 1 || r < 0 || r > 2 || in == out) return MVSNERF_EINVAL;
    if (r > 0 && (!workspace || workspace == in || workspace == out)) return MVSNERF_EINVAL;
    if ((int64_t)D * H * W >= ((int64_t)1 << 31)) return MVSNERF_EUNSUPPORTED;
    auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; };
    if (mis(in) || mis(out) || mis(workspace)) return MVSNERF_EALIGN;
    const unsigned n = (unsigned)((int64_t)D * H * W);
    const unsigned grid = mvs_cdiv(n, 256);
    hipStream_t st = (hipStream_t)stream;
    if ((W & 3) == 0 && mvs_aligned16(in) && mvs_aligned16(out) && (r == 0 || mvs_aligned16(workspace))) {
        const unsigned n4 = n / 4, w4 = (unsigned)W / 4, grid4 = mvs_cdiv(n4, 256);
        const f32x4* in4 = reinterpret_cast<const f32x4*>(in);
        f32x4 *out4 = reinterpret_cast<f32x4*>(out), *ws4 = reinterpret_cast<f32x4*>(workspace);
        max_dilate_axis4_kernel<<<grid4, 256, 0, st>>>(in4, out4, n4, 1u, w4, r, 1);
        MVS_LAUNCH_CHECK();
        if (r == 0) return MVSNERF_OK;
        max_dilate_axis4_kernel<<<grid4, 256, 0, st>>>(out4, ws4, n4, w4, (unsigned)H, r, 0);
        MVS_LAUNCH_CHECK();
        max_dilate_axis4_kernel<<<grid4, 256, 0, st>>>(ws4, out4, n4, w4 * (unsigned)H, (unsigned)D, r, 0);
        MVS_LAUNCH_CHECK();
        return MVSNERF_OK;
    }
    if (r == 0) {
        max_dilate_axis_kernel<<<grid, 256, 0, st>>>(in, out, n, 1u, (unsigned)W, 0);                 // a window of one voxel: the copy
        MVS_LAUNCH_CHECK();
        return MVSNERF_OK;
    }
    max_dilate_axis_kernel<<<grid, 256, 0, st>>>(in, out, n, 1u, (unsigned)W, r);
    MVS_LAUNCH_CHECK();
    max_dilate_axis_kernel<<<grid, 256, 0, st>>>(out, workspace, n, (unsigned)W, (unsigned)H, r);
    MVS_LAUNCH_CHECK();
    max_dilate_axis_kernel<<<grid, 256, 0, st>>>(workspace, out, n, (unsigned)W * (unsigned)H, (unsigned)D, r);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
