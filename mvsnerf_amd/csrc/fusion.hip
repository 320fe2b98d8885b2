// Fusing per-view neural volumes into one scene volume (reference train_mvs_nerf_fusion_finetuning_pl.py): the splat of ray samples into a
// world-space voxel grid (update_volume, :35-76), its normalisation (fuse_local_volumes, :190-192) and the ray march against an axis-aligned
// box (dda / ray_marcher(bbox_3D=), data/ray_utils.py:143-197).
#include "common.h"

// ---------------------------------------------------------------------------------------------
// update_volume with a DEFINED sum.  The reference writes `vol[..., idx] += x` with repeated indices (:74-76), which keeps one of the colliding
// writes on a GPU; here every contribution is accumulated, through the order-independent 64-bit fixed-point scatter of
// volume_sample_bwd_det_scatter_kernel (sample.hip): the fp32 product is rounded ONCE to a multiple of 2^-32 and added with an integer atomic, so
// the sums do not depend on the order of the points, of the views or of the ranks.  The scale is FIXED (the gradient scatter finds one per call):
// an accumulator outlives a call and is added to others filled elsewhere.  |product| >= 2^20 (and anything non-finite) is refused and recorded
// in the header; 2^11 maximal contributions fit a word.
// workspace (int64 words, zeroed by the caller):
//   [0] number of refused contributions (non-zero: the accumulator is invalid)   [1] log2 of the scale (32; written by the first non-empty splat)
//   [2..7] unused
//   [8 + v * (C + 4) ..] voxel v = (d * H + h) * W + w: C feature sums, the alpha sum, the weight sum, 2 pad words - one corner update touches
//   one contiguous row (192 B at C = 20).
// The arithmetic is the reference's, quirks included: v = ndc / (1 / (dim - 1)) by two correctly rounded divisions, the index truncated toward zero
// (v in (-1, 0) lands on voxel 0 with local = v + 1), the weight |local - shift| - that of the OPPOSITE corner - and the x / z shifts swapped
// between weight and target voxel.
// G = 16 / 32 / 64 lanes per point run along the C + 2 summed words of a voxel row (an atomic wave-instruction covers 64 / G contiguous runs);
// points spread the rows.  Packing C + 2 lanes per point instead, so that no lane idles, measured 4-7 % SLOWER at C = 12, 20 and 40 (the runs of a
// wave-instruction then straddle its points); the kernel runs at the atomic rate either way, the per-lane recomputation of the weights is hidden.
// ---------------------------------------------------------------------------------------------
#define FUSE_HEADER_WORDS 8
#define FUSE_SCALE_LOG2 32

template <int G>
__global__ __launch_bounds__(256) void volume_fuse_splat_kernel(
    int D, int H, int W, int C, const float* __restrict__ ndc, int64_t P, const float* __restrict__ feat, int feat_stride,
    const float* __restrict__ alpha, unsigned long long* __restrict__ ws)
{
#pragma clang fp contract(off)      // the reference's roundings: a contracted local - shift or weight product would skip one
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid == 0) ws[1] = FUSE_SCALE_LOG2;
    const int64_t p = tid / G;
    const int w = (int)(tid - p * G);                                                   // the word of the row this lane adds to
    if (p >= P || w >= C + 2) return;                                                   // (G >= C + 2: the last G - C - 2 lanes of a group idle)
    const float vx = ndc[p * 3 + 0] / (1.0f / (float)(W - 1));       // :43, :52 - a division by the voxel size, not a product with dim - 1
    const float vy = ndc[p * 3 + 1] / (1.0f / (float)(H - 1));
    const float vz = ndc[p * 3 + 2] / (1.0f / (float)(D - 1));
    // :54-59 on the truncated index: trunc(v) >= 0 <=> v > -1, trunc(v) < dim - 1 <=> v < dim - 1; a NaN fails both, +-inf one of them
    if (!(vx > -1.0f && vx < (float)(W - 1) && vy > -1.0f && vy < (float)(H - 1) && vz > -1.0f && vz < (float)(D - 1))) return;
    const int ix = (int)vx, iy = (int)vy, iz = (int)vz;
    const float lx = vx - floorf(vx), ly = vy - floorf(vy), lz = vz - floorf(vz);       // :53
    unsigned long long* const rows = ws + FUSE_HEADER_WORDS;
    const float val = w < C ? feat[p * feat_stride + w] : (w == C ? alpha[p] : 1.0f);
    unsigned refused = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int x = k >> 2, y = (k >> 1) & 1, z = k & 1;                              // :68 [x, y, z]
        const float wl = (fabsf(lx - (float)x) * fabsf(ly - (float)y)) * fabsf(lz - (float)z);      // :70-72
        const float prod = w == C + 1 ? wl : wl * val;                                  // :74 | :75-76
        if (!(fabsf(prod) < 0x1p20f)) { ++refused; continue; }
        const long long q = __double2ll_rn((double)prod * 0x1p32);
        if (q == 0) continue;
        const int64_t row = ((int64_t)(iz + x) * H + (iy + y)) * W + (ix + z);          // :74 [vox_z + x, vox_y + y, vox_x + z]
        atomicAdd(rows + row * (C + 4) + w, (unsigned long long)q);                     // (two's complement: unsigned addition is the signed one)
    }
    if (refused) atomicAdd(ws, (unsigned long long)refused);
}

extern "C" size_t mvsnerf_volume_fuse_workspace_words(int D, int H, int W, int C)
{
    if (D < 2 || H < 2 || W < 2 || C < 4 || (C & 3) || C > 40) return 0;
    return (size_t)FUSE_HEADER_WORDS + (size_t)D * H * W * (size_t)(C + 4);
}

extern "C" int mvsnerf_volume_fuse_splat(int D, int H, int W, int C, const float* ndc, int64_t P, const float* feat, int feat_stride,
                                         const float* alpha, void* workspace, void* stream)
{
    if (!workspace || D < 2 || H < 2 || W < 2 || P < 0 || feat_stride < C || (P > 0 && (!ndc || !feat || !alpha))) return MVSNERF_EINVAL;
    if (C < 4 || (C & 3) || C > 40) return MVSNERF_EUNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return MVSNERF_EALIGN;
    if (P == 0) return MVSNERF_OK;
    if (P > ((int64_t)1 << 32)) return MVSNERF_EINVAL;                  // P * 64 / 256 workgroups must fit the grid
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* ws = reinterpret_cast<unsigned long long*>(workspace);
    if (C + 2 <= 16) volume_fuse_splat_kernel<16><<<mvs_cdiv(P * 16, 256), 256, 0, st>>>(D, H, W, C, ndc, P, feat, feat_stride, alpha, ws);
    else if (C + 2 <= 32) volume_fuse_splat_kernel<32><<<mvs_cdiv(P * 32, 256), 256, 0, st>>>(D, H, W, C, ndc, P, feat, feat_stride, alpha, ws);
    else volume_fuse_splat_kernel<64><<<mvs_cdiv(P * 64, 256), 256, 0, st>>>(D, H, W, C, ndc, P, feat, feat_stride, alpha, ws);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// fuse_local_volumes :190-192 on the rounded sums: inv = 1 / (weight + 1e-6), volume = sum * inv, sigma = alpha sum * inv.  One thread per voxel,
// x fastest: every store of a wave is 256 contiguous bytes of one channel plane (NCDHW).  An untouched voxel gives 0 * 1e6 = 0 exactly.
__global__ __launch_bounds__(256) void volume_fuse_finish_kernel(int64_t n_vox, int C, const long long* __restrict__ ws,
                                                                 float* __restrict__ feat_volume, float* __restrict__ density_volume)
{
#pragma clang fp contract(off)
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vox) return;
    const long long* row = ws + FUSE_HEADER_WORDS + v * (C + 4);
    const float w = (float)((double)row[C + 1] * 0x1p-32);
    const float inv = 1.0f / (w + 1e-6f);
    density_volume[v] = (float)((double)row[C] * 0x1p-32) * inv;
    for (int c = 0; c < C; c += 2) {
        const longlong2 q = *reinterpret_cast<const longlong2*>(row + c);      // rows start 16-byte aligned: header 64 B, C + 4 even
        feat_volume[(int64_t)c * n_vox + v] = (float)((double)q.x * 0x1p-32) * inv;
        feat_volume[(int64_t)(c + 1) * n_vox + v] = (float)((double)q.y * 0x1p-32) * inv;
    }
}

extern "C" int mvsnerf_volume_fuse_finish(int D, int H, int W, int C, const void* workspace, float* feat_volume, float* density_volume, void* stream)
{
    if (!workspace || !feat_volume || !density_volume || D < 2 || H < 2 || W < 2) return MVSNERF_EINVAL;
    if (C < 4 || (C & 3) || C > 40) return MVSNERF_EUNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return MVSNERF_EALIGN;
    const int64_t n_vox = (int64_t)D * H * W;
    volume_fuse_finish_kernel<<<mvs_cdiv(n_vox, 256), 256, 0, (hipStream_t)stream>>>(n_vox, C, reinterpret_cast<const long long*>(workspace),
                                                                                    feat_volume, density_volume);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// ---------------------------------------------------------------------------------------------
// ray_marcher(rays, N_samples, lindisp, perturb, bbox_3D) (data/ray_utils.py:152-197) with near / far from dda (:143-150) and the box
// coordinates of the fusion script (train_mvs_nerf_fusion_finetuning_pl.py:263).  The uniform draw stays with the caller (jitter = its
// torch.rand, :190).  torch.min / torch.max hand a NaN on; so do these.  A ray that misses the box keeps the reference's near > far.
// One thread per sample.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

__global__ __launch_bounds__(256) void ray_march_bbox_kernel(const float* __restrict__ rays, const float* __restrict__ bbox, const float* __restrict__ t,
                                                             const float* __restrict__ jitter, float perturb, int lindisp, int64_t N, int S,
                                                             float* __restrict__ z_out, float* __restrict__ pts, float* __restrict__ ndc)
{
#pragma clang fp contract(off)      // eager torch rounds every product and sum
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * S) return;
    const int64_t n = i / S;
    const int s = (int)(i - n * S);
    float o[3], d[3], near = 0.0f, far = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a] = rays[n * 8 + a];
        d[a] = rays[n * 8 + 3 + a];
        const float inv = 1.0f / (d[a] + 1e-6f);                                        // :144
        const float t0 = (bbox[a] - o[a]) * inv, t1 = (bbox[3 + a] - o[a]) * inv;       // :145-146
        const float lo = nan_min(t0, t1), hi = nan_max(t0, t1);                         // :148-149
        near = a == 0 ? lo : nan_max(near, lo);
        far = a == 0 ? hi : nan_min(far, hi);
    }
    auto zplain = [&](int k) {                                                          // :177-180
        const float tv = t[k];
        return lindisp ? 1.0f / (1.0f / near * (1.0f - tv) + 1.0f / far * tv) : near * (1.0f - tv) + far * tv;
    };
    float z = zplain(s);
    if (perturb > 0.0f) {                                                               // :184-191
        const float lower = s == 0 ? z : 0.5f * (zplain(s - 1) + z);
        const float upper = s == S - 1 ? z : 0.5f * (z + zplain(s + 1));
        z = lower + (upper - lower) * (perturb * jitter[i]);
    }
    z_out[i] = z;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = o[a] + d[a] * z;                                                // :193-194
        pts[i * 3 + a] = p;
        ndc[i * 3 + a] = (p - bbox[a]) / (bbox[3 + a] - bbox[a]);
    }
}

extern "C" int mvsnerf_ray_march_bbox_fwd(const float* rays, const float* bbox, const float* t, const float* jitter, float perturb, int lindisp,
                                          int64_t N, int S, float* z, float* pts, float* ndc, void* stream)
{
    if (!rays || !bbox || !t || !z || !pts || !ndc || N < 0 || S < 1 || (perturb > 0.0f && !jitter) || !(perturb >= 0.0f)) return MVSNERF_EINVAL;
    if (N == 0) return MVSNERF_OK;
    if (N * S > ((int64_t)1 << 38)) return MVSNERF_EINVAL;
    ray_march_bbox_kernel<<<mvs_cdiv(N * S, 256), 256, 0, (hipStream_t)stream>>>(rays, bbox, t, jitter, perturb, lindisp, N, S, z, pts, ndc);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
