// The training rays of a scene as a device-resident bank: what read_meta of the reference's datasets builds on the CPU as an all-rays buffer
// (data/dtu_ft.py:143-188, data/blender.py:49-85: get_ray_directions, get_rays, the [o | d | near | far] rows, ToTensor, the RGBA blend onto white) is formed
// here per sampled index from the 8-bit images and the cameras.
//   scene_rays_gather   idx[B] -> rays[B][8], rgb[B][3] (+ depth[B], mask[B]): all_rays[idx], all_rgbs[idx]
//   scene_rays_march    idx[B] -> the same rows and the front end of a fine-tuning step: ray_marcher's depths (data/ray_utils.py:152-197), o + d*z and
//                       get_ndc_coordinate (utils.py:112-146) in one launch
//   source_images       ids[V] -> imgs[V][3][H][W]: the normalised source views of read_source_views
// Bank: images [M][H][W][4] uint8 RGBA (a ray's colour is one 32-bit load), c2w [M][3][4], K [M][3][3], near_far [M][2], depth [M][H][W] or NULL.
// Every operation is rounded on its own, as eager torch on the CPU rounds it (tests/scene_rays_refs.py is the elementwise restatement); an index outside
// [0, M*H*W) reads nothing and gives an all-zero row in every output.  Both kernels are bandwidth-bound: no LDS, no atomics.
#include "common.h"
#include "ray_dev.h"

struct SceneBank {
    const unsigned char* images;
    const float* c2w;
    const float* K;
    const float* near_far;
    const float* depth;
    int M, H, W;
    int64_t n_rays;            // M*H*W
};

// rays[8] = [o | d | near | far] and (x, y, view) of flat index i (view-major, then row-major: the order of torch.cat(all_rays, 0)).  i must be in range.
__device__ __forceinline__ void scene_ray_row(const SceneBank& b, int64_t i, float r[8])
{
#pragma clang fp contract(off)      // eager torch rounds every product and sum
    int x, y, m;
    mvs_unflatten3(i, b.W, b.H, x, y, m);
    const float* c2w = b.c2w + (int64_t)m * 12;
    const float* K = b.K + (int64_t)m * 9;
    // get_ray_directions (data/ray_utils.py:27): ((x - cx) / fx, (y - cy) / fy, 1), no half-pixel offset
    const float dx = ((float)x - K[2]) / K[0], dy = ((float)y - K[5]) / K[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r[k] = c2w[k * 4 + 3];                                                          // rays_o = c2w[:3, 3]
        r[3 + k] = (dx * c2w[k * 4 + 0] + dy * c2w[k * 4 + 1]) + c2w[k * 4 + 2];        // directions @ c2w[:3, :3].T, dz = 1
    }
    r[6] = b.near_far[(int64_t)m * 2];
    r[7] = b.near_far[(int64_t)m * 2 + 1];
}

// ToTensor (c / 255, an IEEE division) and the blend onto white of data/blender.py:70, rgb * a + (1 - a): alpha 255 gives rgb * 1 + 0 = rgb.
__device__ __forceinline__ unsigned scene_ray_colour(const SceneBank& b, int64_t i, float rgb[3])
{
#pragma clang fp contract(off)
    const uchar4 p = reinterpret_cast<const uchar4*>(b.images)[i];
    const float a = (float)p.w / 255.0f;
    const float ia = 1.0f - a;
    rgb[0] = ((float)p.x / 255.0f) * a + ia;
    rgb[1] = ((float)p.y / 255.0f) * a + ia;
    rgb[2] = ((float)p.z / 255.0f) * a + ia;
    return p.w;
}

// One thread per ray.  VEC: rays is 16-byte aligned and a row leaves as two 16-byte stores (a wave writes 2 KB of contiguous bytes).
template <bool VEC>
__global__ __launch_bounds__(256) void scene_rays_gather_kernel(SceneBank b, const int64_t* __restrict__ idx, int64_t B, float* __restrict__ rays,
                                                                float* __restrict__ rgb, float* __restrict__ depth, unsigned char* __restrict__ mask)
{
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= B) return;
    const int64_t i = idx[n];
    float r[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, c[3] = {0.f, 0.f, 0.f}, d = 0.0f;
    unsigned a = 0;
    if ((uint64_t)i < (uint64_t)b.n_rays) {
        scene_ray_row(b, i, r);
        a = scene_ray_colour(b, i, c);
        if (depth) d = b.depth[i];
    }
    if (VEC) {
        f32x4* o = reinterpret_cast<f32x4*>(rays + n * 8);
        o[0] = f32x4{r[0], r[1], r[2], r[3]};
        o[1] = f32x4{r[4], r[5], r[6], r[7]};
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) rays[n * 8 + k] = r[k];
    }
    rgb[n * 3 + 0] = c[0]; rgb[n * 3 + 1] = c[1]; rgb[n * 3 + 2] = c[2];
    if (depth) depth[n] = d;
    if (mask) mask[n] = a > 0 ? 1 : 0;                                                  // data/blender.py:69
}

// One thread per sample, t = n * S + s, the mapping and the [B][S][3] stores of ray_points_kernel (importance.hip); the thread of s == 0 also writes the ray's
// row and colour.  The S threads of a ray form its row again each (a dozen cached loads and two divisions) instead of exchanging it: no LDS, no barrier.
__global__ __launch_bounds__(256) void scene_rays_march_kernel(SceneBank b, const int64_t* __restrict__ idx, int64_t B, const float* __restrict__ tvals, int S,
                                                               const float* __restrict__ jitter, float perturb, int lindisp,
                                                               const float* __restrict__ w2c, const float* __restrict__ Kr, const float* __restrict__ nf_ref,
                                                               int W_ref, int H_ref, int pad, float* __restrict__ rays, float* __restrict__ rgb,
                                                               float* __restrict__ z_out, float* __restrict__ pts, float* __restrict__ ndc)
{
#pragma clang fp contract(off)
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * S) return;
    const int64_t n = t / S;
    const int s = (int)(t - n * S);
    const int64_t i = idx[n];
    if ((uint64_t)i >= (uint64_t)b.n_rays) {                                            // outside the bank: zero rows, nothing read
        z_out[t] = 0.0f;
        pts[t * 3 + 0] = 0.0f; pts[t * 3 + 1] = 0.0f; pts[t * 3 + 2] = 0.0f;
        if (ndc) { ndc[t * 3 + 0] = 0.0f; ndc[t * 3 + 1] = 0.0f; ndc[t * 3 + 2] = 0.0f; }
        if (s == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) rays[n * 8 + k] = 0.0f;
            rgb[n * 3 + 0] = 0.0f; rgb[n * 3 + 1] = 0.0f; rgb[n * 3 + 2] = 0.0f;
        }
        return;
    }
    float r[8];
    scene_ray_row(b, i, r);
    if (s == 0) {
        float c[3];
        scene_ray_colour(b, i, c);
#pragma unroll
        for (int k = 0; k < 8; ++k) rays[n * 8 + k] = r[k];
        rgb[n * 3 + 0] = c[0]; rgb[n * 3 + 1] = c[1]; rgb[n * 3 + 2] = c[2];
    }
    // ray_marcher (data/ray_utils.py:176-191): coarse depths and the stratified jitter, ray_dev.h's roundings
    const float near = r[6], far = r[7];
    float z = coarse_depth(near, far, tvals[s], lindisp);
    if (perturb > 0.0f) {
        const float lo = s == 0 ? z : 0.5f * (z + coarse_depth(near, far, tvals[s - 1], lindisp));
        const float up = s == S - 1 ? z : 0.5f * (coarse_depth(near, far, tvals[s + 1], lindisp) + z);
        const float rnd = perturb * jitter[t];                                          // :190, rounded once
        z = jittered_depth(lo, up, rnd);
    }
    z_out[t] = z;
    const float px = ray_point(r[0], r[3], z), py = ray_point(r[1], r[4], z), pz = ray_point(r[2], r[5], z);
    pts[t * 3 + 0] = px; pts[t * 3 + 1] = py; pts[t * 3 + 2] = pz;
    if (!ndc) return;
    float nx, ny, nz;
    ray_ndc(px, py, pz, w2c, Kr, nf_ref[0], nf_ref[1], W_ref, H_ref, pad, lindisp, nx, ny, nz);
    ndc[t * 3 + 0] = nx; ndc[t * 3 + 1] = ny; ndc[t * 3 + 2] = nz;
}

// The source views of read_source_views (data/dtu_ft.py:72-119, data/blender.py:91-146) from the bank: ToTensor, the blend onto white, then
// T.Normalize's sub_(mean).div_(std), each an fp32 operation rounded on its own.  One thread per element of out [V][3][H][W], t = (v * 3 + k) * HW + px:
// a wave stores 256 contiguous bytes and the three threads of a pixel read its four bytes again (cached).  One channel per thread also leaves the compiler
// no pair of channels to pack into a v_pk_*_f32 (check_isa.sh refuses the form it chose for three per thread).  An id outside [0, M) reads nothing and
// gives zeros.
struct Norm3 { float mean[3], std[3]; };

__global__ __launch_bounds__(256) void source_images_kernel(SceneBank b, const int64_t* __restrict__ ids, int64_t total, int64_t HW, Norm3 nrm,
                                                            float* __restrict__ out)
{
#pragma clang fp contract(off)
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t plane = t / HW, px = t - plane * HW, v = plane / 3;
    const int k = (int)(plane - v * 3);
    const int64_t id = ids[v];
    float x = 0.0f;
    if ((uint64_t)id < (uint64_t)b.M) {
        float c[3];
        scene_ray_colour(b, id * HW + px, c);                                           // the colour of the training rays: one device function
        const float ck = k == 0 ? c[0] : (k == 1 ? c[1] : c[2]);
        const float mean = k == 0 ? nrm.mean[0] : (k == 1 ? nrm.mean[1] : nrm.mean[2]), std = k == 0 ? nrm.std[0] : (k == 1 ? nrm.std[1] : nrm.std[2]);
        x = (ck - mean) / std;
    }
    out[t] = x;
}

static inline bool aligned_to(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The bank and the index batch: NULL or misaligned pointers and sizes < 1 are MVSNERF_EINVAL, a bank beyond INT64_MAX / 8 rays MVSNERF_EUNSUPPORTED
static int scene_bank_args(const unsigned char* images, const float* c2w, const float* K, const float* near_far, const float* depth_bank, int M, int H, int W,
                           const int64_t* idx, int64_t B, SceneBank* b)
{
    if (!images || !c2w || !K || !near_far || M < 1 || H < 1 || W < 1 || B < 0 || (B > 0 && !idx)) return MVSNERF_EINVAL;
    if (!aligned_to(images, 4) || !aligned_to(c2w, 4) || !aligned_to(K, 4) || !aligned_to(near_far, 4) || !aligned_to(depth_bank, 4) || !aligned_to(idx, 8))
        return MVSNERF_EINVAL;
    int64_t n;
    if (__builtin_mul_overflow((int64_t)M, (int64_t)H, &n) || __builtin_mul_overflow(n, (int64_t)W, &n) || n > INT64_MAX / 8) return MVSNERF_EUNSUPPORTED;
    *b = SceneBank{images, c2w, K, near_far, depth_bank, M, H, W, n};
    return MVSNERF_OK;
}

extern "C" int mvsnerf_scene_rays_gather_fwd(const unsigned char* images_rgba, const float* c2w, const float* K, const float* near_far, const float* depth_bank,
                                             int M, int H, int W, const int64_t* idx, int64_t B, float* rays, float* rgb, float* depth, unsigned char* mask,
                                             void* stream)
{
    SceneBank b;
    if (int rc = scene_bank_args(images_rgba, c2w, K, near_far, depth_bank, M, H, W, idx, B, &b)) return rc;
    if (!rays || !rgb || (depth && !depth_bank) || !aligned_to(rays, 4) || !aligned_to(rgb, 4) || !aligned_to(depth, 4)) return MVSNERF_EINVAL;
    if (B == 0) return MVSNERF_OK;
    if (B > ((int64_t)1 << 38)) return MVSNERF_EUNSUPPORTED;                            // B / 256 workgroups must fit the grid
    if (aligned_to(rays, 16)) scene_rays_gather_kernel<true><<<mvs_cdiv(B, 256), 256, 0, (hipStream_t)stream>>>(b, idx, B, rays, rgb, depth, mask);
    else scene_rays_gather_kernel<false><<<mvs_cdiv(B, 256), 256, 0, (hipStream_t)stream>>>(b, idx, B, rays, rgb, depth, mask);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_scene_rays_march_fwd(const unsigned char* images_rgba, const float* c2w, const float* K, const float* near_far, int M, int H, int W,
                                            const int64_t* idx, int64_t B, const float* t, int S, const float* jitter, float perturb, int lindisp,
                                            const float* w2c_ref, const float* K_ref, const float* near_far_ref, int W_ref, int H_ref, int pad,
                                            float* rays, float* rgb, float* z, float* pts, float* ndc, void* stream)
{
    SceneBank b;
    if (int rc = scene_bank_args(images_rgba, c2w, K, near_far, nullptr, M, H, W, idx, B, &b)) return rc;
    if (!t || S < 1 || !rays || !rgb || !z || !pts || !(perturb >= 0.0f) || (perturb > 0.0f && !jitter)) return MVSNERF_EINVAL;
    if (ndc && (!w2c_ref || !K_ref || !near_far_ref || W_ref < 2 || H_ref < 2 || pad < 0)) return MVSNERF_EINVAL;
    if (!aligned_to(t, 4) || !aligned_to(jitter, 4) || !aligned_to(w2c_ref, 4) || !aligned_to(K_ref, 4) || !aligned_to(near_far_ref, 4) || !aligned_to(rays, 4) ||
        !aligned_to(rgb, 4) || !aligned_to(z, 4) || !aligned_to(pts, 4) || !aligned_to(ndc, 4))
        return MVSNERF_EINVAL;
    if (B == 0) return MVSNERF_OK;
    if (B > ((int64_t)1 << 38) / S) return MVSNERF_EUNSUPPORTED;                        // B * S / 256 workgroups must fit the grid
    scene_rays_march_kernel<<<mvs_cdiv(B * S, 256), 256, 0, (hipStream_t)stream>>>(b, idx, B, t, S, jitter, perturb > 0.0f ? perturb : 0.0f, lindisp,
                                                                                  ndc ? w2c_ref : nullptr, K_ref, near_far_ref, W_ref, H_ref, pad, rays, rgb, z,
                                                                                  pts, ndc);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_source_images_fwd(const unsigned char* images_rgba, const int64_t* ids, int V, int M, int H, int W, const float* mean, const float* std,
                                         float* out, void* stream)
{
    if (!images_rgba || !ids || !mean || !std || !out || V < 1 || M < 1 || H < 1 || W < 1) return MVSNERF_EINVAL;
    if (!aligned_to(images_rgba, 4) || !aligned_to(ids, 8) || !aligned_to(out, 4)) return MVSNERF_EALIGN;
    const int64_t HW = (int64_t)H * W;
    if (HW > 0x7fffffff || HW > ((int64_t)1 << 38) / 3 / V) return MVSNERF_EUNSUPPORTED;    // 3 V H W / 256 workgroups must fit the grid
    const Norm3 nrm{{mean[0], mean[1], mean[2]}, {std[0], std[1], std[2]}};             // host arrays, read here
    const SceneBank b{images_rgba, nullptr, nullptr, nullptr, nullptr, M, H, W, M * HW};
    source_images_kernel<<<mvs_cdiv(3 * V * HW, 256), 256, 0, (hipStream_t)stream>>>(b, ids, 3 * V * HW, HW, nrm, out);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
