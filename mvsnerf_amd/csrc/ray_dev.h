// Arithmetic shared by the two kernels that put samples on rays: raygen_kernel (sample.hip: rays from pixel ids) and ray_points_kernel (importance.hip:
// caller-supplied rays).  A frame rendered from pixels and the same frame rendered from explicit rays must march the same depths and the same points, so the
// depths, the jitter and o + d*z have ONE definition each.
#pragma once
#include "common.h"

// The coarse depths of ray_marcher (data/ray_utils.py:152-197) / build_rays (utils.py:211-221) as eager torch forms them: (1 - t) rounded, two rounded
// products, one sum; lindisp: the reciprocals are IEEE divisions like torch's.  Contracted, near*(1-t) + far*t loses the rounding of one product and lands one
// unit in the last place away from torch on a fifth to a half of the depths.
__device__ __forceinline__ float coarse_depth(float near, float far, float t, int lindisp)
{
#pragma clang fp contract(off)
    const float omt = 1.0f - t;
    if (lindisp) {
        const float a = (1.0f / near) * omt, b = (1.0f / far) * t;
        return 1.0f / (a + b);
    }
    const float a = near * omt, b = far * t;
    return a + b;
}

// Stratified jitter lower + (upper - lower) * t_rand (utils.py:217-221, data/ray_utils.py:183-188), every operation rounded like torch's.
__device__ __forceinline__ float jittered_depth(float lower, float upper, float r)
{
#pragma clang fp contract(off)
    const float span = upper - lower;
    const float step = span * r;
    return lower + step;
}

// One coordinate of o + d*z: a single fused multiply-add in both kernels.
__device__ __forceinline__ float ray_point(float o, float d, float z) { return fmaf(d, z, o); }

// get_ndc_coordinate (utils.py:112-146) of one world point for ray_points_kernel (importance.hip) and scene_rays_march_kernel (scene_rays.hip): reference
// camera R x + t, K p, /z, /(W-1, H-1), depth normalisation (lindisp: in disparity), pad re-scale.  w2c: the reference view's [4][4] (rows 0..2 read), Kr [3][3].
__device__ __forceinline__ void ray_ndc(float px, float py, float pz, const float* __restrict__ w2c, const float* __restrict__ Kr, float near_ref,
                                        float far_ref, int W_ref, int H_ref, int pad, int lindisp, float& nx, float& ny, float& nz)
{
    const float cx = fmaf(pz, w2c[2], fmaf(py, w2c[1], px * w2c[0])) + w2c[3];
    const float cy = fmaf(pz, w2c[6], fmaf(py, w2c[5], px * w2c[4])) + w2c[7];
    const float cz = fmaf(pz, w2c[10], fmaf(py, w2c[9], px * w2c[8])) + w2c[11];
    const float qx = fmaf(cz, Kr[2], fmaf(cy, Kr[1], cx * Kr[0]));
    const float qy = fmaf(cz, Kr[5], fmaf(cy, Kr[4], cx * Kr[3]));
    const float qz = fmaf(cz, Kr[8], fmaf(cy, Kr[7], cx * Kr[6]));
    nx = (qx / qz + 0.0f) / (float)(W_ref - 1);
    ny = (qy / qz + 0.0f) / (float)(H_ref - 1);
    nz = lindisp ? (1.0f / qz - 1.0f / near_ref) / (1.0f / far_ref - 1.0f / near_ref) : (qz - near_ref) / (far_ref - near_ref);
    if (pad > 0) {
        const float Wf = (float)W_ref / 4.0f, Hf = (float)H_ref / 4.0f;               // (inv_scale+1)/4
        ny = ny * Hf / (Hf + (float)(pad * 2)) + (float)pad / (Hf + (float)(pad * 2));
        nx = nx * Wf / (Wf + (float)(pad * 2)) + (float)pad / (Wf + (float)(pad * 2));
    }
}
