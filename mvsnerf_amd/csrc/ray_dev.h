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
