// The trilinear cell of a single-channel (D,H,W) volume as index_point_feature addresses it (grid = coord*2-1, zeros padding,
// align_corners=True): the index arithmetic that density_lookup (importance.hip) and the empty-space predicate (sparse.hip) share, so that
// "the corners the lookup would read" means the same voxels in both.  fp32, the operations in the order written here.
#pragma once

struct DensityCell {
    float ix, iy, iz;       // continuous voxel coordinates
    float fx, fy, fz;       // their floors: the cell's low corner
};

__device__ __forceinline__ DensityCell density_cell(int D, int H, int W, float cx, float cy, float cz)
{
    DensityCell c;
    const float gx = cx * 2.0f - 1.0f, gy = cy * 2.0f - 1.0f, gz = cz * 2.0f - 1.0f;
    c.ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1);
    c.iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
    c.iz = ((gz + 1.0f) / 2.0f) * (float)(D - 1);
    c.fx = floorf(c.ix); c.fy = floorf(c.iy); c.fz = floorf(c.iz);
    return c;
}

// corner (x, y, z) - whole numbers held as floats - lies in the grid (the comparison is made in fp32, before any cast: a huge or NaN
// coordinate is simply outside)
__device__ __forceinline__ bool density_corner_in_grid(int D, int H, int W, float x, float y, float z)
{
    return x >= 0.0f && x <= (float)(W - 1) && y >= 0.0f && y <= (float)(H - 1) && z >= 0.0f && z <= (float)(D - 1);
}

__device__ __forceinline__ int64_t density_corner_index(int H, int W, float x, float y, float z)
{
    return ((int64_t)z * H + (int)y) * W + (int)x;
}
