// One ray-march batch (march_batch, raymarch.hip) and the helpers of other files that it calls; internal, not exported.  Every file that
// defines or calls one of these helpers includes this header, so the compiler checks both sides against one prototype.
#pragma once
#include "common.h"

// N rays x S samples of rendering() (renderer.py:138-165): an mvsnerf_raymarch_args batch or one sub-batch of mvsnerf_render_args
struct MarchBatch {
    const float* vol; int D, H, W, vol_layout;      // volume, memory order MVSNERF_VOL_*
    int C;                                          // its channels: 8 (neural volume; colours gathered from the source images) or 8 + 4V (colour volume: imgs*, K, pts unused)
    const float* imgs; const float* imgs_nhwc4; int V, IH, IW;   // [V][3][IH][IW] (three stand-alone lookups), [V][IH][IW][4] or NULL (one gather)
    const float* w2c; const float* K;               // [V][4][4], [V][3][3]; view 0 is the reference view
    const float* pts; const float* ndc; const float* z; const float* rays_dir;   // [N][S][3], [N][S][3], [N][S], [N][3]
    int64_t N; int S; int white_bkgd;
    float* feat; float* dirs; float* raw;           // [N][S][8+4V], [N][3], [N][S][4]: temporaries, outputs too
    float* rgb_map; float* disp; float* acc; float* weights; float* depth; float* alpha;   // outputs, may be NULL
    // the MLP: fp32 weights (always: every variant takes its bias and head vectors there) + bf16 weights or split planes or neither;
    // a guard only with n_split = MVSNERF_SPLIT_FP16 (the guarded sequence)
    const float* packed; const void* packed_bf16; const void* packed_split; int n_split; int* guard;
};

// composite.hip: mvsnerf_composite_fwd; guard != NULL: the launch also ends a guarded sequence (counts a fallback, re-arms the guard)
int mvs_composite_fwd(const float* raw, const float* z, int64_t N, int S, int white_bkgd, float* rgb_map, float* disp, float* acc, float* weights,
                      float* depth, float* alpha, int* guard, void* stream);
// mlp.hip: mvsnerf_mlp_fwd predicated on a guard word (the fp32 re-run of a guarded fp16x3 batch)
int mvs_mlp_fwd_if(const float* packed, int F, const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                   const float* dirs, int dirs_stride, int64_t N, int S, int alpha_only, float* raw, const int* run_if, void* stream);
// mlp_f16x3.hip: the two-piece fp16 MLP on P = N * S points; reports a non-finite weight or value through guard[0] when guard != NULL
int mvs_mlp_f16x3_fwd(const void* packed_h, const float* packed_f32, int F, const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                      const float* dirs, int dirs_stride, int64_t P, int S, int alpha_only, float* raw, hipStream_t st, int* guard = nullptr);
// The counted forms of the two: rows [0, min(max(*count, 0), cap)) of dense (cap, 3 | F | 3) row buffers, S = 1, the count read on
// the device.  mvs_mlp_fwd_counted checks its arguments (run_if may be NULL); mvs_mlp_f16x3_fwd_counted's callers do, and pass cap >= 1.
int mvs_mlp_fwd_counted(const float* packed, int F, const float* ndc, const float* feat, const float* dirs, int64_t cap, const int* count,
                        int alpha_only, float* raw, const int* run_if, void* stream);
int mvs_mlp_f16x3_fwd_counted(const void* packed_h, const float* packed_f32, int F, const float* ndc, const float* feat, const float* dirs,
                              int cap, const int* count, int alpha_only, float* raw, hipStream_t st, int* guard = nullptr);
// mlp_f16x3.hip: elements and packing of that MLP's weight buffer, behind mvsnerf_mlp_{packed_split_elems, pack_split}(n_split = MVSNERF_SPLIT_FP16)
size_t mvs_mlp_f16x3_elems(int F);
int mvs_mlp_f16x3_pack(const float* const w[11], int F, void* packed, hipStream_t st);
// guarded.hip: ends a guarded sequence whose last kernel does not: counts a tripped guard, re-arms it
int mvs_guard_consume(int* guard, hipStream_t st);
// mlp.hip: the one-launch fp32 ray march (raymarch_fused_kernel) and whether it applies to a batch: fp32 MLP, no guard, channel-last images,
// HWDC volume, pointers present (volume, images, weights, feat and raw 16-byte aligned), F <= MAX_F, N >= 1, 32-bit offsets (gather_fits_32bit).
// When 128 % S != 0 the launcher enqueues the compositing as a separate mvs_composite_fwd launch.
bool mvs_raymarch_fused_applies(const MarchBatch& b);
int mvs_raymarch_fused_fwd(const MarchBatch& b, hipStream_t st);
// importance.hip: mvsnerf_ray_points_fwd with row strides for the origins / directions (rays kept as [N][8] rows) and, with tvals != NULL, the
// coarse depths near (1 - t) + far t formed in the launch from near_far_rays[n * nf_stride + 0 / 1] and written to z_out (dir_out: directions as [N][3])
int mvs_ray_points(const float* rays_o, int o_stride, const float* rays_d, int d_stride, const float* z_vals,
                   const float* w2c_ref, const float* K_ref, const float* near_far_ref, int W_ref, int H_ref, int pad, int lindisp,
                   int64_t N, int S, float* rays_pts, float* rays_ndc,
                   const float* tvals, const float* near_far_rays, int nf_stride, float* z_out, float* dir_out, void* stream);
