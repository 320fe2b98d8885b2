/* mvsnerf_hip_internal.h - the INTERNAL tier of libmvsnerf_hip.so's exports (see include/mvsnerf_hip.h for the stable one and the conventions).
 *
 * What mvsnerf_amd/encoder.py, ops.py and train.py drive their tuned layer loop with: one entry per kernel family and layout (matrix-core
 * convolutions per shape, blocked / bf16 / two-piece-fp16 cost volumes, InPlaceABN partial-sum plumbing, multi-job weight packing and
 * reduction, the guarded conv sequences of the scene encode, a census probe).  Exported because the layer loop lives in Python; NOT part of the
 * interface a reference-side maintainer binds, and free to change with the kernels (no ABI bump).  The reference call sites are the same as
 * those of the stable entries they specialise (CostRegNet models.py:725-769, FeatureNet models.py:688-722, plane sweep models.py:839-893).
 */
#ifndef MVSNERF_HIP_INTERNAL_H
#define MVSNERF_HIP_INTERNAL_H

#include "mvsnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same sweep writing the cost volume in channel blocks of FOUR: cost_blocked[CP/4][D*Hp*Wp][4] (block b holds channels 4b..4b+3
 * of every voxel).  This is the layout the matrix-core conv0 (mvsnerf_conv3d_c8_blocked_fwd) stages from by LDS-DMA: it multiplies four
 * input channels at a time, and with the channel-last layout every such pass touched all of a voxel's 176-byte row again
 * (measured: 5.4x the algorithmic HBM reads); in blocks, 64 consecutive voxels of a pass are 1 KB of contiguous, fully used bytes. */
int mvsnerf_planesweep_costvar_blocked_fwd(const float* feats_cl, const float* imgs_cl, const float* proj, const float* depth,
                                           int V, int C, int H, int W, int D, int pad, float* cost_blocked, int CP, float* masks,
                                           int with_img, void* stream);
/* bf16 encoder (the reference's AMP switch, train_mvs_nerf_pl.py:317-318 `precision=16 if args.use_amp`; BASELINE config 3 "bf16"):
 * conv0 of CostRegNet (models.py:756, 74.5 % of the encoder's FLOPs) on v_mfma_f32_16x16x32_bf16 - operands rounded to bf16, fp32
 * accumulation, fp32 master weights / statistics / gradients.
 *   planesweep_costvar_bf16_fwd  the plane sweep above storing the cost volume as bf16 in channel blocks of sixteen:
 *                                cost16[ceil(CP/16)][D*Hp*Wp][16] (channels >= CP zero); the sweep's arithmetic stays fp32
 *   conv0_bf16_pack              nn.Conv3d weight w[8][Cin][3][3][3] -> the kernel's B fragments (conv0_bf16_packed_elems(Cin) bf16 values)
 *   conv0_bf16_fwd               out[D][H][W][8] fp32 (raw, before InPlaceABN); stats_part: NULL or conv0_bf16_tiles(D,H,W) * 16 floats of
 *                                per-tile sums / sums of squares for mvsnerf_abn_finalize */
int mvsnerf_planesweep_costvar_bf16_fwd(const float* feats_cl, const float* imgs_cl, const float* proj, const float* depth,
                                        int V, int C, int H, int W, int D, int pad, void* cost16, int CP, float* masks,
                                        int with_img, void* stream);
size_t mvsnerf_conv0_bf16_packed_elems(int Cin);
int mvsnerf_conv0_bf16_pack(const float* w, int Cin, void* packed, void* stream);
int mvsnerf_conv0_bf16_tiles(int D, int H, int W);
int mvsnerf_conv0_bf16_fwd(const void* x16, int Cin, int D, int H, int W, const void* packed, float* out, float* stats_part, void* stream);
/* conv0 with fp32-GRADE results from the fp16 matrix cores (csrc/conv_f16x3.hip; opt-in `encoder.encoder_precision("fp16x3")`, inference): every
 * operand as two fp16 pieces, x*w ~= x0*w0 + x0*w1 + x1*w0 on v_mfma_f32_16x16x32_f16 (dropped: <= 2^-22 of a product), fp32 accumulation.
 *   planesweep_costvar_f16x2_fwd  the plane sweep (fp32 arithmetic) storing fp16(x/16) and fp16(x/16 - hi): cost16x2[2][ceil(CP/16)][D*Hp*Wp][16],
 *                                 hi plane then lo plane (the reference operation it replaces: models.py:839-893, as mvsnerf_planesweep_costvar_fwd)
 *   conv0_f16x3_pack / _fwd       w[8][Cin][3][3][3] -> fp16 pieces of 16 w; out / stats_part / tiles as mvsnerf_conv0_bf16_fwd (models.py:756) */
int mvsnerf_planesweep_costvar_f16x2_fwd(const float* feats_cl, const float* imgs_cl, const float* proj, const float* depth,
                                         int V, int C, int H, int W, int D, int pad, void* cost16x2, int CP, float* masks,
                                         int with_img, void* stream);
size_t mvsnerf_conv0_f16x3_packed_elems(int Cin);
int mvsnerf_conv0_f16x3_pack(const float* w, int Cin, void* packed, void* stream);
int mvsnerf_conv0_f16x3_fwd(const void* x16x2, int Cin, int D, int H, int W, const void* packed, float* out, float* stats_part, void* stream);
/*   conv0_bf16_dgrad_pack / conv0_bf16_dgrad   data gradient w.r.t. the n_ci (16 or 32) input channels starting at c_first (the plane sweep's
 *                                backward needs the 32 variance channels only): g = gradient of conv0's raw output, fp32 [D][H][W][8], rounded
 *                                to bf16 on the way into the matrix cores; gx[D][H][W][n_ci] fp32 */
size_t mvsnerf_conv0_bf16_dgrad_packed_elems(int n_ci);
int mvsnerf_conv0_bf16_dgrad_pack(const float* w, int Cin, int c_first, int n_ci, void* packed, void* stream);
int mvsnerf_conv0_bf16_dgrad(const float* g, int D, int H, int W, const void* packed, int n_ci, float* gx, void* stream);
/*   conv0_bf16_wgrad             gw[8][Cin][3][3][3] from the bf16 cost volume and g (fp32, rounded to bf16 while staged): voxels are the
 *                                reduction dimension, both operands are transposed by the LDS read (ds_read_b64_tr_b16); deterministic.
 *                                workspace: mvsnerf_conv3d_wgrad_workspace_floats(8, Cin) floats; gw NULL leaves conv0_bf16_wgrad_parts(D,H,W)
 *                                partial results (rows of 8*Cin*27 floats) at its start for mvsnerf_partial_sum_multi */
int mvsnerf_conv0_bf16_wgrad_parts(int D, int H, int W);
int mvsnerf_conv0_bf16_wgrad(const void* x16, int Cin, int D, int H, int W, const float* g, float* gw, float* workspace, void* stream);
/* conv2 of CostRegNet (16 -> 16, stride 1; models.py:736 ConvBnReLU3D -> InPlaceABN) with the InPlaceABN partial sums of its raw output from the
 * same launch: stats_part[2][16][mvsnerf_conv3d_tiled_tiles(D, H, W)] floats for mvsnerf_abn_finalize.  One lazily-activated source; other
 * shapes return MVSNERF_EUNSUPPORTED. */
int mvsnerf_conv3d_tiled_tiles(int D, int H, int W);
int mvsnerf_conv3d_fwd_stats(const float* x1, const float* scale1, const float* shift1, int Cin, int cin_ld, int D, int H, int W,
                             const float* wpacked, int Cout, int stride, float* out, float* stats_part, void* stream);
/* conv0 of CostRegNet (models.py:756; k3, stride 1, Cout = 8, raw input) on v_mfma_f32_4x4x1_16B_f32, input in channel
 * blocks of four (see mvsnerf_planesweep_costvar_blocked_fwd), Cin = 4*ceil((32+3V)/4) channels of which the first Cin_real = 32+3V exist
 * (products with the zero padding are skipped).  Weights: wq[ci/4][tap][co][4] = mvsnerf_conv3d_pack_weights_c8 of the
 * packed[tap][ci][8] layout of mvsnerf_conv3d_pack_weights (27*Cin*8 floats either way). */
int mvsnerf_conv3d_pack_weights_c8(const float* wpacked, int Cin, float* wq, void* stream);
int mvsnerf_conv3d_c8_blocked_fwd(const float* x_blocked, int Cin, int Cin_real, int D, int H, int W, const float* wq, float* out, void* stream);
/* Weight gradient of that convolution from the same blocked input (the training path keeps the cost volume blocked; autograd of
 * models.py:756 through nn.Conv3d): gw[co][ci][tap] = sum_o g[o][co] * x[o + tap - 1][ci] on v_mfma_f32_4x4x1 with the voxels as the k
 * dimension.  g: gradient of the raw conv0 output, channel-last [D][H][W][8]; gw: (8, Cin_real, 3,3,3) floats; workspace:
 * mvsnerf_conv3d_wgrad_workspace_floats(8, Cin_real).  Deterministic. */
int mvsnerf_conv3d_c8_blocked_wgrad(const float* x_blocked, int Cin, int Cin_real, int D, int H, int W, const float* g, float* gw,
                                    float* workspace, void* stream);
/* All weight re-layouts of a step in one launch (<= 64 jobs, host arrays): job j gathers from the layer's own weight tensor w[j] with
 * params[9 j ..] = {kind, ntaps, ci_real, co_real, ci_pad, co_pad, s_ci, s_co, flip}; kind 0 = conv3d/conv2d_pack_weights' [tap][ci][co],
 * 1 = conv3d_pack_weights_c8's [ci/4][tap][co][4], 2 = conv3d_pack_weights_mfma's [tap][ci/8][co][8] (both straight from w, not from a packed
 * copy), 3 / 4 = the bf16 fragments of mvsnerf_conv3d_bf16_fwd / mvsnerf_conv_transpose3d_bf16_fwd (dst[j] is then a bf16 buffer of
 * mvsnerf_conv3d_bf16_packed_elems(ci_pad, co_pad, kind == 4) elements; ntaps = 27).  The weights change with every optimizer step;
 * separately these are ~70 launches of a few microseconds each. */
int mvsnerf_pack_weights_multi(int n_jobs, const float* const* w, float* const* dst, const int* params, void* stream);
int mvsnerf_conv3d_mfma_supported(int Cin, int Cout, int stride);
int mvsnerf_conv3d_pack_weights_mfma(const float* wpacked, int Cin, int Cout, float* w32, void* stream);
int mvsnerf_conv3d_mfma_fwd(const float* x1, const float* scale1, const float* shift1, int Cin, int cin_ld, int D, int H, int W,
                            const float* w32, int Cout, int stride, float* out, float* stats_part, void* stream);
/* stats_part (NULL = not wanted): per-workgroup InPlaceABN partial sums of the output, 2 * Cout floats per workgroup,
 * mvsnerf_conv3d_mfma_tiles(D, H, W, stride) workgroups, finished by mvsnerf_abn_finalize. */
int mvsnerf_conv3d_mfma_tiles(int D, int H, int W, int stride);
/* The transposed convolutions (conv7/9/11) on v_mfma_f32_32x32x2_f32: plain (already activated) input x[D][H][W][Cin], weights from
 * mvsnerf_conv3d_pack_weights_mfma; raw out[2D][2H][2W][Cout]. */
int mvsnerf_conv_transpose3d_mfma_supported(int Cin, int Cout);
int mvsnerf_conv_transpose3d_mfma_fwd(const float* x, int Cin, int D, int H, int W, const float* w32, int Cout, float* out, void* stream);
/* ... and the InPlaceABN partial sums of the raw output from the same launch (conv7 / conv9: models.py:739-746 feed an InPlaceABN): stats_part
 * [2][Cout][mvsnerf_conv_transpose3d_mfma_tiles(Cin, Cout, D, H, W)] floats for mvsnerf_abn_finalize (0 tiles: layer not built). */
int mvsnerf_conv_transpose3d_mfma_tiles(int Cin, int Cout, int D, int H, int W);
int mvsnerf_conv_transpose3d_mfma_fwd_stats(const float* x, int Cin, int D, int H, int W, const float* w32, int Cout, float* out,
                                            float* stats_part, void* stream);
/* The 16 -> 8 layer (conv11, and conv1's data gradient) without padded products on v_mfma_f32_4x4x1 (the parity-class form above spends
 * 44 % of its products on zero weights at 8 output channels).  wq: [ci/4][tap][co][4] = mvsnerf_pack_weights_multi kind 1 of the layer. */
int mvsnerf_conv_transpose3d_c8_supported(int Cin, int Cout);
/* (described in mvsnerf_hip.h: "The input is leaky(x1*scale1+shift1) [+ leaky(x2*scale2+shift2)] like mvsnerf_conv_transpose3d_fwd's (scale ...") */
int mvsnerf_conv_transpose3d_c8_fwd(const float* x1, const float* scale1, const float* shift1, const float* x2, const float* scale2, const float* shift2,
                                    int Cin, int D, int H, int W, const float* wq, float* out, float* stats_part, void* stream);
int mvsnerf_conv_transpose3d_c8_tiles(int D, int H, int W);
int mvsnerf_conv3d_c8_blocked_tiles(int D, int H, int W);
int mvsnerf_conv3d_c8_blocked_fwd_stats(const float* x_blocked, int Cin, int Cin_real, int D, int H, int W, const float* wq, float* out,
                                        float* stats_part, void* stream);
int mvsnerf_abn_finalize(const float* part, int n_blocks, int C, int64_t n_vox, const float* weight, const float* bias,
                         float* running_mean, float* running_var, float momentum, float eps,
                         float* scale, float* shift, float* mean_out, float* invstd_out, void* stream);
/* ---- conv1 ... conv11 of CostRegNet on the bf16 matrix cores (use_amp: train_mvs_nerf_pl.py:317-318 `precision=16`; models.py:725-769) ----
 * Forward and data gradients of the nine 3x3x3 layers behind conv0 (conv0 itself: the mvsnerf_conv0_bf16_* entries above): the arguments of
 * mvsnerf_conv3d_fwd / mvsnerf_conv_transpose3d_fwd - two lazily-activated fp32 sources, channel-last - with bf16 weight fragments
 * (mvsnerf_conv3d_bf16_pack from the generic [27][Cin][Cout] layout of mvsnerf_conv3d_pack_weights: the layer's own weights or the re-packed
 * ones of its data gradient) and, when stats_part != NULL, the InPlaceABN partial sums of the output (mvsnerf_conv3d_bf16_tiles /
 * mvsnerf_conv_transpose3d_bf16_tiles slots x 2 x Cout floats, for mvsnerf_abn_finalize).  Operands are rounded to bf16 on load (round to
 * nearest even), products accumulate in fp32, outputs are fp32.  Cin, Cout in {8, 16, 32, 64} (transposed: Cin >= 16); other shapes:
 * MVSNERF_EUNSUPPORTED (mvsnerf_conv3d_bf16_packed_elems returns 0). */
size_t mvsnerf_conv3d_bf16_packed_elems(int Cin, int Cout, int transposed);
int mvsnerf_conv3d_bf16_pack(const float* wpacked, int Cin, int Cout, int transposed, void* wq, void* stream);
int mvsnerf_conv3d_bf16_tiles(int D, int H, int W, int stride);
int mvsnerf_conv3d_bf16_fwd(const float* x1, const float* scale1, const float* shift1,
                            const float* x2, const float* scale2, const float* shift2,
                            int Cin, int cin_ld, int D, int H, int W, const void* wq, int Cout, int stride,
                            float* out, float* stats_part, void* stream);
int mvsnerf_conv_transpose3d_bf16_tiles(int D, int H, int W);
int mvsnerf_conv_transpose3d_bf16_fwd(const float* x1, const float* scale1, const float* shift1,
                                      const float* x2, const float* scale2, const float* shift2,
                                      int Cin, int D, int H, int W, const void* wq, int Cout, float* out, float* stats_part, void* stream);
/* FeatureNet's 2-D layers (models.py:688-722) on the same bf16 kernels under use_amp: [N][H][W][C] images, ksize 1 | 3 | 5, stride 1 | 2,
 * padding ksize / 2, one lazily-activated source, optional bias (the 1x1 toplayer); weights = mvsnerf_pack_weights_multi kind 3 with
 * ntaps = ksize^2.  Built for the eight ConvBnReLU layers, the toplayer and their stride-1 data gradients (the two 5x5 stride-2 data
 * gradients stay on mvsnerf_conv2d_dgrad_k5s2). */
size_t mvsnerf_conv2d_bf16_packed_elems(int Cin, int Cout, int ksize);
int mvsnerf_conv2d_bf16_tiles(int N, int H, int W, int ksize, int stride);
int mvsnerf_conv2d_bf16_fwd(const float* x, const float* scale, const float* shift, int Cin, int cin_ld, int N, int H, int W,
                            const void* wq, const float* bias, int Cout, int ksize, int stride, float* out, float* stats_part, void* stream);
/* (described in mvsnerf_hip.h: "The same weight gradients with bf16 operands (use_amp; csrc/wgrad_bf16.hip): G and X are rounded to bf16 wh ...") */
int mvsnerf_conv_wgrad_bf16_parts(int A, int B, int Do, int Ho, int Wo, int kz, int k, int stride);
size_t mvsnerf_conv_wgrad_bf16_workspace_floats(int A, int B, int kz, int k);
int mvsnerf_conv_wgrad_bf16(const float* g1, const float* g1_scale, const float* g1_shift,
                            const float* g2, const float* g2_scale, const float* g2_shift, int A,
                            const float* x1, const float* x1_scale, const float* x1_shift,
                            const float* x2, const float* x2_scale, const float* x2_shift, int B, int ldx,
                            int Do, int Ho, int Wo, int Di, int Hi, int Wi, int kz, int k, int stride,
                            float* gw, float* workspace, void* stream);
/* Every weight-gradient entry (conv3d_wgrad, conv3d_c8_blocked_wgrad, conv2d_wgrad) leaves per-workgroup partial results at the start of
 * its workspace and then reduces them (two small launches).  With gw == NULL the reduction is skipped: the caller collects the
 * (workspace, *_wgrad_parts(...) rows, A*B*taps floats per row, gw) of all layers of a backward pass and finishes them together with
 * ONE call of partial_sum_multi (<= 32 jobs; host arrays; two launches in total; a training step has ~30 weight gradients).
 * scratch: mvsnerf_partial_sum_multi_scratch_floats(sum of the jobs' n_out) floats.  Same fixed summation order either way. */
int mvsnerf_conv3d_wgrad_parts(int A, int B, int Do, int Ho, int Wo, int stride, int two_x_sources);
int mvsnerf_conv3d_c8_blocked_wgrad_parts(int Cin, int Cin_real, int D, int H, int W);
int mvsnerf_conv2d_wgrad_parts(int A, int B, int N, int Ho, int Wo, int ksize, int stride);
size_t mvsnerf_partial_sum_multi_scratch_floats(int64_t total_n_out);
int mvsnerf_partial_sum_multi(int n_jobs, const float* const* partial, const int* n_part, const int64_t* n_out, float* const* dst,
                              float* scratch, void* stream);
/* (described in mvsnerf_hip.h: "The 16- / 32-output-channel layers (conv1.x, conv2.x, and the stride-1 data gradients) run on the fp32 matr ...") */
int mvsnerf_conv2d_mfma_tiles(int Cin, int Cout, int N, int H, int W, int ksize, int stride);
int mvsnerf_conv2d_fwd_stats(const float* x, const float* scale, const float* shift, int Cin, int cin_ld, int N, int H, int W,
                             const float* wpacked, int Cout, int ksize, int stride, float* out, float* stats_part, void* stream);
/* mvsnerf_resize_bilinear (models.py:859) of N three-channel images written as [N][Ho][Wo][4] (fourth channel 0) - the plane sweep's thumbnail input - in one
 * launch instead of resize + mvsnerf_nchw_to_nhwc; the same values. */
int mvsnerf_resize_bilinear_nhwc4(const float* src_n3hw, float* dst_nhw4, int N, int Hi, int Wi, int Ho, int Wo, void* stream);
/* The depth hypotheses of MVSNet.forward (models.py:903-906, linear in depth): out[i] = near_far[0] * (1 - t[i]) + near_far[1] * t[i] with the roundings of the
 * four elementwise kernels the reference runs; t = linspace(0, 1, D) and near_far on the device (one launch, no host synchronisation). */
int mvsnerf_depth_values(const float* t, const float* near_far, int D, float* out, void* stream);
/* FeatureNet's first layer (models.py:693) from the caller's (N, 3, H, W) images, without the channel-last copy: a no-grad encode; the bits of
 * mvsnerf_conv2d_fwd_stats(Cin = 4) on the zero-padded copy.  wpacked: that layer's packed weights (cin_pad 4, cout 8). */
int mvsnerf_conv2d_c3_nchw_fwd_stats(const float* imgs_nchw, int N, int H, int W, const float* wpacked, float* out, float* stats_part, void* stream);
int mvsnerf_conv2d_dgrad_k5s2(const float* g, int Cin, int N, int Ho, int Wo, const float* wpacked, int Cout,
                              int Hi, int Wi, float* out, void* stream);
/* The same launch, additionally filling a caller-owned timing record (stateless; bench.py derives the shader clock the chip sustains
 * under this kernel from it): census[(N*S + 127) / 128][16] int64 = {start, end (100 MHz wall clock), HW_ID, XCC_ID,
 * phase stamps [4..12], shader-clock ticks of the workgroup [13], -, -}. */
int mvsnerf_mlp_fwd_census(const float* packed, int F,
                           const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                           const float* dirs, int dirs_stride, int64_t N, int S, int alpha_only,
                           float* raw, long long* census, void* stream);
/* Test entry: the 32 positional-encoding B operands of the fp32 MLP tiles (csrc/mlp_fp32_dev.h) for both lane halves of every point,
 * out[P][32][2] from ndc[P][3] (contiguous).  variant 0: one evaluation per lane and k-step (pe_operand, what mvsnerf_mlp_fwd_wide runs);
 * variant 1: the half-shared packed evaluation (pe_all, what mvsnerf_mlp_fwd, mvsnerf_mlp_fwd_train and mvsnerf_raymarch_fwd run).  The two
 * must agree bit for bit (tests/test_gpu_pe_packed.py).  One wave per 32 points: P must be a multiple of 32 (nothing is padded), else -1. */
int mvsnerf_pe_operands_fwd(const float* ndc, int64_t P, int variant, float* out, void* stream);
/* Folded pack.  feature_linear and views_linears.0 have no activation between them, so a no-grad forward may run them as one affine map
 * (W' = Wv[:, :128] * Wf, b' = bv + Wv[:, :128] * bf, formed on the device in double and rounded to fp32 once).  mvsnerf_mlp_pack_fold writes
 * everything mvsnerf_mlp_pack writes - the standard layout, same offsets, same bits - sets one of the vector block's pad floats to 1.0f and appends
 * the folded views segment and bias behind the standard buffer: `packed` holds mvsnerf_mlp_packed_fold_floats(F) floats.  The buffer describes
 * itself: every fp32 no-grad kernel handed it (mvsnerf_mlp_fwd, mvsnerf_mlp_fwd_guarded's fp32 half, mvsnerf_raymarch_fwd*, mvsnerf_render_*)
 * skips the feature_linear GEMM and returns the same bits as every other; mvsnerf_mlp_fwd_train, the backward and the 16-bit kernels read the
 * standard part only and compute what they compute from a mvsnerf_mlp_pack buffer.  The stable mvsnerf_mlp_pack always writes 0.0f to that pad,
 * so a stable-tier caller with an exact mvsnerf_mlp_packed_floats(F) buffer can never make a kernel read past it - also when it re-packs into
 * memory that held a folded buffer before. */
size_t mvsnerf_mlp_packed_fold_floats(int F);
int mvsnerf_mlp_pack_fold(const float* const w[11], const float* const b[11], int F, float* packed, void* stream);
/* Network variant.  The reference has two radiance MLPs with the same layers and state_dict keys: Renderer_ours (net_type v0),
 * h_i = relu(pts_linears.i(h) * bias), and Renderer_linear (net_type v2), h_i = relu(pts_linears.i(h) + bias), bias = pts_bias(feat); v2's
 * forward_alpha also returns alpha_linear(h) without the ReLU.  The packed buffer carries the variant like the fold: the vector block is
 * [.. | alpha bias (V_BA) | fold flag (V_BA + 1) | variant flag (V_BA + 2) | pad | rgb_linear ..] and variant = 1 writes 1.0f to the variant
 * flag; everything else is mvsnerf_mlp_pack_fold's output bit for bit (mvsnerf_mlp_packed_fold_floats(F) floats).  mvsnerf_mlp_pack and
 * mvsnerf_mlp_pack_fold always write 0.0f there.  Every fp32 kernel handed the buffer reads the flag: mvsnerf_mlp_fwd (alpha_only = 1 on a
 * v2 buffer writes the un-clamped sigma, which can be negative; the full forward clamps), mvsnerf_mlp_fwd_guarded's fp32 half,
 * mvsnerf_raymarch_fwd*, mvsnerf_render_*, mvsnerf_mlp_fwd_train / mvsnerf_raymarch_train_fwd and mvsnerf_mlp_bwd / mvsnerf_raymarch_bwd with
 * bf16 = 0.  The 16-bit kernels (bf16, split, fp16x3, the bf16 backward) do NOT read it and compute the v0 network from any buffer: their
 * scaling assumes the multiplicative form.  A v2 network must therefore stay on the fp32 kernels (the Python layer enforces it).
 * variant: 0 = v0 (multiplicative), 1 = v2 (additive); anything else is MVSNERF_EINVAL.
 * F: even, 2 <= F <= 40 for every entry above and for the training entries that consume these buffers (mvsnerf_mlp_fwd_train, mvsnerf_mlp_bwd:
 * v0 and v2 alike; the saved-activation format keeps feature operands 16..19 of an F > 32 row in slots 2..5 of its direction block,
 * csrc/mlp_layout.h S_FV_HI). */
int mvsnerf_mlp_pack_fold_variant(const float* const w[11], const float* const b[11], int F, int variant, float* packed, void* stream);
/* ---- netwidth 256 (csrc/mlp_wide.hip, csrc/mlp_wide_layout.h): the no-grad fp32 forward of the same two networks at W = 256 ----
 * netdepth 6, skips [4], multires 10, raw 3-d view directions as above; the 11 tensors have the shapes of the reference's W = 256 network
 * (pts_linears 256x63, 4 x 256x256, 256x319; pts_bias 256xF; feature_linear 256x256; alpha_linear 1x256; views_linears.0 128x259; rgb_linear
 * 3x128), in the order of mvsnerf_mlp_pack.
 * mvsnerf_mlp_wide_packed_floats(F, width): floats of the packed buffer; 0 when unsupported: width != 256, F odd, F < 4 or F > 40.
 * mvsnerf_mlp_pack_wide: variant as for mvsnerf_mlp_pack_fold_variant (0 = v0, 1 = v2; the buffer carries it, no fold tail exists at this width).
 * mvsnerf_mlp_fwd_wide: the arguments and results of mvsnerf_mlp_fwd from `ndc` on (strided inputs, direction of point p = dirs[(p / S) *
 *   dirs_stride], alpha_only: raw[P][1], un-clamped on a v2 buffer).  One 256-thread workgroup per 128 points, 139 KB of LDS, one workgroup
 *   per CU.  ONLY a buffer written by mvsnerf_mlp_pack_wide may be passed, and such a buffer to no other entry: the 128-wide kernels would read
 *   it with their own offsets.  No training forward, backward, 16-bit, ray-march or whole-frame entry exists at this width.
 * Return codes as everywhere: -1 invalid argument, -2 unsupported shape, -3 misaligned pointer (packed, raw: 16 bytes).  Nothing is allocated. */
size_t mvsnerf_mlp_wide_packed_floats(int F, int width);
int mvsnerf_mlp_pack_wide(const float* const w[11], const float* const b[11], int F, int width, int variant, float* packed, void* stream);
int mvsnerf_mlp_fwd_wide(const float* packed, int F, int width,
                         const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                         const float* dirs, int dirs_stride, int64_t N, int S, int alpha_only,
                         float* raw, void* stream);
/* (described in mvsnerf_hip.h: "---- Guarded 16-bit sequences (ABI v10) ---- ...") */
typedef struct {
    const float* feats_cl; const float* imgs_cl;   /* [V][H][W][32], [V][H][W][4] as for mvsnerf_planesweep_costvar_fwd (with_img = 1) */
    const float* proj; const float* depth;         /* [V][3][4], [D] */
    int V, H, W, D, pad, CP;                       /* CP = 3V + 32 rounded up to a multiple of 4 */
    float* masks;                                  /* [V][D][Hp][Wp] */
    void* cost16x2;                                /* two fp16 planes: 2 * ceil(CP/16) * D*Hp*Wp * 16 halfs */
    float* cost32;                                 /* fp32 blocks of four channels: (CP/4) * D*Hp*Wp * 4 floats (written only on fallback) */
    const void* w_f16x3;                           /* mvsnerf_conv0_f16x3_pack */
    const float* w_c8;                             /* mvsnerf_conv3d_pack_weights_c8 (the fp32-MFMA conv0's layout) */
    int Cin;                                       /* real input channels 3V + 32 */
    float* out;                                    /* raw conv0 output [D][Hp][Wp][8] */
    float* stats_part;                             /* InPlaceABN partial sums (see above) or NULL */
    int* guard;
} mvsnerf_sweep_conv0_args;
int mvsnerf_sweep_conv0_guarded_fwd(const mvsnerf_sweep_conv0_args* a, void* stream);
/* ---- conv1 / conv2 of CostRegNet on the fp16 matrix cores with fp32-grade results (ABI v11; models.py:743-746 `conv1 = ConvBnReLU3D(8, 16, stride=2)`,
 * `conv2 = ConvBnReLU3D(16, 16)`, called at models.py:757-758) - what a no-grad encode runs for these two layers from 256 K output voxels on.
 * Two fp16 pieces per operand (activations x 2^4, weights x 2^8, exact), x1 w0 + x0 w1 + x0 w0 on v_mfma_f32_16x16x32_f16, fp32 accumulation
 * (csrc/conv_f16x3_tiled.hip).  Shapes: (Cin 8, stride 2) and (Cin 16, stride 1), Cout <= 16 (mvsnerf_conv3d_f16x3_supported).
 *   x: [D][H][W][cin_ld] fp32 RAW output of the previous layer with its pending InPlaceABN (scale, shift; both NULL: x is taken as it is);
 *   out: [Do][Ho][Wo][Cout] fp32 raw; stats_part: NULL or 2 * Cout * mvsnerf_conv3d_f16x3_slots() floats for mvsnerf_abn_finalize (n_blocks = slots).
 *   mvsnerf_conv3d_f16x3_pack: nn.Conv3d weight w[Cout][Cin][3][3][3] -> mvsnerf_conv3d_f16x3_packed_elems(Cin) fp16 elements (16-byte aligned);
 *   a weight outside fp16's range is recorded in a status tail and reported through the guard by the kernel.
 *   mvsnerf_conv3d_f16x3_fwd: the UNGUARDED kernel (an operand beyond |x| < 4094 leaves NaNs in the outputs it touches).
 *   The other end of fp16 is NOT reported by these kernels: activated inputs that are ALL below ~2^-7, or weights below 2^-11, put the second
 *   pieces into fp16's subnormals and the result silently drops from fp32 grade towards 2^-11 + log2(largest |x|) bits.  The layers this serves (conv1 / conv2
 *   behind an InPlaceABN: unit-variance inputs, |w| ~ 1e-2 .. 1) are four to seven binary orders above that floor; a caller with other data uses the fp32 entry.
 *   (The MLP kernel manages both ends itself since ABI v12; the same per-tile power-of-two scale would work here and is not built.)
 *   mvsnerf_conv3d_f16x3_guarded_fwd: the guarded sequence (see "Guarded 16-bit sequences"): the kernel above sets guard[0] when an operand left the
 *   range, the layer's fp32 kernel (w_f32: mvsnerf_conv3d_pack_weights_mfma layout for Cin 8, mvsnerf_conv3d_pack_weights layout for Cin 16) and a
 *   statistics pass run behind it predicated on that word; consume != 0 counts the event in guard[1] and re-arms guard[0] at the end. */
int mvsnerf_conv3d_f16x3_supported(int Cin, int Cout, int stride);
int mvsnerf_conv3d_f16x3_slots(void);
size_t mvsnerf_conv3d_f16x3_packed_elems(int Cin);
int mvsnerf_conv3d_f16x3_pack(const float* w, int Cin, int Cout, void* packed, void* stream);
int mvsnerf_conv3d_f16x3_fwd(const float* x, const float* scale, const float* shift, int Cin, int cin_ld, int D, int H, int W, const void* packed, int Cout,
                             int stride, float* out, float* stats_part, void* stream);
int mvsnerf_conv3d_f16x3_guarded_fwd(const float* x, const float* scale, const float* shift, int Cin, int cin_ld, int D, int H, int W,
                                     const void* w_f16x3, const float* w_f32, int Cout, int stride, float* out, float* stats_part,
                                     int* guard, int consume, void* stream);
/* ---- rendering a fine-tuned scene (train_mvs_nerf_finetuning_pl.py:192-252, validation_step of the fine-tuning script) ----
 * gather_colorvol: gen_pts_feats of --use_color_volume (renderer.py:134-135: the per-sample feature row is ONE trilinear lookup of the
 *   (8 + 4V)-channel volume) and gen_dir_feature (renderer.py:111-122, 142-147) in one launch.  vol: C channels per voxel, C % 4 == 0,
 *   8 < C <= 40 (other C: MVSNERF_EUNSUPPORTED), memory order vol_layout, 16-byte aligned; ndc[N][S][3]; feat[N*S][feat_stride]
 *   (feat_stride % 4 == 0, 16-byte aligned) receives channels 0..C-1, bit-identical to mvsnerf_volume_sample_fwd's; rays_dir[N][3] and
 *   dirs_out[N][3] may both be NULL (lookup only), w2c_ref[4][4] may be NULL (no rotation): dirs_out = mvsnerf_dir_feature_fwd(normalize = 1).
 *   force_offsets64 != 0 runs the 64-bit-offset form of the kernel whatever the sizes (what a volume or batch beyond 2^31 floats takes; for tests).
 * raymarch_colorvol_fwd_batched: K batches of mvsnerf_raymarch_fwd_batched on a C = 8 + 4V-channel colour volume (a->vol: [..][C] in a->vol_layout):
 *   gather_colorvol instead of the image gather, then the batch's MLP choice and compositing.  imgs, imgs_nhwc4, K and rays_pts are not read.
 * render_rays: the chunk loop of that validation_step enqueued from one host call - per sub-batch of batch_rays rays taken from
 *   rays[first_ray .. first_ray + n_rays) ([..][8] = origin, direction, near, far): coarse depths near (1 - t[s]) + far t[s] (lindisp: in
 *   disparity) with points and reference-view NDC coordinates; with a density volume and n_importance > 0 ray_marcher_fine on
 *   u[first_ray + ..][n_importance] and the points of the merged S + n_importance depths; the ray march (C == 8: image gather as
 *   mvsnerf_render_pixels_fwd; C == 8 + 4V: gather_colorvol, no images / K needed; else MVSNERF_EUNSUPPORTED); rgb[n_rays][3] and, when
 *   non-NULL, depth / acc / disp[n_rays] leave the call.  Results do not depend on batch_rays.  workspace: render_rays_workspace_floats(
 *   batch_rays, S, n_importance, F = 8 + 4V) floats, 16-byte aligned, reused by every sub-batch.  Arguments are validated before the first launch. */
int mvsnerf_gather_colorvol_fwd(const float* vol, int D, int H, int W, int C, const float* ndc, int64_t N, int S,
                                const float* rays_dir, const float* w2c_ref, float* feat, int feat_stride, float* dirs_out,
                                int vol_layout, int force_offsets64, void* stream);
int mvsnerf_raymarch_colorvol_fwd_batched(const mvsnerf_raymarch_args* a, int K, int C, void* stream);
typedef struct {
    const float* vol; int D, H, W, C, vol_layout;  /* C = 8 (neural volume + source images) or 8 + 4V (colour volume) */
    const float* imgs_nhwc4; int V, IH, IW;        /* [V][IH][IW][4] source images (C == 8; else NULL); V source views either way */
    const float* w2c; const float* K;              /* [V][4][4], [V][3][3] source views (C == 8; else NULL) */
    const float* K_ref; const float* w2c_ref; const float* near_far_ref;   /* reference view [3][3], [4][4], [2] */
    int W_ref, H_ref, pad, lindisp;
    const float* packed_mlp; const void* packed_mlp_bf16; const void* packed_mlp_split; int n_split; int* guard;   /* as mvsnerf_render_args */
    const float* rays; int64_t first_ray, n_rays;  /* [>= first_ray + n_rays][8] */
    const float* t; int S;                         /* [S] = linspace(0, 1, S) */
    const float* density; int DD, DH, DW;          /* NULL, or the density volume [DD][DH][DW] of ray_marcher_fine */
    const float* u; int n_importance;              /* NULL / 0, or uniform draws [>= first_ray + n_rays][n_importance] */
    int white_bkgd, batch_rays;
    float* workspace; size_t workspace_floats;
    float* rgb; float* depth; float* acc; float* disp;     /* rgb required, others may be NULL */
} mvsnerf_render_rays_args;
size_t mvsnerf_render_rays_workspace_floats(int batch_rays, int S, int n_importance, int F);
int mvsnerf_render_rays_fwd(const mvsnerf_render_rays_args* a, void* stream);
/* ---- frame metrics (renderer.ipynb cells 8 and 16; mvsnerf_amd/evaluate.py is the host statement of the same protocol) ----
 * The evaluation record of K finished frames in two launches (csrc/metrics.hip), no atomics, bit-reproducible and independent of K.
 *   pred, gt: [K][H][W][3] fp32 (HWC, what render_view / render_rays return); depth_pred, depth_gt: [K][H][W] or both NULL.
 *   out: [K][MVSNERF_METRICS_ROW] doubles, every entry written:
 *      0 sum of squared error over all pixels and channels      1 pixel count H*W
 *      2 the same over the centre crop (H/10 rows, W/10 columns off every side: psnr_center_crop)      3 its pixel count (0 when H/10 or W/10 is 0)
 *      4 the same over depth_gt != 0 (psnr_masked)              5 its pixel count          (both 0 without depth)
 *      6..8 sum of the SSIM map of channel 0..2 over the valid region (window wholly inside the image)    9 its pixel count (H-win+1)(W-win+1)
 *      10 sum of |depth_pred - depth_gt * gt_scale| over depth_gt > 0     11..13 how many of those errors are below thresholds[0..2]     14 pixel count of depth_gt > 0
 *      A mean squared error is entry / (3 * count); counts are whole numbers.
 *   SSIM: structural_similarity of skimage 0.19 with multichannel defaults - uniform win_size x win_size window (odd, 3..11), sample covariance,
 *      C1 = (K1 data_range)^2, C2 = (K2 data_range)^2.  Window sums are fp32 and centred (a constant image has variance exactly 0); squared errors are
 *      fp32 per pixel and channel; depth errors and every sum across pixels are double.
 *   thresholds: HOST array of three doubles.  workspace: mvsnerf_frame_metrics_workspace_bytes(K, H, W, win_size) bytes (one row per frame and tile;
 *      0 for arguments the entry refuses), 8-byte aligned like out; the images need 4-byte alignment only (a frame of a batch is a valid input).
 *   Returns MVSNERF_EINVAL for a NULL pred / gt / out / workspace / thresholds, one depth pointer without the other, K < 1, H or W < 1, an even
 *   win_size or one outside 3..11; MVSNERF_EUNSUPPORTED for min(H, W) < win_size; MVSNERF_EALIGN; all before the first launch. */
#define MVSNERF_METRICS_ROW 15
size_t mvsnerf_frame_metrics_workspace_bytes(int K, int H, int W, int win_size);
int mvsnerf_frame_metrics_fwd(const float* pred, const float* gt, const float* depth_pred, const float* depth_gt, int K, int H, int W,
                              int win_size, double data_range, double K1, double K2, double gt_scale, const double* thresholds,
                              double* out, void* workspace, void* stream);
/* ---- fusing per-view volumes into one scene volume (train_mvs_nerf_fusion_finetuning_pl.py; csrc/fusion.hip) ----
 * volume_fuse_splat: update_volume (:35-76) of P samples into a [D][H][W] voxel grid with every colliding write ACCUMULATED (the reference's
 *   `vol[..., idx] += x` keeps one of them on a GPU): ndc[P][3] box coordinates (x -> W, y -> H, z -> D), feat[P][feat_stride] (C channels, C % 4 == 0,
 *   4 <= C <= 40; other C: MVSNERF_EUNSUPPORTED), alpha[P].  Sums live in a caller-owned, caller-ZEROED int64 workspace of
 *   volume_fuse_workspace_words(D, H, W, C) words (0: arguments refused), 16-byte aligned, that outlives the call:
 *     [0] number of refused contributions   [1] log2 of the fixed-point scale (32, written by the first non-empty splat)   [2..7] unused
 *     [8 + ((d H + h) W + w)(C + 4) ..] C feature sums, the alpha sum, the weight sum, 2 pad words.
 *   Each contribution is the fp32 product rounded once to a multiple of 2^-32 (__double2ll_rn(prod * 2^32)) and added with a 64-bit integer atomic:
 *   the words do not depend on the order of points, calls, views or ranks, and two workspaces add word by word.  A contribution with
 *   |prod| >= 2^20, or not finite, is not added and counted in word 0 (2^11 maximal contributions fit a word); a caller must not use such sums.
 *   The reference's arithmetic is kept: v = ndc / (1.0f / (dim - 1)), index truncated toward zero and kept when 0 <= idx < dim - 1 on all axes
 *   (non-finite coordinates drop the point), local = v - floor(v), weight of shift (x, y, z) = (|local_x - x| |local_y - y|) |local_z - z| - the
 *   OPPOSITE corner's - added at voxel (idx_z + x, idx_y + y, idx_x + z) - x and z swapped.  ray_weight of the reference's signature is unused there.
 * volume_fuse_finish: :190-192 per voxel on the rounded sums - s = (float)(sum 2^-32), inv = 1.0f / ((float)(weight sum 2^-32) + 1e-6f), out = s * inv -
 *   into feat_volume[C][D][H][W] and density_volume[D][H][W] (the reference's NCDHW order); untouched voxels are 0.  Word 0 is the caller's to check.
 * ray_march_bbox: ray_marcher(bbox_3D=) (data/ray_utils.py:143-197) and the box coordinates of the fusion script (:263): rays[N][8], bbox[2][3],
 *   t[S] = linspace(0, 1, S), jitter[N][S] = the caller's torch.rand draw (read when perturb > 0; NULL otherwise), -> z[N][S], pts[N][S][3] = o + d z,
 *   ndc[N][S][3] = (pts - bbox[0]) / (bbox[1] - bbox[0]).  near / far = dda: inv = 1 / (d + 1e-6), max over axes of the slab minima, min of the maxima
 *   (NaNs are handed on like torch.min / torch.max); a ray that misses the box keeps near > far. */
size_t mvsnerf_volume_fuse_workspace_words(int D, int H, int W, int C);
int mvsnerf_volume_fuse_splat(int D, int H, int W, int C, const float* ndc, int64_t P, const float* feat, int feat_stride,
                              const float* alpha, void* workspace_zeroed, void* stream);
int mvsnerf_volume_fuse_finish(int D, int H, int W, int C, const void* workspace, float* feat_volume, float* density_volume, void* stream);
int mvsnerf_ray_march_bbox_fwd(const float* rays, const float* bbox, const float* t, const float* jitter, float perturb, int lindisp,
                               int64_t N, int S, float* z, float* pts, float* ndc, void* stream);
/* ---- 8-bit video frames (renderer_video.ipynb: clamp * 255 -> uint8, visualize_depth_numpy of utils.py:30-45, crop, rgb | depth; csrc/frames.hip) ----
 * depth_range: x0 = nan_to_num(depth[n]) (NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX); out2[0] = min{x0 : x0 > 0} (+inf when no element is positive),
 *   out2[1] = max x0 (utils.py:35-38), both written on the device.  Two launches, no atomics; min and max never round, so every run gives the same bits.
 *   workspace: depth_range_workspace_floats(n) floats (0: n < 1), 4-byte aligned like depth and out2.
 * frame_u8: rgb [H][W][3] and depth [H][W] fp32 -> out [H'][W' * panels][3] bytes, H' = H - 2 crop_h, W' = W - 2 crop_w: crop_h rows and crop_w columns are
 *   removed from every side of each panel, then the colour panel (rgb != NULL) and the depth panel (depth_panel = 1) are placed side by side.
 *   rgb may be NULL with depth_panel = 1 (the depth panel alone: visualize_depth*); depth / minmax / lut may be NULL with depth_panel = 0.
 *   minmax: DEVICE pointer to {mi, ma}; lut: DEVICE pointer to [256][3] bytes, copied as they are (the channel order is the table's).
 *   All arithmetic is fp32 with every operation rounded on its own (no FMA contraction, IEEE division):
 *     colour  byte = trunc(clamp(rgb, 0, 1) * 255), NaN -> 0
 *     depth   x0 = nan_to_num(depth), t = (x0 - mi) / ((ma - mi) + 1e-8f), i = trunc(255 t) SATURATED to [0, 255] (numpy's cast wraps or is undefined
 *             out of range), NaN -> 0, pixel = lut[i][0..2]
 *   out needs NO alignment (frame k of a (K,H',Wout,3) tensor with odd sizes starts anywhere); rgb, depth, minmax 4 bytes.  Exactly H' * W' * panels * 3
 *   bytes are written.  MVSNERF_EINVAL: NULL out, no panel at all, a missing pointer of a requested panel, H or W < 1, a negative crop or one that leaves
 *   nothing, depth_panel not 0 / 1; MVSNERF_EALIGN; MVSNERF_EUNSUPPORTED for H * W >= 2^28; all before the launch. */
size_t mvsnerf_depth_range_workspace_floats(int64_t n);
int mvsnerf_depth_range_fwd(const float* depth, int64_t n, float* out2, float* workspace, void* stream);
int mvsnerf_frame_u8_fwd(const float* rgb, const float* depth, int H, int W, const float* minmax, const unsigned char* lut,
                         int crop_h, int crop_w, int depth_panel, unsigned char* out, void* stream);
/* ---- empty-space skipping (no reference counterpart: its renderer queries every sample; csrc/sparse.hip) ----
 * live_samples: which of the P = N*S samples of a ray batch can contribute, and their stable compaction.  density [D][H][W] (update_density_volume's sigma
 *   at the voxel centres), ndc [N][S][3] reference-view NDC.  A sample is LIVE iff one of its three coordinates is non-finite, or some IN-GRID corner of
 *   its trilinear cell holds a value v with !(v <= thr) (strictly above; a NaN voxel is live).  The cell is floor(ix), floor(iy), floor(iz) with
 *   ix = ((gx + 1) / 2) * (W - 1), gx = x * 2 - 1 (iy from y, H; iz from z, D), fp32 with every operation rounded on its own - the index arithmetic of
 *   the density lookup of mvsnerf_ray_marcher_fine_fwd (csrc/density_cell.h holds it for both).  Corners outside the grid do not count (the lookup pads
 *   with zeros): for thr >= 0 a dead sample's trilinear density is <= thr.
 *   Outputs: count[0] = number of live samples (int32, on the device); idx[j] = flat index n*S + s of the j-th live sample, ASCENDING; ndc_c[j][3],
 *   pts_c[j][3] = the rows of ndc / pts [N][S][3] at idx[j]; dir_c[j][3] = rays_dir[idx[j] / S][3] as given.  pts / pts_c and rays_dir / dir_c may be NULL.
 *   idx holds P entries, the compact rows P rows (the worst case); entries from count on are not written.  No atomics, three launches in stream order,
 *   no workgroup waits on another: two runs give the same bytes.
 *   workspace: live_samples_workspace_bytes(P) bytes (0: P < 1 or P >= 2^31), 8-byte aligned; everything else 4-byte aligned.
 *   MVSNERF_EINVAL: a NULL density / count (ndc / idx / ndc_c / workspace with P > 0), pts without pts_c or rays_dir without dir_c, D, H or W < 1, N < 0,
 *   S < 1, a NaN thr; MVSNERF_EUNSUPPORTED: P >= 2^31; MVSNERF_EALIGN; all before the first launch.  P == 0 writes count = 0.
 * expand_rows: dst[P][C] with dst[idx[j]] = src[j] for j < min(count[0], src_rows) and every other row zero; every element of dst is written by the call.
 *   idx ascending as live_samples leaves it (an entry can only ever select a row of dst: it is range-checked per tile); count is read on the device, so
 *   a caller that sized src from an earlier read of it needs no second one.  src / idx may be NULL with src_rows == 0.
 *   MVSNERF_EINVAL: NULL count / dst, src_rows < 0 or > P, P < 0, C < 1; MVSNERF_EUNSUPPORTED: C > 64, P >= 2^31; MVSNERF_EALIGN (4 bytes).
 * compact_rows: the inverse, dst[dst_rows][C] with dst[j] = src[idx[j]] for j < min(count[0], dst_rows), src [P][C], and every other row zero; every
 *   element of dst is written by the call.  It brings the dense d_raw of the compositing backward down to the live rows of a training step that skips
 *   empty space (ops.raymarch_sparse_train).  count is read on the device.  An idx[j] outside [0, P) gives a zero row: the entry is range-checked
 *   before the load, src is never read outside its P rows, whatever idx holds.  C == 4 with 16-byte aligned src and dst moves one 16-byte load and
 *   one 16-byte store per row (4 + 16 + 16 bytes per live row, 16 per dead one); other C one element per thread.  One launch, no atomics, no LDS.
 *   src / idx may be NULL with dst_rows == 0, which launches nothing.
 *   MVSNERF_EINVAL: NULL count / dst, P < 0, dst_rows < 0 or > P, C < 1; MVSNERF_EUNSUPPORTED: C > 64, P >= 2^31; MVSNERF_EALIGN (4 bytes). */
size_t mvsnerf_live_samples_workspace_bytes(int64_t P);
int mvsnerf_live_samples_fwd(const float* density, int D, int H, int W, float thr, const float* ndc, const float* pts, const float* rays_dir,
                             int64_t N, int S, int* count, int* idx, float* ndc_c, float* pts_c, float* dir_c, void* workspace, void* stream);
int mvsnerf_expand_rows_fwd(const float* src, const int* idx, const int* count, int64_t src_rows, int64_t P, int C, float* dst, void* stream);
int mvsnerf_compact_rows_fwd(const float* src, const int* idx, const int* count, int64_t P, int64_t dst_rows, int C, float* dst, void* stream);
/* ---- early ray termination in no-grad renders (no reference counterpart: renderer.py:18-26 composites all S samples; csrc/sparse.hip) ----
 * A ray batch is marched in segments of stop_every samples; between two segments the transmittance in front of the next one decides which rays go on.
 * These three entries answer a misaligned pointer with MVSNERF_EINVAL, like a NULL one; every check comes before the first launch.
 * ray_transmittance: ray_T[n] *= prod_{s0 <= s < s1} ((1 - alpha) + 1e-10f), alpha = 1 - expf(-raw[n][s][3]): the two expressions of compositing
 *   (csrc/composite_wave.h holds them for both).  raw [N][S][4], 16-byte aligned; ray_T [N], caller-owned, set to 1 by the host before the first
 *   window.  The order is fixed: T = ray_T[n]; for s = s0 .. s1 - 1 ascending: T = fl(T * factor_s); ray_T[n] = T - so consecutive windows give the bits
 *   of one left-to-right product, and two runs give the same bytes.  A NaN sigma gives a NaN ray_T.  Four lanes own a ray and read rows s, s+1, s+2, s+3:
 *   (s1 - s0) * 16 bytes of raw are touched per ray, in whole 64-byte lines when n * S + s0 is a multiple of 4.  One launch, no LDS, no atomics.
 *   MVSNERF_EINVAL: NULL or misaligned raw / ray_T, N < 0, S < 1, a window with s0 < 0, s1 > S or s0 >= s1; MVSNERF_EUNSUPPORTED: N * S >= 2^31.
 * live_samples_range: live_samples over the window s0 <= s < s1 of every ray.  A sample is SELECTED iff !(ray_T[n] < eps) when ray_T is given (fp32
 *   compare; a NaN ray_T never stops its ray) and its cell is live by live_samples' predicate when density is given (both NULL: the whole window).
 *   count[0] = number selected; idx[j] = n * S + s of the j-th, ASCENDING; ndc_c / pts_c / dir_c as live_samples leaves them.  idx and the compact
 *   rows hold N * (s1 - s0) entries (the worst case); entries from count on are not written.  The same three launches as live_samples (its scan kernel,
 *   the RANGE instantiations of its count and write tiles): no atomics, no workgroup waits on another, two runs give the same bytes, count stays on
 *   the device.  workspace: live_samples_range_workspace_bytes(N, s1 - s0) bytes (0: N < 1, a window < 1 or N * window >= 2^31), 8-byte aligned.
 *   MVSNERF_EINVAL: NULL count (ndc / idx / ndc_c / workspace with N > 0), pts without pts_c or rays_dir without dir_c, a misaligned pointer, N < 0,
 *   S < 1, a bad window, a NaN eps, and with density: D, H or W < 1 or a NaN thr; MVSNERF_EUNSUPPORTED: N * S >= 2^31.  N == 0 writes count = 0.
 * scatter_rows: dst[idx[j]] = src[j] for j < min(count[0], src_rows); every other row of dst [P][C] is left untouched (expand_rows rewrites all P
 *   rows; this one adds a segment's rows to a raw the host zero-filled once).  idx[j] is range-checked against [0, P) before the store: an entry
 *   outside writes nothing.  Distinct entries (what live_samples_range leaves) make the result independent of the order of the stores.  C == 4 with
 *   16-byte aligned src and dst moves one 16-byte load and store per row; src / idx may be NULL with src_rows == 0, which launches nothing.
 *   MVSNERF_EINVAL: NULL or misaligned count / dst (src / idx with src_rows > 0), src_rows < 0 or > P, P < 0, C < 1; MVSNERF_EUNSUPPORTED: C > 64, P >= 2^31. */
int mvsnerf_ray_transmittance_fwd(const float* raw, int64_t N, int S, int s0, int s1, float* ray_T, void* stream);
size_t mvsnerf_live_samples_range_workspace_bytes(int64_t N, int G);
int mvsnerf_live_samples_range_fwd(const float* density, int D, int H, int W, float thr, const float* ndc, const float* pts, const float* rays_dir,
                                   int64_t N, int S, int s0, int s1, const float* ray_T, float eps, int* count, int* idx, float* ndc_c,
                                   float* pts_c, float* dir_c, void* workspace, void* stream);
int mvsnerf_scatter_rows_fwd(const float* src, const int* idx, const int* count, int64_t src_rows, int64_t P, int C, float* dst, void* stream);
/* ---- a density volume in the renderer's own frame (no reference counterpart; csrc/occupancy.hip) ----
 * voxel_points: the nodes (k,j,i) of planes [d0, d1) of a [D][H][W] volume, rows in [k][j][i] order: ndc[(d1-d0) H W][3] = (i/(W-1), j/(H-1), k/(D-1)), IEEE
 *   divisions, 0 on an axis of size 1 - the coordinates whose trilinear cell starts exactly on the node, whether the volume is a reference frustum or a
 *   world-space box.  pts (may be NULL: a box volume has no camera) receives the world positions that mvsnerf_ray_points_fwd / get_ndc_coordinate map to
 *   those coordinates: u = ((x (wf + 2 pad) - pad) / wf) (W_img - 1), wf = W_img / 4 (v alike), z = near + z_ndc (far - near) (lindisp: in 1 / z),
 *   world = c2w (K^-1 (u z, v z, z)).  K_ref[9], c2w_ref[12 or 16, row-major 3x4 part] and near_far[2] are HOST arrays, read during the call: the entry
 *   inverts K and forms c2w K^-1 once, in double; the kernel does nine multiply-adds per node.  Both outputs are written for every row of the range
 *   and nothing else; 16-byte aligned outputs are written with 16-byte stores.
 *   MVSNERF_EINVAL: NULL ndc, D, H or W < 1, a plane range outside 0 <= d0 <= d1 <= D; with pts: a NULL camera array, W_img or H_img < 2, pad < 0, a
 *   singular or non-finite K, non-finite near / far (zero under lindisp); MVSNERF_EUNSUPPORTED: D H W >= 2^31; MVSNERF_EALIGN (4 bytes); all before the
 *   launch.  d0 == d1 launches nothing.
 * max_dilate3d: out[k][j][i] = max of in over the (2r+1)^3 window clipped to the grid, r in {0, 1, 2}; a NaN in the window gives NaN (a NaN voxel must
 *   stay live for live_samples); r == 0 copies.  Three separable passes (W, H, D); workspace: D H W floats (may be NULL when r == 0), distinct from in
 *   and out.  Per voxel 4 bytes are read and 4 written in each pass (the neighbours come from cache): 24 bytes for r > 0, 8 for r == 0.  With W % 4 == 0 and
 *   16-byte aligned buffers a thread moves four voxels of a row per access; the results do not depend on which form runs.
 *   MVSNERF_EINVAL: NULL in / out (workspace with r > 0), in == out or a workspace equal to either, D, H or W < 1, r outside 0..2;
 *   MVSNERF_EUNSUPPORTED: D H W >= 2^31; MVSNERF_EALIGN (4 bytes); all before the first launch. */
int mvsnerf_voxel_points_fwd(int D, int H, int W, int d0, int d1, const float* K_ref, const float* c2w_ref, const float* near_far,
                             int W_img, int H_img, int pad, int lindisp, float* ndc, float* pts, void* stream);
int mvsnerf_max_dilate3d_fwd(const float* in, int D, int H, int W, int r, float* out, float* workspace, void* stream);
/* ---- counted launches: the gather and MLP stage of the compacted marches on a row count that stays on the device ----
 * The rows form of their namesakes (S = 1: every row is its own ray and has its own direction row; dense rows - ndc / pts / dirs / rays_dir / dirs_out
 * [cap][3], feat [cap][F or feat_stride], raw [cap][4 or 1]) with (cap, count) in place of (N, S): cap is the capacity of the buffers in rows, a host
 * integer; count the int32 word mvsnerf_live_samples_fwd / _range_fwd leave on the device.  A launch works on rows [0, n), n = min(max(count[0], 0), cap),
 * read by every workgroup with one scalar load before any other global load; it produces the bits of its namesake at N = n, S = 1 on those rows and
 * touches no row >= n of its outputs.  Nothing is read on the host, so a sequence of these can be enqueued ahead or captured into a graph.  The grid
 * is sized by cap: the fp32 128-wide kernel walks the ceil(n / 128) tiles with min(ceil(cap / 128), 512) workgroups (the form of the predicated kernel
 * behind a guard); every other kernel launches a workgroup per tile of cap, and one whose tile starts at or behind row n returns at once.
 * mlp_fwd_split_counted takes n_split = MVSNERF_SPLIT_FP16 only and mlp_fwd_guarded_counted is the guarded sequence (counted fp16x3 -> counted fp32
 * predicated on the guard -> consume; all enqueued whatever the count); the bf16 kernels have no counted form.
 * MVSNERF_EINVAL: NULL count or a NULL buffer its namesake refuses, cap < 0, the namesake's other refusals; MVSNERF_EALIGN: count off 4 bytes, the buffers
 * the namesake wants on 16 bytes; MVSNERF_EUNSUPPORTED: cap >= 2^31, an F / width / C / n_split outside the kernel's; cap == 0 enqueues nothing. */
int mvsnerf_mlp_fwd_counted(const float* packed, int F, const float* ndc, const float* feat, const float* dirs, int64_t cap, const int* count,
                            int alpha_only, float* raw, void* stream);
int mvsnerf_mlp_fwd_guarded_counted(const void* packed_fp16, const float* packed_f32, int F, const float* ndc, const float* feat, const float* dirs,
                                    int64_t cap, const int* count, int alpha_only, float* raw, int* guard, void* stream);
int mvsnerf_mlp_fwd_split_counted(const void* packed_split, const float* packed_f32, int F, int n_split, const float* ndc, const float* feat,
                                  const float* dirs, int64_t cap, const int* count, int alpha_only, float* raw, void* stream);
int mvsnerf_mlp_fwd_wide_counted(const float* packed, int F, int width, const float* ndc, const float* feat, const float* dirs, int64_t cap,
                                 const int* count, int alpha_only, float* raw, void* stream);
int mvsnerf_gather_fwd_counted(const float* vol, int D, int H, int W, const float* imgs_nhwc4, int V, int IH, int IW, const float* w2c, const float* K,
                               const float* pts, const float* ndc, int64_t cap, const int* count, const float* rays_dir, float* feat, int feat_stride,
                               float* dirs_out, int vol_layout, void* stream);
int mvsnerf_gather_colorvol_fwd_counted(const float* vol, int D, int H, int W, int C, const float* ndc, int64_t cap, const int* count,
                                        const float* rays_dir, const float* w2c_ref, float* feat, int feat_stride, float* dirs_out, int vol_layout,
                                        int force_offsets64, void* stream);
/* ---- the training rays of a scene as a device-resident bank (data/dtu_ft.py:143-188 and data/blender.py:49-85, read_meta's all-rays buffer;
 *      csrc/scene_rays.hip) ----
 * Bank: images_rgba [M][H][W][4] uint8 (three-channel input is stored with alpha 255; a ray's colour is one 32-bit load), c2w [M][3][4], K [M][3][3],
 *   near_far [M][2] fp32, depth_bank [M][H][W] fp32 or NULL.  idx [B] int64: flat indices into M*H*W, view-major then row-major - the order of
 *   torch.cat(all_rays, 0): m = idx / (H W), y = (idx % (H W)) / W, x = idx % W.  An index outside [0, M H W) gives an all-zero row in every output and
 *   nothing is read for it; no index makes a kernel read outside the bank.
 * scene_rays_gather: rays [B][8] = [o | d | near | far] and rgb [B][3] - all_rays[idx], all_rgbs[idx] - plus depth [B] = depth_bank[idx] and
 *   mask [B] (bytes 0 / 1, alpha > 0; data/blender.py:69) when those pointers are non-NULL (depth needs a depth_bank).
 * scene_rays_march: the same rows and the front end of a fine-tuning step (train_mvs_nerf_finetuning_pl.py:147-156) in ONE launch: z [B][S] of
 *   ray_marcher (data/ray_utils.py:152-197) from t [S] = the caller's linspace(0, 1, S), jitter [B][S] = the caller's torch.rand draw (read when
 *   perturb > 0; NULL otherwise) and lindisp, pts [B][S][3] = o + d z, and, when ndc is non-NULL, ndc [B][S][3] = get_ndc_coordinate (utils.py:112-146)
 *   in the reference camera (w2c_ref [4][4], K_ref [3][3], near_far_ref [2], W_ref, H_ref, pad), what mvsnerf_ray_points_fwd computes from the same rays.
 * Arithmetic, fp32 with every operation rounded on its own unless stated (no contraction, IEEE divisions):
 *   direction ((x - cx) / fx, (y - cy) / fy, 1) (data/ray_utils.py:27); rays_d[k] = (dx R[k][0] + dy R[k][1]) + R[k][2]; rays_o = c2w[:, 3]; near, far copied;
 *   colour c / 255 (torch's ToTensor on the CPU), then rgb a + (1 - a) with a = alpha / 255 (data/blender.py:70; alpha 255 leaves rgb as it is);
 *   z = near (1 - t) + far t (lindisp: 1 / ((1 / near)(1 - t) + (1 / far) t)); perturb > 0: lower + (upper - lower) * (perturb * jitter) between the
 *   mid points 0.5 (z[s-1] + z[s]) (csrc/ray_dev.h, shared with mvsnerf_raygen_fwd and mvsnerf_ray_points_fwd); pts = fma(d, z, o) and the NDC coordinates
 *   exactly as mvsnerf_ray_points_fwd forms them (one device function).
 * One thread per ray (gather) / per sample (march); no LDS, no atomics; two runs give the same bytes.
 * MVSNERF_EINVAL: a NULL required pointer (idx with B > 0; jitter with perturb > 0; depth without depth_bank; a reference-camera pointer, W_ref or
 *   H_ref < 2, or pad < 0 with ndc), a pointer misaligned for its element type (idx 8 bytes, images and every float array 4), M, H, W or S < 1, B < 0,
 *   a negative or NaN perturb; MVSNERF_EUNSUPPORTED: M H W > INT64_MAX / 8, B (B S for the march) > 2^38.  All before the launch; B == 0 launches nothing. */
int mvsnerf_scene_rays_gather_fwd(const unsigned char* images_rgba, const float* c2w, const float* K, const float* near_far, const float* depth_bank,
                                  int M, int H, int W, const int64_t* idx, int64_t B, float* rays, float* rgb, float* depth, unsigned char* mask,
                                  void* stream);
int mvsnerf_scene_rays_march_fwd(const unsigned char* images_rgba, const float* c2w, const float* K, const float* near_far, int M, int H, int W,
                                 const int64_t* idx, int64_t B, const float* t, int S, const float* jitter, float perturb, int lindisp,
                                 const float* w2c_ref, const float* K_ref, const float* near_far_ref, int W_ref, int H_ref, int pad,
                                 float* rays, float* rgb, float* z, float* pts, float* ndc, void* stream);
/* source_images: the source views of read_source_views (data/dtu_ft.py:72-119) from the bank: out [V][3][H][W] fp32 for ids [V] int64 (device).  Per
 *   channel c / 255 and a / 255 (IEEE divisions), rgb a + (1 - a) in three roundings (the colour of the training rays above, one device function), then
 *   T.Normalize's sub_(mean).div_(std): (x - mean[k]) / std[k], an IEEE subtraction and division.  mean, std: HOST float[3], read before the launch.  An id
 *   outside [0, M) gives zeros and reads nothing.  MVSNERF_EINVAL: a NULL pointer, V, M, H or W < 1; MVSNERF_EALIGN: images_rgba or out not 4-byte,
 *   ids not 8-byte aligned; MVSNERF_EUNSUPPORTED: H W > 2^31 - 1 or 3 V H W > 2^38. */
int mvsnerf_source_images_fwd(const unsigned char* images_rgba, const int64_t* ids, int V, int M, int H, int W, const float* mean, const float* std,
                              float* out, void* stream);
/* ---- Pillow's 8-bit resampler on the bank's images: Image.resize(size, LANCZOS | BILINEAR) of the reference's per-scene datasets (data/dtu_ft.py:108,
 *      data/blender.py:66, data/llff.py:241; data/dtu.py:160), byte for byte, without box= and reducing_gap= (csrc/resample.hip) ----
 * src [M][Hin][Win][4], dst [M][Hout][Wout][4] uint8.  The horizontal pass runs first, over all input rows and only if Win != Wout, into workspace when a
 *   vertical pass (only if Hin != Hout) follows; equal sizes give a copy.  (Pillow 12's Image.resize runs the vertical pass first for an image more than
 *   100 times as tall as wide whose height shrinks; this entry does not.)
 * Tables per axis, int32, built by the caller (mvsnerf_amd/ops.py _resample_tables; tests/resample_refs.py tables): win [n_out][2] = (xmin, n) and
 *   kk [n_out][ks], Pillow's precompute_coeffs and normalize_coeffs_8bpc (PRECISION_BITS 22).  A pass computes per channel
 *   clamp((2^21 + sum_{x < n} src[xmin + x] kk[x]) >> 22, 0, 255) in int32.  The tables of an axis whose size does not change are not read (NULL, 0).
 *   Every thread checks its own window before any load: xmin >= 0, 0 <= n <= ks, xmin + n <= n_in; a bad window gives an all-zero pixel and reads nothing
 *   (when a vertical pass follows, it resamples the zero pixels a bad horizontal window left in the workspace: zeros again, alpha 255 in alpha_mode 0).
 * alpha_mode 0 (an RGB image): three channels are resampled and dst's alpha byte is written as 255 (also by the copy).
 * alpha_mode 1 (an image with alpha): Pillow resamples premultiplied bytes (RGBA -> RGBa -> RGBA): the first pass loads c' = ((t >> 8) + t) >> 8 with
 *   t = c a + 128, all four channels are resampled, and the last pass stores c' when the resampled a is 0 or 255, else min(255 c' / a, 255).  The copy copies.
 * workspace_bytes: M Hin Wout 4 when both passes run, else 0 (also for sizes the entry refuses).
 * MVSNERF_EINVAL: NULL src or dst, a size < 1, an alpha_mode other than 0 / 1, a NULL table or ks < 1 for an axis that changes, a NULL workspace when both
 *   passes run; MVSNERF_EALIGN: src, dst, workspace or a table not 4-byte aligned; MVSNERF_EUNSUPPORTED: Hin Win, Hin Wout or Hout Wout > 2^31 - 1, any of
 *   them times M > 2^38 (a pass is one 256-thread workgroup per 256 pixels), ks > 65535.  All before the first launch. */
size_t mvsnerf_resample_u8_workspace_bytes(int M, int Hin, int Win, int Hout, int Wout);
int mvsnerf_resample_u8_fwd(const unsigned char* src, int M, int Hin, int Win, unsigned char* dst, int Hout, int Wout, const int* xwin, const int* xkk,
                            int xks, const int* ywin, const int* ykk, int yks, int alpha_mode, void* workspace, void* stream);
/* ---- LPIPS-VGG, the third column of the reference's tables (renderer.ipynb: lpips.LPIPS(net='vgg') per held-out view): the VGG-16 trunk and the five
 *      1x1 heads on channel-last fp32 activations act[n][y][x][C] (csrc/lpips.hip).  Every entry is one layer, so each can be tested alone. ----
 * Supported (Cin, Cout): (3, 64) = conv1_1, and Cin, Cout in {64, 128, 256, 512}; C of the pool and the head in {64, 128, 256, 512}.
 * conv_packed_floats: Cin Cout 9 + Cout (weights in MFMA fragment order, then the bias); 0 for an unsupported pair.  Runs without a GPU.
 * conv_pack: w [Cout][Cin][3][3] and b [Cout] (torch's layout, on the device) -> packed.
 * conv_fwd: out[n][y][x][co] = relu(b[co] + sum_{ci,ky,kx} w[co][ci][ky][kx] in[n][y+ky-1][x+kx-1][ci]), taps outside the image contributing 0; exact fp32
 *   (v_mfma_f32_32x32x2_f32; one fmaf chain per output in a fixed order, so image n of a batch has the bits of the image alone).  For Cin == 3 the input
 *   is an image in [0,1] and every tap INSIDE the image is first scaled as LPIPS's scaling layer does: ((2 x - 1) - shift_c) / scale_c with
 *   shift = (-.030, -.088, -.188), scale = (.458, .448, .450); padding stays 0.  out [N][H][W][Cout] is fully written.
 * pool_fwd: max over 2x2 windows at stride 2, out [N][H/2][W/2][C] (floor: an odd last row or column is dropped; a NaN in a window gives NaN).
 * head_fwd: f0, f1 [K][h][w][C], lin [C].  Per pixel n0 = sqrt(sum_c f0_c^2) + 1e-10 (n1 likewise), d = sum_c lin_c (f0_c / n0 - f1_c / n1)^2 in double;
 *   the layer value of frame k is the mean of d over its h w pixels: per-workgroup partial sums in workspace, then one summing launch in a fixed order (no
 *   atomics; an all-zero feature vector gives 0, never NaN).  layer_out[k] (may be NULL) receives the value; total[k] (may be NULL, not both) receives it
 *   (accumulate == 0) or has it added (accumulate != 0), so five calls on one stream leave the metric in total.  workspace: head_workspace_bytes(K, h, w, C)
 *   bytes, 8-byte aligned (0 for arguments the entry refuses; runs without a GPU).
 * MVSNERF_EINVAL: a NULL pointer or a size < 1; MVSNERF_EUNSUPPORTED: another channel count, H or W < 2 for the pool, H W max(Cin, Cout) >= 2^31 or a grid of
 *   2^31 workgroups; MVSNERF_EALIGN: activations / packed weights not 16-byte (the conv1_1 image, the head's maps and lin: 4-byte; doubles: 8-byte) aligned.
 *   All before the first launch. */
size_t mvsnerf_lpips_conv_packed_floats(int Cin, int Cout);
int mvsnerf_lpips_conv_pack(const float* w, const float* b, int Cin, int Cout, float* packed, void* stream);
int mvsnerf_lpips_conv_fwd(const float* in, const float* packed, int N, int H, int W, int Cin, int Cout, float* out, void* stream);
int mvsnerf_lpips_pool_fwd(const float* in, int N, int H, int W, int C, float* out, void* stream);
size_t mvsnerf_lpips_head_workspace_bytes(int K, int h, int w, int C);
int mvsnerf_lpips_head_fwd(const float* f0, const float* f1, const float* lin, int K, int h, int w, int C, double* layer_out, double* total,
                           int accumulate, void* workspace, void* stream);
/* ---- the depth maps of a scene's views -> a coloured point cloud: the cross-view geometric-consistency filter of the MVSNet line of work and the stable
 *      compaction of the kept pixels (csrc/depth_fusion.hip).  No counterpart in the reference. ----
 * Conventions are the bank's (scene_rays above): pixel centres at integer coordinates, camera direction ((x - cx) / fx, (y - cy) / fy, 1), a depth z the
 *   parameter of o + d z with that unnormalised d (camera-space z); c2w, w2c [M][3][4] (w2c: the inverse of c2w, formed by the caller), K [M][3][3].
 * depth_consistency: depth [M][H][W] fp32, valid [M][H][W] uint8 or NULL, images_rgba [M][H][W][4] uint8 or NULL (only its alpha bytes are read),
 *   src_ids [M][n_src] int32 (device).  A depth is INVALID when it is not finite, <= 0, valid is given and 0 there, or images_rgba is given and its alpha
 *   is 0 there: such a pixel gets seen = 0, fused = 0, mask = 0.  For source j of view r, s = src_ids[r][j] (an id outside [0, M), -1 being the padding,
 *   or equal to r is skipped and reads nothing): P = o_r + d_r z; q = R_s P + t_s, q.z > 0; (u, v) = (fx_s q.x / q.z + cx_s, fy_s q.y / q.z + cy_s) inside
 *   [0, W-1] x [0, H-1]; the bilinear cell x0 = min(floor u, W-2), y0 = min(floor v, H-2) with weights u - x0, v - y0, all four taps of depth[s] valid;
 *   (u, v, z_s) lifted through view s and projected into view r gives (x', y', z').  The pair is consistent iff z' > 0, sqrt((x'-x)^2 + (y'-y)^2) < pix_thr
 *   and |z' - z| / z < rel_thr.  seen [M][H][W] uint32: bit j; fused [M][H][W] fp32 = (z + sum of z' over consistent sources) / (1 + popcount(seen));
 *   mask [M][H][W] uint8 = popcount(seen) >= min_views.  fp32 throughout (products may contract into fmas).  One thread per reference pixel; no atomics;
 *   every output element is written.
 * point_cloud: the pixels with mask != 0 in flat-ray-index order (view-major, then row-major: torch.nonzero's order), count -> scan -> write, no atomics, two
 *   runs give the same bytes.  Row j < min(count, capacity): points [.][3] fp32 = o_r + d_r fused, colors [.][3] uint8 = the bank's RGB bytes, n_views [.]
 *   uint8 = popcount(seen), index [.] int64 = the flat ray index.  *count (device int64) always receives the true total; rows >= capacity are neither read
 *   nor written, so a caller that guessed too small runs again.  capacity == 0 runs the count alone (every pointer but mask, count and workspace may be NULL).
 *   workspace: point_cloud_workspace_bytes(M H W) bytes, 4-byte aligned (0 for n_pixels < 1 or >= 2^31; runs without a GPU).
 * MVSNERF_EINVAL: a NULL required pointer, M, H or W < 1, n_src outside 1..32, min_views < 0, a threshold that is not finite or <= 0, capacity < 0;
 *   MVSNERF_EUNSUPPORTED: H < 2 or W < 2 (no bilinear cell), M H W >= 2^31; MVSNERF_EALIGN: a float / int32 / uint32 / RGBA array not 4-byte, index or count
 *   not 8-byte aligned.  All before the first launch. */
int mvsnerf_depth_consistency_fwd(const float* depth, const unsigned char* valid, const unsigned char* images_rgba, const float* c2w, const float* w2c,
                                  const float* K, const int* src_ids, int M, int H, int W, int n_src, float pix_thr, float rel_thr, int min_views,
                                  unsigned* seen, float* fused, unsigned char* mask, void* stream);
size_t mvsnerf_point_cloud_workspace_bytes(int64_t n_pixels);
int mvsnerf_point_cloud_fwd(const unsigned char* images_rgba, const float* c2w, const float* K, int M, int H, int W, const float* fused,
                            const unsigned* seen, const unsigned char* mask, int64_t capacity, float* points, unsigned char* colors,
                            unsigned char* n_views, int64_t* index, int64_t* count, void* workspace, void* stream);
/* ---- a (D,H,W) scalar field (a scene's node density) -> a triangle mesh of its level set: marching tetrahedra over the Kuhn split of every grid cell
 *      (csrc/mesh.hip, DESIGN.md 4n, where the definition is written out).  No counterpart in the reference. ----
 * field [D][H][W] fp32 (device): node (i,j,k) = field[k][j][i], flat index n = (k H + j) W + i, inside iff field >= level (a NaN is outside).  A node owns
 *   the edges to the node at +(dx,dy,dz), e = 0..6: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1).  An edge with exactly one end inside carries a
 *   vertex at t = (level - s0) / (s1 - s0) from its owner (0.5 when an end is not finite); vertices are ordered by the key n * 8 + e.  Row j of a vertex:
 *   ndc [.][3] = ((i,j,k) + t (dx,dy,dz)) / (W-1, H-1, D-1); vertices [.][3] = box[0..2] + ndc * (box[3..5] - box[0..2]) (box: 6 HOST floats, lo then hi), or
 *   P0 + t (P1 - P0) (positions [D][H][W][3], device: the nodes' positions), or the grid coordinates themselves (neither); vertex_edge [.] int64 = the key.
 *   fp32, every operation rounded on its own, IEEE division.  faces [.][3] int32 vertex numbers: per cell 6 tetrahedra (one per permutation of the axes,
 *   lexicographic), ordered by cell, tetrahedron, triangle; counter-clockwise seen from the side where the field is below the level.
 * count (device, int64 [2]) always receives the true numbers of vertices and faces.  Rows >= cap_vertices / cap_faces are not written; both capacities 0
 *   runs the count alone (the output pointers of a capacity of 0 may be NULL).  classify -> scan -> vertices -> faces, no atomics, two runs give the same bytes.
 * workspace: mesh_workspace_bytes(D, H, W) bytes (5 per node + 16 per workgroup of 256 nodes), 4-byte aligned; 0 for a shape the entry refuses (runs
 *   without a GPU).
 * mesh_dirs: dirs [n][3] = vertices [n][3] - origin (3 device floats).  mesh_rgb_u8: rgb [n][3] uint8 = trunc(clamp(c, 0, 1) * 255) of the first three of
 *   the four floats of row rgba [n][4] (NaN -> 0: the rule of frame_u8).  n == 0 launches nothing.
 * MVSNERF_EINVAL: a NULL pointer that is needed, a capacity or n < 0; MVSNERF_EUNSUPPORTED: D, H or W < 2, D H W > 2^27, a level that is not finite, both
 *   positions and box, n >= 2^31; MVSNERF_EALIGN: a float / int32 array or the workspace not 4-byte, vertex_edge or count not 8-byte, rgba not 16-byte
 *   aligned.  All before the first launch. */
size_t mvsnerf_mesh_workspace_bytes(int D, int H, int W);
int mvsnerf_mesh_extract_fwd(const float* field, int D, int H, int W, float level, const float* positions, const float* box, int64_t cap_vertices,
                             int64_t cap_faces, float* vertices, float* ndc, int64_t* vertex_edge, int* faces, int64_t* count, void* workspace,
                             void* stream);
int mvsnerf_mesh_dirs_fwd(const float* vertices, const float* origin, int64_t n, float* dirs, void* stream);
int mvsnerf_mesh_rgb_u8_fwd(const float* rgba, int64_t n, unsigned char* rgb, void* stream);
/* mesh_extract_masked: mesh_extract with a node mask, valid [D][H][W] uint8 (device) or NULL, any non-zero byte = valid.  An owned edge carries a vertex only
 *   if both its ends are valid and a tetrahedron emits faces only if its four corners are valid; the field is still read at invalid nodes.  Equivalently: the
 *   unmasked extraction with every vertex whose edge has an invalid end and every face that uses such a vertex dropped, and the rest renumbered (the triangles
 *   of every tetrahedron case touch all four corners).  Vertices that no surviving face uses are kept; the surface is closed only away from invalid nodes.
 *   mesh_extract is this entry with valid = NULL.  Codes, workspace and capacities as mesh_extract. */
int mvsnerf_mesh_extract_masked_fwd(const float* field, const unsigned char* valid, int D, int H, int W, float level, const float* positions,
                                    const float* box, int64_t cap_vertices, int64_t cap_faces, float* vertices, float* ndc, int64_t* vertex_edge, int* faces,
                                    int64_t* count, void* workspace, void* stream);
/* ---- the depth maps of a scene's views -> a truncated signed distance volume (Curless-Levoy / KinectFusion) on a (D,H,W) grid of nodes over a world box, and
 *      a mesh's vertex colours from it (csrc/tsdf.hip, DESIGN.md 4o, where the definition is written out).  No counterpart in the reference. ----
 * Conventions: the bank's (depth_consistency above: pixel centres at integer coordinates, depth = camera-space z, w2c [M][3][4], K [M][3][3]) and the mesher's
 *   (node (i,j,k) = [k][j][i], n = (k H + j) W + i).  box: 6 HOST floats, lo then hi; node position X = lo + ((i,j,k) / (W-1, H-1, D-1)) * (hi - lo), the
 *   operations of mesh_extract's box mapping.
 * tsdf_integrate: for a node and each view m of view_ids [n_views] (device int32; NULL: the views 0..M-1; an id outside [0, M) is skipped), in the list's
 *   order, each step only if the one before held:  1. q = ((w0 X + w1 Y) + w2 Z) + w3 per row of w2c_m, q.z > z_min;  2. u = fx q.x / q.z + cx,
 *   v = fy q.y / q.z + cy, 0 <= u + 0.5 < W_img, 0 <= v + 0.5 < H_img, the NEAREST pixel x = floor(u + 0.5), y = floor(v + 0.5);  3. d = depth[m][y][x] is
 *   finite, > 0, valid (when given) != 0 there and, when alpha != 0, the image's alpha byte != 0;  4. sdf = d - q.z >= -trunc;  5. tsum += min(sdf / trunc, 1),
 *   wsum += 1;  6. if sdf <= trunc: csum[0:3] += images_rgba[m][y][x][0:3], cw += 1.  Outputs: tsdf [D][H][W] fp32 = tsum / wsum (+1 where wsum == 0);
 *   weight [D][H][W] int32 = wsum; colors [D][H][W][4] uint8 = ((2 csum + cw) / (2 cw) in integers, 255), four zero bytes where cw == 0, one 32-bit store.
 *   fp32, every operation rounded on its own, IEEE division; one thread per node, no atomics, two runs give the same bytes; pixel indices are 64-bit.
 * tsdf_vertex_colors: row r < min(count[0], rows) (count: device int64) of colors [rows][3] uint8 from the ends n = vertex_edge[r] >> 3 and its neighbour
 *   along owned edge vertex_edge[r] & 7: t = (0 - f0) / (f1 - f0) on f = -tsdf (0.5 when an end is not finite), byte = clamp(floor(c0 + t (c1 - c0) + 0.5),
 *   0, 255) per channel of node_colors [D][H][W][4]; only one end with alpha 255: that end's bytes; neither, or a key outside the grid: 0.  Rows past the
 *   count are not written.  rows == 0 launches nothing.
 * MVSNERF_EINVAL: a NULL pointer that is needed (valid and view_ids may be NULL), rows < 0; MVSNERF_EUNSUPPORTED: D, H or W < 2, D H W > 2^27, trunc not
 *   finite or <= 0, z_min not finite or < 0, a box that is not finite, M < 1, M or n_views >= 2^22, n_views < 1 with view_ids, an image smaller than 1 x 1
 *   or larger than 2^24 in a dimension, rows >= 2^31; MVSNERF_EALIGN: a float / int32 / RGBA array not 4-byte, vertex_edge or count not 8-byte aligned.
 *   All before the first launch. */
int mvsnerf_tsdf_integrate_fwd(const float* depth, const unsigned char* valid, const unsigned char* images_rgba, int alpha, const float* w2c, const float* K,
                               const int* view_ids, int n_views, int M, int H_img, int W_img, const float* box, int D, int H, int W, float trunc,
                               float z_min, float* tsdf, int* weight, unsigned char* colors, void* stream);
int mvsnerf_tsdf_vertex_colors_fwd(const float* tsdf, const unsigned char* node_colors, int D, int H, int W, const int64_t* vertex_edge,
                                   const int64_t* count, int64_t rows, unsigned char* colors, void* stream);
/* ---- geometric scores of clouds and meshes: a uniform grid over a target cloud, the EXACT nearest neighbour within a radius, the DTU / Tanks-and-Temples
 *      reductions, and points on a mesh (csrc/cloud_metrics.hip, DESIGN.md 4p, where the definitions are written out).  No counterpart in the reference. ----
 * grid_bounds: bounds [6] (device) = min xyz, max xyz over the rows of points [n][3] whose three coordinates are finite; +inf, -inf when there is none
 *   (n == 0 included).  workspace: grid_bounds_workspace_bytes(n) bytes, 4-byte aligned (0: n < 0 or n >= 2^31; runs without a GPU).
 * grid_build: the grid of dx x dy x dz cells of edge `cell` from lo (3 HOST floats).  The cell of a point is floorf((p - lo) * (1.0f / cell)) per axis, clamped
 *   to [0, dim - 1] (a point outside the box lands in a border cell), flat cell (cz dy + cy) dx + cx.  Rows with a non-finite coordinate are left out.
 *   cell_start [dx dy dz + 1] int32 = the exclusive prefix of the cells' counts (the last entry: the number of points kept); records [n][4] fp32 = x, y, z
 *   and the bits of the ORIGINAL row index, grouped by cell, 16-byte aligned; only the first cell_start[cells] records are written.  Integer atomics count
 *   and place the points: the order of the records inside a cell may differ between two runs, cell_start does not.  n == 0 writes zeros to cell_start.
 *   workspace: grid_build_workspace_bytes(n, dx, dy, dz) bytes, 4-byte aligned (0 for arguments the entry refuses).
 * grid_nearest: per row of query [n_query][3] the minimum, in lexicographic order, of (d2, original index) over the grid's points with
 *   d2 = (dx dx + dy dy) + dz dz <= max_dist max_dist (both fp32, every operation rounded on its own): dist [.] = sqrtf(d2), index [.] int32; +inf and -1
 *   when there is no such point or a coordinate of the query is not finite.  The same bits for every (lo, cell, dims) the grid was built with, and for a
 *   query inside or outside the box.  lo, cell, dims: those of grid_build.
 * cloud_metrics: out [10] doubles (device) = {the sum of the finite entries of dist [n], their number, the number of entries with dist < taus[k] (fp32
 *   compare), k < n_tau <= 8, zeros behind}; taus: HOST floats.  Two launches, fixed summation order, no atomics.  workspace:
 *   cloud_metrics_workspace_bytes(n) bytes, 8-byte aligned like out.
 * mesh_sample: points on the faces [n_faces][3] (int32 rows of vertices [n_vertices][3]).  Per face n = max(1, ceilf(L / spacing)), L its longest edge, an
 *   edge sqrtf((dx dx + dy dy) + dz dz); the face emits the centroids of the n n sub-triangles of its barycentric lattice: rows j = 0..n-1, in a row
 *   i = 0..n-1-j the upward triangle, weights (wb, wc) = (3i+1, 3j+1), then (while i < n-1-j) the downward one, (3i+2, 3j+2); point = ((wa A + wb B) +
 *   wc C) / (3n), wa = 3n - wb - wc.  A face with a non-finite vertex, a vertex number outside [0, n_vertices) or n > 1024 emits nothing.  mesh_count: NULL, or
 *   the device {vertices, faces} counts of a mesh extracted with a capacity (rows past them are not read).  points [capacity][3] fp32, face [capacity] int32,
 *   ordered by face and then by lattice order; rows >= min(count[0], capacity) are not written.  count (device, int64 [2]) = {the true number of points, the
 *   largest n of any face: above 1024 means faces were refused}; capacity == 0 runs the count alone.  No atomics: two runs give the same bytes.
 *   workspace: mesh_sample_workspace_bytes(n_faces) bytes, 8-byte aligned.
 * MVSNERF_EINVAL: a NULL pointer that is needed, a negative count or capacity; MVSNERF_EUNSUPPORTED: a count or capacity >= 2^31, a dimension < 1 or more than
 *   2^24 cells, lo / cell / max_dist / spacing not finite or cell / max_dist / spacing <= 0 (or 1 / cell, max_dist^2 not finite), n_tau > 8; MVSNERF_EALIGN: a
 *   float / int32 array not 4-byte, records not 16-byte, doubles / int64 / the 8-byte workspaces not 8-byte aligned.  All before the first launch. */
size_t mvsnerf_grid_bounds_workspace_bytes(int64_t n);
int mvsnerf_grid_bounds_fwd(const float* points, int64_t n, float* bounds, void* workspace, void* stream);
size_t mvsnerf_grid_build_workspace_bytes(int64_t n, int dx, int dy, int dz);
int mvsnerf_grid_build_fwd(const float* points, int64_t n, const float* lo, float cell, int dx, int dy, int dz, int* cell_start, float* records,
                           void* workspace, void* stream);
int mvsnerf_grid_nearest_fwd(const float* lo, float cell, int dx, int dy, int dz, const int* cell_start, const float* records, const float* query,
                             int64_t n_query, float max_dist, float* dist, int* index, void* stream);
size_t mvsnerf_cloud_metrics_workspace_bytes(int64_t n);
int mvsnerf_cloud_metrics_fwd(const float* dist, int64_t n, const float* taus, int n_tau, double* out, void* workspace, void* stream);
size_t mvsnerf_mesh_sample_workspace_bytes(int64_t n_faces);
int mvsnerf_mesh_sample_fwd(const float* vertices, int64_t n_vertices, const int* faces, int64_t n_faces, const int64_t* mesh_count, float spacing,
                            int64_t capacity, float* points, int* face, int64_t* count, void* workspace, void* stream);
/* ---- a triangle mesh -> depth, face and colour maps in pinhole cameras (a z-buffer rasteriser), the views a face owns pixels in, and a mesh cut down to a
 *      subset of its faces (csrc/raster.hip, DESIGN.md 4r, where the definition is written out too).  No counterpart in the reference. ----
 * Conventions: tsdf_integrate's (w2c [M][3][4], K [M][3][3], pixel centres at integer coordinates, depth = camera-space z, fp32, every operation rounded on
 *   its own, IEEE division).  Sub-pixel grid SUB = 256.  mesh_count: NULL, or the device {vertices, faces} counts of a mesh extracted with a capacity: rows
 *   past min(count, rows) are never read (mesh_sample's convention).  view_ids [n_views] (device int32; NULL: the views 0..M-1): output slot a shows view
 *   view_ids[a]; an id outside [0, M) is skipped (tsdf_integrate's rule) and its slot is empty.
 * mesh_raster, per view m and vertex i:  q = ((w0 X + w1 Y) + w2 Z) + w3 per row of w2c_m;  u = K0 q.x / q.z + K2, v = K4 q.y / q.z + K5;
 *   X = floor(u 256 + 0.5), Y = floor(v 256 + 0.5) as integers;  iz = 1 / q.z.  The vertex is usable iff q.z > z_min, u and v are finite and
 *   |X|, |Y| <= 2^23 (every edge product then fits int64).
 *   Per face f = (a, b, c): dropped whole (no clipping) if a vertex number lies outside [0, n_vertices), a vertex is unusable, A == 0 with
 *   A = (x1-x0)(y2-y0) - (y1-y0)(x2-x0) in int64, or it is culled: cull = 0 keeps both signs, +1 drops A > 0, -1 drops A < 0 (the front faces of the
 *   library's own meshes seen from outside have A < 0: cull = +1 is back-face culling for them).  If A < 0, b and c are swapped so that A > 0.  Edge functions
 *   e_i(px,py) = (xb-xa)(py-ya) - (yb-ya)(px-xa) in int64 at px = 256 x, py = 256 y: e0 on (b,c), e1 on (c,a), e2 on (a,b).  Pixel (x,y) of the snapped
 *   bounding box clipped to the image is covered iff for each edge e > 0, or e == 0 and the edge is top-left (dy < 0, or dy == 0 and dx > 0): shared edges
 *   are watertight and no pixel is hit twice.  A covered pixel:  b1 = (float)e1 / (float)A, b2 = (float)e2 / (float)A, b0 = (1 - b1) - b2;  t_k = b_k iz_k;
 *   invz = (t0 + t1) + t2;  z = 1 / invz; the fragment counts iff z is finite and z > z_min.
 *   Depth test: the smallest z wins, the lowest face number among equal z bits; nothing depends on arrival order (one 64-bit word per pixel,
 *   float_bits(z) << 32 | face, an unsigned atomic min), so two runs give the same bytes.
 *   Outputs per slot: depth [.][H][W] fp32 (0 where nothing was hit: the bank's hole), face [.][H][W] int32 (-1 for nothing), and, iff colors [n_vertices][3]
 *   uint8 is given, out_colors [.][H][W][3] uint8: byte = clamp(floor(((t0 c_a + t1 c_b) + t2 c_c) z + 0.5), 0, 255) per channel (perspective-correct); a
 *   hole takes background = R | G << 8 | B << 16.
 *   workspace: mesh_raster_workspace_bytes(n_faces, n_views, H, W) bytes (n_views: the number of output slots), 8-byte aligned; 0 for shapes the entry refuses.
 * mesh_face_views: face [n_maps][H][W] int32 (mesh_raster's face maps; map a shows view view_ids[a], or view a with view_ids NULL, then n_maps == M) ->
 *   seen [n_faces][ceil(M / 32)] int32 with bit m & 31 of word m >> 5 set iff face f owns a pixel of view m, and n [n_faces] int32 = the number of such views.
 *   Entries outside [0, min(count, n_faces)) are ignored.  Integer atomic OR: order-free.
 * mesh_filter: the faces with keep [n_faces] != 0 (uint8) below the mesh's count whose vertex numbers lie inside the mesh, in order, and the vertices they
 *   use, in order, renumbered.  vertices / ndc / vertex_edge / colors rows are carried over (ndc, vertex_edge, colors and their outputs may be NULL);
 *   vertex_index / face_index (int64) hold the original numbers.  count (device, int64 [2]) always receives the true numbers of vertices and faces; rows
 *   >= cap_vertices / cap_faces are not written and both capacities 0 runs the count alone (mesh_extract's convention).  mark -> count -> scan -> write, no
 *   atomics, stable.  workspace: mesh_filter_workspace_bytes(n_vertices, n_faces) bytes, 4-byte aligned.
 * MVSNERF_EINVAL: a NULL pointer that is needed, colors without out_colors or the reverse, a negative count or capacity, M, H, W or n_maps < 1, n_views < 1
 *   with view_ids, n_maps != M without, a cull outside {-1, 0, 1}; MVSNERF_EUNSUPPORTED: a count or capacity >= 2^31, more than 65535 output slots, M >= 2^22,
 *   an image larger than 2^15 in a dimension, more than 2^22 workgroups of 256 (face, view) items, z_min not finite or < 0; MVSNERF_EALIGN: a float / int32
 *   array not 4-byte, an int64 array or the raster workspace not 8-byte aligned.  All before the first launch. */
size_t mvsnerf_mesh_raster_workspace_bytes(int64_t n_faces, int n_views, int H, int W);
int mvsnerf_mesh_raster_fwd(const float* vertices, int64_t n_vertices, const int* faces, int64_t n_faces, const unsigned char* colors,
                            const int64_t* mesh_count, const float* w2c, const float* K, const int* view_ids, int n_views, int M, int H, int W, int cull,
                            float z_min, unsigned background, float* depth, int* face, unsigned char* out_colors, void* workspace, void* stream);
int mvsnerf_mesh_face_views_fwd(const int* face, int n_maps, int H, int W, const int* view_ids, int M, int64_t n_faces, const int64_t* mesh_count, int* seen,
                                int* n, void* stream);
size_t mvsnerf_mesh_filter_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int mvsnerf_mesh_filter_fwd(const float* vertices, const float* ndc, const int64_t* vertex_edge, const unsigned char* colors, int64_t n_vertices,
                            const int* faces, int64_t n_faces, const int64_t* mesh_count, const unsigned char* keep, int64_t cap_vertices, int64_t cap_faces,
                            float* out_vertices, float* out_ndc, int64_t* out_vertex_edge, unsigned char* out_colors, int64_t* vertex_index, int* out_faces,
                            int64_t* face_index, int64_t* count, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
