// The host launchers that one convolution, InPlaceABN, weight-gradient or plane-sweep file defines and another calls; internal, not exported.
// Every file that defines or calls one of them includes this header, so the compiler checks both sides against one prototype; default
// arguments are stated here and nowhere else.  MVSNERF_EUNSUPPORTED = no kernel for the shape (the caller takes its other kernel).
#pragma once
#include "act.h"

// planesweep.hip: the forward sweep behind every mvsnerf_planesweep_costvar_*_fwd (blocked: 0 channel-last, 1 blocks of four, 2 bf16, 3 two fp16
// pieces); guard != NULL: the 16-bit store reports through guard[0]; run_if != NULL: the launch is predicated on that word
int mvs_planesweep_launch(const float* feats_cl, const float* imgs_cl, const float* proj, const float* depth,
                          int V, int C, int H, int W, int D, int pad, float* cost, int CP, float* masks,
                          int with_img, int blocked, void* stream, int* guard = nullptr, const int* run_if = nullptr);

// conv_mfma.hip: conv0-shaped layers (8 output channels, stride 1) of a channel-last input on v_mfma_f32_4x4x1
int mvs_conv3d_c8_mfma(const ActSrc& a, const ActSrc& b, int Cin, int cin_real, int cin_ld, int D, int H, int W, const float* wpacked, float* out,
                       hipStream_t st);
// conv_mfma.hip: the same layer on a cost volume in channel blocks of four; stats != NULL: InPlaceABN partial sums, one slot per workgroup
int mvs_conv3d_c8_mfma4(const float* x4, int Cin, int cin_real, int D, int H, int W, const float* wq, float* out, float* stats, hipStream_t st,
                        const int* run_if = nullptr);
// conv_mfma.hip: workgroups (= statistics slots) of mvs_conv3d_c8_mfma4
int mvs_conv3d_c8_mfma4_tiles(int D, int H, int W);
// conv_mfma.hip: w[tap][ci][co] -> [ci/4][tap][co][4]
int mvs_conv_w4_repack(const float* wpacked, float* wq, int Cin, hipStream_t st);
// conv_mfma.hip: the layers with 16 / 32 / 64 output channels on v_mfma_f32_32x32x2_f32 (conv1: 16x16x4); run_if: conv1's kernel only
int mvs_conv3d_mfma32(const ActSrc& a, const ActSrc& b, int Cin, int cin_ld, int D, int H, int W, const float* w32, int Cout, int stride,
                      float* out, float* stats, hipStream_t st, const int* run_if = nullptr);
// conv_mfma.hip: M-tiles (= statistics slots) of mvs_conv3d_mfma32
int mvs_conv3d_mfma32_tiles(int D, int H, int W, int stride);
// conv_mfma.hip: whether mvs_conv3d_mfma32 has a kernel for the shape
bool mvs_conv3d_mfma32_supported(int Cin, int Cout, int stride);
// conv_mfma.hip: w[tap][ci][co] -> [tap][ci/8][co][8]
int mvs_conv_w32_repack(const float* wpacked, float* w32, int Cin, int Cout, hipStream_t st);
// conv_mfma.hip: conv7 / conv9 / conv11 (transposed, stride 2) of a plain tensor on the 32x32x2 matrix instruction
int mvs_convT3d_mfma32(const float* x, int Cin, int D, int H, int W, const float* w32, int Cout, float* out, float* stats, hipStream_t st);
// conv_mfma.hip: rows of InPlaceABN partial sums mvs_convT3d_mfma32 leaves
int mvs_convT3d_mfma32_tiles(int Cin, int Cout, int D, int H, int W);
// conv_mfma.hip: conv11 (16 -> 8, transposed) of up to two lazily-activated sources on v_mfma_f32_4x4x1
int mvs_convT3d_c16to8_mfma4(const ActSrc& xa, const ActSrc& xb, int D, int H, int W, const float* wq, float* out, float* stats, hipStream_t st);
// conv_mfma.hip: workgroups (= statistics slots) of mvs_convT3d_c16to8_mfma4
int mvs_convT3d_c16to8_tiles(int D, int H, int W);
// conv_mfma.hip: conv0's weight gradient from the blocked cost volume; gw == NULL: the partials stay in workspace
int mvs_conv3d_c8_wgrad4(const float* x4, int Cin, int cin_real, int D, int H, int W, const float* g, float* gw, float* workspace, int cap_parts,
                         hipStream_t st);
// conv_mfma.hip: partial results mvs_conv3d_c8_wgrad4 leaves
int mvs_conv3d_c8_wgrad4_parts(int Cin, int D, int H, int W, int cap_parts);

// conv_f16x3.hip: conv0 on the two fp16 pieces of the cost volume; guard != NULL: reports a non-finite output through guard[0]
int mvs_conv0_f16x3_fwd(const void* x16, int Cin, int D, int H, int W, const void* packed, float* out, float* stats_part, int* guard, hipStream_t st);
// conv_f16x3_tiled.hip: conv1 / conv2 on fp16 pieces staged through LDS; guard != NULL: reports NaN partial sums through guard[0]
int mvs_conv3d_f16x3_tiled_fwd(const float* x, const float* scale, const float* shift, int Cin, int cin_ld, int D, int H, int W, const void* wq, int Cout,
                               int stride, float* out, float* stats_part, int* guard, hipStream_t st);

// wgrad_mfma.hip: partial results mvs_conv3d_wgrad_mfma4 leaves; 0: no matrix-core kernel for the shape
int mvs_conv3d_wgrad_mfma4_parts(int A, int B, int Do, int Ho, int Wo, int stride, int cap_parts);
// wgrad_mfma.hip: weight gradient of a 3-D layer with 16 / 32 / 64 `a` channels on the matrix cores, as partial results
int mvs_conv3d_wgrad_mfma4(const ActSrc& g1, const ActSrc& g2, int A, const ActSrc& x1, const ActSrc& x2, int B, int ldx, int Do, int Ho, int Wo,
                           int Di, int Hi, int Wi, int stride, float* partial, int cap_parts, hipStream_t st);
// wgrad_mfma.hip: partial results mvs_conv2d_wgrad_mfma4 leaves; 0: no matrix-core kernel for the shape
int mvs_conv2d_wgrad_mfma4_parts(int A, int B, int N, int Ho, int Wo, int ksize, int stride, int cap_parts);
// wgrad_mfma.hip: weight gradient of one of FeatureNet's k3 / k5 layers on the matrix cores, as partial results
int mvs_conv2d_wgrad_mfma4(const float* g, int A, const ActSrc& x1, int B, int ldx, int N, int Ho, int Wo, int Hi, int Wi, int ksize, int stride,
                           float* partial, int cap_parts, hipStream_t st);

// conv3d.hip: conv2 (16 -> 16, stride 1) on the LDS-tiled VALU kernel, mvsnerf_conv3d_tiled_tiles(D, H, W) workgroups; stats != NULL: InPlaceABN
// partial sums, one slot per workgroup; run_if != NULL: the launch is predicated on that word
int mvs_conv3d_tiled16(const ActSrc& a, int cin_ld, int D, int H, int W, const float* wpacked, float* out, float* stats, const int* run_if, hipStream_t st);
// abn.hip: stage 1 of the InPlaceABN statistics of x[n][C], C in {8, 16, 32, 64}, into part[2][C][slots]; run_if != NULL: predicated on that word
int mvs_abn_partial(const float* x, int64_t n, int C, int slots, float* part, const int* run_if, hipStream_t st);
