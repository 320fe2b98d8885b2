// Packed-weight layout of the netwidth-256 fp32 MLP kernel (mlp_wide.hip): shared by its pack kernel, its compute kernel and the host-side
// size query.  The formulation is the 128-wide kernel's (mlp_layout.h, header comment): every layer transposed on v_mfma_f32_32x32x2_f32, the
// weights the A operand, 32 points the B operand, and one layer's C/D registers the next layer's B operands through act_n(q, half) - the map
// extends unchanged to q < 128, i.e. n < 256.  What differs is the counts: 8 output blocks of 32 per 256-wide layer, 128 k-steps per 256-wide
// input, 4 blocks for views_linears.0 (259 -> 128).
//
// A segment is pack_segment's order: float index = ((t4 * nb + b) * 64 + lane) * 4 + j for k-step t = 4*t4 + j, output block b (rows
// b*32 + (lane & 31)) and lane half h = lane >> 5 (column kmap_col(kmap, t, h, F)); padding columns hold 0.  32 k-steps of 8 blocks (or 64 of 4)
// are therefore 16 384 contiguous floats = one 64 KB slab of the kernel's LDS double buffer.
#pragma once
#include <stddef.h>
#include "mlp_layout.h"

namespace mlpw {

using mlp::act_n;
using mlp::feat_steps;
using mlp::seg_floats;

constexpr int WIDTH = 256;      // netwidth (the constructor default of the reference's MVSNeRF, models.py:541; run_batch.py:34)
constexpr int NB = WIDTH / 32;  // output blocks of a 256-wide layer
constexpr int PE_DIM = mlp::PE_DIM;
constexpr int PE_STEPS = mlp::PE_STEPS;
constexpr int ACT_STEPS = WIDTH / 2;          // 128
constexpr int VIEW_NB = WIDTH / 2 / 32;       // 4 output blocks of views_linears.0
constexpr int VIEW_STEPS = ACT_STEPS + 4;     // 128 (feature) + 2 (dir xyz + pad) rounded up to a multiple of 4
constexpr int MIN_F = 4, MAX_F = mlp::MAX_F;
constexpr int SLAB_FLOATS = 16384;            // 64 KB = 32 k-steps x 8 blocks x 64 lanes (views: 64 x 4)

enum KMap { K_PE = 0, K_FEAT = 1, K_ACT = 2, K_VIEWS = 3 };

__host__ __device__ inline int kmap_col(int kmap, int t, int h, int F)
{
    switch (kmap) {
    case K_PE:   return mlp::kmap_col(mlp::K_PE, t, h, F);
    case K_FEAT: return mlp::kmap_col(mlp::K_FEAT, t, h, F);
    case K_ACT:  return t < ACT_STEPS ? act_n(t, h) : -1;
    case K_VIEWS:   // [feature(256) | dir(3)]
        if (t < ACT_STEPS) return act_n(t, h);
        if (t == ACT_STEPS) return WIDTH + h;
        if (t == ACT_STEPS + 1) return h ? -1 : WIDTH + 2;
        return -1;
    }
    return -1;
}

// Offsets (floats) of the weight segments, in the order the kernel streams them; l1 .. l4 are consecutive 128 x 8 segments from `l1`.
struct Layout {
    size_t biasw, l0, l1, l5a, l5b, feat, views, vec, total;
    int fsteps;
};
// vector block (fragment-ordered biases and the two small heads), floats from `vec`
constexpr int V_BIASG = 0;                  // [2][128] pts_bias bias
constexpr int V_L0 = 256;                   // V_L0 + 256*i : pts_linears.i bias, i = 0..5
constexpr int V_FEAT = 256 * 7;             // feature_linear bias
constexpr int V_VIEWS = 256 * 8;            // [2][64] views_linears.0 bias
constexpr int V_WA = V_VIEWS + 128;         // [2][128] alpha_linear weight
constexpr int V_BA = V_WA + 256;            // alpha bias (+3 pad)
constexpr int V_ADD = V_BA + 2;             // third float: 0.0f = h_i = relu(pts_linears.i(h) * bias) (v0), 1.0f = relu(.. + bias) (v2); the place V_ADD has in mlp_layout.h
constexpr int V_WR = V_BA + 4;              // [3][2][64] rgb_linear weight
constexpr int V_BR = V_WR + 384;            // rgb bias (3, +1 pad)
constexpr int V_TOTAL = V_BR + 4;           // 2824

__host__ __device__ inline Layout layout(int F)
{
    Layout L;
    L.fsteps = feat_steps(F);
    size_t o = 0;
    L.biasw = o; o += seg_floats(L.fsteps, NB);
    L.l0 = o;    o += seg_floats(PE_STEPS, NB);
    L.l1 = o;    o += 4 * seg_floats(ACT_STEPS, NB);
    L.l5a = o;   o += seg_floats(PE_STEPS, NB);
    L.l5b = o;   o += seg_floats(ACT_STEPS, NB);
    L.feat = o;  o += seg_floats(ACT_STEPS, NB);
    L.views = o; o += seg_floats(VIEW_STEPS, VIEW_NB);
    L.vec = o;   o += V_TOTAL;
    L.total = o;
    return L;
}

}  // namespace mlpw
