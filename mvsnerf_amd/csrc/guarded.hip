// The guarded 16-bit sequences of a no-grad scene encode (include/mvsnerf_hip.h "guarded 16-bit sequences"): an fp16x3 kernel that reports
// through guard[0], then the fp32 kernels of the same layer predicated on that word.  Host sequences only, apart from the one-thread
// kernel that counts a tripped guard and re-arms it; every kernel they enqueue lives in the file named for it.
#include "common.h"
#include "act.h"
#include "conv.h"
#include "march.h"

__global__ void guard_consume_kernel(int* guard)
{
    if (guard[0]) { guard[1] += 1; guard[0] = 0; }
}

int mvs_guard_consume(int* guard, hipStream_t st)
{
    guard_consume_kernel<<<1, 1, 0, st>>>(guard);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// ---- guarded scene-encode head: models.py:839-893 + conv0 of :756
extern "C" int mvsnerf_sweep_conv0_guarded_fwd(const mvsnerf_sweep_conv0_args* a, void* stream)
{
    if (!a || !a->guard || !a->cost16x2 || !a->cost32 || !a->w_f16x3 || !a->w_c8 || !a->out || !a->imgs_cl) return MVSNERF_EINVAL;
    if (a->Cin != 3 * a->V + 32 || a->CP != ((a->Cin + 3) & ~3)) return MVSNERF_EINVAL;
    if (!mvs_aligned16(a->cost32) || !mvs_aligned16(a->out) || !mvs_aligned16(a->w_c8)) return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int Hp = a->H + 2 * a->pad, Wp = a->W + 2 * a->pad;
    int rc;
    // 1. the fp16 pair; both report through guard[0]
    if ((rc = mvs_planesweep_launch(a->feats_cl, a->imgs_cl, a->proj, a->depth, a->V, 32, a->H, a->W, a->D, a->pad, reinterpret_cast<float*>(a->cost16x2), a->CP,
                                a->masks, 1, 3, stream, a->guard, nullptr))) return rc;
    if ((rc = mvs_conv0_f16x3_fwd(a->cost16x2, a->Cin, a->D, Hp, Wp, a->w_f16x3, a->out, a->stats_part, a->guard, st))) return rc;
    // 2. the fp32 pair, predicated on guard[0]: same masks, same output, the statistics in the fp16 kernel's slots
    if ((rc = mvs_planesweep_launch(a->feats_cl, a->imgs_cl, a->proj, a->depth, a->V, 32, a->H, a->W, a->D, a->pad, a->cost32, a->CP,
                                a->masks, 1, 1, stream, nullptr, a->guard))) return rc;
    if ((rc = mvs_conv3d_c8_mfma4(a->cost32, a->CP, a->Cin, a->D, Hp, Wp, a->w_c8, a->out, nullptr, st, a->guard))) return rc;
    if (a->stats_part) {
        const int slots = ((Wp + 15) / 16) * ((Hp + 7) / 8) * ((a->D + 3) / 4);           // mvsnerf_conv0_bf16_tiles(D, Hp, Wp)
        if ((rc = mvs_abn_partial(a->out, (int64_t)a->D * Hp * Wp, 8, slots, a->stats_part, a->guard, st))) return rc;
    }
    // 3. count the event, re-arm
    return mvs_guard_consume(a->guard, st);
}

// conv1 / conv2 of a no-grad encode as a guarded sequence (include/mvsnerf_hip.h): the fp16x3 LDS-tiled kernel (conv_f16x3_tiled.hip) reporting through guard[0],
// then the layer's fp32 kernel and a statistics pass over its output, both predicated on that word (they cost a launch when it is clear, recompute the
// layer - the same out, the same stats_part slots - when it is set).  consume != 0: count the event in guard[1] and re-arm guard[0] (the LAST guarded
// layer of the encode passes 1; earlier ones may pass 0: a set guard then also makes the later layers take their fp32 kernels, which is harmless).
extern "C" int mvsnerf_conv3d_f16x3_guarded_fwd(const float* x, const float* scale, const float* shift, int Cin, int cin_ld, int D, int H, int W,
                                                const void* w_f16x3, const float* w_f32, int Cout, int stride, float* out, float* stats_part,
                                                int* guard, int consume, void* stream)
{
    if (!act_ok(x, scale, shift) || !w_f16x3 || !w_f32 || !out || !guard || D < 1 || H < 1 || W < 1) return MVSNERF_EINVAL;
    if (Cout != 16 || !((Cin == 8 && stride == 2) || (Cin == 16 && stride == 1))) return MVSNERF_EUNSUPPORTED;
    if ((cin_ld & 3) || cin_ld < Cin || !mvs_aligned16(out)) return MVSNERF_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    // 1. fp16x3; the guard is set from the (NaN) partial sums, so the statistics are always computed
    if ((rc = mvs_conv3d_f16x3_tiled_fwd(x, scale, shift, Cin, cin_ld, D, H, W, w_f16x3, Cout, stride, out, stats_part, guard, st))) return rc;
    // 2. the fp32 kernel of the layer, predicated: conv1 = conv3d_k3_mfma16_kernel<8, 2> (w_f32: mvsnerf_conv3d_pack_weights_mfma layout),
    //    conv2 = conv3d_k3s1_tiled_kernel<16, 16, 16> (w_f32: mvsnerf_conv3d_pack_weights layout)
    const ActSrc a{x, scale, shift}, b{nullptr, nullptr, nullptr};
    if (Cin == 8) {
        if ((rc = mvs_conv3d_mfma32(a, b, Cin, cin_ld, D, H, W, w_f32, Cout, stride, out, nullptr, st, guard))) return rc;
    } else {
        if ((rc = mvs_conv3d_tiled16(a, cin_ld, D, H, W, w_f32, out, nullptr, guard, st))) return rc;
    }
    if (stats_part) {
        const int Do = (D - 1) / stride + 1, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
        if ((rc = mvs_abn_partial(out, (int64_t)Do * Ho * Wo, 16, mvsnerf_conv3d_f16x3_slots(), stats_part, guard, st))) return rc;
    }
    return consume ? mvs_guard_consume(guard, st) : MVSNERF_OK;
}
