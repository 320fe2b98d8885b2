// One-call ray march = rendering() of the reference (renderer.py:138-165): enqueues the kernels of
// the batch on one stream from a single host call (one FFI crossing per 1024-ray batch instead of ~40
// ATen launches).
#include "common.h"
#include "march.h"

extern "C" int mvsnerf_abi_version(void) { return 12; }

// fp16x3 kernel reporting through guard[0], then the fp32-MFMA kernel predicated on it (same inputs, same output buffer)
static int mlp_guarded_pair(const void* packed_h, const float* packed_f32, int F, const float* ndc, int ndc_stride, const float* feat, int feat_stride,
                            const float* dirs, int dirs_stride, int64_t N, int S, int alpha_only, float* raw, int* guard, void* stream)
{
    if (!packed_h || !packed_f32 || !ndc || !feat || !raw || !guard || N < 0 || S < 1 || feat_stride < F || ndc_stride < 3) return MVSNERF_EINVAL;
    if (!alpha_only && (!dirs || dirs_stride < 3)) return MVSNERF_EINVAL;
    if (F < 2 || F > 40 || (F & 1)) return MVSNERF_EUNSUPPORTED;
    if (!mvs_aligned16(packed_h) || !mvs_aligned16(packed_f32) || !mvs_aligned16(raw)) return MVSNERF_EALIGN;
    if (N * S == 0) return MVSNERF_OK;
    if (int rc = mvs_mlp_f16x3_fwd(packed_h, packed_f32, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, N * S, S, alpha_only, raw, (hipStream_t)stream, guard)) return rc;
    return mvs_mlp_fwd_if(packed_f32, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, N, S, alpha_only, raw, guard, stream);
}

extern "C" int mvsnerf_mlp_fwd_guarded(const void* packed_fp16, const float* packed_f32, int F, const float* ndc, int ndc_stride,
                                       const float* feat, int feat_stride, const float* dirs, int dirs_stride,
                                       int64_t N, int S, int alpha_only, float* raw, int* guard, void* stream)
{
    if (int rc = mlp_guarded_pair(packed_fp16, packed_f32, F, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, N, S, alpha_only, raw, guard, stream)) return rc;
    if (N * S == 0) return MVSNERF_OK;
    return mvs_guard_consume(guard, (hipStream_t)stream);
}

// The guarded sequence on a device-side row count: counted fp16x3 kernel -> counted fp32 kernel predicated on the guard -> consume.
// All three are enqueued whatever the count is; at a count of 0 the guard is neither tripped nor counted.
extern "C" int mvsnerf_mlp_fwd_guarded_counted(const void* packed_fp16, const float* packed_f32, int F, const float* ndc, const float* feat,
                                               const float* dirs, int64_t cap, const int* count, int alpha_only, float* raw, int* guard, void* stream)
{
    if (!packed_fp16 || !packed_f32 || !ndc || !feat || !raw || !guard || (!alpha_only && !dirs)) return MVSNERF_EINVAL;
    if (int rc = mvs_counted_args(count, cap)) return rc;
    if (F < 2 || F > 40 || (F & 1)) return MVSNERF_EUNSUPPORTED;
    if (!mvs_aligned16(packed_fp16) || !mvs_aligned16(packed_f32) || !mvs_aligned16(raw)) return MVSNERF_EALIGN;
    if (cap == 0) return MVSNERF_OK;
    if (int rc = mvs_mlp_f16x3_fwd_counted(packed_fp16, packed_f32, F, ndc, feat, dirs, (int)cap, count, alpha_only, raw, (hipStream_t)stream, guard)) return rc;
    if (int rc = mvs_mlp_fwd_counted(packed_f32, F, ndc, feat, dirs, cap, count, alpha_only, raw, guard, stream)) return rc;
    return mvs_guard_consume(guard, (hipStream_t)stream);
}

// A guard needs the fp16 split planes (the guarded sequence); checked before anything of the batch is launched.
static bool mlp_choice_ok(const MarchBatch& b) { return !b.guard || (b.packed_split && b.n_split == MVSNERF_SPLIT_FP16); }

// The kernels of one batch, enqueued on `st`: the one-launch ray march when it applies, else lookups -> MLP -> compositing.  The launchers
// validate the rest of the arguments.
static int march_batch(const MarchBatch& b, hipStream_t st)
{
    if (!mlp_choice_ok(b)) return MVSNERF_EINVAL;
    const int F = 8 + 4 * b.V;
    if (b.C != 8 && b.C != F) return MVSNERF_EUNSUPPORTED;
    // fp32 MLP: lookups, MLP and (when a tile holds whole rays) compositing in one launch, when the shapes allow it
    if (b.C == 8 && mvs_raymarch_fused_applies(b)) return mvs_raymarch_fused_fwd(b, st);
    int rc;
    if (b.C != 8) {
        // --use_color_volume (renderer.py:134-135): the feature row is one lookup of the (8 + 4V)-channel volume; same launch: the direction feature
        if ((rc = mvsnerf_gather_colorvol_fwd(b.vol, b.D, b.H, b.W, b.C, b.ndc, b.N, b.S, b.rays_dir, b.w2c, b.feat, F, b.dirs, b.vol_layout, 0, st))) return rc;
    } else if (b.imgs_nhwc4) {
        // gen_dir_feature + gen_pts_feats in one launch (channel-last source images supplied by the caller)
        if ((rc = mvsnerf_gather_fwd(b.vol, b.D, b.H, b.W, b.imgs_nhwc4, b.V, b.IH, b.IW, b.w2c, b.K, b.pts, b.ndc, b.N, b.S, b.rays_dir, b.feat, F,
                                     b.dirs, b.vol_layout, st))) return rc;
    } else {
        // view-direction feature in the reference camera frame (renderer.py:142-147)
        if ((rc = mvsnerf_dir_feature_fwd(b.rays_dir, b.w2c, b.N, 1, b.dirs, st))) return rc;
        // gen_pts_feats (renderer.py:124-136): input_feat[..., :8] = volume lookup, [..., 8:] = colours + masks
        if ((rc = mvsnerf_volume_sample_fwd(b.vol, b.D, b.H, b.W, 8, b.ndc, b.N * b.S, b.feat, F, b.vol_layout, st))) return rc;
        if ((rc = mvsnerf_color_sample_fwd(b.imgs, b.V, b.IH, b.IW, b.w2c, b.K, b.pts, b.N * b.S, 1, b.feat + 8, F, st))) return rc;
    }
    // network_query_fn (renderer.py:156 -> run_network_mvs 42-63)
    if (b.guard)
        rc = mlp_guarded_pair(b.packed_split, b.packed, F, b.ndc, 3, b.feat, F, b.dirs, 3, b.N, b.S, 0, b.raw, b.guard, st);
    else if (b.packed_split)
        rc = mvsnerf_mlp_fwd_split(b.packed_split, b.packed, F, b.n_split, b.ndc, 3, b.feat, F, b.dirs, 3, b.N, b.S, 0, b.raw, st);
    else if (b.packed_bf16)
        rc = mvsnerf_mlp_fwd_bf16(b.packed_bf16, b.packed, F, b.ndc, 3, b.feat, F, b.dirs, 3, b.N, b.S, 0, b.raw, st);
    else
        rc = mvsnerf_mlp_fwd(b.packed, F, b.ndc, 3, b.feat, F, b.dirs, 3, b.N, b.S, 0, b.raw, st);
    if (rc) return rc;
    // raw2outputs (renderer.py:162); in a guarded sequence the same launch counts a fallback and re-arms the guard
    return mvs_composite_fwd(b.raw, b.z, b.N, b.S, b.white_bkgd, b.rgb_map, b.disp, b.acc, b.weights, b.depth, b.alpha, b.guard, st);
}

extern "C" int mvsnerf_raymarch_fwd(const mvsnerf_raymarch_args* a, void* stream)
{
    if (!a) return MVSNERF_EINVAL;
    if (!a->vol || !a->imgs || !a->w2c || !a->K || !a->packed_mlp || !a->rays_pts || !a->rays_ndc || !a->z_vals ||
        !a->rays_dir || !a->dirs_tmp || !a->input_feat || !a->raw)
        return MVSNERF_EINVAL;
    if (a->N < 0 || a->S < 1 || a->V < 1) return MVSNERF_EINVAL;
    return march_batch({.vol = a->vol, .D = a->D, .H = a->H, .W = a->W, .vol_layout = a->vol_layout, .C = 8, .imgs = a->imgs, .imgs_nhwc4 = a->imgs_nhwc4,
                        .V = a->V, .IH = a->IH, .IW = a->IW, .w2c = a->w2c, .K = a->K, .pts = a->rays_pts, .ndc = a->rays_ndc, .z = a->z_vals,
                        .rays_dir = a->rays_dir, .N = a->N, .S = a->S, .white_bkgd = a->white_bkgd, .feat = a->input_feat, .dirs = a->dirs_tmp, .raw = a->raw,
                        .rgb_map = a->rgb_map, .disp = a->disp, .acc = a->acc, .weights = a->weights, .depth = a->depth, .alpha = a->alpha,
                        .packed = a->packed_mlp, .packed_bf16 = a->packed_mlp_bf16, .packed_split = a->packed_mlp_split, .n_split = a->n_split,
                        .guard = a->guard}, (hipStream_t)stream);
}

extern "C" int mvsnerf_raymarch_fwd_batched(const mvsnerf_raymarch_args* a, int K, void* stream)
{
    if (!a || K < 0) return MVSNERF_EINVAL;
    for (int k = 0; k < K; ++k)
        if (int rc = mvsnerf_raymarch_fwd(a + k, stream)) return rc;
    return MVSNERF_OK;
}

// ---------------------------------------------------------------------------------------------
// Full-frame / pixel-range render = the chunk loop of validation_step (train_mvs_nerf_pl.py:198-208):
//   for each chunk: build_rays_test (utils.py:243-297) -> rendering (renderer.py:138-165) -> keep rgb and depth.
// The whole loop is enqueued from ONE host call (4 launches per sub-batch: ray generation, fused gather, MLP,
// compositing; 2 with the fp32 MLP: ray generation, one-launch ray march), so a frame is not paced by ~0.1 ms of Python/ctypes work per 1024-ray chunk.  Rays are independent,
// so the sub-batch size is free (results do not depend on it); temporaries live in a caller-provided workspace that is
// reused by every sub-batch (stream order makes that safe).
// ---------------------------------------------------------------------------------------------
// The workspace of both whole-frame renders: the float offset of every block and the float count, from one walk (so that the size a caller is told
// and the pointers a render carves cannot disagree).  B rays per sub-batch, S coarse + NI importance samples per ray, F feature channels; every block
// starts on 16 bytes.  render_pixels is NI = 0, F = 8 + 4V.
struct RenderWs {
    int64_t pts, ndc, z, zc, feat, raw, rdir, dirs, total;
    RenderWs(int64_t B, int S, int NI, int F)
    {
        const int64_t P = B * (S + NI);
        int64_t at = 0;
        auto block = [&at](int64_t n) { const int64_t o = at; at += (n + 3) & ~(int64_t)3; return o; };
        pts = block(3 * P);
        ndc = block(3 * P);
        z = block(P);
        zc = block(NI > 0 ? B * S : 0);                            // coarse depths of a sub-batch (importance sampling only; else z itself is used)
        feat = block(F * P);
        raw = block(4 * P);
        rdir = block(3 * B);
        dirs = block(3 * B);
        total = at;
    }
};

// Rows [off, off + b.N) of a render's outputs as the outputs of sub-batch b (weights and alpha are not produced)
template <class Args>
static void march_outputs(MarchBatch& b, const Args* a, int64_t off)
{
    b.rgb_map = a->rgb + off * 3;
    b.disp = a->disp ? a->disp + off : nullptr;
    b.acc = a->acc ? a->acc + off : nullptr;
    b.depth = a->depth ? a->depth + off : nullptr;
}

extern "C" size_t mvsnerf_render_workspace_floats(int batch_rays, int S, int V)
{
    if (batch_rays < 1 || S < 1 || V < 1) return 0;
    return (size_t)RenderWs(batch_rays, S, 0, 8 + 4 * V).total;
}

extern "C" int mvsnerf_render_pixels_fwd(const mvsnerf_render_args* a, void* stream)
{
    if (!a) return MVSNERF_EINVAL;
    if (a->n_pixels == 0) return MVSNERF_OK;                       // empty pixel range (a rank with no chunks): nothing to do
    if (!a->vol || !a->imgs_nhwc4 || !a->w2c || !a->K || !a->packed_mlp || !a->K_tgt || !a->c2w_tgt || !a->K_ref || !a->w2c_ref ||
        !a->near_far_tgt || !a->near_far_ref || !a->workspace || !a->rgb)
        return MVSNERF_EINVAL;
    if (a->n_pixels < 0 || a->first_pixel < 0 || a->S < 1 || a->V < 1 || a->batch_rays < 1 || a->W_img < 2 || a->H_img < 2) return MVSNERF_EINVAL;
    if (a->first_pixel + a->n_pixels > (int64_t)a->W_img * a->H_img) return MVSNERF_EINVAL;
    const int F = 8 + 4 * a->V, S = a->S;
    const int64_t B = a->batch_rays;
    const RenderWs ws(B, S, 0, F);
    if (a->workspace_floats < (size_t)ws.total) return MVSNERF_EINVAL;
    float *w = a->workspace, *pts = w + ws.pts, *ndc = w + ws.ndc, *z = w + ws.z, *rdir = w + ws.rdir;
    // every sub-batch: the same workspace slices, its own ray count and output rows (set in the loop); weights and alpha are not produced
    MarchBatch b{.vol = a->vol, .D = a->D, .H = a->H, .W = a->W, .vol_layout = a->vol_layout, .C = 8, .imgs_nhwc4 = a->imgs_nhwc4, .V = a->V, .IH = a->IH,
                 .IW = a->IW, .w2c = a->w2c, .K = a->K, .pts = pts, .ndc = ndc, .z = z, .rays_dir = rdir, .S = S, .white_bkgd = a->white_bkgd,
                 .feat = w + ws.feat, .dirs = w + ws.dirs, .raw = w + ws.raw, .packed = a->packed_mlp, .packed_bf16 = a->packed_mlp_bf16,
                 .packed_split = a->packed_mlp_split, .n_split = a->n_split, .guard = a->guard};
    if (!mlp_choice_ok(b)) return MVSNERF_EINVAL;
    for (int64_t off = 0; off < a->n_pixels; off += B) {
        b.N = a->n_pixels - off < B ? a->n_pixels - off : B;
        if (int rc = mvsnerf_raygen_fwd(nullptr, nullptr, a->first_pixel + off, a->W_img, a->H_img, a->W_ref, a->H_ref, a->K_tgt, a->c2w_tgt, a->K_ref,
                                        a->w2c_ref, a->near_far_tgt, a->near_far_ref, a->pad, a->lindisp, nullptr, b.N, S, pts, rdir, ndc, z, nullptr, stream))
            return rc;
        march_outputs(b, a, off);
        if (int rc = march_batch(b, (hipStream_t)stream)) return rc;
    }
    return MVSNERF_OK;
}

// K batches on a colour volume (rendering_batched under --use_color_volume): the stable batch struct, the channel count beside it
extern "C" int mvsnerf_raymarch_colorvol_fwd_batched(const mvsnerf_raymarch_args* a, int K, int C, void* stream)
{
    if (!a || K < 0) return MVSNERF_EINVAL;
    for (int k = 0; k < K; ++k) {
        const mvsnerf_raymarch_args* x = a + k;
        if (!x->vol || !x->w2c || !x->packed_mlp || !x->rays_ndc || !x->z_vals || !x->rays_dir || !x->dirs_tmp || !x->input_feat || !x->raw) return MVSNERF_EINVAL;
        if (x->N < 0 || x->S < 1 || x->V < 1) return MVSNERF_EINVAL;
        if (C != 8 + 4 * x->V) return MVSNERF_EUNSUPPORTED;
        if (int rc = march_batch({.vol = x->vol, .D = x->D, .H = x->H, .W = x->W, .vol_layout = x->vol_layout, .C = C, .V = x->V, .w2c = x->w2c,
                                  .ndc = x->rays_ndc, .z = x->z_vals, .rays_dir = x->rays_dir, .N = x->N, .S = x->S, .white_bkgd = x->white_bkgd,
                                  .feat = x->input_feat, .dirs = x->dirs_tmp, .raw = x->raw, .rgb_map = x->rgb_map, .disp = x->disp, .acc = x->acc,
                                  .weights = x->weights, .depth = x->depth, .alpha = x->alpha, .packed = x->packed_mlp, .packed_bf16 = x->packed_mlp_bf16,
                                  .packed_split = x->packed_mlp_split, .n_split = x->n_split, .guard = x->guard}, (hipStream_t)stream)) return rc;
    }
    return MVSNERF_OK;
}

// ---------------------------------------------------------------------------------------------
// A frame of a fine-tuned scene from explicit rays = the chunk loop of the fine-tuning script's validation_step
// (train_mvs_nerf_finetuning_pl.py:192-252: ray_marcher -> get_ndc_coordinate -> [ray_marcher_fine -> get_ndc_coordinate] -> rendering per chunk),
// enqueued from ONE host call like mvsnerf_render_pixels_fwd above.  Per sub-batch: coarse depths + points + NDC (one launch), with a density
// volume the merged depths (ray_marcher_fine) and their points (two launches), then march_batch (image gather or colour-volume gather, MLP,
// compositing).  Temporaries live in the caller's workspace, reused by every sub-batch (stream order makes that safe).
// ---------------------------------------------------------------------------------------------
extern "C" size_t mvsnerf_render_rays_workspace_floats(int batch_rays, int S, int n_importance, int F)
{
    if (batch_rays < 1 || S < 1 || n_importance < 0 || F < 12 || (F & 3)) return 0;
    return (size_t)RenderWs(batch_rays, S, n_importance, F).total;
}

extern "C" int mvsnerf_render_rays_fwd(const mvsnerf_render_rays_args* a, void* stream)
{
    if (!a) return MVSNERF_EINVAL;
    if (a->n_rays == 0) return MVSNERF_OK;                         // empty ray range (a rank with no chunks): nothing to do
    if (!a->vol || !a->packed_mlp || !a->K_ref || !a->w2c_ref || !a->near_far_ref || !a->rays || !a->t || !a->workspace || !a->rgb) return MVSNERF_EINVAL;
    if (a->n_rays < 0 || a->first_ray < 0 || a->S < 1 || a->V < 1 || a->batch_rays < 1 || a->W_ref < 2 || a->H_ref < 2 || a->pad < 0 ||
        a->D < 1 || a->H < 1 || a->W < 1 || a->n_importance < 0)
        return MVSNERF_EINVAL;
    if (a->vol_layout != MVSNERF_VOL_DHWC && a->vol_layout != MVSNERF_VOL_HWDC) return MVSNERF_EINVAL;
    const bool fine = a->density && a->n_importance > 0;
    if (fine && (!a->u || a->DD < 1 || a->DH < 1 || a->DW < 1 || a->S < 3)) return MVSNERF_EINVAL;
    const int F = 8 + 4 * a->V, S = a->S, NI = fine ? a->n_importance : 0, St = S + NI;
    if (a->C != 8 && a->C != F) return MVSNERF_EUNSUPPORTED;
    if (F > 40 || (fine && (S > 512 || NI > 512))) return MVSNERF_EUNSUPPORTED;
    if (a->C == 8 && (!a->imgs_nhwc4 || !a->w2c || !a->K || a->IH < 2 || a->IW < 2)) return MVSNERF_EINVAL;
    const int64_t B = a->batch_rays;
    const RenderWs ws(B, S, NI, F);
    if (a->workspace_floats < (size_t)ws.total) return MVSNERF_EINVAL;
    if (!mvs_aligned16(a->workspace) || !mvs_aligned16(a->vol) || !mvs_aligned16(a->packed_mlp) || (a->C == 8 && !mvs_aligned16(a->imgs_nhwc4))) return MVSNERF_EALIGN;
    float *w = a->workspace, *pts = w + ws.pts, *ndc = w + ws.ndc, *z = w + ws.z, *zc = w + ws.zc, *rdir = w + ws.rdir;
    // a colour volume needs the reference view's w2c only (the direction feature); the image gather reads view 0 of w2c as the reference view
    MarchBatch b{.vol = a->vol, .D = a->D, .H = a->H, .W = a->W, .vol_layout = a->vol_layout, .C = a->C, .imgs_nhwc4 = a->C == 8 ? a->imgs_nhwc4 : nullptr,
                 .V = a->V, .IH = a->IH, .IW = a->IW, .w2c = a->C == 8 ? a->w2c : a->w2c_ref, .K = a->K, .pts = pts, .ndc = ndc, .z = z, .rays_dir = rdir,
                 .S = St, .white_bkgd = a->white_bkgd, .feat = w + ws.feat, .dirs = w + ws.dirs, .raw = w + ws.raw, .packed = a->packed_mlp, .packed_bf16 = a->packed_mlp_bf16,
                 .packed_split = a->packed_mlp_split, .n_split = a->n_split, .guard = a->guard};
    if (!mlp_choice_ok(b)) return MVSNERF_EINVAL;
    for (int64_t off = 0; off < a->n_rays; off += B) {
        b.N = a->n_rays - off < B ? a->n_rays - off : B;
        const float* r = a->rays + (a->first_ray + off) * 8;
        // ray_marcher + get_ndc_coordinate: depths from (near, far) = r[6], r[7] of every ray and t, points, NDC; directions compacted to [N][3]
        if (int rc = mvs_ray_points(r, 8, r + 3, 8, nullptr, a->w2c_ref, a->K_ref, a->near_far_ref, a->W_ref, a->H_ref, a->pad, a->lindisp, b.N, S, pts, ndc,
                                    a->t, r + 6, 8, fine ? zc : z, rdir, stream))
            return rc;
        if (fine) {
            // ray_marcher_fine + get_ndc_coordinate of the merged depths
            if (int rc = mvsnerf_ray_marcher_fine_fwd(a->density, a->DD, a->DH, a->DW, ndc, zc, a->u + (a->first_ray + off) * NI, b.N, S, NI, z, stream)) return rc;
            if (int rc = mvs_ray_points(r, 8, r + 3, 8, z, a->w2c_ref, a->K_ref, a->near_far_ref, a->W_ref, a->H_ref, a->pad, a->lindisp, b.N, St, pts, ndc,
                                        nullptr, nullptr, 0, nullptr, nullptr, stream))
                return rc;
        }
        march_outputs(b, a, off);
        if (int rc = march_batch(b, (hipStream_t)stream)) return rc;
    }
    return MVSNERF_OK;
}

// ---------------------------------------------------------------------------------------------
// The differentiable ray march as two host calls: forward with activation store, backward to the MLP
// parameters and the volume.
// ---------------------------------------------------------------------------------------------
extern "C" int mvsnerf_raymarch_train_fwd(const mvsnerf_raymarch_train_args* a, void* stream)
{
    if (!a) return MVSNERF_EINVAL;
    if (!a->vol || !a->w2c || !a->packed_mlp || !a->rays_ndc || !a->z_vals || !a->rays_dir || !a->dirs_tmp || !a->input_feat || !a->raw || !a->saved)
        return MVSNERF_EINVAL;
    if (a->N < 0 || a->S < 1 || a->V < 1 || (a->bf16 && !a->packed_mlp_bf16)) return MVSNERF_EINVAL;
    const int F = 8 + 4 * a->V;
    const int64_t P = a->N * a->S;
    int rc;
    if (a->C == F && a->C != 8) {
        // --use_color_volume (renderer.py:134-135): the volume already holds the projected colours
        if ((rc = mvsnerf_dir_feature_fwd(a->rays_dir, a->w2c, a->N, 1, a->dirs_tmp, stream))) return rc;
        if ((rc = mvsnerf_volume_sample_fwd(a->vol, a->D, a->H, a->W, a->C, a->rays_ndc, P, a->input_feat, F, a->vol_layout, stream))) return rc;
    } else if (a->C == 8) {
        if (!a->imgs_nhwc4 || !a->K || !a->rays_pts) return MVSNERF_EINVAL;
        if ((rc = mvsnerf_gather_fwd(a->vol, a->D, a->H, a->W, a->imgs_nhwc4, a->V, a->IH, a->IW, a->w2c, a->K, a->rays_pts, a->rays_ndc,
                                     a->N, a->S, a->rays_dir, a->input_feat, F, a->dirs_tmp, a->vol_layout, stream))) return rc;
    } else {
        return MVSNERF_EUNSUPPORTED;
    }
    if (a->bf16) rc = mvsnerf_mlp_fwd_bf16_train(a->packed_mlp_bf16, a->packed_mlp, F, a->rays_ndc, 3, a->input_feat, F, a->dirs_tmp, 3, a->N, a->S, a->raw, a->saved, stream);
    else rc = mvsnerf_mlp_fwd_train(a->packed_mlp, F, a->rays_ndc, 3, a->input_feat, F, a->dirs_tmp, 3, a->N, a->S, a->raw, a->saved, stream);
    if (rc) return rc;
    return mvsnerf_composite_fwd(a->raw, a->z_vals, a->N, a->S, a->white_bkgd, a->rgb_map, a->disp, a->acc, a->weights, a->depth, a->alpha, stream);
}

extern "C" int mvsnerf_raymarch_bwd(const mvsnerf_raymarch_bwd_args* a, void* stream)
{
    if (!a) return MVSNERF_EINVAL;
    if (!a->packed_mlp || !a->packed_bwd || !a->raw || !a->saved || !a->z_vals || !a->rays_ndc || !a->d_raw || !a->gslots || !a->d_feat || !a->gw ||
        !a->gb || !a->maps || !a->workspace)
        return MVSNERF_EINVAL;
    if (a->N < 0 || a->S < 1) return MVSNERF_EINVAL;
    if (a->gvol && a->C != a->n_feat_out) return MVSNERF_EINVAL;
    int rc;
    if ((rc = mvsnerf_composite_bwd(a->raw, a->z_vals, a->N, a->S, a->white_bkgd, a->g_rgb, a->g_depth, nullptr, a->g_weights, a->g_alpha, a->d_raw, stream)))
        return rc;
    if (a->bf16) rc = mvsnerf_mlp_bwd_bf16(a->packed_mlp, a->packed_bwd, a->F, a->raw, a->d_raw, a->saved, a->N, a->S, a->gslots, a->d_feat, a->n_feat_out,
                                          a->gw, a->gb, a->maps, a->workspace, stream);
    else rc = mvsnerf_mlp_bwd(a->packed_mlp, reinterpret_cast<const float*>(a->packed_bwd), a->F, a->raw, a->d_raw, a->saved, a->N, a->S, a->gslots, a->d_feat,
                              a->n_feat_out, a->gw, a->gb, a->maps, a->workspace, stream);
    if (rc) return rc;
    if (a->gvol)
        return mvsnerf_volume_sample_bwd(a->D, a->H, a->W, a->C, a->rays_ndc, a->N * a->S, a->d_feat, a->n_feat_out, a->gvol, stream);
    return MVSNERF_OK;
}
