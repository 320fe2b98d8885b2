// CostRegNet's convolutions (models.py:674-685, 725-769), forward: the weight packers, the VALU kernels (k3 conv, LDS-tiled k3 s1 conv, k3 s2
// transposed conv) and every mvsnerf_conv3d_* / mvsnerf_conv_transpose3d_* forward entry, those that launch a matrix-core kernel of
// conv_mfma.hip included.
//
// Layouts (all fp32, channel-last so that a voxel's channels are one contiguous vector):
//   cost volume       cost[d][y][x][CP]          CP = round_up4(3V+32): [ref rgb | src rgb.. | variance(32) | 0-pad]
//   activations       act[d][y][x][C]            C in {8,16,32,64}
// InPlaceABN is applied lazily: a conv writes its RAW output; a stats kernel (abn.hip) turns the batch statistics
// into per-channel (scale, shift); every consumer applies leaky_relu(x*scale+shift) while loading.
// Skip additions (models.py:762-766) are the sum of two such lazily-activated tensors.
#include "common.h"
#include "conv3d_bf16_layout.h"
#include "act.h"
#include "conv.h"

// weights re-laid as w[tap][ci][co] (co fastest) so that a thread's CT output channels are contiguous and
// wave-uniform => the compiler fetches them through the scalar cache (s_load) and feeds v_fma from SGPRs.
__global__ void conv3d_pack_kernel(const float* __restrict__ w, int ci_real, int co_real, int cin_pad, int cout_pad,
                                   int s_ci, int s_co, int flip, float* __restrict__ packed)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = 27 * cin_pad * cout_pad;
    if (i >= total) return;
    const int co = i % cout_pad, ci = (i / cout_pad) % cin_pad;
    int tap = i / (cout_pad * cin_pad);
    if (flip) tap = 26 - tap;                                                    // spatially mirrored kernel (data gradient)
    packed[i] = (ci < ci_real && co < co_real) ? w[(int64_t)ci * s_ci + (int64_t)co * s_co + tap] : 0.f;
}

extern "C" int mvsnerf_conv3d_pack_weights(const float* w, int ci_real, int co_real, int cin_pad, int cout_pad,
                                           int s_ci, int s_co, int flip, float* packed, void* stream)
{
    if (!w || !packed || ci_real < 1 || co_real < 1 || cin_pad < ci_real || cout_pad < co_real) return MVSNERF_EINVAL;
    conv3d_pack_kernel<<<mvs_cdiv(27 * cin_pad * cout_pad, 256), 256, 0, (hipStream_t)stream>>>(w, ci_real, co_real, cin_pad, cout_pad, s_ci, s_co, flip, packed);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// Every re-layout a training step needs (the weights change with every optimizer step: ~50 of them, each a 5-us launch of its own) in ONE
// launch.  A job gathers straight from the nn.Conv / nn.ConvTranspose weight tensor:
//   value(tap, ci, co) = (ci < ci_real && co < co_real) ? w[ci * s_ci + co * s_co + (flip ? ntaps - 1 - tap : tap)] : 0
// into layout kind 0: dst[tap][ci][co] (conv3d_pack_weights / conv2d_pack_weights), 1: dst[ci/4][tap][co][ci%4] (conv3d_pack_weights_c8),
// 2: dst[tap][ci/8][co][ci%8] (conv3d_pack_weights_mfma), 3 / 4: the bf16 B fragments of conv3d_bf16.hip for a convolution / a transposed
// convolution (dst is a __bf16 buffer of mvsnerf_conv3d_bf16_packed_elems(ci_pad, co_pad, kind == 4) elements; 27 taps).
constexpr int MVS_PACK_JOBS = 64;

struct PackJobs {
    const float* w[MVS_PACK_JOBS];
    float* dst[MVS_PACK_JOBS];
    int ci_real[MVS_PACK_JOBS], co_real[MVS_PACK_JOBS], ci_pad[MVS_PACK_JOBS], co_pad[MVS_PACK_JOBS], s_ci[MVS_PACK_JOBS], s_co[MVS_PACK_JOBS];
    short ntaps[MVS_PACK_JOBS];
    signed char flip[MVS_PACK_JOBS], kind[MVS_PACK_JOBS];
    int blk[MVS_PACK_JOBS + 1];
    int n_elems[MVS_PACK_JOBS];
    int n;
};

__global__ __launch_bounds__(256) void pack_weights_multi_kernel(PackJobs J)
{
    int j = 0;
    while (j + 1 < J.n && (int)blockIdx.x >= J.blk[j + 1]) ++j;
    const int i = (blockIdx.x - J.blk[j]) * 256 + threadIdx.x;
    const int ntaps = J.ntaps[j], cip = J.ci_pad[j], cop = J.co_pad[j];
    if (J.kind[j] >= 3) {                                         // bf16 fragments (conv3d_bf16.hip)
        if (i >= J.n_elems[j]) return;
        int tap, ci, co;
        float v = 0.f;
        if (mvs_conv3d_bf16_coords(i, cip, cop, J.kind[j] == 4, tap, ci, co, ntaps) && ci < J.ci_real[j] && co < J.co_real[j]) {
            if (J.flip[j]) tap = ntaps - 1 - tap;
            v = J.w[j][(int64_t)ci * J.s_ci[j] + (int64_t)co * J.s_co[j] + tap];
        }
        reinterpret_cast<__bf16*>(J.dst[j])[i] = (__bf16)v;
        return;
    }
    if (i >= ntaps * cip * cop) return;
    int tap, ci, co;
    if (J.kind[j] == 0) { co = i % cop; ci = (i / cop) % cip; tap = i / (cop * cip); }
    else if (J.kind[j] == 1) { co = (i >> 2) % cop; tap = (i / (4 * cop)) % ntaps; ci = (i / (4 * cop * ntaps)) * 4 + (i & 3); }
    else { co = (i >> 3) % cop; ci = ((i / (8 * cop)) % (cip / 8)) * 8 + (i & 7); tap = i / (cip * cop); }
    if (J.flip[j]) tap = ntaps - 1 - tap;
    J.dst[j][i] = (ci < J.ci_real[j] && co < J.co_real[j]) ? J.w[j][(int64_t)ci * J.s_ci[j] + (int64_t)co * J.s_co[j] + tap] : 0.f;
}

// params[j] = {kind, ntaps, ci_real, co_real, ci_pad, co_pad, s_ci, s_co, flip}; host arrays
extern "C" int mvsnerf_pack_weights_multi(int n_jobs, const float* const* w, float* const* dst, const int* params, void* stream)
{
    if (n_jobs < 1 || n_jobs > MVS_PACK_JOBS || !w || !dst || !params) return MVSNERF_EINVAL;
    PackJobs J;
    J.n = n_jobs;
    int b = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int* q = params + 9 * j;
        if (!w[j] || !dst[j] || q[0] < 0 || q[0] > 4 || q[1] < 1 || q[1] > 27 || q[2] < 1 || q[3] < 1 || q[4] < q[2] || q[5] < q[3]) return MVSNERF_EINVAL;
        size_t n_el = (size_t)q[1] * q[4] * q[5];
        if (q[0] >= 3) {
            n_el = mvs_conv3d_bf16_elems(q[4], q[5], q[0] == 4, q[1]);
            if (n_el == 0) return MVSNERF_EUNSUPPORTED;
        }
        if ((q[0] == 1 && (q[4] & 3)) || (q[0] == 2 && (q[4] & 7))) return MVSNERF_EINVAL;
        J.w[j] = w[j]; J.dst[j] = dst[j];
        J.kind[j] = (signed char)q[0]; J.ntaps[j] = (short)q[1]; J.ci_real[j] = q[2]; J.co_real[j] = q[3]; J.ci_pad[j] = q[4]; J.co_pad[j] = q[5];
        J.s_ci[j] = q[6]; J.s_co[j] = q[7]; J.flip[j] = (signed char)(q[8] ? 1 : 0);
        J.blk[j] = b;
        J.n_elems[j] = (int)n_el;
        b += (int)((n_el + 255) / 256);
    }
    J.blk[n_jobs] = b;
    pack_weights_multi_kernel<<<b, 256, 0, (hipStream_t)stream>>>(J);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// Direct 3x3x3 convolution, padding 1, stride S.  One thread = one output voxel x CT output channels.
// Neighbouring threads re-read each other's input voxels through L1/L2 (27-fold reuse).
template <int CIN, int CT, int S, int COUT>      // COUT a template constant: weight offsets become s_load immediates
__global__ __launch_bounds__(256) void conv3d_k3_kernel(ActSrc a, ActSrc b, int ld, int Di, int Hi, int Wi,
                                                       const float* __restrict__ wp,
                                                       float* __restrict__ out, int Do, int Ho, int Wo, int swz)
{
    const int64_t nvox = (int64_t)Do * Ho * Wo;
    const int64_t i = (int64_t)(swz ? xcd_contiguous_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x) * blockDim.x + threadIdx.x;   // an XCD walks contiguous voxels
    const int cg = blockIdx.y * CT;                       // first output channel of this thread
    if (i >= nvox) return;
    const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho), z = (int)(i / ((int64_t)Wo * Ho));
    float acc[CT];
#pragma unroll
    for (int k = 0; k < CT; ++k) acc[k] = 0.f;
    for (int tap = 0; tap < 27; ++tap) {
        const int dz = tap / 9, dy = (tap / 3) % 3, dx = tap % 3;
        const int zi = z * S - 1 + dz, yi = y * S - 1 + dy, xi = x * S - 1 + dx;
        const bool in = zi >= 0 && zi < Di && yi >= 0 && yi < Hi && xi >= 0 && xi < Wi;
        const int64_t vox = in ? ((int64_t)zi * Hi + yi) * Wi + xi : 0;
        const float* wt = wp + (int64_t)tap * CIN * COUT + cg;
#pragma unroll 2
        for (int c = 0; c < CIN; c += 4) {
            f32x4 v;
            load_act4<CIN>(a, b, vox, ld, c, v);
            if (!in) v = f32x4{0, 0, 0, 0};              // zero padding of the *activated* input
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4)
#pragma unroll
                for (int k = 0; k < CT; ++k) acc[k] = fmaf(v[k4], wt[(c + k4) * COUT + k], acc[k]);
        }
    }
    float* o = out + i * COUT + cg;
#pragma unroll
    for (int k = 0; k < CT; k += 4) *reinterpret_cast<f32x4*>(o + k) = f32x4{acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
}

// LDS-tiled variant for the stride-1 layers (conv0 = 74.5 % of CostRegNet's FLOPs).  A workgroup owns a 4x8x8
// block of output voxels; the (6x10x10)-voxel input halo is staged through LDS in chunks of <= 12 channels with
// fully coalesced loads (a voxel's channels are contiguous; the generic kernel's per-tap gathers at a 176-B lane
// stride touch one cache line per lane).  The pending InPlaceABN of the producer is applied once per staged
// element instead of once per tap.  Chunk sizes are compile-time and the x-taps are unrolled so that the LDS reads
// and the scalar weight loads of one (dz,dy) step are in flight while the previous step's FMAs issue.
template <int CIN, int CT, int COUT, int C0, int CKC>     // one channel chunk [C0, C0+CKC) of the tile
__device__ __forceinline__ void conv_tile_chunk(const ActSrc& a, const ActSrc& b, int ld, int D, int H, int W, int x0, int y0, int z0,
                                                const float* __restrict__ wp, int cg, float* __restrict__ tile,
                                                int tid, int tx, int ty, int tz, float (&acc)[CT])
{
    constexpr int CK = 12, IY = 10, IX = 10, NV = 6 * IY * IX, K4 = CKC / 4;
    __syncthreads();
    for (int idx = tid; idx < NV * K4; idx += 256) {
        const int v = idx / K4, c4 = idx - v * K4;
        const int vx = v % IX, vy = (v / IX) % IY, vz = v / (IX * IY);
        const int gx = x0 + vx, gy = y0 + vy, gz = z0 + vz;
        f32x4 val = {0, 0, 0, 0};
        if (gx >= 0 && gx < W && gy >= 0 && gy < H && gz >= 0 && gz < D)
            load_act4<CIN>(a, b, ((int64_t)gz * H + gy) * W + gx, ld, C0 + c4 * 4, val);
        *reinterpret_cast<f32x4*>(tile + v * CK + c4 * 4) = val;
    }
    __syncthreads();
#pragma unroll 1
    for (int dzy = 0; dzy < 9; ++dzy) {
        const int dz = dzy / 3, dy = dzy - dz * 3;
        const float* tv = tile + (((tz + dz) * IY + ty + dy) * IX + tx) * CK;
        const float* wt = wp + ((int64_t)(dzy * 3) * CIN + C0) * COUT + cg;   // COUT is a template constant: the weight offsets below are s_load immediates
        f32x4 v[3][K4];
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
            for (int c4 = 0; c4 < K4; ++c4) v[dx][c4] = *reinterpret_cast<const f32x4*>(tv + dx * CK + c4 * 4);
        if constexpr (CT <= 16) {
            // Weights in groups of 32 (scalar loads, SGPRs), group g+1 requested before the FMAs of group g and a scheduling
            // fence after each group: left alone the scheduler hoists several groups of s_load_dwordx16, runs out of SGPRs and
            // parks weights in VGPR lanes (v_writelane / v_readlane per weight) - and this kernel is bound by the NUMBER of
            // instructions a SIMD can issue, scalar ones included (PMC: 0.6 scalar instructions per packed FMA cost 27 % of
            // the issue cycles; with Cout a template constant the weight offsets are s_load immediates: conv0 2.0 -> 1.5 ms).
            // Tried and dropped: groups of 16 with the requests for the next pair issued after the first FMAs of a pair (so that
            // the compiler's lgkmcnt(0) only covers loads that are ~50 cycles old): CostRegNet 3.03 -> 3.39 ms; 8 instead of 12
            // channels staged per pass (8 instead of 5 workgroups per CU): -1 %, 4 channels: +6 %.
            constexpr int KPG = CT <= 8 ? 4 : 2;                 // k4 values per weight group
            constexpr int GPC = 4 / KPG, NG = 3 * K4 * GPC;       // groups per float4 of x, groups per row
            float w[2][KPG * CT];
            auto wload = [&](float (&wd)[KPG * CT], int g) {
                const int dx = g / (K4 * GPC), r = g - dx * (K4 * GPC), c4 = r / GPC, kb = (r - c4 * GPC) * KPG;
#pragma unroll
                for (int j = 0; j < KPG; ++j)
#pragma unroll
                    for (int k = 0; k < CT; ++k) wd[j * CT + k] = wt[(dx * CIN + c4 * 4 + kb + j) * COUT + k];
            };
            wload(w[0], 0);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (g + 1 < NG) wload(w[(g + 1) & 1], g + 1);
                const int dx = g / (K4 * GPC), r = g - dx * (K4 * GPC), c4 = r / GPC, kb = (r - c4 * GPC) * KPG;
#pragma unroll
                for (int j = 0; j < KPG; ++j)
#pragma unroll
                    for (int k = 0; k < CT; ++k) acc[k] = fmaf(v[dx][c4][kb + j], w[g & 1][j * CT + k], acc[k]);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                for (int c4 = 0; c4 < K4; ++c4)
#pragma unroll
                    for (int k4 = 0; k4 < 4; ++k4)
#pragma unroll
                        for (int k = 0; k < CT; ++k)
                            acc[k] = fmaf(v[dx][c4][k4], wt[(dx * CIN + c4 * 4 + k4) * COUT + k], acc[k]);
        }
    }
}

// Tiles are renumbered so that each XCD walks a contiguous range of them (halo neighbours then share an L2: fabric fetch of conv0
// 6.4 -> 4.4 GB, layer -5 %).  Measured and dropped (conv0, 2.19 ms baseline): two output voxels per thread (half the scalar-load
// traffic and 2/3 of the LDS reads per FMA) -2.5 %; the same with 8-channel chunks -4 %; next chunk's halo prefetched into
// registers during the FMAs (software pipeline, 128 VGPRs) +9 %.  PMC of the kernel as it is: waves spend 62 % of their cycles in
// s_waitcnt, VALU issues 45 % of the time, scalar-cache miss rate 1.5 %, LDS busy 24 % (63 % of that bank conflicts).
template <int CIN, int CT, int COUT>
__global__ __launch_bounds__(256) void conv3d_k3s1_tiled_kernel(ActSrc a, ActSrc b, int ld, int D, int H, int W,
                                                               const float* __restrict__ wp, float* __restrict__ out, int swz,
                                                               float* __restrict__ stats = nullptr, const int* __restrict__ run_if = nullptr)
{
    if (run_if && *run_if == 0) return;                          // fp32 half of a guarded sequence (mvsnerf_conv3d_f16x3_guarded_fwd)
    __shared__ __attribute__((aligned(16))) float tile[600 * 12];
    const int nbx = (W + 7) / 8, nby = (H + 7) / 8;
    const int tile_id = swz ? xcd_contiguous_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;   // halo neighbours share an XCD's L2
    const int bx = tile_id % nbx, by = (tile_id / nbx) % nby, bz = tile_id / (nbx * nby);
    const int cg = blockIdx.y * CT;
    const int tid = threadIdx.x, tx = tid & 7, ty = (tid >> 3) & 7, tz = tid >> 6;
    const int x0 = bx * 8 - 1, y0 = by * 8 - 1, z0 = bz * 4 - 1;
    float acc[CT];
#pragma unroll
    for (int k = 0; k < CT; ++k) acc[k] = 0.f;
#define MVS_CHUNK(C0_, CKC_) conv_tile_chunk<CIN, CT, COUT, C0_, CKC_>(a, b, ld, D, H, W, x0, y0, z0, wp, cg, tile, tid, tx, ty, tz, acc)
    if constexpr (CIN >= 12) MVS_CHUNK(0, 12); else MVS_CHUNK(0, CIN);
    if constexpr (CIN >= 24) MVS_CHUNK(12, 12); else if constexpr (CIN > 12) MVS_CHUNK(12, CIN - 12);
    if constexpr (CIN >= 36) MVS_CHUNK(24, 12); else if constexpr (CIN > 24) MVS_CHUNK(24, CIN - 24);
    if constexpr (CIN >= 48) MVS_CHUNK(36, 12); else if constexpr (CIN > 36) MVS_CHUNK(36, CIN - 36);
    if constexpr (CIN >= 60) MVS_CHUNK(48, 12); else if constexpr (CIN > 48) MVS_CHUNK(48, CIN - 48);
    if constexpr (CIN > 60) MVS_CHUNK(60, CIN - 60);
#undef MVS_CHUNK
    const int ox = bx * 8 + tx, oy = by * 8 + ty, oz = bz * 4 + tz;
    const bool inside = ox < W && oy < H && oz < D;
    if (inside) {
        float* o = out + (((int64_t)oz * H + oy) * W + ox) * COUT + cg;
#pragma unroll
        for (int k = 0; k < CT; k += 4) *reinterpret_cast<f32x4*>(o + k) = f32x4{acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
    }
    if constexpr (256 % CT == 0 && CT >= 4 && CT * 256 <= 600 * 12) {     // the channel values must fit the input tile they reuse
        if (stats) {
            // InPlaceABN partial sums of this tile's CT channels (conv2: no statistics pass re-reads the output).  The 256 voxel values of a
            // channel go through the (now free) input tile: channel k gets 256 / CT lanes of one wave, each adds CT values and their squares,
            // a shuffle tree finishes; fixed order.  Slot = tile, gridDim.x slots (abn_part_at).
            constexpr int LPC = 256 / CT;                        // lanes per channel (8 .. 64: inside a wave)
            __syncthreads();
#pragma unroll
            for (int k = 0; k < CT; ++k) tile[k * 256 + tid] = inside ? acc[k] : 0.0f;
            __syncthreads();
            const int k = tid / LPC, part = tid % LPC;
            float ssum = 0.f, ssq = 0.f;
#pragma unroll
            for (int i = 0; i < CT; ++i) { const float v = tile[k * 256 + part * CT + i]; ssum += v; ssq = fmaf(v, v, ssq); }
#pragma unroll
            for (int o = 1; o < LPC; o <<= 1) { ssum += __shfl_xor(ssum, o); ssq += __shfl_xor(ssq, o); }
            if (part == 0) {
                stats[abn_part_at(0, cg + k, COUT, tile_id, gridDim.x)] = ssum;
                stats[abn_part_at(1, cg + k, COUT, tile_id, gridDim.x)] = ssq;
            }
        }
    }
}

// Transposed 3x3x3 convolution, stride 2, padding 1, output_padding 1 (models.py:739-752): output size = 2x input.
// out[o] = sum over taps k with o = 2*i - 1 + k.  One thread = one output voxel x CT channels; per dimension an even
// output coordinate has one tap (k=1), an odd one two (k=0 from i=(o+1)/2, k=2 from i=(o-1)/2).  The tap loop is wave-uniform
// (only its predicate is per lane), so weights stay on the scalar path; a wave spans one (z,y) row, i.e. it skips the
// (kz,ky) combinations of the wrong parity as a whole.  Measured alternatives, both slower: one workgroup per output parity
// class with strided stores (conv11 436 -> ~600 us), and one thread per x pair with three weight sets per channel chunk.
template <int CIN, int CT, int COUT>
__global__ __launch_bounds__(256) void convT3d_k3s2_kernel(ActSrc a, ActSrc b, int Di, int Hi, int Wi,
                                                          const float* __restrict__ wp, float* __restrict__ out, int swz)
{
    const int Do = 2 * Di, Ho = 2 * Hi, Wo = 2 * Wi;
    const int64_t nvox = (int64_t)Do * Ho * Wo;
    const int64_t i = (int64_t)(swz ? xcd_contiguous_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x) * blockDim.x + threadIdx.x;
    const int cg = blockIdx.y * CT;
    if (i >= nvox) return;
    const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho), z = (int)(i / ((int64_t)Wo * Ho));
    float acc[CT];
#pragma unroll
    for (int k = 0; k < CT; ++k) acc[k] = 0.f;
    for (int tap = 0; tap < 27; ++tap) {
        const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        const int tz = z + 1 - kz, ty = y + 1 - ky, tx = x + 1 - kx;      // = 2*i
        if ((tz | ty | tx) & 1) continue;
        if (tz < 0 || ty < 0 || tx < 0) continue;
        const int zi = tz >> 1, yi = ty >> 1, xi = tx >> 1;
        if (zi >= Di || yi >= Hi || xi >= Wi) continue;
        const int64_t vox = ((int64_t)zi * Hi + yi) * Wi + xi;
        const float* wt = wp + (int64_t)tap * CIN * COUT + cg;
#pragma unroll 1                                            // unrolled, a tap's CIN*CT weights overflow the SGPR file into VGPR lanes
        for (int c = 0; c < CIN; c += 4) {
            f32x4 v;
            load_act4<CIN>(a, b, vox, CIN, c, v);
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4)
#pragma unroll
                for (int k = 0; k < CT; ++k) acc[k] = fmaf(v[k4], wt[(c + k4) * COUT + k], acc[k]);
        }
    }
    float* o = out + i * COUT + cg;
#pragma unroll
    for (int k = 0; k < CT; k += 4) *reinterpret_cast<f32x4*>(o + k) = f32x4{acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
}

// Which kernel a shape takes: the matrix cores where a kernel exists (conv_mfma.hip), the LDS-tiled VALU kernel for the other stride-1
// shapes, the direct VALU kernel for the stride-2 ones.
extern "C" int mvsnerf_conv3d_fwd(const float* x1, const float* scale1, const float* shift1,
                                  const float* x2, const float* scale2, const float* shift2,
                                  int Cin, int cin_ld, int D, int H, int W, const float* wpacked, int Cout, int stride,
                                  float* out, void* stream)
{
    if (!act_ok(x1, scale1, shift1) || !wpacked || !out || D < 1 || H < 1 || W < 1) return MVSNERF_EINVAL;
    if (x2 && (!act_ok(x2, scale2, shift2) || !scale2)) return MVSNERF_EINVAL;
    if (stride != 1 && stride != 2) return MVSNERF_EUNSUPPORTED;
    if ((cin_ld & 3) || cin_ld < Cin || !mvs_aligned16(out)) return MVSNERF_EALIGN;
    const ActSrc a{x1, scale1, shift1}, b{x2, scale2, shift2};
    const int Do = (D - 1) / stride + 1, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;   // k3 p1
    const int64_t nvox = (int64_t)Do * Ho * Wo;
    hipStream_t st = (hipStream_t)stream;
#define MVS_CONV(CIN, CT, S, COUT)                                                                    \
    conv3d_k3_kernel<CIN, CT, S, COUT><<<dim3(mvs_cdiv(nvox, 256), COUT / CT), 256, 0, st>>>(a, b, cin_ld, D, H, W, wpacked, out, Do, Ho, Wo, MVS_XCD_CONTIGUOUS)
#define MVS_CONV_TILED(CIN, CT, COUT)                                                                 \
    conv3d_k3s1_tiled_kernel<CIN, CT, COUT><<<dim3(((W + 7) / 8) * ((H + 7) / 8) * ((D + 3) / 4), COUT / CT), 256, 0, st>>>(a, b, cin_ld, D, H, W, wpacked, out, MVS_XCD_CONTIGUOUS)
    if (Cout == 8 && stride == 1) {
        const int rc = mvs_conv3d_c8_mfma(a, b, Cin, Cin, cin_ld, D, H, W, wpacked, out, st);
        if (rc != MVSNERF_EUNSUPPORTED) return rc;
    }
    // (Cin rounded up to a multiple of 4 by the caller's channel padding; Cout in {8,16,32,64})
    const int key = Cin * 1000 + Cout * 10 + stride;
    switch (key) {
        case 44 * 1000 + 8 * 10 + 1:  MVS_CONV_TILED(44, 8, 8); break;   // conv0 (41 real channels + 3 zero pad)
        case 8 * 1000 + 44 * 10 + 1:  MVS_CONV_TILED(8, 44, 44); break;  // data gradient of conv0
        // conv0 for other source-view counts: Cin = 32 + 3V rounded up to 4 (V=0: plain variance volume; V=1,2,5,6,7,8)
        case 32 * 1000 + 8 * 10 + 1:  MVS_CONV_TILED(32, 8, 8); break;   case 8 * 1000 + 32 * 10 + 1:  MVS_CONV_TILED(8, 32, 32); break;
        case 36 * 1000 + 8 * 10 + 1:  MVS_CONV_TILED(36, 8, 8); break;   case 8 * 1000 + 36 * 10 + 1:  MVS_CONV_TILED(8, 36, 36); break;
        case 40 * 1000 + 8 * 10 + 1:  MVS_CONV_TILED(40, 8, 8); break;   case 8 * 1000 + 40 * 10 + 1:  MVS_CONV_TILED(8, 40, 40); break;
        case 48 * 1000 + 8 * 10 + 1:  MVS_CONV_TILED(48, 8, 8); break;   case 8 * 1000 + 48 * 10 + 1:  MVS_CONV_TILED(8, 48, 48); break;
        case 52 * 1000 + 8 * 10 + 1:  MVS_CONV_TILED(52, 8, 8); break;   case 8 * 1000 + 52 * 10 + 1:  MVS_CONV_TILED(8, 52, 52); break;
        case 56 * 1000 + 8 * 10 + 1:  MVS_CONV_TILED(56, 8, 8); break;   case 8 * 1000 + 56 * 10 + 1:  MVS_CONV_TILED(8, 56, 56); break;
        case 8 * 1000 + 16 * 10 + 2:  MVS_CONV(8, 16, 2, 16); break;     // conv1
        case 16 * 1000 + 16 * 10 + 1: MVS_CONV_TILED(16, 16, 16); break; // conv2
        case 16 * 1000 + 32 * 10 + 2: MVS_CONV(16, 16, 2, 32); break;    // conv3
        case 32 * 1000 + 32 * 10 + 1: MVS_CONV_TILED(32, 16, 32); break; // conv4
        case 32 * 1000 + 64 * 10 + 2: MVS_CONV(32, 16, 2, 64); break;    // conv5
        case 64 * 1000 + 64 * 10 + 1: MVS_CONV_TILED(64, 16, 64); break; // conv6
        default: return MVSNERF_EUNSUPPORTED;
    }
#undef MVS_CONV
#undef MVS_CONV_TILED
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

// conv2 (16 -> 16, stride 1: the LDS-tiled VALU kernel) leaving the InPlaceABN partial sums of its raw output from the same launch:
// stats_part[2][16][mvsnerf_conv3d_tiled_tiles(D, H, W)] for mvsnerf_abn_finalize.  Other shapes: MVSNERF_EUNSUPPORTED (mvsnerf_conv3d_fwd
// + mvsnerf_abn_stats, or the matrix-core entries with their own statistics).
extern "C" int mvsnerf_conv3d_tiled_tiles(int D, int H, int W) { return (D < 1 || H < 1 || W < 1) ? 0 : ((W + 7) / 8) * ((H + 7) / 8) * ((D + 3) / 4); }

int mvs_conv3d_tiled16(const ActSrc& a, int cin_ld, int D, int H, int W, const float* wpacked, float* out, float* stats, const int* run_if, hipStream_t st)
{
    const ActSrc b{nullptr, nullptr, nullptr};
    conv3d_k3s1_tiled_kernel<16, 16, 16><<<dim3((unsigned)mvsnerf_conv3d_tiled_tiles(D, H, W), 1), 256, 0, st>>>(a, b, cin_ld, D, H, W, wpacked, out,
                                                                                                             MVS_XCD_CONTIGUOUS, stats, run_if);
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}

extern "C" int mvsnerf_conv3d_fwd_stats(const float* x1, const float* scale1, const float* shift1, int Cin, int cin_ld, int D, int H, int W,
                                        const float* wpacked, int Cout, int stride, float* out, float* stats_part, void* stream)
{
    if (!act_ok(x1, scale1, shift1) || !wpacked || !out || !stats_part || D < 1 || H < 1 || W < 1) return MVSNERF_EINVAL;
    if ((cin_ld & 3) || cin_ld < Cin || !mvs_aligned16(out)) return MVSNERF_EALIGN;
    if (Cin != 16 || Cout != 16 || stride != 1) return MVSNERF_EUNSUPPORTED;
    return mvs_conv3d_tiled16(ActSrc{x1, scale1, shift1}, cin_ld, D, H, W, wpacked, out, stats_part, nullptr, (hipStream_t)stream);
}

extern "C" int mvsnerf_conv3d_pack_weights_c8(const float* wpacked, int Cin, float* wq, void* stream)
{
    if (!wpacked || !wq || Cin < 4 || (Cin & 3)) return MVSNERF_EINVAL;
    return mvs_conv_w4_repack(wpacked, wq, Cin, (hipStream_t)stream);
}

extern "C" int mvsnerf_conv3d_c8_blocked_fwd(const float* x_blocked, int Cin, int Cin_real, int D, int H, int W, const float* wq, float* out, void* stream)
{
    if (!x_blocked || !wq || !out || D < 1 || H < 1 || W < 1 || Cin < 4 || (Cin & 3) || Cin_real < 1 || Cin_real > Cin) return MVSNERF_EINVAL;
    if (!mvs_aligned16(x_blocked) || !mvs_aligned16(out) || !mvs_aligned16(wq)) return MVSNERF_EALIGN;
    return mvs_conv3d_c8_mfma4(x_blocked, Cin, Cin_real, D, H, W, wq, out, nullptr, (hipStream_t)stream);
}

// The same convolution leaving the InPlaceABN statistics of its output as per-workgroup partial sums (stats_part: 2 * 8 floats per
// workgroup, mvsnerf_conv3d_c8_blocked_tiles(D, H, W) workgroups; finish with mvsnerf_abn_finalize): the 150 MB output is not read again.
extern "C" int mvsnerf_conv3d_c8_blocked_tiles(int D, int H, int W) { return mvs_conv3d_c8_mfma4_tiles(D, H, W); }

extern "C" int mvsnerf_conv3d_c8_blocked_fwd_stats(const float* x_blocked, int Cin, int Cin_real, int D, int H, int W, const float* wq, float* out,
                                                   float* stats_part, void* stream)
{
    if (!x_blocked || !wq || !out || !stats_part || D < 1 || H < 1 || W < 1 || Cin < 4 || (Cin & 3) || Cin_real < 1 || Cin_real > Cin) return MVSNERF_EINVAL;
    if (!mvs_aligned16(x_blocked) || !mvs_aligned16(out) || !mvs_aligned16(wq)) return MVSNERF_EALIGN;
    return mvs_conv3d_c8_mfma4(x_blocked, Cin, Cin_real, D, H, W, wq, out, stats_part, (hipStream_t)stream);
}

// ---- the deep layers (32 / 64 output channels) on v_mfma_f32_32x32x2_f32 (conv_mfma.hip)
extern "C" int mvsnerf_conv3d_mfma_supported(int Cin, int Cout, int stride) { return mvs_conv3d_mfma32_supported(Cin, Cout, stride) ? 1 : 0; }

extern "C" int mvsnerf_conv3d_pack_weights_mfma(const float* wpacked, int Cin, int Cout, float* w32, void* stream)
{
    if (!wpacked || !w32 || Cin < 8 || (Cin & 7) || Cout < 8 || (Cout & 7)) return MVSNERF_EINVAL;
    return mvs_conv_w32_repack(wpacked, w32, Cin, Cout, (hipStream_t)stream);
}

extern "C" int mvsnerf_conv3d_mfma_tiles(int D, int H, int W, int stride) { return (stride == 1 || stride == 2) ? mvs_conv3d_mfma32_tiles(D, H, W, stride) : 0; }

extern "C" int mvsnerf_conv3d_mfma_fwd(const float* x1, const float* scale1, const float* shift1, int Cin, int cin_ld, int D, int H, int W,
                                       const float* w32, int Cout, int stride, float* out, float* stats_part, void* stream)
{
    if (!act_ok(x1, scale1, shift1) || !w32 || !out || D < 1 || H < 1 || W < 1) return MVSNERF_EINVAL;
    if (stride != 1 && stride != 2) return MVSNERF_EUNSUPPORTED;
    if ((cin_ld & 3) || cin_ld < Cin || !mvs_aligned16(out) || !mvs_aligned16(w32)) return MVSNERF_EALIGN;
    const ActSrc a{x1, scale1, shift1}, b{nullptr, nullptr, nullptr};
    return mvs_conv3d_mfma32(a, b, Cin, cin_ld, D, H, W, w32, Cout, stride, out, stats_part, (hipStream_t)stream);
}

extern "C" int mvsnerf_conv_transpose3d_mfma_supported(int Cin, int Cout)
{
    const int k = Cin * 100 + Cout;
    return (k == 6432 || k == 3216 || k == 1608) ? 1 : 0;
}

extern "C" int mvsnerf_conv_transpose3d_mfma_fwd(const float* x, int Cin, int D, int H, int W, const float* w32, int Cout, float* out, void* stream)
{
    if (!x || !w32 || !out || D < 1 || H < 1 || W < 1) return MVSNERF_EINVAL;
    if (!mvs_aligned16(x) || !mvs_aligned16(w32) || !mvs_aligned16(out)) return MVSNERF_EALIGN;
    return mvs_convT3d_mfma32(x, Cin, D, H, W, w32, Cout, out, nullptr, (hipStream_t)stream);
}

// the same launch + the InPlaceABN partial sums of the raw output (conv7 / conv9: no statistics pass re-reads it):
// stats_part[2][Cout][mvsnerf_conv_transpose3d_mfma_tiles(Cin, Cout, D, H, W)] for mvsnerf_abn_finalize
extern "C" int mvsnerf_conv_transpose3d_mfma_tiles(int Cin, int Cout, int D, int H, int W)
{
    if (!mvsnerf_conv_transpose3d_mfma_supported(Cin, Cout) || D < 1 || H < 1 || W < 1) return 0;
    return mvs_convT3d_mfma32_tiles(Cin, Cout, D, H, W);
}

extern "C" int mvsnerf_conv_transpose3d_mfma_fwd_stats(const float* x, int Cin, int D, int H, int W, const float* w32, int Cout, float* out,
                                                       float* stats_part, void* stream)
{
    if (!x || !w32 || !out || !stats_part || D < 1 || H < 1 || W < 1) return MVSNERF_EINVAL;
    if (!mvs_aligned16(x) || !mvs_aligned16(w32)) return MVSNERF_EALIGN;
    if (!mvsnerf_conv_transpose3d_mfma_supported(Cin, Cout)) return MVSNERF_EUNSUPPORTED;
    return mvs_convT3d_mfma32(x, Cin, D, H, W, w32, Cout, out, stats_part, (hipStream_t)stream);
}

// ConvTranspose3d(16, 8, 3, stride 2, padding 1, output_padding 1) of a plain tensor x[D][H][W][16] -> out[2D][2H][2W][8] on
// v_mfma_f32_4x4x1 without padded products; wq: the layer's weights as [ci/4][tap][co][4].
extern "C" int mvsnerf_conv_transpose3d_c8_supported(int Cin, int Cout) { return (Cin == 16 && Cout == 8) ? 1 : 0; }

extern "C" int mvsnerf_conv_transpose3d_c8_fwd(const float* x1, const float* scale1, const float* shift1,
                                               const float* x2, const float* scale2, const float* shift2,
                                               int Cin, int D, int H, int W, const float* wq, float* out, float* stats_part, void* stream)
{
    if (!act_ok(x1, scale1, shift1) || !wq || !out || D < 1 || H < 1 || W < 1) return MVSNERF_EINVAL;
    if (x2 && (!act_ok(x2, scale2, shift2) || !scale2)) return MVSNERF_EINVAL;
    if (Cin != 16) return MVSNERF_EUNSUPPORTED;
    if (!mvs_aligned16(wq) || !mvs_aligned16(out)) return MVSNERF_EALIGN;
    const ActSrc a{x1, scale1, shift1}, b{x2, scale2, shift2};
    return mvs_convT3d_c16to8_mfma4(a, b, D, H, W, wq, out, stats_part, (hipStream_t)stream);
}

extern "C" int mvsnerf_conv_transpose3d_c8_tiles(int D, int H, int W) { return mvs_convT3d_c16to8_tiles(D, H, W); }

extern "C" int mvsnerf_conv_transpose3d_fwd(const float* x1, const float* scale1, const float* shift1,
                                            const float* x2, const float* scale2, const float* shift2,
                                            int Cin, int D, int H, int W, const float* wpacked, int Cout, float* out, void* stream)
{
    if (!act_ok(x1, scale1, shift1) || !wpacked || !out || D < 1 || H < 1 || W < 1) return MVSNERF_EINVAL;
    if (x2 && (!act_ok(x2, scale2, shift2) || !scale2)) return MVSNERF_EINVAL;
    const ActSrc a{x1, scale1, shift1}, b{x2, scale2, shift2};
    const int64_t nvox = (int64_t)8 * D * H * W;
    hipStream_t st = (hipStream_t)stream;
#define MVS_CONVT(CIN, CT, COUT) convT3d_k3s2_kernel<CIN, CT, COUT><<<dim3(mvs_cdiv(nvox, 256), COUT / CT), 256, 0, st>>>(a, b, D, H, W, wpacked, out, MVS_XCD_CONTIGUOUS)
    switch (Cin * 100 + Cout) {
        case 64 * 100 + 32: MVS_CONVT(64, 16, 32); break;   // conv7
        case 32 * 100 + 16: MVS_CONVT(32, 16, 16); break;   // conv9
        case 16 * 100 + 8:  MVS_CONVT(16, 8, 8); break;    // conv11
        default: return MVSNERF_EUNSUPPORTED;
    }
#undef MVS_CONVT
    MVS_LAUNCH_CHECK();
    return MVSNERF_OK;
}
