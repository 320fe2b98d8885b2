"""CPU float64 references for the 16-bit no-grad radiance MLP kernels (csrc/mlp_bf16.hip, csrc/mlp_f16x3.hip).

weights(F)    the checkpoint's 11 (weight, bias) pairs at F = 20; at any other F the same pairs with pts_bias.weight replaced by its columns
              arange(F) % 20 times sqrt(20 / F) (rounded to fp32 once): the modulation keeps the checkpoint's range, so the network stays alive
              (test_mlp16_refs.py: sigma > 0 on 40 .. 90 % of the points of every case); uniform(-0.15, 0.15) weights leave it nearly dead.
inputs(...)   tests/test_gpu_mlp_fold.py's _inputs; wide=True draws ndc in [-0.5, 1.5] (points outside the frustum: the sine's range reduction).
exact(...)    Renderer_ours (models.py:199-217) with the Embedder (models.py:47-51) in float64 on the fp32 weights and inputs -> (N*S, 4) = rgb | sigma.
emulate(mode, ...)  the same network in float64 with every GEMM that the kernel runs on the matrix cores replaced by the float64 sum of exactly the
              piece products the kernel keeps.  An operand x is cut into pieces p0 = rnd(x), p1 = rnd(x - p0), ...; rnd keeps `bits` significant bits,
              to nearest even or by truncation, with no exponent limit.  Per mode (a = the layer input, w = the weight):

    mode                 a pieces          w pieces          products kept                                   read from
    "bf16"               1 x 8 bits, RN    1 x 8 bits, RN    a0w0                                            mlp_bf16.hip:119-130 (pack8), :52 (pack_b_segment)
    "split1"             1 x 8 bits, RN    1 x 8 bits, RN    a0w0                                            mlp_bf16.hip:633-642, :579, :682 (NPROD = 1)
    "split2"             2 x 8 bits, RN    2 x 8 bits, RN    a0w0 + a0w1 + a1w0                              mlp_bf16.hip:633-642, :579-580, :706 (PA / PB, last 3)
    "split3"             3 x 8 bits, TRUNC 3 x 8 bits, RN    a0w0 + a0w1 + a1w0 + a1w1 + a0w2 + a2w0         mlp_bf16.hip:617-632, :579-580, :706 (all 6)
    "fp16x3", "guarded"  2 x 11 bits, RN   2 x 11 bits, RN   a0w0 + a0w1 + a1w0                              mlp_f16x3.hip:7-9, :137-139, :175-177, :250-268
    "none"               the float64 operands themselves: emulate("none") is exact()

    (split3: the ACTIVATIONS are cut by truncation, split8<3>, but the WEIGHTS of every n_split are cut by the pack kernel's round-to-nearest
    conversion; three pieces of either kind sum to an fp32 value exactly.)

    Emulated GEMMs, the same nine in all five kernels: pts_bias on the features; pts_linears.0 on the encoding; pts_linears.1-4; pts_linears.5 on
    [encoding | h4] (two segments onto one accumulator); feature_linear; views_linears.0 on [feature | direction] (mlp_bf16.hip:458-531 pair
    kernel, :899-960 split kernel; mlp_f16x3.hip:418-612).  The features, the encoding and the view direction are layer inputs and are cut like
    the activations.  Not emulated, float64 here and fp32 VALU in the kernels: alpha_linear, which reads the UN-ROUNDED activations of
    pts_linears.5 (mlp_bf16.hip:498-506, :930-935; mlp_f16x3.hip:541-549), rgb_linear (mlp_bf16.hip:532-541, :961-970; mlp_f16x3.hip:613-622),
    the biases (the accumulators' initial values), the multiplicative modulation, ReLU, the sigmoid and the encoding's sin / cos.

    The emulation holds the operand ROUNDING and the dropped products only.  What a kernel adds on top - fp32 accumulation, fp32 epilogues, its
    fp32 sin / cos - is the error of the fp32 kernel on the same case, which the GPU tests allow for separately.  The fp16 rows are idealised (no
    exponent-range loss: the kernel scales by exact powers of two to stay clear of it): a lower bound of that mode's error.
"""
import functools

import numpy as np
import torch

from tests.test_gpu_mlp_fold import _embed, _inputs

ORDER = [f"pts_linears.{i}" for i in range(6)] + ["pts_bias", "feature_linear", "alpha_linear", "views_linears.0", "rgb_linear"]      # ops.MLP_ORDER
RN, TRUNC = "rn", "trunc"

# mode -> ((activation pieces, bits, rounding), (weight pieces, bits, rounding), kept (activation piece, weight piece) products)
SPECS = {
    "bf16":   ((1, 8, RN), (1, 8, RN), ((0, 0),)),
    "split1": ((1, 8, RN), (1, 8, RN), ((0, 0),)),
    "split2": ((2, 8, RN), (2, 8, RN), ((0, 0), (0, 1), (1, 0))),
    "split3": ((3, 8, TRUNC), (3, 8, RN), ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))),
    "fp16x3": ((2, 11, RN), (2, 11, RN), ((0, 0), (0, 1), (1, 0))),
}
SPECS["guarded"] = SPECS["fp16x3"]
ALL9 = tuple((i, j) for i in range(3) for j in range(3))


@functools.lru_cache(maxsize=None)
def weights(F):
    """-> (ws, bs): 11 fp32 CPU tensors each, in ops.MLP_ORDER"""
    from tests.util import load_weights
    sd = load_weights()[0]
    ws = [sd[f"nerf.{n}.weight"].clone().contiguous() for n in ORDER]
    bs = [sd[f"nerf.{n}.bias"].clone().contiguous() for n in ORDER]
    if F != 20:
        ws[6] = (ws[6][:, torch.arange(F) % 20].double() * float(np.sqrt(20.0 / F))).float().contiguous()
    return ws, bs


def inputs(N, S, F, wide=False):
    """-> ndc (N, S, 3), feat (N, S, F), dirs (N, 3), fp32 CPU.  (A case that test_mlp16_refs.py finds outside the 40 .. 90 % liveness band gets
    another seed here; none of the current ones needed it.)"""
    ndc, feat, dirs = _inputs(N, S, F)
    if wide:
        g = torch.Generator().manual_seed(77000 + 1000 * N + 10 * S + F)
        ndc = torch.rand((N, S, 3), generator=g) * 2.0 - 0.5
    return ndc, feat, dirs


def pieces(x, n, bits, rounding):
    """x (float64) -> n float64 tensors p0, p1, ...: p_k = the `bits`-significant-bit rounding of x - p0 - .. - p_(k-1)"""
    out, rem = [], x.double().clone()
    for _ in range(n):
        m, e = torch.frexp(rem)                                  # rem = m 2^e, |m| in [0.5, 1)
        m = m * 2.0 ** bits
        m = torch.round(m) if rounding == RN else torch.trunc(m)      # torch.round: half to even
        p = torch.ldexp(m, e - bits)
        out.append(p)
        rem = rem - p                                            # exact: p shares rem's leading bits
    return out


def piece_gemm(a, w, b, spec, kept=None):
    """b + sum over the kept (i, j) of a_i w_j^T in float64"""
    (na, ba, ra), (nw, bw, rw), products = spec
    ap, wp = pieces(a, na, ba, ra), pieces(w, nw, bw, rw)
    out = b.double().expand(*a.shape[:-1], w.shape[0]).clone()
    for i, j in (products if kept is None else kept):
        out = out + ap[i] @ wp[j].T
    return out


def _network(ws, bs, ndc, feat, dirs, mm):
    """mm(x, i) = the matrix-core GEMM of linear i of ORDER (bias included); everything else float64"""
    lin = torch.nn.functional.linear
    N, S = ndc.shape[:2]
    w64, b64 = [w.double() for w in ws], [b.double() for b in bs]
    pts = _embed(ndc.double())
    bias = mm(feat.double(), 6)
    h = pts
    for i in range(6):
        h = torch.relu(mm(h, i) * bias)
        if i == 4:
            h = torch.cat([pts, h], -1)
    sigma = torch.relu(lin(h, w64[8], b64[8]))                                         # alpha_linear on the un-rounded activations
    d = dirs.double()[:, None, :].expand(N, S, 3)
    hv = torch.relu(mm(torch.cat([mm(h, 7), d], -1), 9))
    rgb = torch.sigmoid(lin(hv, w64[10], b64[10]))
    return torch.cat([rgb, sigma], -1).reshape(N * S, 4)


def exact(ws, bs, ndc, feat, dirs):
    w64, b64 = [w.double() for w in ws], [b.double() for b in bs]
    return _network(ws, bs, ndc, feat, dirs, lambda x, i: torch.nn.functional.linear(x, w64[i], b64[i]))


def emulate(mode, ws, bs, ndc, feat, dirs, kept=None):
    """kept: another set of (activation piece, weight piece) products than the mode's (the sensitivity checks of test_mlp16_refs.py)"""
    if mode == "none":
        return exact(ws, bs, ndc, feat, dirs)
    spec = SPECS[mode]
    return _network(ws, bs, ndc, feat, dirs, lambda x, i: piece_gemm(x, ws[i].double(), bs[i], spec, kept))


def mean_errs(got, ref):
    """-> (mean |rgb error|, mean |sigma error|) in float64"""
    d = (got.double() - ref.double()).abs()
    return float(d[:, :3].mean()), float(d[:, 3].mean())


def live_fraction(ref):
    return float((ref[:, 3] > 0).double().mean())
