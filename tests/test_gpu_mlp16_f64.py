"""The five 16-bit no-grad radiance MLP kernels against float64, and their row layouts (csrc/mlp_bf16.hip, csrc/mlp_f16x3.hip, csrc/mlp_b16_dev.h).

Modes: "bf16" = mlp_fwd_bf16_pair_kernel (mvsnerf_mlp_fwd_bf16); "split1" / "split2" / "split3" = mlp_fwd_split_kernel<NS> (mvsnerf_mlp_fwd_split,
n_split 1 / 2 = "bf16x3" / 3 = "bf16x6"); "fp16x3" = mlp_fwd_f16x3_kernel (n_split 18); "guarded" = the same kernel inside mvsnerf_mlp_fwd_guarded,
what "auto" runs.  All through ops.mlp_forward on the packs of ops.mlp_pack / mlp_pack_bf16 / mlp_pack_split.  References: tests/mlp16_refs.py.

A  the bits of a result do not depend on the row layout.  Baseline: dense, 16-byte-aligned rows - the bf16 and fp16 kernels then stage a full wave's
   features through LDS with 16-byte vectors (stage_features, csrc/mlp_b16_dev.h:119) when F <= 32.  Against it: `feat` one float into a larger
   buffer (dense but misaligned: every wave loads per lane); feat_stride = F + 3, ndc_stride = 5, dirs_stride = 4 with NaN in the gaps; and ndc,
   feat, dirs as three views of one row of 63 + F + 3 floats, S = 1 (include/mvsnerf_hip.h:283).
B  alpha_only = 1 -> (N S, 1), the bits of column 3 of the full launch: every kernel's sigma-only instantiation runs the same GEMMs in the same
   order and leaves out what follows the sigma head.
C  mean absolute errors against float64, rgb and sigma apart: e_k (kernel), E_M (the mode's emulation: operand rounding and dropped products only),
   e_32 (the fp32 kernel, stable pack, same case; pinned by test_gpu_mlp_fold.py / test_gpu_net_v2.py).
       e_k <= 1.25 E_M + 2 e_32         1.25: this project's margin for mean-error ratios; 2 e_32: fp32 accumulation in another order and k-step
                                        width on top of the modelled rounding - the factor 2 is not derived, (e_k - 1.25 E_M) / e_32 is recorded
       e_k >= 0.5 E_M                   for bf16, split1, split2 where E_M > 10 e_32: a kernel much better than its emulation is not running the
                                        emulated arithmetic
D  a ray's rows do not depend on its position in the batch; a launch writes its rows and nothing else; N = 0 writes nothing.
E  refusals before any launch, output untouched (what tests/test_error_behaviour.py does not already assert).

F: 2 (minimum), 10 (F/2 odd), 12, 16 (one whole 16-wide k-step), 20 (the checkpoint), 28, 32 (the last staged width), 34 (the first unstaged), 40.
(N, S): (5, 7) one partial wave; (37, 24) = 888 points: full and partial workgroups of 128 and 256, rays straddling waves; (3, 300) one ray
across workgroups; (300, 1) rows.
"""
import functools

import pytest
import torch

from tests import mlp16_refs as R
from tests.test_gpu_mlp_fold import _bits, _pack_stable
from tests.util import record_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
MODES = ["bf16", "split1", "split2", "split3", "fp16x3"]
N_SPLIT = {"split1": 1, "split2": 2, "split3": 3, "fp16x3": 18, "guarded": 18}
FS = [2, 10, 12, 16, 20, 28, 32, 34, 40]
SHAPES = [(5, 7), (37, 24), (3, 300), (300, 1)]
C_CASES = [(37, 24, False), (37, 24, True), (3, 300, False)]
NAN = float("nan")


# ------------------------------------------------------------------ packs, cases, launches
@functools.lru_cache(maxsize=None)
def _net(F):
    from mvsnerf_amd import ops
    ws, bs = R.weights(F)
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    net = dict(f32=ops.mlp_pack(wd, bd, F), stable=_pack_stable(ws, bs, F), bf16=ops.mlp_pack_bf16(wd, F),
               split={n: ops.mlp_pack_split(wd, F, n) for n in (1, 2, 3, 18)})
    torch.cuda.synchronize()
    return net


def _choice(net, mode):
    """the keywords of ops.mlp_forward that select the mode's kernel"""
    from mvsnerf_amd import ops
    if mode == "bf16":
        return dict(packed_bf16=net["bf16"])
    kw = dict(packed_split=(net["split"][N_SPLIT[mode]], N_SPLIT[mode]))
    if mode == "guarded":
        kw["guard"] = ops.guard_words()
    return kw


def _fwd(F, mode, ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, N, S, alpha_only=0, out=None):
    """ndc / feat / dirs: device tensors (or views) whose data_ptr() is the first row"""
    from mvsnerf_amd import ops
    net = _net(F)
    if mode == "fp32":
        raw = ops.mlp_forward(net["stable"], F, ndc.data_ptr(), ndc_stride, feat.data_ptr(), feat_stride, dirs.data_ptr(), dirs_stride, N, S, alpha_only, DEV, out=out)
    else:
        raw = ops.mlp_forward(net["f32"], F, ndc.data_ptr(), ndc_stride, feat.data_ptr(), feat_stride, dirs.data_ptr(), dirs_stride, N, S, alpha_only, DEV,
                              out=out, **_choice(net, mode))
    torch.cuda.synchronize()
    return raw


@functools.lru_cache(maxsize=None)
def _x(N, S, F, wide=False):
    return tuple(t.to(DEV).contiguous() for t in R.inputs(N, S, F, wide))


@functools.lru_cache(maxsize=None)
def _dense(mode, N, S, F, wide=False):
    """the dense aligned launch: every part's baseline"""
    ndc, feat, dirs = _x(N, S, F, wide)
    assert feat.data_ptr() % 16 == 0
    raw = _fwd(F, mode, ndc, 3, feat, F, dirs, 3, N, S)
    assert raw.shape == (N * S, 4) and bool(torch.isfinite(raw).all())
    return raw


@functools.lru_cache(maxsize=None)
def _exact(N, S, F, wide):
    return R.exact(*R.weights(F), *R.inputs(N, S, F, wide))


@functools.lru_cache(maxsize=None)
def _emulated_errs(spec, N, S, F, wide):
    """E_M; keyed by the arithmetic, which bf16 and split1 share"""
    mode = next(m for m in MODES if R.SPECS[m] == spec)
    return R.mean_errs(R.emulate(mode, *R.weights(F), *R.inputs(N, S, F, wide)), _exact(N, S, F, wide))


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("mode", MODES + ["guarded"])
def test_bits_do_not_depend_on_the_row_layout(mode, F):
    for N, S in [(37, 24), (5, 7)]:
        ndc, feat, dirs = _x(N, S, F)
        P = N * S
        want = _dense(mode, N, S, F)
        # dense rows one float off 16-byte alignment: no wave stages
        buf = torch.full((P * F + 8,), NAN, device=DEV)
        off = buf[1:1 + P * F]
        off.copy_(feat.reshape(-1))
        assert off.data_ptr() % 16 == 4
        got = _fwd(F, mode, ndc, 3, off, F, dirs, 3, N, S)
        assert _bits(got, want), ("misaligned", N, S, float((got - want).abs().max()))
        # padded rows, NaN in the gaps
        ndc_p, feat_p, dirs_p = torch.full((P, 5), NAN, device=DEV), torch.full((P, F + 3), NAN, device=DEV), torch.full((N, 4), NAN, device=DEV)
        ndc_p[:, :3], feat_p[:, :F], dirs_p[:, :3] = ndc.reshape(P, 3), feat.reshape(P, F), dirs
        got = _fwd(F, mode, ndc_p, 5, feat_p, F + 3, dirs_p, 4, N, S)
        assert _bits(got, want), ("strided", N, S, float((got - want).abs().max()))
        # one row of [63 embedding slots | F features | 3 direction] per point, S = 1: the embedding's first three are the point itself
        dirs_pt = dirs[:, None, :].expand(N, S, 3).reshape(P, 3).contiguous()
        want_rows = _fwd(F, mode, ndc.reshape(P, 3), 3, feat.reshape(P, F), F, dirs_pt, 3, P, 1)
        rows = torch.full((P, 63 + F + 3), NAN, device=DEV)
        rows[:, :3], rows[:, 63:63 + F], rows[:, 63 + F:] = ndc.reshape(P, 3), feat.reshape(P, F), dirs_pt
        got = _fwd(F, mode, rows, 66 + F, rows[0, 63:], 66 + F, rows[0, 63 + F:], 66 + F, P, 1)
        assert _bits(got, want_rows), ("rows", N, S, float((got - want_rows).abs().max()))
        # a point's result does not depend on how its ray is told either: (N, S) with one direction per ray is (N S, 1) with one per point
        assert _bits(want_rows, want), ("rows vs rays", N, S)


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("mode", MODES)
def test_sigma_only_launch_is_column_3(mode, F):
    for N, S in SHAPES:
        ndc, feat, dirs = _x(N, S, F)
        a = _fwd(F, mode, ndc, 3, feat, F, dirs, 3, N, S, alpha_only=1)
        full = _dense(mode, N, S, F)
        assert a.shape == (N * S, 1)
        assert _bits(a[:, 0], full[:, 3]), (N, S, float((a[:, 0] - full[:, 3]).abs().max()))


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("mode", MODES)
def test_accuracy_against_float64(mode, F):
    failures = []
    for N, S, wide in C_CASES:
        ref = _exact(N, S, F, wide)
        e_k = R.mean_errs(_dense(mode, N, S, F, wide).cpu(), ref)
        e_32 = R.mean_errs(_dense("fp32", N, S, F, wide).cpu(), ref)
        E_M = _emulated_errs(R.SPECS[mode], N, S, F, wide)
        for c, what in enumerate(("rgb", "sigma")):
            excess, ratio = (e_k[c] - 1.25 * E_M[c]) / e_32[c], e_k[c] / E_M[c]
            tag = f"mlp16_f64:{mode}:F{F}:({N},{S}){':wide' if wide else ''}:{what}"
            record_err(tag + ":(e_k-1.25E_M)/e_32", excess, scale=e_32[c], tol=2.0)
            record_err(tag + ":e_k/E_M", ratio, scale=E_M[c])
            print(f"{tag}: e_k {e_k[c]:.3e}  E_M {E_M[c]:.3e}  e_32 {e_32[c]:.3e}  (e_k - 1.25 E_M) / e_32 {excess:+.3f}  e_k / E_M {ratio:.3f}")
            if not e_k[c] <= 1.25 * E_M[c] + 2.0 * e_32[c]:
                failures.append((tag, "above", e_k[c], E_M[c], e_32[c]))
            if mode in ("bf16", "split1", "split2") and E_M[c] > 10.0 * e_32[c] and not e_k[c] >= 0.5 * E_M[c]:
                failures.append((tag, "below", e_k[c], E_M[c], e_32[c]))
    assert not failures, failures


# ------------------------------------------------------------------ D
@pytest.mark.parametrize("F", [12, 20, 34])
@pytest.mark.parametrize("mode", MODES + ["guarded"])
def test_rows_do_not_depend_on_the_position_in_the_batch(mode, F):
    N, S, PRE = 5, 7, 33
    ndc, feat, dirs = _x(N, S, F)
    ndc0, feat0, dirs0 = _x(PRE, S, F)
    alone = _dense(mode, N, S, F)
    both = _fwd(F, mode, torch.cat([ndc0, ndc]).contiguous(), 3, torch.cat([feat0, feat]).contiguous(), F, torch.cat([dirs0, dirs]).contiguous(), 3, PRE + N, S)
    assert both.shape == ((PRE + N) * S, 4)
    assert _bits(both[PRE * S:], alone), float((both[PRE * S:] - alone).abs().max())
    assert _bits(both[:PRE * S], _dense(mode, PRE, S, F))


@pytest.mark.parametrize("F", [12, 20, 34])
@pytest.mark.parametrize("mode", MODES + ["guarded"])
def test_a_launch_writes_its_rows_and_nothing_else(mode, F):
    from mvsnerf_amd import _lib
    for N, S in SHAPES:
        ndc, feat, dirs = _x(N, S, F)
        P = N * S
        for alpha_only, C in ((0, 4), (1, 1)):
            big = torch.full((P + 8, C), NAN, device=DEV)
            out = big[4:4 + P]                                       # 16 C bytes in: aligned
            raw = _fwd(F, mode, ndc, 3, feat, F, dirs, 3, N, S, alpha_only=alpha_only, out=out)
            assert raw.data_ptr() == out.data_ptr()
            assert bool(torch.isfinite(out).all()), (N, S, C)
            assert bool(torch.isnan(big[:4]).all()) and bool(torch.isnan(big[4 + P:]).all()), (N, S, C)
            assert _bits(out, _dense(mode, N, S, F) if C == 4 else _dense(mode, N, S, F)[:, 3:4]), (N, S, C)
    # N = 0: OK, no launch, nothing written
    net, l = _net(F), _lib.lib()
    ndc, feat, dirs = _x(5, 7, F)
    out = torch.full((64, 4), NAN, device=DEV)
    io = (ndc.data_ptr(), 3, feat.data_ptr(), F, dirs.data_ptr(), 3, 0, 7, 0, out.data_ptr())
    assert _entry(l, net, mode, F, io) == OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def _entry(l, net, mode, F, io):
    """the mode's C entry on io = (ndc, ndc_stride, feat, feat_stride, dirs, dirs_stride, N, S, alpha_only, raw) -> return code"""
    from mvsnerf_amd import ops
    st = ops.stream_ptr()
    if mode == "bf16":
        return l.mvsnerf_mlp_fwd_bf16(net["bf16"].data_ptr(), net["f32"].data_ptr(), F, *io, st)
    planes = net["split"][N_SPLIT[mode]].data_ptr()
    if mode == "guarded":
        return l.mvsnerf_mlp_fwd_guarded(planes, net["f32"].data_ptr(), F, *io, ops.guard_words().data_ptr(), st)
    return l.mvsnerf_mlp_fwd_split(planes, net["f32"].data_ptr(), F, N_SPLIT[mode], *io, st)


# ------------------------------------------------------------------ E
@pytest.mark.parametrize("mode", MODES + ["guarded"])
def test_refusals_leave_the_output_untouched(mode):
    from mvsnerf_amd import _lib
    l, net = _lib.lib(), _net(20)
    N, S = 5, 7
    ndc, feat, dirs = _x(N, S, 20)
    big = torch.full((N * S + 8, 4), NAN, device=DEV)
    out = big[4:4 + N * S]
    n, f, d, r = ndc.data_ptr(), feat.data_ptr(), dirs.data_ptr(), out.data_ptr()
    refused = [
        ("odd F", 21, (n, 3, f, 21, d, 3, N, S, 0, r), EUNSUPPORTED),
        ("F = 0", 0, (n, 3, f, 20, d, 3, N, S, 0, r), EUNSUPPORTED),
        ("F = 42", 42, (n, 3, f, 42, d, 3, N, S, 0, r), EUNSUPPORTED),
        ("feat_stride < F", 20, (n, 3, f, 18, d, 3, N, S, 0, r), EINVAL),
        ("ndc_stride < 3", 20, (n, 2, f, 20, d, 3, N, S, 0, r), EINVAL),
        ("dirs_stride < 3", 20, (n, 3, f, 20, d, 2, N, S, 0, r), EINVAL),
        ("S = 0", 20, (n, 3, f, 20, d, 3, N, 0, 0, r), EINVAL),
        ("N < 0", 20, (n, 3, f, 20, d, 3, -1, S, 0, r), EINVAL),
        ("raw off 16-byte alignment", 20, (n, 3, f, 20, d, 3, N, S, 0, r + 4), EALIGN),
        ("raw off 16-byte alignment, sigma only", 20, (n, 3, f, 20, 0, 3, N, S, 1, r + 8), EALIGN),
    ]
    for what, F, io, want in refused:
        assert _entry(l, net, mode, F, io) == want, what
    torch.cuda.synchronize()
    assert bool(torch.isnan(big).all())
    # and the same arguments, put right, run
    assert _entry(l, net, mode, 20, (n, 3, f, 20, d, 3, N, S, 0, r)) == OK
    torch.cuda.synchronize()
    assert _bits(out, _dense(mode, N, S, 20)) and bool(torch.isnan(big[:4]).all()) and bool(torch.isnan(big[4 + N * S:]).all())
