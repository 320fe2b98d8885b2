"""The two order-independent gradient scatters, held to what they claim.

mvsnerf_volume_sample_bwd_det (csrc/sample.hip) against its integer definition, tests/scatter_det_refs.py: the 64-bit accumulators the kernel leaves in its
workspace, the max |g| word and the fp32 output are compared with torch.equal - no tolerance - and so are the properties that follow from integer sums: a
row permutation, rows that add zero, a power-of-two scale of the gradient.  A float addition hidden in the accumulation, another rounding or another scale
exponent changes bits and fails these (tests/test_scatter_det_refs.py shows that a float32 sum of the same products moves in 31-75 % of the elements under
the permutation used here).  ops.volume_grad_from_gathered_rows - the N-rank path - is held to "the single-call scatter of all rows, divided by world".

mvsnerf_planesweep_costvar_bwd_det (csrc/planesweep_bwd.hip) accumulates along a column in registers with v_rcp_f32, which a CPU restatement cannot follow bit for
bit: property tests only (power-of-two scales of either operand, torch.equal).

Both entries must hand an inf or NaN gradient on to the elements the float-atomic entries hand it to.  The only tolerance in this file is 3e-6 of the largest
finite magnitude, the project's bound for "fixed point against float atomics" (tests/test_gpu_backward.py), and it is used only against the float-atomic
kernels."""
import functools

import pytest
import torch

from tests import scatter_det_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOMIC_TOL = 3e-6

# (C, (D, H, W), P, extra columns of g): the last case hands the kernel the leading C columns of a wider tensor (g_stride = C + 4)
CASES = [(C, dims, P, 0) for C, dims, P in R.SHAPES] + [(8, (6, 7, 9), 5000, 4)]
IDS = [f"C{C}-{'x'.join(map(str, dims))}-P{P}" + ("-wide" if extra else "") for C, dims, P, extra in CASES]


def _dev_rows(g, extra=0):
    """g (P,C) on the GPU as the leading columns of a (P, C + extra) tensor whose other columns hold 2^20: read by mistake, they would change max |g|."""
    wide = torch.full((g.shape[0], g.shape[1] + extra), 2.0 ** 20)
    wide[:, :g.shape[1]] = g
    return wide.to(DEV), g.shape[1] + extra


def _det(ndc, g, dims, extra=0):
    """One call of the entry on a zeroed volume gradient and a zeroed caller-owned workspace -> (gvol, accumulators (D,H,W,C) int64, low word of ws[0]) on the CPU."""
    from mvsnerf_amd import _lib
    from mvsnerf_amd.ops import stream_ptr
    L = _lib.lib()
    D, H, W = dims
    P, C = g.shape
    words = L.mvsnerf_volume_sample_bwd_det_workspace_words(D, H, W, C)
    assert words == 8 + D * H * W * C
    gd, stride = _dev_rows(g, extra)
    nd = ndc.to(DEV)
    gv = torch.zeros((D, H, W, C), device=DEV)
    ws = torch.zeros(words, device=DEV, dtype=torch.int64)
    assert L.mvsnerf_volume_sample_bwd_det(D, H, W, C, nd.data_ptr(), P, gd.data_ptr(), stride, gv.data_ptr(), ws.data_ptr(), stream_ptr()) == 0
    ws = ws.cpu()
    assert not bool(ws[1:8].any())
    return gv.cpu(), ws[8:].view(D, H, W, C), int(ws[0]) & 0xFFFFFFFF, int(ws[0]) >> 32


def _atomic(ndc, g, dims, extra=0):
    from mvsnerf_amd import _lib
    from mvsnerf_amd.ops import stream_ptr
    D, H, W = dims
    P, C = g.shape
    gd, stride = _dev_rows(g, extra)
    nd = ndc.to(DEV)
    gv = torch.zeros((D, H, W, C), device=DEV)
    assert _lib.lib().mvsnerf_volume_sample_bwd(D, H, W, C, nd.data_ptr(), P, gd.data_ptr(), stride, gv.data_ptr(), stream_ptr()) == 0
    return gv.cpu()


@functools.lru_cache(maxsize=None)
def _case(i):
    """The inputs, the restatement's accumulators and the kernel's, once per case."""
    C, dims, P, extra = CASES[i]
    ndc, g = R.inputs(C, dims, P)
    acc, e = R.scatter_ints(ndc, g, dims)
    return dict(C=C, dims=dims, P=P, extra=extra, ndc=ndc, g=g, acc=acc, e=e, gpu=_det(ndc, g, dims, extra))


def _bits(x):
    return int(torch.tensor(float(x), dtype=torch.float32).view(torch.int32)) & 0xFFFFFFFF


# ------------------------------------------------------------------ the volume scatter against its integer definition
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_accumulators_and_output_are_the_integer_definition(i):
    """The kernel's fp32 coordinates, weights and products are plain IEEE operations (`fp contract(off)`), the ones torch's CPU fp32 performs: the accumulators
    are predicted exactly, not approached."""
    c = _case(i)
    out, acc, max_bits, high = c["gpu"]
    assert max_bits == _bits(c["g"].abs().max()) and high == 0
    diff = int((acc != c["acc"]).sum())
    print(f"[{IDS[i]}] accumulators that differ from the restatement: {diff} of {acc.numel()}; largest |accumulator| 2^{float(c['acc'].abs().max().double().log2()):.1f}")
    assert torch.equal(acc, c["acc"])
    assert torch.equal(out, R.finish(c["acc"], c["e"]))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_row_order_and_zero_rows_change_no_bit(i):
    c = _case(i)
    out, acc, max_bits, _ = c["gpu"]
    ndc, g = c["ndc"], c["g"]
    gen = torch.Generator().manual_seed(5)
    perm = torch.randperm(c["P"], generator=gen)
    out_p, acc_p, bits_p, _ = _det(ndc[perm], g[perm], c["dims"], c["extra"])
    assert bits_p == max_bits and torch.equal(acc_p, acc) and torch.equal(out_p, out)
    more = torch.rand((101, 3), generator=gen) * 1.1 - 0.05                     # rows whose gradient is zero, inside and outside the volume
    out_z, acc_z, bits_z, _ = _det(torch.cat([ndc, more]), torch.cat([g, torch.zeros((101, c["C"]))]), c["dims"], c["extra"])
    assert bits_z == max_bits and torch.equal(acc_z, acc) and torch.equal(out_z, out)


@pytest.mark.parametrize("k", [20, -30])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_a_power_of_two_scale_is_exact(i, k):
    """det(g * 2^k) = det(g) * 2^k: the exponent of max |g| moves by k, so every product lands on the same integer."""
    c = _case(i)
    out, acc, max_bits, _ = c["gpu"]
    out_k, acc_k, bits_k, _ = _det(c["ndc"], c["g"] * 2.0 ** k, c["dims"], c["extra"])
    assert bits_k == _bits(c["g"].abs().max() * 2.0 ** k)
    assert torch.equal(acc_k, acc)
    assert torch.equal(out_k, out * 2.0 ** k)


def test_an_all_zero_gradient_adds_nothing():
    c = _case(0)
    out, acc, max_bits, _ = _det(c["ndc"], torch.zeros_like(c["g"]), c["dims"])
    assert max_bits == 0 and not bool(acc.any()) and not bool(out.any())


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_a_non_finite_gradient_reaches_the_elements_it_reaches_with_float_atomics(i, bad):
    """One NaN or +inf in g: the elements mvsnerf_volume_sample_bwd makes non-finite - and no others - are non-finite here, and the finite ones agree with it
    to the float atomics' noise.  (Until this test existed the entry returned a volume gradient of zeros.)"""
    c = _case(i)
    ndc, dims, C = c["ndc"], c["dims"], c["C"]
    inside = ((ndc > 0.1) & (ndc < 0.9)).all(-1).nonzero().reshape(-1)           # a row with all eight corners in the volume, when there is one
    row = int(inside[len(inside) // 2]) if len(inside) else 0
    g = c["g"].clone()
    g[row, C - 3] = bad
    ref = _atomic(ndc, g, dims, c["extra"])
    out, acc, max_bits, _ = _det(ndc, g, dims, c["extra"])
    bad_ref, bad_out = ~torch.isfinite(ref), ~torch.isfinite(out)
    touched = any(bool(ok[row]) for ok, _, _ in R.corners(ndc, dims))
    print(f"[{IDS[i]}] row {row}: non-finite elements: float atomics {int(bad_ref.sum())}, fixed-point entry {int(bad_out.sum())}")
    assert bool(bad_ref.any()) == touched and (touched or c["P"] == 1)
    assert torch.equal(bad_out, bad_ref)
    assert max_bits >= 0x7F800000 and not bool(acc.any())                        # no scale exists: nothing went through the accumulators
    fin = ~bad_ref
    scale = float(ref[fin].abs().max())
    err = float((out[fin] - ref[fin]).abs().max())
    print(f"[{IDS[i]}] finite elements: max distance to the float-atomic entry {err / max(scale, 1e-30):.2e} of its largest finite magnitude")
    assert err <= ATOMIC_TOL * scale


@pytest.mark.parametrize("i", [j for j in range(len(CASES)) if not CASES[j][3]], ids=[n for n, c in zip(IDS, CASES) if not c[3]])
def test_the_python_switch_gives_the_bits_of_the_direct_call(i, monkeypatch):
    from mvsnerf_amd import ops
    c = _case(i)
    D, H, W = c["dims"]
    monkeypatch.setattr(ops, "VOLUME_BWD_DETERMINISTIC", True)
    gv = torch.zeros((D, H, W, c["C"]), device=DEV)
    ops._scatter_hip(gv, c["ndc"].to(DEV), c["g"].to(DEV))
    assert torch.equal(gv.cpu(), c["gpu"][0])


def test_the_accumulator_word_holds_the_largest_input_the_entry_accepts():
    """P = 2^22 points on ONE voxel with g = 1 - 2^-24, the largest value under 2^0: every contribution is 2^40 - 2^16, the sum 2^62 - 2^38 - the capacity
    the P cap is derived from - and the output 2^22 - 2^-2, exact in fp32."""
    P, dims = R.MAX_POINTS, (2, 2, 2)
    out, acc, max_bits, _ = _det(torch.zeros((P, 3)), torch.full((P, 4), 1.0 - 2.0 ** -24), dims)
    expect = torch.zeros((2, 2, 2, 4), dtype=torch.int64)
    expect[0, 0, 0] = P * (2 ** 40 - 2 ** 16)
    assert max_bits == _bits(1.0 - 2.0 ** -24)
    assert torch.equal(acc, expect)
    assert torch.equal(out, R.finish(expect, 0)) and float(out[0, 0, 0, 0]) == 2.0 ** 22 - 0.25


# ------------------------------------------------------------------ N ranks: ops.volume_grad_from_gathered_rows
def _shards(K):
    """Case 0's rows cut into uneven shards; from two ranks on, rank 1 holds only the single zero row a rank without samples enters with (ops._volume_grad)."""
    c = _case(0)
    g, ndc, P, C = c["g"], c["ndc"], c["P"], c["C"]
    holders = K if K == 1 else K - 1
    weights = torch.arange(1, holders + 1, dtype=torch.float64)
    cuts = [0] + [int(x) for x in (P * weights.cumsum(0) / weights.sum()).floor().tolist()]
    cuts[-1] = P
    shards = [(g[a:b], ndc[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    if K > 1:
        shards.insert(1, (torch.zeros((1, C)), torch.zeros((1, 3))))
    assert len(shards) == K and len({s[0].shape[0] for s in shards}) == K          # K different counts
    return shards


def _gathered(shards, C):
    """The buffer the all_gather leaves: rank r's rows at [r * width, r * width + cnts[r]).  The rows behind a rank's count and the pad column hold 7.0:
    scattered or read by mistake, they show."""
    cnts = [s[0].shape[0] for s in shards]
    width = max(cnts)
    allrows = torch.full((len(shards) * width, C + 4), 7.0)
    for r, (g, ndc) in enumerate(shards):
        allrows[r * width:r * width + cnts[r], :C] = g
        allrows[r * width:r * width + cnts[r], C:C + 3] = ndc
    return allrows.to(DEV), cnts, width


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_ranks_get_the_single_call_scatter_of_all_rows_divided_by_world(K, monkeypatch):
    """Under VOLUME_BWD_DETERMINISTIC: finish(scatter_ints(all valid rows)) / K bit for bit, whatever the order of the shards (the division is the fp32 one
    the helper performs, gvol.div_(K), applied here to the restated value).  With float atomics: the same value to their noise."""
    from mvsnerf_amd import ops
    c = _case(0)
    C, (D, H, W) = c["C"], c["dims"]
    shards = _shards(K)
    orders = [shards, shards[::-1], shards[1:] + shards[:1]]
    acc, e = R.scatter_ints(torch.cat([s[1] for s in shards]), torch.cat([s[0] for s in shards]), c["dims"])
    assert torch.equal(acc, c["acc"]) and e == c["e"]                              # the zero row adds nothing
    expect = R.finish(acc, e).to(DEV).div_(K).cpu()
    for flag in (True, False):
        monkeypatch.setattr(ops, "VOLUME_BWD_DETERMINISTIC", flag)
        for order in orders:
            gv = torch.zeros((D, H, W, C), device=DEV)
            got = ops.volume_grad_from_gathered_rows(*_gathered(order, C), gv)
            assert got is gv
            if flag:
                assert torch.equal(gv.cpu(), expect), f"K = {K}: {int((gv.cpu() != expect).sum())} elements differ from the single-call scatter / K"
            else:
                assert float((gv.cpu() - expect).abs().max()) <= ATOMIC_TOL * float(expect.abs().max())


# ------------------------------------------------------------------ the plane sweep: properties
PSW = [(3, 30, 41, 3, 10, True), (3, 24, 33, 2, 37, False)]
PSW_IDS = ["V3-30x41-D10-img", "V3-24x33-D37"]


@functools.lru_cache(maxsize=None)
def _psw_case(j):
    from mvsnerf_amd.synth import make_rig
    V, H, W, pad, D, with_img = PSW[j]
    bscale = (1.0, 6.0)[j]
    base = tuple(b * bscale for b in (0.0, 0.25, -0.25, 0.12, -0.12, 0.1, -0.3, 0.3, 0.2))
    rig = make_rig(H * 4, W * 4, n_views=V + 1, seed=77, baselines=base[:V + 1], rot_deg=2.0, smooth=True)
    proj = rig["proj_mats"][0, :V].contiguous().to(DEV)
    nf = rig["near_fars"][0, 0]
    depth = torch.linspace(float(nf[0]), float(nf[1]), D).to(DEV)
    g = torch.Generator().manual_seed(V * 100 + D)
    feats = torch.randn((V, H, W, 32), generator=g)
    CP = (32 + 3 * V + 3) // 4 * 4 if with_img else 32
    g_cost = torch.randn((D, H + 2 * pad, W + 2 * pad, CP), generator=g)
    c = dict(V=V, H=H, W=W, pad=pad, D=D, with_img=with_img, proj=proj, depth=depth, feats=feats, g_cost=g_cost, CP=CP, c_var=3 * V if with_img else 0)
    c["base"] = _psw(c, feats, g_cost, True)
    return c


def _psw(c, feats, g_cost, det):
    """mvsnerf_planesweep_costvar_bwd_det (V >= 2: its column form) or the float-atomic entry on zeroed gradients -> g_feats (V,H,W,32) on the CPU."""
    from mvsnerf_amd import _lib
    from mvsnerf_amd.ops import stream_ptr
    L = _lib.lib()
    V, H, W = c["V"], c["H"], c["W"]
    assert V >= 2
    f, gc = feats.to(DEV).contiguous(), g_cost.to(DEV).contiguous()
    gf = torch.zeros((V, H, W, 32), device=DEV)
    head = (f.data_ptr(), c["proj"].data_ptr(), c["depth"].data_ptr(), V, 32, H, W, c["D"], c["pad"], gc.data_ptr(), c["CP"], int(c["with_img"]), gf.data_ptr())
    if det:
        ws = torch.zeros(L.mvsnerf_planesweep_costvar_bwd_det_workspace_words(V, 32, H, W), device=DEV, dtype=torch.int64)
        assert L.mvsnerf_planesweep_costvar_bwd_det(*head, ws.data_ptr(), stream_ptr()) == 0
    else:
        assert L.mvsnerf_planesweep_costvar_bwd(*head, stream_ptr()) == 0
    return gf.cpu()


@pytest.mark.parametrize("j", range(len(PSW)), ids=PSW_IDS)
def test_planesweep_power_of_two_scale_of_the_cost_gradient_is_exact(j):
    c = _psw_case(j)
    assert float(c["base"].abs().max()) > 0
    assert torch.equal(_psw(c, c["feats"], c["g_cost"] * 2.0 ** 12, True), c["base"] * 2.0 ** 12)


@pytest.mark.parametrize("j", range(len(PSW)), ids=PSW_IDS)
def test_planesweep_power_of_two_scale_of_the_features_is_exact(j):
    """The gradient is linear in the features and the geometry does not depend on them."""
    c = _psw_case(j)
    assert torch.equal(_psw(c, c["feats"] * 2.0 ** -6, c["g_cost"], True), c["base"] * 2.0 ** -6)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("j", range(len(PSW)), ids=PSW_IDS)
def test_planesweep_non_finite_gradient_reaches_the_elements_it_reaches_with_float_atomics(j, bad):
    """One NaN or +inf in the variance channels of g_cost: the non-finite elements are those of mvsnerf_planesweep_costvar_bwd, the finite ones agree with it."""
    c = _psw_case(j)
    g_cost = c["g_cost"].clone()
    g_cost[c["D"] // 2, c["pad"] + c["H"] // 2, c["pad"] + c["W"] // 2, c["c_var"] + 5] = bad
    ref = _psw(c, c["feats"], g_cost, False)
    out = _psw(c, c["feats"], g_cost, True)
    bad_ref, bad_out = ~torch.isfinite(ref), ~torch.isfinite(out)
    print(f"[{PSW_IDS[j]}] non-finite elements: float atomics {int(bad_ref.sum())}, fixed-point entry {int(bad_out.sum())}")
    assert bool(bad_ref.any()) and torch.equal(bad_out, bad_ref)
    fin = ~bad_ref
    scale = float(ref[fin].abs().max())
    err = float((out[fin] - ref[fin]).abs().max())
    print(f"[{PSW_IDS[j]}] finite elements: max distance to the float-atomic entry {err / scale:.2e} of its largest finite magnitude")
    assert scale > 0 and err <= ATOMIC_TOL * scale
