"""The positional encoding of the fp32 MLP tiles, evaluated once per point (pe_all, csrc/mlp_fp32_dev.h), against the per-lane evaluation it
replaces (pe_operand): bit identity.

pe_operand makes both lanes of a point reduce the same 30 angles and evaluate both polynomials, one lane keeps sin and the other cos.  pe_all lets
each lane half evaluate 15 of the angles - multiplies and fmas packed two to an instruction - keep both values and trade with its partner lane
(v_permlane32_swap).  A packed fma is the IEEE fma per component, so every operand must have pe_operand's bits; mvsnerf_pe_operands_fwd writes
the 32 operands of both lane halves with either routine (variant 0: pe_operand, variant 1: pe_all).

A  variant 0 is what it says it is: deterministic, finite from operand 2 on whatever the coordinate (the clamp to +-65536 is written with
   fminf / fmaxf, which return the number when the other argument is NaN; +-inf and NaN therefore encode as the clamp's end points), operands 0 / 1
   are the raw coordinates, and on |angle| <= 1600 it is within 4e-7 of sin / cos in float64: three roundings of the reduced argument (half an ulp
   of pi/4, 3e-8, each), the cephes minimax error (< 6e-8) and four roundings of a value <= 1 in the two Horner chains (6e-8 each).
B  variant 1 has variant 0's bits on 4 096 points: uniform in [0, 1) and [-3, 3), and every one of 0.0, -0.0, 1.0, the fp32 neighbours of
   k pi/4 / 2^f (quadrant ties of rintf), 127.99, 128.0, 128.01 (the clamp at f = 9), +-1e30, +-inf, NaN in each coordinate.
C  the tile itself: mvsnerf_mlp_fwd and mvsnerf_mlp_fwd_train return the same raw, and the S_E block of the activation store holds variant 0's
   operands of the same points (N = 3, S = 32: one partial tile with a dead wave; N = 5, S = 64: two tiles and a half).
D  the entry refuses what it does not take.
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
P_POINTS = 4096
SLOTS_SAVED, S_E = 608, 0                   # csrc/mlp_layout.h


def _bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _specials():
    f32 = np.float32
    v = [0.0, -0.0, 1.0, 127.99, 128.0, 128.01, 1e30, -1e30, math.inf, -math.inf, math.nan]
    for k in (1, 2, 3, 5, 8, 41721):        # k pi/4 / 2^f and its two fp32 neighbours: rintf(x * 2/pi) at or next to a tie (odd k) / a quadrant edge
        for f in (0, 3, 9):
            x = f32(k * math.pi / 4 / 2.0 ** f)
            v += [float(np.nextafter(x, f32(-np.inf))), float(x), float(np.nextafter(x, f32(np.inf))), -float(x)]
    return np.array(v, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _points():
    """(4096, 3) fp32 on the device: every special value alone in each coordinate and in all three, then the two uniform families"""
    sp = torch.from_numpy(_specials())
    g = torch.Generator().manual_seed(20)
    rows = []
    for c in range(3):
        r = torch.rand((sp.numel(), 3), generator=g)
        r[:, c] = sp
        rows.append(r)
    rows.append(sp[:, None].expand(-1, 3).clone())
    n = P_POINTS - 4 * sp.numel()
    assert n >= 2048
    rows.append(torch.rand((n // 2, 3), generator=g))
    rows.append(torch.rand((n - n // 2, 3), generator=g) * 6.0 - 3.0)
    pts = torch.cat(rows).contiguous()
    assert pts.shape == (P_POINTS, 3)
    return pts.to(DEV)


def _operands(ndc, variant):
    from mvsnerf_amd import _lib, ops
    P = ndc.numel() // 3
    out = torch.full((P, 32, 2), float("nan"), device=DEV)
    ops.check(_lib.lib().mvsnerf_pe_operands_fwd(ndc.data_ptr(), P, variant, out.data_ptr(), ops.stream_ptr()), "pe_operands")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _ref():
    """variant 0 on the 4 096 points, computed once and left alone"""
    return _operands(_points(), 0)


# ------------------------------------------------------------------ A
def test_variant0_is_the_per_lane_encoding():
    pts, e = _points(), _ref()
    assert _bits(_operands(pts, 0), e)
    # operands 0 / 1: (x, y), (z, 0) - the raw coordinates, NaN and inf included
    zero = torch.zeros(P_POINTS, device=DEV)
    assert _bits(e[:, 0, 0], pts[:, 0]) and _bits(e[:, 0, 1], pts[:, 1]) and _bits(e[:, 1, 0], pts[:, 2]) and _bits(e[:, 1, 1], zero)
    enc = e[:, 2:, :]
    assert bool(torch.isfinite(enc).all())
    assert float(enc.abs().max()) <= 1.0 + 4e-7
    # (P, 30) angles, operand 2 + 3 f + c, clamped as the kernel clamps them (NaN -> the lower end point is one of the two values fmaxf may
    # not return: only finite coordinates are compared against float64)
    freq = (2.0 ** torch.arange(10, dtype=torch.float64, device=DEV)).view(1, 10, 1)
    ang = (pts.double().view(P_POINTS, 1, 3) * freq).reshape(P_POINTS, 30)
    ok = torch.isfinite(ang) & (ang.abs() <= 1600.0)
    err_s = ((enc[:, :, 0].double() - torch.sin(ang)).abs() * ok).nan_to_num(0.0)
    err_c = ((enc[:, :, 1].double() - torch.cos(ang)).abs() * ok).nan_to_num(0.0)
    print(f"pe variant 0: max abs err on |angle| <= 1600: sin {float(err_s.max()):.3e} cos {float(err_c.max()):.3e} ({int(ok.sum())} angles)")
    assert int(ok.sum()) > 100000
    assert float(err_s.max()) <= 4e-7 and float(err_c.max()) <= 4e-7


# ------------------------------------------------------------------ B
def test_packed_half_shared_encoding_has_the_per_lane_bits():
    want, got = _ref(), _operands(_points(), 1)
    bad = (want.view(torch.int32) != got.view(torch.int32)).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), want[tuple(bad[0])].item(), got[tuple(bad[0])].item())
    assert _bits(got, want)


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("N,S,F", [(3, 32, 20), (5, 64, 20)])
def test_tile_operands_and_training_forward(N, S, F):
    from tests.test_gpu_mlp_fold import _fwd, _fwd_train, _inputs, _net
    net = _net(F)
    x = tuple(t.to(DEV) for t in _inputs(N, S, F))
    P = N * S
    raw = _fwd(net["stable"], F, x)
    raw_t, saved = _fwd_train(net["stable"], F, x)
    assert raw.shape == (P, 4) and torch.equal(raw, raw_t) and _bits(raw, raw_t)
    assert torch.equal(_fwd(net["folded"], F, x)[:, 3], raw_t[:, 3])              # the folded no-grad tile shares everything up to sigma
    # S_E: saved[wave][slot t][lane = half * 32 + m] -> [point = wave * 32 + m][t][half]
    n_waves = (P + 127) // 128 * 4
    se = saved.view(n_waves, SLOTS_SAVED, 64)[:, S_E:S_E + 32, :].reshape(n_waves, 32, 2, 32).permute(0, 3, 1, 2).reshape(n_waves * 32, 32, 2)
    want = _operands(x[0].reshape(P, 3).contiguous(), 0)
    assert _bits(se[:P], want)
    assert _bits(se[:P], _operands(x[0].reshape(P, 3).contiguous(), 1))


# ------------------------------------------------------------------ D
def test_entry_argument_checks():
    from mvsnerf_amd import _lib, ops
    pts = _points()
    out = torch.zeros((64, 32, 2), device=DEV)
    f = _lib.lib().mvsnerf_pe_operands_fwd
    assert f(pts.data_ptr(), 33, 0, out.data_ptr(), ops.stream_ptr()) == -1          # not a multiple of 32: nothing is padded
    assert f(pts.data_ptr(), 32, 2, out.data_ptr(), ops.stream_ptr()) == -1
    assert f(None, 32, 0, out.data_ptr(), ops.stream_ptr()) == -1
    assert f(pts.data_ptr(), 32, 0, None, ops.stream_ptr()) == -1
    assert f(pts.data_ptr(), 0, 1, out.data_ptr(), ops.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
