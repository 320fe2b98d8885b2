"""CPU-only: the float64 references of tests/mlp16_refs.py hold what tests/test_gpu_mlp16_f64.py relies on.

* three 8-bit pieces (truncated, as split8<3> cuts activations, or rounded, as the pack kernel cuts weights) sum to the fp32 value exactly, and a
  GEMM over all nine products of three pieces is the float64 GEMM (1e-12 relative);
* emulate("none") is exact(); a mode's kept products are the kernel header's (csrc/mlp_bf16.hip:546-556);
* the modes are far apart: mean errors E_1 > 10 E_2 > 100 E_3 at every F, swapping split3 for split2 or dropping one kept product moves E by
  more than 10x - the GPU tests' margin of 1.25 tells one mode's arithmetic from the next;
* every case of the GPU tests is alive: sigma > 0 on 40 .. 90 % of its points.
"""
import functools

import pytest
import torch

from tests import mlp16_refs as R

FS = [2, 10, 12, 16, 20, 28, 32, 34, 40]
SHAPES = [(5, 7), (37, 24), (3, 300), (300, 1)]
CASES = [(N, S, False) for (N, S) in SHAPES] + [(37, 24, True)]


@functools.lru_cache(maxsize=None)
def _errs(F):
    """E_M (rgb, sigma) of the three bf16 splits and the fp16 split at (37, 24)"""
    ws, bs = R.weights(F)
    x = R.inputs(37, 24, F)
    ref = R.exact(ws, bs, *x)
    return ref, {m: R.mean_errs(R.emulate(m, ws, bs, *x), ref) for m in ("split1", "split2", "split3", "fp16x3")}


def test_three_pieces_sum_to_the_fp32_value_exactly():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4096, generator=g) * torch.exp2(torch.randint(-20, 20, (4096,), generator=g).float())
    x = torch.cat([x, torch.tensor([0.0, 1.0, -1.0, 2.0 ** -126, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 255.0, 257.0, 65535.0])]).double()
    for rounding in (R.TRUNC, R.RN):
        p = R.pieces(x, 3, 8, rounding)
        assert torch.equal(p[0] + p[1] + p[2], x) and torch.equal((p[0] + p[1]) + p[2], x), rounding
        for k in range(3):          # each piece is a bf16 value: it survives the conversion
            assert torch.equal(p[k].float().to(torch.bfloat16).double(), p[k]), (rounding, k)
    # two pieces do not: the third is needed (a value with 24 significant bits)
    p = R.pieces(x, 2, 8, R.RN)
    assert not torch.equal(p[0] + p[1], x)
    # round to nearest EVEN, like v_cvt_pk_bf16_f32 and torch's conversion
    assert torch.equal(R.pieces(x, 1, 8, R.RN)[0], x.float().to(torch.bfloat16).double())
    in_range = (x.abs() > 1e-4) & (x.abs() < 6e4)          # fp16's normal range; the pieces have no exponent limit
    assert torch.equal(R.pieces(x, 1, 11, R.RN)[0][in_range], x.float().to(torch.float16).double()[in_range])


@pytest.mark.parametrize("F", [2, 20, 40])
def test_all_nine_products_of_three_pieces_are_the_float64_gemm(F):
    ws, bs = R.weights(F)
    ndc, feat, dirs = R.inputs(37, 24, F)
    spec3 = R.SPECS["split3"]
    for a, i in ((feat, 6), (R._embed(ndc).float(), 0), (torch.randn(64, 191, generator=torch.Generator().manual_seed(F)), 5)):
        want = torch.nn.functional.linear(a.double(), ws[i].double(), bs[i].double())
        got = R.piece_gemm(a.double(), ws[i].double(), bs[i], spec3, kept=R.ALL9)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        six = R.piece_gemm(a.double(), ws[i].double(), bs[i], spec3)
        assert 0 < float((six - want).abs().max()) <= 2.0 ** -20 * float(want.abs().max())      # the three dropped products: ~2^-24 of a term


@pytest.mark.parametrize("F", [2, 20, 34])
def test_emulation_without_rounding_is_the_exact_network(F):
    ws, bs = R.weights(F)
    x = R.inputs(5, 7, F)
    ref = R.exact(ws, bs, *x)
    assert ref.shape == (35, 4) and ref.dtype == torch.float64
    assert torch.equal(R.emulate("none", ws, bs, *x), ref)
    # pieces wide enough to hold an fp32 operand whole: the piece GEMM is the exact one but for the order of the float64 sums, and for the
    # rounding of the float64 ACTIVATIONS to 53 bits' worth of pieces
    got = R._network(ws, bs, *x, lambda a, i: R.piece_gemm(a, ws[i].double(), bs[i], ((2, 26, R.RN), (1, 24, R.RN), ((0, 0), (1, 0)))))
    assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max())


def test_kept_products_are_the_kernel_headers():
    assert R.SPECS["split1"][2] == ((0, 0),) and R.SPECS["bf16"] == R.SPECS["split1"]
    assert sorted(R.SPECS["split2"][2]) == [(0, 0), (0, 1), (1, 0)] == sorted(R.SPECS["fp16x3"][2])
    assert sorted(R.SPECS["split3"][2]) == sorted((i, j) for i in range(3) for j in range(3) if i + j < 3)      # "combined order < NS"
    assert R.SPECS["split3"][0][2] == R.TRUNC and R.SPECS["split3"][1][2] == R.RN


@pytest.mark.parametrize("F", FS)
def test_the_modes_are_an_order_of_magnitude_apart(F):
    _, E = _errs(F)
    for c, what in enumerate(("rgb", "sigma")):
        e1, e2, e3 = E["split1"][c], E["split2"][c], E["split3"][c]
        print(f"F={F} {what}: E_1 {e1:.3e} E_2 {e2:.3e} E_3 {e3:.3e}  E_1/E_2 {e1 / e2:.0f}  E_2/E_3 {e2 / e3:.0f}  fp16x3 {E['fp16x3'][c]:.3e}")
        assert e1 > 10 * e2 > 100 * e3 > 0, (what, e1, e2, e3)
        assert 10 * E["fp16x3"][c] < e2, (what, E["fp16x3"][c], e2)          # 22 significant bits against 16


@pytest.mark.parametrize("F", [12, 20, 34])
def test_one_dropped_product_moves_the_error_tenfold(F):
    ws, bs = R.weights(F)
    x = R.inputs(37, 24, F)
    ref, E = _errs(F)
    for mode, drop in (("split3", (1, 1)), ("split3", (0, 2)), ("split3", (2, 0)), ("split2", (0, 1)), ("split2", (1, 0)), ("fp16x3", (0, 1)), ("fp16x3", (1, 0))):
        kept = tuple(p for p in R.SPECS[mode][2] if p != drop)
        e = R.mean_errs(R.emulate(mode, ws, bs, *x, kept=kept), ref)
        for c in range(2):
            assert e[c] > 10 * E[mode][c], (mode, drop, c, e[c], E[mode][c])


@pytest.mark.parametrize("F", FS)
def test_every_case_is_alive(F):
    ws, bs = R.weights(F)
    assert all(w.dtype == torch.float32 and w.is_contiguous() for w in ws) and tuple(ws[6].shape) == (128, F)
    if F != 20:          # the checkpoint's own pairs but for pts_bias.weight
        ws20, bs20 = R.weights(20)
        assert all(torch.equal(ws[i], ws20[i]) for i in range(11) if i != 6) and all(torch.equal(a, b) for a, b in zip(bs, bs20))
    for N, S, wide in CASES:
        ndc, feat, dirs = R.inputs(N, S, F, wide)
        assert ndc.shape == (N, S, 3) and feat.shape == (N, S, F) and dirs.shape == (N, 3)
        if wide:
            assert float(ndc.min()) < -0.4 and float(ndc.max()) > 1.4
        ref = R.exact(ws, bs, ndc, feat, dirs)
        live = R.live_fraction(ref)
        assert 0.40 <= live <= 0.90, (N, S, F, wide, live)
        assert bool(torch.isfinite(ref).all()) and 0.0 <= float(ref[:, :3].min()) and float(ref[:, :3].max()) <= 1.0
        # (many colours saturate - the modulated trunk reaches 1e3 .. 1e4 on unit-normal features; the ones in between carry the rgb errors)
        mid = ((ref[:, :3] > 0.01) & (ref[:, :3] < 0.99)).double().mean()
        assert float(mid) > 0.05, (N, S, F, wide, float(mid))
