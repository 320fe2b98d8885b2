"""CPU-only: the torch restatement of early ray termination (tests/early_stop_refs.py) keeps the bound of DESIGN.md 4h.

w_s = alpha_s T_s = T_s - T_{s+1} + 1e-10 T_s, so the weights of the samples from a boundary b on sum to T_b - T_S + 1e-10 sum T_s < T_b (1 + S 1e-10);
a ray is stopped only where T_b < eps.  With colours in [0, 1] that bounds |rgb diff| and |acc diff| (either background: 1 - acc moves by the same
amount with the opposite sign, and rgb + (1 - acc) by at most the larger of the two), and with z > 0 the depth by eps max z."""
import functools

import pytest
import torch

from tests import early_stop_refs as E

S = 45                                       # no multiple of 8 or 32
EPSS = (0.0, 1e-3, 1e-2, 0.5)
GS = (1, 8, 32, S, S + 5)


@functools.lru_cache(maxsize=None)
def _case():
    g = torch.Generator().manual_seed(45)
    N = 400
    raw = torch.rand((N, S, 4), generator=g)
    scale = torch.rand((N, 1), generator=g) * 0.6                                     # mean sigma 0 .. 0.6: from transparent rays to rays opaque after a few samples
    raw[..., 3] = torch.empty((N, S)).exponential_(1.0, generator=g) * scale
    z = torch.sort(torch.rand((N, S), generator=g) * 3.0 + 2.0, 1)[0]
    return raw, z


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("eps", EPSS)
def test_restatement_keeps_the_bound(eps, G):
    raw, z = _case()
    zeroed, stop, und = E.early_stop(raw, eps, G)
    N = raw.shape[0]
    assert zeroed.shape == raw.shape and stop.shape == (N,) and und.shape == (N,) and und.dtype == torch.bool
    bs = E.boundaries(S, G)
    assert bs == [k * G for k in range(1, -(-S // G))]
    T = E.transmittance64(raw)
    for n in range(N):                                                                 # the rule, ray by ray
        first = next((b for b in bs if T[n, b] < eps), -1)
        assert int(stop[n]) == first
        cut = S if first < 0 else first
        assert torch.equal(zeroed[n, :cut], raw[n, :cut]) and not bool(zeroed[n, cut:].any())
    if eps == 0.0 or G >= S:
        assert torch.equal(zeroed, raw) and not bool((stop >= 0).any()) and not bool(und.any())
    elif eps >= 1e-2 and G <= 8:
        assert 0 < int((stop >= 0).sum()) < N                                          # rays do saturate, and not all of them
    bound = eps * (1.0 + S * 1e-10)
    for white in (False, True):
        rgb0, acc0, depth0, _ = E.composite64(raw, z, white)
        rgb1, acc1, depth1, _ = E.composite64(zeroed, z, white)
        assert float((rgb1 - rgb0).abs().max()) <= bound and float((acc1 - acc0).abs().max()) <= bound
        assert float((depth1 - depth0).abs().max()) <= bound * float(z.max())


def test_undecided_marks_a_transmittance_next_to_eps():
    raw = torch.zeros((3, 16, 4))
    raw[:, :8, 3] = torch.tensor([4.0, 4.60517, 5.0])[:, None] / 8                     # T(8) = e^-4, 0.01 to about 2e-7, e^-5
    zeroed, stop, und = E.early_stop(raw, 1e-2, 8)
    assert stop.tolist()[0] == -1 and stop.tolist()[2] == 8 and und.tolist() == [False, True, False]
    assert not bool(E.early_stop(raw, 0.0, 8)[2].any())


def test_a_nan_transmittance_never_stops():
    raw = torch.full((1, 16, 4), 2.0)
    raw[0, 1, 3] = float("nan")
    zeroed, stop, und = E.early_stop(raw, 0.5, 4)
    assert int(stop[0]) == -1 and torch.equal(zeroed.view(torch.int32), raw.view(torch.int32))
