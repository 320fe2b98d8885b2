"""The fp32 ray-march tile (mlp_fwd_pipe_tile, csrc/mlp.hip) computes a sample's bits from the sample alone.

The tile's instruction stream is laid out by hand in places: the DMA pieces of the next weight slab sit between the k-steps of the running GEMM.  Such a
reordering adds and removes no arithmetic, so a wrong one - a piece that lands in a buffer still being read, a barrier that no longer covers a fetch -
shows up as a dependence of a sample's result on WHERE it was computed (lane, wave, tile, ragged last tile) or WHEN (alone on its CU, next to a second
workgroup, in the second round of a grid).  Every comparison here is torch.equal.

1  position: 96 fixed samples (N = 96, S = 1: each has a direction of its own) behind k other samples, k = 0, 1, 37, 128, 133
2  company: 600 tiles in one launch against the same rays sent one ray (= one tile) per launch; the large launch twice
3  the one-launch path with the compositing outside the tile (S = 7, S = 200) behind a prefix of 3 rays
"""
import functools

import pytest
import torch

from tests.test_gpu_mlp_fold import _fwd, _fwd_train, _pack_stable, _weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = (0, 1, 37, 128, 133)
FS = (12, 20, 28, 32, 40)          # feature k-steps 8, 12, 16, 16, 20: three of gemm_stage's four bias-GEMM paths, both placements of the staged rows
N_FIXED = 96


# ------------------------------------------------------------------ 1: position
@functools.lru_cache(maxsize=None)
def _buffers(F):
    """folded Renderer_ours buffer, folded Renderer_linear buffer (same weights, the additive flag), unfolded stable buffer"""
    from mvsnerf_amd import ops
    ws, bs = _weights(F)
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    return {"v0": ops.mlp_pack(wd, bd, F), "v2": ops.mlp_pack(wd, bd, F, variant=1), "stable": _pack_stable(ws, bs, F)}


@functools.lru_cache(maxsize=None)
def _samples(F):
    """the 96 fixed samples and 133 others to put in front of them: (ndc (n,1,3), feat (n,1,F), dirs (n,3)) on the GPU"""
    g = torch.Generator().manual_seed(77 + F)
    n = N_FIXED + max(KS)
    ndc = torch.rand((n, 1, 3), generator=g)
    feat = torch.randn((n, 1, F), generator=g)
    dirs = torch.nn.functional.normalize(torch.randn((n, 3), generator=g), dim=-1)
    return tuple(t.to(DEV) for t in (ndc, feat, dirs))


def _behind(F, k):
    """k other samples, then the 96 fixed ones (the last 96 of _samples)"""
    n = N_FIXED + max(KS)
    idx = torch.cat([torch.arange(k), torch.arange(n - N_FIXED, n)]).to(DEV)
    return tuple(t[idx].contiguous() for t in _samples(F))


@pytest.mark.parametrize("variant", ["v0", "v2"])
@pytest.mark.parametrize("F", FS)
def test_bits_do_not_depend_on_position(F, variant):
    packed = _buffers(F)[variant]
    for alpha_only in (0, 1):
        base = _fwd(packed, F, _behind(F, 0), alpha_only)
        assert base.shape == (N_FIXED, 1 if alpha_only else 4) and bool(torch.isfinite(base).all())
        for k in KS[1:]:
            got = _fwd(packed, F, _behind(F, k), alpha_only)
            assert got.shape[0] == k + N_FIXED
            assert torch.equal(got[k:], base), (F, variant, alpha_only, k, float((got[k:] - base).abs().max()))


def test_training_forward_bits_do_not_depend_on_position():
    from mvsnerf_amd import _lib
    F = 20
    packed = _buffers(F)["stable"]
    blk = _lib.lib().mvsnerf_mlp_saved_floats(128) // 4            # one wave's (32 points') block of the activation store
    base_raw = _fwd(packed, F, _behind(F, 0))
    base_saved = None
    for k in KS:
        raw, saved = _fwd_train(packed, F, _behind(F, k))
        assert torch.equal(raw[k:], base_raw), (k, float((raw[k:] - base_raw).abs().max()))      # the no-grad kernel's bits on the unfolded buffer
        if k % 32 == 0:                                              # the fixed samples fill whole waves: their blocks are comparable
            mine = saved[(k // 32) * blk:(k // 32 + N_FIXED // 32) * blk]
            if base_saved is None:
                base_saved = mine.clone()
            assert mine.shape == base_saved.shape and torch.equal(mine.view(torch.int32), base_saved.view(torch.int32)), k


# ------------------------------------------------------------------ 2: company
N_BIG, S_BIG, EDGE = 600, 128, 16      # 600 tiles > 512: every CU holds two workgroups and a second round starts
CMP = ("raw", "weights", "alpha", "rgb_map", "depth", "input_feat")


@functools.lru_cache(maxsize=None)
def _big():
    from tests.test_gpu_raymarch_onelaunch import _hwdc, _inputs, _packed
    x = _inputs(N_BIG, S_BIG, seed=21)
    return _hwdc(x["vol"]), x, _packed(3)


def _march(vol_cl, x, packed, lo, hi):
    from mvsnerf_amd import ops
    with torch.no_grad():
        out = ops.raymarch(vol_cl, x["imgs"], x["w2cs"], x["Ks"], packed, x["pts"][lo:hi].contiguous(), x["ndc"][lo:hi].contiguous(),
                           x["z"][lo:hi].contiguous(), x["dirs"][lo:hi].contiguous(), want=())
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _big_out():
    vol_cl, x, packed = _big()
    return _march(vol_cl, x, packed, 0, N_BIG)


def _edge_rays():
    return list(range(EDGE)) + list(range(N_BIG - EDGE, N_BIG))


def test_onelaunch_tile_alone_and_in_company():
    vol_cl, x, packed = _big()
    big = _big_out()
    again = _march(vol_cl, x, packed, 0, N_BIG)
    for key in CMP + ("_dirs_tmp",):
        assert torch.equal(big[key], again[key]), key
    for r in _edge_rays():
        one = _march(vol_cl, x, packed, r, r + 1)
        for key in CMP:
            assert torch.equal(one[key][0], big[key][r]), (r, key, float((one[key][0] - big[key][r]).abs().max()))


def test_mlp_forward_tile_alone_and_in_company():
    _, x, packed = _big()
    big = _big_out()
    feat, dirs, ndc, F = big["input_feat"], big["_dirs_tmp"], x["ndc"], 20
    raw = _fwd(packed, F, (ndc, feat, dirs)).view(N_BIG, S_BIG, 4)
    assert torch.equal(raw, _fwd(packed, F, (ndc, feat, dirs)).view(N_BIG, S_BIG, 4))
    assert torch.equal(raw, big["raw"])                            # the one-launch path's bits (tests/test_gpu_raymarch_onelaunch.py), at this size
    for r in _edge_rays():
        one = _fwd(packed, F, (ndc[r:r + 1].contiguous(), feat[r:r + 1].contiguous(), dirs[r:r + 1].contiguous()))
        assert torch.equal(one.view(S_BIG, 4), raw[r]), (r, float((one.view(S_BIG, 4) - raw[r]).abs().max()))


# ------------------------------------------------------------------ 3: compositing outside the tile
@pytest.mark.parametrize("N,S", [(100, 7), (9, 200)])
def test_onelaunch_behind_a_prefix_of_rays(N, S):
    from tests.test_gpu_raymarch_onelaunch import _hwdc, _inputs, _packed
    k = 3
    x = _inputs(N + k, S, seed=S + 1)
    vol_cl, packed = _hwdc(x["vol"]), _packed(3)
    full, tail = _march(vol_cl, x, packed, 0, N + k), _march(vol_cl, x, packed, k, N + k)
    for key in CMP:
        assert tail[key].shape[0] == N
        assert torch.equal(full[key][k:], tail[key]), (key, float((full[key][k:] - tail[key]).abs().max()))
