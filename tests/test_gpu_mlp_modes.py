"""Renderer_ours.query under each ops.set_mlp_precision mode returns the bits of the mvsnerf_mlp_fwd* entry that the mode names, called directly
through _lib with weights packed here (the library maps a mode to a kernel in one place, Renderer_ours.packed_alt; ops.mlp_forward dispatches
on the keywords it returns).  Full queries and sigma-only queries (forward_alpha) both."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def net20():
    from tests.test_gpu_fp16x3 import _load_net
    return _load_net().nerf


@pytest.mark.parametrize("mode", ["auto", "fp32", "bf16", "bf16x3", "bf16x6", "fp16x3"])
def test_query_returns_the_bits_of_its_modes_entry(net20, mode):
    from mvsnerf_amd import _lib, ops
    N, S, F = 37, 24, 20
    g = torch.Generator().manual_seed(5)
    ndc = torch.rand((N, S, 3), generator=g).to(DEV)
    feat = torch.randn((N, S, F), generator=g).to(DEV)
    dirs = torch.nn.functional.normalize(torch.randn((N, 3), generator=g), dim=-1).to(DEV)
    weights = [l.weight.detach() for l in net20._linears()]
    packed = net20.packed(F)
    guard = torch.zeros(4, device=DEV, dtype=torch.int32)
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    with ops.mlp_precision(mode), torch.no_grad():
        for vd in (dirs, None):
            got = net20.query(ndc, feat, vd, N, S)
            want = torch.full_like(got, float("nan"))
            io = (ndc.data_ptr(), 3, feat.data_ptr(), F, 0 if vd is None else vd.data_ptr(), 3, N, S, int(vd is None), want.data_ptr())
            if mode == "fp32":
                rc = lib.mvsnerf_mlp_fwd(packed.data_ptr(), F, *io, st)
            elif mode == "bf16":
                rc = lib.mvsnerf_mlp_fwd_bf16(ops.mlp_pack_bf16(weights, F).data_ptr(), packed.data_ptr(), F, *io, st)
            elif mode == "auto":                 # no-grad default: the guarded fp16x3 sequence
                rc = lib.mvsnerf_mlp_fwd_guarded(ops.mlp_pack_split(weights, F, 18).data_ptr(), packed.data_ptr(), F, *io, guard.data_ptr(), st)
            else:
                n_split = {"bf16x3": 2, "bf16x6": 3, "fp16x3": 18}[mode]
                rc = lib.mvsnerf_mlp_fwd_split(ops.mlp_pack_split(weights, F, n_split).data_ptr(), packed.data_ptr(), F, n_split, *io, st)
            assert rc == 0
            assert got.shape == (N * S, 1 if vd is None else 4)
            assert torch.equal(got, want), (mode, vd is None)
