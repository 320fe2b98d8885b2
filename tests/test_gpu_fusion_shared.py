"""World size 2 on a ONE-GPU box (the pattern of tests/test_gpu_shared.py: two ranks share cuda:0, collectives over gloo staged through host memory):
MVSSystemFusion.fuse_local_volumes splits the three views 2 + 1 over the ranks and all-reduces the integer accumulators; both ranks end with the
single-process accumulators and volume, bit for bit."""
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _rank_body(rank, world, port, q):
    import torch.distributed as dist
    from mvsnerf_amd import distributed as D, ops
    from tests.test_gpu_fusion import fusion_system, fusion_views
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    res = {}
    try:
        ops.MLP_PRECISION = "fp32"
        scene = fusion_views()
        assert D.shard_range(len(scene[0]), world, rank) == ((0, 2), (2, 3))[rank]
        rec = []
        sysm, fuser = fusion_system(*scene, record=rec)
        res["local_adds"] = len(rec)
        with D.single_rank():
            one, fuser1 = fusion_system(*scene)
        res["accumulators_equal"] = bool(torch.equal(fuser.accumulators(), fuser1.accumulators()))
        res["header"] = (int(fuser.ws[0]), int(fuser.ws[1]))
        res["volume_equal"] = bool(torch.equal(sysm.volume.feat_volume, one.volume.feat_volume) and torch.equal(sysm.density_volume, one.density_volume))
        res["pose_equal"] = bool(torch.equal(sysm.pose_source_ref["w2cs"], one.pose_source_ref["w2cs"]))
        res["nonzero"] = bool(fuser.accumulators().any())
        q.put((rank, res))
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_fusion_two_ranks_on_one_gpu():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_body, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = [q.get(timeout=300) for _ in procs]
    [p.join(timeout=60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    for rank, r in sorted(res):
        print(f"rank {rank}: {r}")
        assert r["local_adds"] == (6, 3)[rank]                     # 2 + 1 views, three chunks each
        assert r["nonzero"] and r["accumulators_equal"] and r["volume_equal"] and r["pose_equal"]
        assert r["header"] == (0, 32)
