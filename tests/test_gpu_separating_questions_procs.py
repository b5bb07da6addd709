"""dist.list_separating_questions_batch over shards in separate processes: spawned ranks with a gloo group share the one GPU of the test
box, each holding its part of the questions (the shape and seeds of test_gpu_record_ranks_procs.py).  Every rank must return the same
records, and they must be a whole engine's listing record for record (a value needs nothing from another rank).  A target that is out
of range on one rank only must fail on every rank with the same text.  Every wait is bounded: the collectives time out, and the parent
takes the results with a time limit."""
import pytest

import ranks_common as rc
from test_gpu_record_ranks_procs import Q, T, engine_of

pytestmark = pytest.mark.gpu

GROUPS = [[0, 1], [5, 9, 20], [4, 4, 6], list(range(30, 94)), [1, 3, 2], [50, 60], [7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 19, 20, 21, 22, 23, 24]]
MAX_COUNT = 10


def _rank_main(rank, world, port):
    import torch
    import torch.distributed as dist

    from probqa_amd import dist as pdist
    from probqa_amd import interop

    eng = engine_of(*pdist.shard_range(Q, world, rank))
    torch.cuda.set_device(0)
    rc.init_group("gloo", rank, world, port)
    res = {}
    res["listed"] = pdist.list_separating_questions_batch(eng, GROUPS, MAX_COUNT, rank, world)
    res["empty"] = pdist.list_separating_questions_batch(eng, [], MAX_COUNT, rank, world)
    bad = [list(g) for g in GROUPS]
    if rank == 1:
        bad[2][1] = T      # out of range on rank 1 only
    try:
        pdist.list_separating_questions_batch(eng, bad, MAX_COUNT, rank, world)
        res["raised"] = None
    except interop.PqaException as e:
        res["raised"] = str(e)
    res["again"] = pdist.list_separating_questions_batch(eng, GROUPS[:3], MAX_COUNT, rank, world)   # the ranks are still in step
    dist.destroy_process_group()
    eng.close()
    return res


def test_processes_list_over_gloo(factory):
    world = 2
    got = rc.run_ranks(_rank_main, world, (world, rc.free_port()))   # (every rank has reported before anything more is started on the device)
    whole = engine_of(0, Q)
    want = whole.list_separating_questions_batch(GROUPS, MAX_COUNT)
    whole.close()
    assert all(len(x) == MAX_COUNT for i, x in enumerate(want) if i != 4) and want[4] == []      # (target 3 is a gap)
    for k in range(world):
        assert got[k]["listed"] == want and got[k]["again"] == want[:3], k
        assert got[k]["empty"] == []
        text = got[k]["raised"]
        assert text is not None and text.startswith("rank 1: ") and "entry=2" in text and "member=1" in text and "targetId=%d" % T in text, (k, text)
        assert text == got[0]["raised"], k
