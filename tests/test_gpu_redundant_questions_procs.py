"""dist.list_redundant_questions_batch over shards in separate processes: spawned ranks with a gloo group share the one GPU of the test
box, each holding its part of the questions (the shape and seeds of test_gpu_record_ranks_procs.py).  Every rank must return the same
records, and they must be a whole engine's listing record for record (the summation over the targets does not depend on the split of
the question axis).  A source id that is out of range on one rank only must fail on every rank with the same text.  Every wait is
bounded: the collectives time out, and the parent takes the results with a time limit."""
import pytest

import ranks_common as rc
from test_gpu_record_ranks_procs import Q, engine_of

pytestmark = pytest.mark.gpu

SOURCES = [0, 36, 3, 9, 9, 18, 19, 12, 13, 24, 25]
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
    res["listed"] = pdist.list_redundant_questions_batch(eng, SOURCES, MAX_COUNT, rank, world)
    res["empty"] = pdist.list_redundant_questions_batch(eng, [], MAX_COUNT, rank, world)
    bad = list(SOURCES)
    if rank == 1:
        bad[2] = Q      # out of range on rank 1 only
    try:
        pdist.list_redundant_questions_batch(eng, bad, MAX_COUNT, rank, world)
        res["raised"] = None
    except interop.PqaException as e:
        res["raised"] = str(e)
    res["again"] = pdist.list_redundant_questions_batch(eng, SOURCES[:3], MAX_COUNT, rank, world)   # the ranks are still in step
    dist.destroy_process_group()
    eng.close()
    return res


@pytest.mark.parametrize("world", [2, 3])
def test_processes_list_over_gloo(world, factory):
    got = rc.run_ranks(_rank_main, world, (world, rc.free_port()))   # (every rank has reported before anything more is started on the device)
    whole = engine_of(0, Q)
    want = whole.list_redundant_questions_batch(SOURCES, MAX_COUNT)
    whole.close()
    assert all(len(x) == MAX_COUNT for x in want)
    for k in range(world):
        assert got[k]["listed"] == want and got[k]["again"] == want[:3], k
        assert got[k]["empty"] == []
        text = got[k]["raised"]
        assert text is not None and text.startswith("rank 1: ") and "entry=2" in text and "questionId=%d" % Q in text, (k, text)
        assert text == got[0]["raised"], k
