"""dist.list_similar_targets_batch over shards in separate processes: spawned ranks with a gloo group share the one GPU of the test
box, each holding its part of the questions (the shape and seeds of test_gpu_record_ranks_procs.py).  Every rank must return the same
bytes, and the listing must be a valid top-k against the model of a whole engine's KB (test_gpu_similar_targets.py: the ranks' sums
use another summation order than the model, so values are held to the bar, not to equality).  A source id that is out of range on one
rank only must fail on every rank with the same text.  Every wait is bounded: the collectives time out, and the parent takes the
results with a time limit."""
import pytest

import ranks_common as rc
from test_gpu_record_ranks_procs import K, Q, T, TGAPS, engine_of

pytestmark = pytest.mark.gpu

SOURCES = [0, 100, 3, 9, 9, 55, 64, 31]
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
    got = pdist.list_similar_targets_batch(eng, SOURCES, MAX_COUNT, rank, world)
    res["listed"] = [[(t.i_target, t.prob) for t in x] for x in got]
    res["empty"] = pdist.list_similar_targets_batch(eng, [], MAX_COUNT, rank, world)
    bad = list(SOURCES)
    if rank == 1:
        bad[2] = T      # out of range on rank 1 only
    try:
        pdist.list_similar_targets_batch(eng, bad, MAX_COUNT, rank, world)
        res["raised"] = None
    except interop.PqaException as e:
        res["raised"] = str(e)
    again = pdist.list_similar_targets_batch(eng, SOURCES[:3], MAX_COUNT, rank, world)   # the ranks are still in step
    res["again"] = [[(t.i_target, t.prob) for t in x] for x in again]
    dist.destroy_process_group()
    eng.close()
    return res


@pytest.mark.parametrize("world", [2, 3])
def test_processes_list_over_gloo(world, factory):
    from test_gpu_similar_targets import model_rows, valid_top_k

    got = rc.run_ranks(_rank_main, world, (world, rc.free_port()))   # (every rank has reported before anything more is started on the device)
    whole = engine_of(0, Q)
    A, D, _ = whole.get_kb()
    whole.close()
    ref = model_rows(A, D, SOURCES, TGAPS, ())
    for k in range(world):
        assert got[k]["listed"] == got[0]["listed"] and got[k]["again"] == got[0]["listed"][:3], k
        assert got[k]["empty"] == []
        text = got[k]["raised"]
        assert text is not None and text.startswith("rank 1: ") and "entry=2" in text and "targetId=%d" % T in text, (k, text)
        assert text == got[0]["raised"], k
    for i, s in enumerate(SOURCES):
        valid_top_k((world, i), got[0]["listed"][i], ref[i], s, TGAPS, MAX_COUNT, Q, K)
