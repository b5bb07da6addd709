"""dist.list_top_questions / dist.list_top_questions_batch over shards in separate processes: two spawned ranks with a gloo group
share the one GPU of the test box, each holding half of the questions; both must return the same lists, equal to the whole engine's
in the parent.  Every wait is bounded: the collectives time out, and the parent takes the results with a time limit."""
import numpy as np
import pytest

import ranks_common as rc

pytestmark = pytest.mark.gpu

K, Q, T, SEED, WORLD = 5, 2300, 40, 31, 2
COUNTS = (1, 10, 256)


def _rank_main(rank, port):
    import torch
    import torch.distributed as dist

    from probqa_amd import dist as pdist
    from probqa_amd import interop

    first, limit = pdist.shard_range(Q, WORLD, rank)
    eng = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1), first, Q, 0)
    eng.fill_synthetic(8.0, 0.5, SEED)
    eng.set_option("workers", 16)
    torch.cuda.set_device(0)
    rc.init_group("gloo", rank, WORLD, port)
    quizzes = eng.start_quiz_batch(3)
    res = {"single": [pdist.list_top_questions(eng, quizzes[0], n) for n in COUNTS],
           "batch": [pdist.list_top_questions_batch(eng, quizzes, n) for n in COUNTS]}
    dist.destroy_process_group()
    eng.close()
    return res


def test_two_processes_list_over_gloo(factory):
    from probqa_amd import interop

    got = rc.run_ranks(_rank_main, WORLD, (rc.free_port(),))   # (both ranks have reported before anything more is started on the device)
    whole = factory.create_hip_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1), 0, Q, 0)
    whole.fill_synthetic(8.0, 0.5, SEED)
    whole.set_option("workers", 16)
    quizzes = whole.start_quiz_batch(3)
    bits = lambda lst: [(q, np.float64(p).view(np.int64)) for q, p in lst]   # noqa: E731
    for r in range(WORLD):
        for k, n in enumerate(COUNTS):
            assert bits(got[r]["single"][k]) == bits(whole.list_top_questions(quizzes[0], n)), (r, n)
            want = whole.list_top_questions_batch(quizzes, n)
            assert [bits(l) for l in got[r]["batch"][k]] == [bits(l) for l in want], (r, n)
    whole.close()
