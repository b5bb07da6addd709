"""dist.review_answers_batch over shards in separate processes: spawned ranks with a gloo group share the one GPU of the test box, each
holding its part of the questions (the shape and seeds of test_gpu_record_ranks_procs.py).  The ranks resume one quiz of 17 answers through
dist.resume_quiz and record one more; every rank must return the same review, and it must be a whole engine's, bit for bit.  A position
that is out of range on one rank only must fail on every rank with the same text, and the ranks stay in step.  Every wait is bounded: the
collectives time out, and the parent takes the results with a time limit."""
import numpy as np
import pytest

import ranks_common as rc
from test_gpu_record_ranks_procs import K, Q, engine_of

pytestmark = pytest.mark.gpu

MAX_COUNT = 10
ANSWERS = [((5 * j + 3) % Q, (j * j + 1) % K) for j in range(17)]   # 17 answers, the questions on both ranks
POSITIONS = list(range(17)) + [4, 4, 16]


def plain(result):
    return [(np.float64(p.likelihood).tobytes(), np.float64(p.entropy).tobytes(), [(t.i_target, t.prob) for t in p.targets]) for p in result]


def _rank_main(rank, world, port):
    import torch
    import torch.distributed as dist

    from probqa_amd import dist as pdist
    from probqa_amd import interop

    eng = engine_of(*pdist.shard_range(Q, world, rank))
    torch.cuda.set_device(0)
    rc.init_group("gloo", rank, world, port)
    quiz = pdist.resume_quiz(eng, [interop.AnsweredQuestion(q, a) for q, a in ANSWERS], rank, world)
    other = eng.start_quiz()
    pairs = [(quiz, i) for i in POSITIONS]
    res = {"quiz": quiz}
    res["review"] = plain(pdist.review_answers_batch(eng, pairs, MAX_COUNT, rank, world))
    res["empty"] = pdist.review_answers_batch(eng, [], MAX_COUNT, rank, world)
    res["none"] = plain(pdist.review_answers_batch(eng, pairs[:2], 0, rank, world))
    bad = list(pairs)
    if rank == 1:
        bad[3] = (other, 0)            # a quiz without answers, on rank 1 only
    try:
        pdist.review_answers_batch(eng, bad, MAX_COUNT, rank, world)
        res["raised"] = None
    except interop.PqaException as e:
        res["raised"] = str(e)
    res["again"] = plain(pdist.review_answers_batch(eng, pairs[:3], MAX_COUNT, rank, world))   # the ranks are still in step
    res["answers"] = [(a.i_question, a.i_answer) for a in eng.get_quiz_answers(quiz)]
    res["priors"] = eng.get_priors(quiz).tobytes()
    dist.destroy_process_group()
    eng.close()
    return res


def test_processes_review_over_gloo(factory):
    from probqa_amd import interop

    world = 2
    got = rc.run_ranks(_rank_main, world, (world, rc.free_port()))   # (every rank has reported before anything more is started on the device)
    whole = engine_of(0, Q)
    quiz = whole.resume_quiz([interop.AnsweredQuestion(q, a) for q, a in ANSWERS])
    assert quiz == got[0]["quiz"] == got[1]["quiz"]
    pairs = [(quiz, i) for i in POSITIONS]
    want = plain(whole.review_answers_batch(pairs, MAX_COUNT))
    assert all(len(p[2]) == MAX_COUNT for p in want)
    none = plain(whole.review_answers_batch(pairs[:2], 0))
    priors = whole.get_priors(quiz).tobytes()
    whole.close()
    for k in range(world):
        assert got[k]["review"] == want and got[k]["again"] == want[:3] and got[k]["none"] == none, k
        assert got[k]["empty"] == []
        assert got[k]["answers"] == ANSWERS and got[k]["priors"] == priors, k
        text = got[k]["raised"]
        assert text is not None and text.startswith("rank 1: ") and "entry=3" in text and "position=0" in text, (k, text)
        assert text == got[0]["raised"], k
