"""dist.preview_answers_batch over shards in separate processes: spawned ranks with a gloo group share the one GPU of the test box, each
holding its part of the questions (the shape and seeds of test_gpu_record_ranks_procs.py).  Every rank must return the same previews, and
they must be a whole engine's, bit for bit.  A question that is out of range on one rank only must fail on every rank with the same
text, and the ranks stay in step.  Every wait is bounded: the collectives time out, and the parent takes the results with a time limit."""
import numpy as np
import pytest

import ranks_common as rc
from test_gpu_record_ranks_procs import K, Q, engine_of

pytestmark = pytest.mark.gpu

N_QUIZZES, MAX_COUNT = 3, 10
QUESTIONS, ANSWERS = [2, 20, 33], [1, 4, 0]          # one round of answers, the questions on different ranks
PREVIEWED = [0, 9, 18, 19, 30, 36, 2, 9]             # (quiz i % 3, question): both ranks' questions, an asked one, one twice


def plain(result):
    return [[(np.float64(p.likelihood).tobytes(), np.float64(p.entropy).tobytes(), [(t.i_target, t.prob) for t in p.targets]) for p in previews] for previews in result]


def _rank_main(rank, world, port):
    import torch
    import torch.distributed as dist

    from probqa_amd import dist as pdist
    from probqa_amd import interop

    eng = engine_of(*pdist.shard_range(Q, world, rank))
    torch.cuda.set_device(0)
    rc.init_group("gloo", rank, world, port)
    quizzes = eng.start_quiz_batch(N_QUIZZES)
    for quiz, q in zip(quizzes, QUESTIONS):
        eng.set_active_question(quiz, q)
    pdist.record_answer_batch(eng, quizzes, ANSWERS, rank, world)
    pairs = [(quizzes[i % N_QUIZZES], q) for i, q in enumerate(PREVIEWED)]
    res = {"quizzes": list(quizzes)}
    res["previews"] = plain(pdist.preview_answers_batch(eng, pairs, MAX_COUNT, rank, world))
    res["empty"] = pdist.preview_answers_batch(eng, [], MAX_COUNT, rank, world)
    res["none"] = plain(pdist.preview_answers_batch(eng, pairs[:2], 0, rank, world))
    bad = list(pairs)
    if rank == 1:
        bad[3] = (bad[3][0], Q)        # out of range on rank 1 only
    try:
        pdist.preview_answers_batch(eng, bad, MAX_COUNT, rank, world)
        res["raised"] = None
    except interop.PqaException as e:
        res["raised"] = str(e)
    res["again"] = plain(pdist.preview_answers_batch(eng, pairs[:3], MAX_COUNT, rank, world))   # the ranks are still in step
    res["priors"] = [eng.get_priors(q).tobytes() for q in quizzes]
    dist.destroy_process_group()
    eng.close()
    return res


def test_processes_preview_over_gloo(factory):
    world = 2
    got = rc.run_ranks(_rank_main, world, (world, rc.free_port()))   # (every rank has reported before anything more is started on the device)
    whole = engine_of(0, Q)
    quizzes = whole.start_quiz_batch(N_QUIZZES)
    assert list(quizzes) == got[0]["quizzes"] == got[1]["quizzes"]
    for quiz, q in zip(quizzes, QUESTIONS):
        whole.set_active_question(quiz, q)
    whole.record_answer_batch(quizzes, ANSWERS)
    pairs = [(quizzes[i % N_QUIZZES], q) for i, q in enumerate(PREVIEWED)]
    want = plain(whole.preview_answers_batch(pairs, MAX_COUNT))
    assert all(len(p[2]) == MAX_COUNT for previews in want for p in previews) and len(want[0]) == K
    none = plain(whole.preview_answers_batch(pairs[:2], 0))
    priors = [whole.get_priors(q).tobytes() for q in quizzes]
    whole.close()
    for k in range(world):
        assert got[k]["previews"] == want and got[k]["again"] == want[:3] and got[k]["none"] == none, k
        assert got[k]["empty"] == []
        assert got[k]["priors"] == priors, k
        text = got[k]["raised"]
        assert text is not None and text.startswith("rank 1: ") and "entry=3" in text and "questionId=%d" % Q in text, (k, text)
        assert text == got[0]["raised"], k
