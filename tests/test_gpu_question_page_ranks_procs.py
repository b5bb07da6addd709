"""dist.list_question_page_batch and dist.eval_conditional_gains_batch over shards in separate processes: spawned ranks with a gloo group
share the one GPU of the test box, each holding its part of the questions (the shape and seeds of test_gpu_record_ranks_procs.py).
Every rank's pages must be the whole engine's record for record, ids and bits; the ranks' Eval columns side by side must be the whole
engine's bytes.  A question that is out of range on one rank only must fail on every rank with the same text, and the ranks stay in
step.  Every wait is bounded: the collectives time out, and the parent takes the results with a time limit."""
import numpy as np
import pytest

import ranks_common as rc
from test_gpu_record_ranks_procs import Q, engine_of

pytestmark = pytest.mark.gpu

N_QUIZZES = 3
QUESTIONS, ANSWERS = [2, 20, 33], [1, 4, 0]          # one round of answers for the quizzes 1 .. 3, the questions on different ranks
GIVEN = [[], [30, 4], [16], [21, 21]]                # quiz 0 stays fresh; members on different ranks, a duplicate member


def bits_of(pages):
    return [[(int(q), np.float64(b).tobytes()) for q, b in page] for page in pages]


def _rank_main(rank, world, port):
    import torch
    import torch.distributed as dist

    from probqa_amd import dist as pdist
    from probqa_amd import interop

    eng = engine_of(*pdist.shard_range(Q, world, rank))
    torch.cuda.set_device(0)
    rc.init_group("gloo", rank, world, port)
    quizzes = eng.start_quiz_batch(N_QUIZZES + 1)
    for quiz, q in zip(quizzes[1:], QUESTIONS):
        eng.set_active_question(quiz, q)
    pdist.record_answer_batch(eng, quizzes[1:], ANSWERS, rank, world)
    res = {"quizzes": list(quizzes)}
    res["pages"] = bits_of(pdist.list_question_page_batch(eng, quizzes, 3, None, rank, world))
    res["given_pages"] = bits_of(pdist.list_question_page_batch(eng, quizzes, 2, GIVEN, rank, world))
    res["single"] = bits_of([pdist.list_question_page(eng, quizzes[2], 2, [30], rank, world)])
    res["eval"] = pdist.eval_conditional_gains_batch(eng, quizzes, GIVEN, rank, world).tobytes()
    res["eval_none"] = pdist.eval_conditional_gains_batch(eng, quizzes[:2], None, rank, world).tobytes()
    bad = [list(s) for s in GIVEN]
    if rank == 1:
        bad[1][0] = Q                  # out of range on rank 1 only (the sets keep their lengths: the packages are of one size)
    for name, call in (("page", lambda: pdist.list_question_page_batch(eng, quizzes, 2, bad, rank, world)),
                       ("eval", lambda: pdist.eval_conditional_gains_batch(eng, quizzes, bad, rank, world))):
        try:
            call()
            res[name + "_raised"] = None
        except interop.PqaException as e:
            res[name + "_raised"] = str(e)
        res[name + "_again"] = bits_of(pdist.list_question_page_batch(eng, quizzes[:2], 2, GIVEN[:2], rank, world))   # the ranks are still in step
    try:
        pdist.list_question_page_batch(eng, quizzes, 3, GIVEN, rank, world)        # 5^(2 + 2) rows: refused before any step
        res["limit"] = None
    except interop.PqaException as e:
        res["limit"] = str(e)
    res["priors"] = [eng.get_priors(q).tobytes() for q in quizzes]
    dist.destroy_process_group()
    eng.close()
    return res


@pytest.mark.parametrize("world", [2, 3])
def test_processes_list_pages_over_gloo(factory, world):
    from probqa_amd import dist as pdist

    got = rc.run_ranks(_rank_main, world, (world, rc.free_port()))   # (every rank has reported before anything more is started on the device)
    whole = engine_of(0, Q)
    quizzes = whole.start_quiz_batch(N_QUIZZES + 1)
    for quiz, q in zip(quizzes[1:], QUESTIONS):
        whole.set_active_question(quiz, q)
    whole.record_answer_batch(quizzes[1:], ANSWERS)
    pages = bits_of(whole.list_question_page_batch(quizzes, 3, None))
    given_pages = bits_of(whole.list_question_page_batch(quizzes, 2, GIVEN))
    single = bits_of([whole.list_question_page(quizzes[2], 2, [30])])
    rows = whole.eval_conditional_gains_batch(quizzes, GIVEN)
    rows_none = whole.eval_conditional_gains_batch(quizzes[:2], None)
    again = bits_of(whole.list_question_page_batch(quizzes[:2], 2, GIVEN[:2]))
    priors = [whole.get_priors(q).tobytes() for q in quizzes]
    whole.close()
    assert all(len(p) == 3 for p in pages) and all(len(p) == 2 for p in given_pages)
    firsts = [0] + pdist.shard_bounds(Q, world)[:-1]
    columns = lambda blob, n: np.frombuffer(blob, dtype=np.float64).reshape(n, -1)
    assert np.concatenate([columns(got[k]["eval"], len(quizzes)) for k in range(world)], axis=1).tobytes() == rows.tobytes()
    assert np.concatenate([columns(got[k]["eval_none"], 2) for k in range(world)], axis=1).tobytes() == rows_none.tobytes()
    for k in range(world):
        assert list(quizzes) == got[k]["quizzes"]
        assert columns(got[k]["eval"], len(quizzes)).shape[1] == pdist.shard_bounds(Q, world)[k] - firsts[k]
        assert got[k]["pages"] == pages and got[k]["given_pages"] == given_pages and got[k]["single"] == single, k
        assert got[k]["priors"] == priors, k
        for name in ("page", "eval"):
            text = got[k][name + "_raised"]
            assert text is not None and text.startswith("rank 1: ") and "questionId=%d" % Q in text, (k, name, text)
            assert text == got[0][name + "_raised"], (k, name)
            assert got[k][name + "_again"] == again, (k, name)
        assert got[k]["limit"] is not None and "entry=1" in got[k]["limit"] and "branches=" in got[k]["limit"], got[k]["limit"]
