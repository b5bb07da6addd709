"""dist.record_answer_page_batch over shards in separate processes: two spawned ranks with a gloo group share the one GPU of the test
box, each holding its part of the questions.  Pages that cross the ranks must leave on every rank the posteriors, answers and
likelihoods a whole engine has, bit for bit; and a page that one rank refuses must fail with the same text on both ranks and leave
both untouched.  Every wait is bounded: the collectives time out, and the parent takes the results with a time limit."""
import numpy as np
import pytest

import ranks_common as rc

pytestmark = pytest.mark.gpu

K, Q, T, TGAPS = 5, 37, 101, (3, 17, 100)
WORLD = 2
PAGES = [[], [(30, 1)], [(2, 0), (20, 3)], [(35, 2), (1, 1), (35, 4), (19, 0), (8, 2)]]
SECOND = [(4, 1), (33, 0), (18, 2)]


def engine_of(first, limit):
    from probqa_amd import interop

    eng = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1), first, Q, 0)
    eng.fill_synthetic(8.0, 0.5, 5)       # (the same seed on every shard: each fills its part of the one cube)
    eng.set_target_gaps(list(TGAPS))
    eng.set_option("workers", 16)
    return eng


def aq_lists(pages):
    from probqa_amd import interop

    return [[interop.AnsweredQuestion(q, a) for q, a in p] for p in pages]


def snapshot(eng, quizzes):
    return [(eng.get_priors(z).tobytes(), [(a.i_question, a.i_answer) for a in eng.get_quiz_answers(z)], eng.get_active_question_id(z)) for z in quizzes]


def _rank_main(rank, world, port):
    import torch
    import torch.distributed as dist

    from probqa_amd import dist as pdist
    from probqa_amd import interop

    eng = engine_of(*pdist.shard_range(Q, world, rank))
    torch.cuda.set_device(0)
    rc.init_group("gloo", rank, world, port)
    quizzes = eng.start_quiz_batch(len(PAGES))
    eng.set_active_question(quizzes[0], 9)
    res = {}
    res["likelihoods"] = pdist.record_answer_page_batch(eng, quizzes, aq_lists(PAGES), rank, world, likelihoods=True)
    res["first"] = snapshot(eng, quizzes)
    assert pdist.record_answer_page(eng, quizzes[1], aq_lists([SECOND])[0], rank, world) is None
    res["second"] = snapshot(eng, quizzes)
    # desynchronised: on rank 1 only, quiz 2 has been released
    if rank == 1:
        eng.release_quiz(quizzes[2])
    live = [z for i, z in enumerate(quizzes) if not (rank == 1 and i == 2)]
    before = snapshot(eng, live)
    try:
        pdist.record_answer_page_batch(eng, quizzes, aq_lists([[(1, 1)], [(2, 2)], [(25, 0)], []]), rank, world)
        res["raised"] = None
    except interop.PqaException as e:
        res["raised"] = str(e)
    res["untouched"] = snapshot(eng, live) == before
    dist.destroy_process_group()
    eng.close()
    return res


def test_processes_record_pages_over_gloo(factory):
    from probqa_amd import dist as pdist

    bounds = pdist.shard_bounds(Q, WORLD)
    for page in PAGES + [SECOND]:                   # the pages cross the ranks
        assert len(page) < 2 or len({pdist.owner_in(bounds, q) for q, _ in page}) == 2, page
    got = rc.run_ranks(_rank_main, WORLD, (WORLD, rc.free_port()))   # (every rank has reported before anything more is started on the device)
    whole = engine_of(0, Q)
    quizzes = whole.start_quiz_batch(len(PAGES))
    whole.set_active_question(quizzes[0], 9)
    want = whole.record_answer_page_batch(quizzes, aq_lists(PAGES), likelihoods=True)
    first = snapshot(whole, quizzes)
    whole.record_answer_page(quizzes[1], aq_lists([SECOND])[0])
    second = snapshot(whole, quizzes)
    assert first[0][2] == 9 and [s[2] for s in first[1:]] == [-1] * 3
    for k in range(WORLD):
        assert [np.asarray(l).tobytes() for l in got[k]["likelihoods"]] == [np.asarray(l).tobytes() for l in want], k
        assert got[k]["first"] == first and got[k]["second"] == second, k
        text = got[k]["raised"]
        assert text is not None and text.startswith("rank 1: ") and "entry=2" in text and "quizId=%d" % quizzes[2] in text, (k, text)
        assert text == got[0]["raised"] and got[k]["untouched"], k
    whole.close()
