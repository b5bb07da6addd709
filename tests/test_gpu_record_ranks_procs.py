"""dist.record_answer_batch over shards in separate processes: spawned ranks with a gloo group share the one GPU of the test box,
each holding its part of the questions.  A scripted quiz loop -- set_active_question, then the collective, three rounds with the
questions crossing the ranks -- must leave on every rank the posteriors a whole engine has, bit for bit; and a batch that one rank
refuses must fail with the same text on every rank and leave the others' quizzes as they were.  Every wait is bounded: the
collectives time out, and the parent takes the results with a time limit."""
import numpy as np
import pytest

import ranks_common as rc

pytestmark = pytest.mark.gpu

K, Q, T, TGAPS = 5, 37, 101, (3, 17, 100)
N_QUIZZES, ROUNDS = 3, 3


def engine_of(first, limit):
    from probqa_amd import interop

    eng = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1), first, Q, 0)
    eng.fill_synthetic(8.0, 0.5, 5)       # (the same seed on every shard: each fills its part of the one cube)
    eng.set_target_gaps(list(TGAPS))
    eng.set_option("workers", 16)
    return eng


def script(world):
    """(questions, answers) per round: quiz i's question of round r lies on rank (i + r) % world."""
    from probqa_amd import dist as pdist

    bounds = pdist.shard_bounds(Q, world)
    firsts = [0] + bounds[:-1]
    rounds = []
    for r in range(ROUNDS):
        ranks = [(i + r) % world for i in range(N_QUIZZES)]
        rounds.append(([firsts[k] + (i + 5 * r) % (bounds[k] - firsts[k]) for i, k in enumerate(ranks)], [(2 * i + r) % K for i in range(N_QUIZZES)]))
    return rounds


def _rank_main(rank, world, port):
    import torch
    import torch.distributed as dist

    from probqa_amd import dist as pdist
    from probqa_amd import interop

    eng = engine_of(*pdist.shard_range(Q, world, rank))
    torch.cuda.set_device(0)
    rc.init_group("gloo", rank, world, port)
    quizzes = eng.start_quiz_batch(N_QUIZZES)
    res = {"posteriors": [], "active": []}
    for questions, answers in script(world):
        for quiz, q in zip(quizzes, questions):
            eng.set_active_question(quiz, q)
        pdist.record_answer_batch(eng, quizzes, answers, rank, world)
        res["posteriors"].append([eng.get_priors(q).tobytes() for q in quizzes])
        res["active"].append([eng.get_active_question_id(q) for q in quizzes])
    # desynchronised: on rank 1 only, quiz 1 has no active question
    questions, answers = script(world)[0]
    questions = [(q + 11) % Q for q in questions]
    for quiz, q in zip(quizzes, questions):
        eng.set_active_question(quiz, q)
    if rank == 1:
        eng.set_active_question(quizzes[1], -1)
    try:
        pdist.record_answer_batch(eng, quizzes, answers, rank, world)
        res["raised"] = None
    except interop.PqaException as e:
        res["raised"] = str(e)
    res["after_refusal"] = [eng.get_priors(q).tobytes() for q in quizzes]
    res["active_after_refusal"] = [eng.get_active_question_id(q) for q in quizzes]
    res["wanted_active"] = questions
    pdist.record_answer(eng, quizzes[0], answers[0], rank, world)      # the ranks are still in step: the batch of one goes through
    res["single"] = eng.get_priors(quizzes[0]).tobytes()
    dist.destroy_process_group()
    eng.close()
    return res


@pytest.mark.parametrize("world", [2, 3])
def test_processes_record_over_gloo(world, factory):
    rounds = script(world)
    from probqa_amd import dist as pdist

    bounds = pdist.shard_bounds(Q, world)
    for questions, _ in rounds:                    # the script crosses the ranks: no rank holds all of a round's questions
        assert len({pdist.owner_in(bounds, q) for q in questions}) >= 2, questions
    assert all(len({qs[i] for qs, _ in rounds} | {(rounds[0][0][i] + 11) % Q}) == ROUNDS + 1 for i in range(N_QUIZZES))
    got = rc.run_ranks(_rank_main, world, (world, rc.free_port()))   # (every rank has reported before anything more is started on the device)
    whole = engine_of(0, Q)
    quizzes = whole.start_quiz_batch(N_QUIZZES)
    for r, (questions, answers) in enumerate(rounds):
        for quiz, q in zip(quizzes, questions):
            whole.set_active_question(quiz, q)
        whole.record_answer_batch(quizzes, answers)
        want = [whole.get_priors(q) for q in quizzes]
        for k in range(world):
            for i in range(N_QUIZZES):
                assert np.array_equal(np.frombuffer(got[k]["posteriors"][r][i]), want[i]), (k, r, i)
            assert got[k]["active"][r] == [-1] * N_QUIZZES, (k, r)
    for k in range(world):
        text = got[k]["raised"]
        assert text is not None and text.startswith("rank 1: ") and "Batch entry 1: " in text and "active question" in text, (k, text)
        assert text == got[0]["raised"], k
        assert got[k]["after_refusal"] == got[k]["posteriors"][-1], k                 # nobody recorded anything
        want_active = list(got[k]["wanted_active"])
        if k == 1:
            want_active[1] = -1
        assert got[k]["active_after_refusal"] == want_active, k
    whole.set_active_question(quizzes[0], (rounds[0][0][0] + 11) % Q)
    whole.record_answer(quizzes[0], rounds[0][1][0])
    want = whole.get_priors(quizzes[0])
    for k in range(world):
        assert np.array_equal(np.frombuffer(got[k]["single"]), want), k
    whole.close()
