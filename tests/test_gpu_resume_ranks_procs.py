"""ResumeQuiz over shards in separate processes (probqa_amd/dist.py: resume_quiz, resume_quiz_batch, ShmRowExchange).  Two spawned
processes share the one GPU of the test box, each holding half of the questions; both must end with the posterior the parent's
whole engine computes, under the same quiz ids, and a failure on one rank must fail both and leave no quiz behind.  Every wait is
bounded: the ranks' collectives and flag waits time out, and the parent takes the results with a time limit."""
import os

import numpy as np
import pytest

import ranks_common as rc

pytestmark = pytest.mark.gpu

K, Q, T, SEED, WORLD = 5, 90, 700, 31, 2
SINGLE = [(3, 1), (80, 0), (44, 2), (45, 4), (3, 3), (61, 1), (12, 0)]
BATCH = [[(1, 0), (89, 1)], [], [(50, 2)], [(10, 3), (70, 4), (20, 0), (46, 1)]]


def _aqs(pairs):
    from probqa_amd import interop

    return [interop.AnsweredQuestion(q, a) for q, a in pairs]


def _quiz_count(eng):
    """How many quizzes the engine holds: the ids of this test stay below 32, and a released quiz's id answers with an error
    (released ids are reused last-in first-out, so the next id alone would not tell)."""
    from probqa_amd import interop

    live = 0
    for i in range(32):
        try:
            eng.get_priors(i)
            live += 1
        except interop.PqaException:
            pass
    return live


def _rank_main(rank, mode, arg):
    import torch
    import torch.distributed as dist

    from probqa_amd import dist as pdist
    from probqa_amd import interop

    first, limit = pdist.shard_range(Q, WORLD, rank)
    dev = rank if mode == "nccl" else 0
    eng = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1), first, Q, dev)
    eng.fill_synthetic(8.0, 0.5, SEED)
    eng.set_option("workers", 16)
    if mode in ("gloo", "nccl"):
        torch.cuda.set_device(dev)
        rc.init_group(mode, rank, WORLD, arg)
        single = lambda l: pdist.resume_quiz(eng, _aqs(l), rank, WORLD)                         # noqa: E731
        batch = lambda ls: pdist.resume_quiz_batch(eng, [_aqs(l) for l in ls], rank, WORLD)     # noqa: E731
        ex = None
    else:
        ex = pdist.ShmRowExchange(rank, WORLD, arg, eng.answer_row_slot_bytes(), 16)
        single = lambda l: ex.resume_quiz(eng, _aqs(l), timeout_s=60.0)                          # noqa: E731
        batch = lambda ls: ex.resume_quiz_batch(eng, [_aqs(l) for l in ls], timeout_s=60.0)      # noqa: E731
    res = {}
    quiz = single(SINGLE)
    res["single"] = (quiz, eng.get_priors(quiz))
    ids = batch(BATCH)
    res["batch"] = (ids, [eng.get_priors(q) for q in ids])
    res["again"] = single(SINGLE[:3])                      # (the second step of the exchange: the other half of the segment)
    # a failure on ONE rank: every target a gap there (I64Underflow); both must raise, neither keeps a quiz
    before = _quiz_count(eng)
    if rank == 1:
        eng.set_target_gaps(list(range(T)))
    errors = []
    for call in (lambda: single(SINGLE), lambda: batch(BATCH)):
        try:
            call()
            errors.append(None)
        except interop.PqaException as e:
            errors.append(str(e))
    res["errors"], res["before"], res["after"] = errors, before, _quiz_count(eng)
    if ex is not None:
        ex.close()
    else:
        dist.destroy_process_group()
    eng.close()
    return res


def _run_ranks(mode, arg):
    return rc.run_ranks(_rank_main, WORLD, (mode, arg))


def _check(got, factory, same_text):
    from probqa_amd import interop

    whole = factory.create_hip_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1), 0, Q, 0)
    whole.fill_synthetic(8.0, 0.5, SEED)
    whole.set_option("workers", 16)
    want_quiz = whole.resume_quiz(_aqs(SINGLE))
    want = whole.get_priors(want_quiz)
    want_ids = whole.resume_quiz_batch([_aqs(l) for l in BATCH])
    want_batch = [whole.get_priors(q) for q in want_ids]
    want_again = whole.resume_quiz(_aqs(SINGLE[:3]))
    whole.close()
    for r in range(WORLD):
        res = got[r]
        assert isinstance(res, dict), res
        assert res["single"][0] == want_quiz and np.array_equal(res["single"][1], want), r
        assert res["batch"][0] == want_ids, r
        for a, b in zip(res["batch"][1], want_batch):
            assert np.array_equal(a, b), r
        assert res["again"] == want_again
        assert all(e is not None and "rank 1" in e for e in res["errors"]), (r, res["errors"])
        if r == 1 or same_text:
            assert all("Max exponent" in e for e in res["errors"]), (r, res["errors"])
        assert res["after"] == res["before"] == want_again + 1, (r, res["before"], res["after"])
    if same_text:
        assert got[0]["errors"] == got[1]["errors"]


def test_two_processes_resume_over_gloo(factory):
    _check(_run_ranks("gloo", rc.free_port()), factory, True)


def test_two_processes_resume_through_shared_memory(factory):
    from probqa_amd import dist as pdist
    from probqa_amd import interop

    probe = factory.create_hip_engine(interop.EngineDefinition(K, Q // 2, T, init_amount=0.1), 0, Q, 0)
    slot = probe.answer_row_slot_bytes()
    probe.close()
    name = "test_%d" % os.getpid()
    path = "/dev/shm/pqa_rows_%s" % name
    with open(path, "wb") as f:                 # the segment exists (zeroed) before either rank opens it
        f.write(b"\0" * pdist.ShmRowExchange.size_for(WORLD, slot, 16))
    try:
        got = _run_ranks("shm", name)
    finally:
        os.unlink(path)
    _check(got, factory, False)


def test_two_processes_resume_over_rccl(factory):
    """The same with an NCCL (RCCL) group: the packages stay on the device."""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("one device: RCCL refuses two ranks on it (the gloo test runs the same helpers with the package through the host)")
    _check(_run_ranks("nccl", rc.free_port()), factory, True)
