"""ListTopQuestions, ListTopQuestionsBatch and ListTopTargets of DIFFERENT quizzes from three client threads at once, on the one-process
sharded engine (PQA_DEVICES=0,0,0) and on the plain one.  The sharded engine has every shard's listing in flight before it waits for
the first, so a shard's lock is free between the two halves of a listing: the single listing, the batch listing and the target listing
must each find their own results whatever ran in between.  Nothing changes a quiz here, so every call has one right answer, taken
beforehand on one thread; equality is exact."""
import threading

import numpy as np
import pytest

import cases
from probqa_amd import interop

pytestmark = pytest.mark.gpu

K, Q, T, ROUNDS = 5, 3000, 400, 25


def bits(lst):
    return [(int(i), np.float64(p).view(np.int64)) for i, p in lst]


@pytest.mark.parametrize("devices", ["0,0,0", None], ids=["sharded", "plain"])
def test_mixed_listings_from_three_threads(devices, factory, monkeypatch):
    if devices:
        monkeypatch.setenv("PQA_DEVICES", devices)
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
    assert err is None and eng is not None, err
    if devices:
        monkeypatch.delenv("PQA_DEVICES")
        assert eng.get_option("shards") == 3
    eng.fill_synthetic(8.0, 0.5, 11)
    eng.set_option("workers", cases.WORKERS)
    rng = np.random.default_rng(2)
    quizzes = eng.start_quiz_batch(8)
    for j, quiz in enumerate(quizzes):          # every quiz in a state of its own
        for q in rng.permutation(Q)[:j + 1]:
            eng.set_active_question(quiz, int(q))
            eng.record_answer(quiz, int(rng.integers(0, K)))
    single, batch, target = quizzes[0], quizzes[1:7], quizzes[7]
    jobs = {   # (10: the device's listing; 300: the host's prefix of the copied vector; 100 targets: the engine's own pinned lines)
        "single": lambda r: bits(eng.list_top_questions(single, 300 if r % 5 == 4 else 10)),
        "batch": lambda r: [bits(l) for l in eng.list_top_questions_batch(batch, 10)],
        "targets": lambda r: bits((t.i_target, t.prob) for t in eng.list_top_targets(target, 100)),
    }
    want = {name: [job(r) for r in range(ROUNDS)] for name, job in jobs.items()}
    assert len(want["single"][0]) == 10 and len(want["single"][4]) == 300 and len(want["targets"][0]) == 100
    start = threading.Barrier(len(jobs))
    wrong = []

    def client(name):
        try:
            start.wait(timeout=30)
            for r in range(ROUNDS):
                if jobs[name](r) != want[name][r]:
                    wrong.append((name, r))
        except Exception as e:  # noqa: BLE001 - reported by the assertion below
            wrong.append((name, repr(e)))

    threads = [threading.Thread(target=client, args=(name,)) for name in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert wrong == []
    eng.close()
