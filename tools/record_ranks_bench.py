"""Cost of RecordAnswer for a batch of quizzes over separately created shards (a tool, not a test).  One process, the shards side by
side on ONE device, the legs interleaved rep by rep, medians with min and max, in recorded answers/s (a call = the work of ALL
shards, one after another -- separate processes on separate devices would run them side by side, so this is an upper bound on the
device work and no model of the exchange):
  a  the single-quiz, caller-driven form, quiz by quiz: PqaEngine_RecordAnswer on the shard that holds the active question,
     PqaHip_RecordAnswerRemote on the others, the holder's posterior copied on the device into every other shard's buffer
  b  PqaHip_PackAnswerPosteriors on every shard (into one zero-filled tensor: the all-reduce's output) +
     PqaEngine_RecordAnswerBatchFromPosteriors on every shard
  c  PqaEngine_RecordAnswerBatch on the whole engine: the floor
and the package's size beside them.  Every round gives every quiz a new question, (quiz + round) % Q, so a round's questions lie on
every shard; setting the active questions is not timed.  After the first round the posteriors of a and b are held to c's, bit for
bit.  One JSON line per shard count.
usage: record_ranks_bench.py Q K T [shards=2,8] [batch=64] [reps=9]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probqa_amd import dist as pdist
from probqa_amd import interop

Q, K, T = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
SHARDS = [int(x) for x in (sys.argv[4] if len(sys.argv) > 4 else "2,8").split(",")]
B = int(sys.argv[5]) if len(sys.argv) > 5 else 64
REPS = int(sys.argv[6]) if len(sys.argv) > 6 else 9
SEED = 20261019
DEVICE = torch.device("cuda", 0)
assert REPS + 1 <= Q, "every round needs a new question per quiz"

factory = interop.PqaEngineFactory()


def engine(first, limit):
    e = factory.create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1), first, Q, 0)
    e.fill_synthetic(8.0, 0.5, SEED)
    return e


def stats(per_s):
    return {"median": round(statistics.median(per_s)), "min": round(min(per_s)), "max": round(max(per_s))}


for world in SHARDS:
    whole = engine(0, Q)
    single = [engine(*pdist.shard_range(Q, world, r)) for r in range(world)]      # leg a's shards
    packed = [engine(*pdist.shard_range(Q, world, r)) for r in range(world)]      # leg b's
    bounds = pdist.shard_bounds(Q, world)
    quizzes = whole.start_quiz_batch(B)
    for e in single + packed:
        assert e.start_quiz_batch(B) == quizzes
    pitch = packed[0].posterior_slot_bytes() // 8

    def leg_single(questions, answers):
        for quiz, q, a in zip(quizzes, questions, answers):
            owner = pdist.owner_in(bounds, q)
            for r, sh in enumerate(single):
                (sh.record_answer if r == owner else sh.record_answer_remote)(quiz, a)
            single[owner].synchronize()
            src, ld = single[owner].prior_device_ptr(quiz)
            for r, sh in enumerate(single):
                if r != owner:
                    dst, _ = sh.prior_device_ptr(quiz)
                    pdist.tensor_from_device_ptr(dst, ld, DEVICE).copy_(pdist.tensor_from_device_ptr(src, ld, DEVICE))
        torch.cuda.synchronize()

    def leg_packed(questions, answers):
        pkg = torch.zeros(B, pitch, dtype=torch.float64, device=DEVICE)
        torch.cuda.synchronize()
        for sh in packed:
            sh.pack_answer_posteriors(quizzes, answers, pkg.data_ptr())
        for sh in packed:
            sh.synchronize()
        for sh in packed:
            sh.record_answer_batch_from_posteriors(quizzes, answers, pkg.data_ptr())

    def leg_whole(questions, answers):
        whole.record_answer_batch(quizzes, answers)
        whole.synchronize()

    legs = {"a_single_quiz_form": (leg_single, single), "b_posterior_package": (leg_packed, packed), "c_whole_engine": (leg_whole, [whole])}
    times = {name: [] for name in legs}
    for rep in range(REPS + 1):          # (the first round warms up -- scratch grown -- and is the one that is checked)
        questions = [(i + rep) % Q for i in range(B)]
        answers = [(i + rep) % K for i in range(B)]
        for name, (fn, engines) in legs.items():
            for e in engines:
                for quiz, q in zip(quizzes, questions):
                    e.set_active_question(quiz, q)
            t0 = time.perf_counter()
            fn(questions, answers)
            dt = time.perf_counter() - t0
            if rep > 0:
                times[name].append(B / dt)
        if rep == 0:
            for quiz in quizzes:
                want = whole.get_priors(quiz)
                for sh in single + packed:
                    assert np.array_equal(sh.get_priors(quiz), want), quiz
    out = {"shape": "%dx%dx%d" % (Q, K, T), "shards": world, "batch": B, "reps": REPS, "package_bytes": 8 * pitch * B,
           "answers_per_s": {name: stats(v) for name, v in times.items()}}
    out["b_over_a"] = round(out["answers_per_s"]["b_posterior_package"]["median"] / out["answers_per_s"]["a_single_quiz_form"]["median"], 2)
    print(json.dumps(out), flush=True)
    for e in single + packed + [whole]:
        e.close()
