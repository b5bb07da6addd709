"""Cost of the sampled selector over separately created shards (a tool, not a test).  One process, the shards side by side on one
device, the legs interleaved rep by rep, medians with min and max, in selections/s (a selection = one quiz of one batch; a call = the
work of ALL shards, one after another -- separate processes on separate devices would run them side by side, so this is an upper bound
on the device work and no model of the exchange):
  a  PqaEngine_NextQuestionSampledBatch on the whole engine
  b  the same on the one-process sharded engine (PQA_DEVICES) with the same shard count
  c  PackSampledParts on every shard (into one tensor: the all-gather's output) + SampledPickFromParts on every shard +
     TakeSampledPicks on every shard
and the part's size beside them.  Before timing, b's and c's questions are held to a's for the random numbers 0 and 2^64 - 1, where
the pick does not depend on the last bits of a priority.  One JSON line per shard count.
usage: sampled_ranks_bench.py Q K T [shards=2,8] [batch=64] [reps=9]"""
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

factory = interop.PqaEngineFactory()
rng = np.random.default_rng(11)


def engine(first, limit):
    e = factory.create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1), first, Q, 0)
    e.fill_synthetic(8.0, 0.5, SEED)
    return e


def stats(per_s):
    return {"median": round(statistics.median(per_s)), "min": round(min(per_s)), "max": round(max(per_s))}


whole = engine(0, Q)
quizzes_w = whole.start_quiz_batch(B)
for world in SHARDS:
    shards = [engine(*pdist.shard_range(Q, world, r)) for r in range(world)]
    saved = os.environ.get("PQA_DEVICES")
    os.environ["PQA_DEVICES"] = ",".join(["0"] * world)
    try:
        one, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
        assert err is None, err
    finally:
        if saved is None:
            os.environ.pop("PQA_DEVICES", None)
        else:
            os.environ["PQA_DEVICES"] = saved
    one.fill_synthetic(8.0, 0.5, SEED)
    assert one.get_option("shards") == world
    quizzes_1 = one.start_quiz_batch(B)
    quizzes = [sh.start_quiz_batch(B) for sh in shards]
    words = shards[0].sampled_part_bytes() // 8
    parts = torch.zeros(world, B, words, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def leg_parts(rnds):
        for r, sh in enumerate(shards):
            sh.pack_sampled_parts(quizzes[r], parts[r].data_ptr())
        for sh in shards:
            sh.synchronize()
        picks = [sh.sampled_pick_from_parts(quizzes[r], rnds, parts.data_ptr(), r, world)[:, 1] for r, sh in enumerate(shards)]
        merged = pdist.merge_sampled_picks(picks)
        return [sh.take_sampled_picks(quizzes[r], merged) for r, sh in enumerate(shards)][0]

    legs = {
        "a_whole": lambda rnds: whole.next_question_sampled_batch(quizzes_w, rnds),
        "b_sharded_engine": lambda rnds: one.next_question_sampled_batch(quizzes_1, rnds),
        "c_parts": leg_parts,
    }
    for rnd in (0, 2**64 - 1):
        want = legs["a_whole"]([rnd] * B)
        assert legs["c_parts"]([rnd] * B) == want and legs["b_sharded_engine"]([rnd] * B) == want, rnd
    times = {name: [] for name in legs}
    for rep in range(REPS + 1):          # (the first round warms up: scratch grown)
        rnds = [int(x) for x in rng.integers(0, 2**64, size=B, dtype=np.uint64)]
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn(rnds)
            dt = time.perf_counter() - t0
            if rep > 0:
                times[name].append(B / dt)
    out = {"shape": "%dx%dx%d" % (Q, K, T), "shards": world, "batch": B, "reps": REPS, "part_bytes": 8 * words,
           "selections_per_s": {name: stats(v) for name, v in times.items()}}
    out["c_over_b"] = round(out["selections_per_s"]["c_parts"]["median"] / out["selections_per_s"]["b_sharded_engine"]["median"], 2)
    print(json.dumps(out), flush=True)
    for e in shards + [one]:
        e.close()
    del parts
whole.close()
