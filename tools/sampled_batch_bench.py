"""Selections per second of the reference's sampled selector for many quizzes (tools, not a test).  In one process, on one fp64
engine per shape, for each batch size it times four legs, interleaved round by round after a warm-up, and reports medians with
the spread (min..max) of the rounds:
  (a) consecutive PqaEngine_NextQuestionSampled calls, one per quiz;
  (b) PqaEngine_NextQuestionSampledBatch with option sampled_batch_host = 1 (the host's selector over the copied priorities);
  (c) PqaEngine_NextQuestionSampledBatch on the device (the selector launched behind the batched sweep);
  (d) PqaEngine_NextQuestionArgmaxBatch: the floor, the same sweep with the argmax pick.
Also the selector kernels' own time between events ("sampled_batch_device_ns" under option time_sweeps), measured in rounds of
their own so that the events do not sit in the timed legs.  Prints one JSON line per shape and batch size.
usage: sampled_batch_bench.py [Q K T [rounds=15]]   (default: 1000x5x1000 at 8, 32, 64, 256 quizzes and 10000x5x10000 at 64, 256)"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probqa_amd import interop

ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 15
if len(sys.argv) > 3:
    SHAPES = [((int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])), [8, 32, 64, 256])]
else:
    SHAPES = [((1000, 5, 1000), [8, 32, 64, 256]), ((10000, 5, 10000), [64, 256])]


def prepare(eng, Q, K, n, rng):
    """n quizzes with 0..5 answered questions each"""
    quizzes = eng.start_quiz_batch(n)
    for r in range(5):
        live = [q for j, q in enumerate(quizzes) if j % 6 > r]
        if not live:
            continue
        for q in live:
            eng.set_active_question(q, int(rng.integers(0, Q)) if r == 0 else eng.next_question_argmax(q))
        eng.record_answer_batch(live, [int(x) for x in rng.integers(0, K, size=len(live))])
    return quizzes


def main():
    f = interop.PqaEngineFactory()
    for (Q, K, T), sizes in SHAPES:
        eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
        assert err is None and eng is not None, err
        eng.fill_synthetic(8.0, 0.5, 7)
        rng = np.random.default_rng(3)
        quizzes = prepare(eng, Q, K, max(sizes), rng)
        for n in sizes:
            ids = quizzes[:n]
            rnds = [int(x) for x in rng.integers(0, 2**64, size=n, dtype=np.uint64)]

            def leg_a():
                for q, r in zip(ids, rnds):
                    eng.next_question_sampled(q, r)

            def leg_b():
                eng.set_option("sampled_batch_host", 1)
                return eng.next_question_sampled_batch(ids, rnds)

            def leg_c():
                eng.set_option("sampled_batch_host", 0)
                return eng.next_question_sampled_batch(ids, rnds)

            def leg_d():
                eng.next_question_argmax_batch(ids)

            legs = {"a_single_calls": leg_a, "b_batch_host": leg_b, "c_batch_device": leg_c, "d_argmax_batch": leg_d}
            for fn in legs.values():   # warm-up: buffers, attributes, clocks
                for _ in range(3):
                    fn()
            assert leg_b() == leg_c(), "host and device selectors disagree"
            times = {k: [] for k in legs}
            for _ in range(ROUNDS):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    fn()
                    times[k].append(time.perf_counter() - t0)
            eng.set_option("time_sweeps", 1)
            kernel_us = []
            for _ in range(ROUNDS):
                before = eng.get_option("sampled_batch_device_ns")
                leg_c()
                kernel_us.append((eng.get_option("sampled_batch_device_ns") - before) / 1e3)
            eng.set_option("time_sweeps", 0)
            out = {"shape": f"{Q}x{K}x{T}", "quizzes": n, "rounds": ROUNDS, "pick0": leg_c()[0]}
            for k, ts in times.items():
                out[k] = {"selections_per_s": round(n / statistics.median(ts)), "ms_median": round(statistics.median(ts) * 1e3, 4),
                          "ms_min": round(min(ts) * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)}
            out["selector_kernels_us"] = {"median": round(statistics.median(kernel_us), 2), "min": round(min(kernel_us), 2), "max": round(max(kernel_us), 2)}
            print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
