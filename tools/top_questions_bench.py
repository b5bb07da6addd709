"""What the best N next questions of a quiz cost (tools, not a test).  In one process, on one engine per shape, it times three legs
per call, interleaved round by round after a warm-up, and reports medians with the spread (min..max) of the rounds:
  (a) what a client did before PqaEngine_ListTopQuestions: PqaEngine_EvalPriorities (or PqaEngine_EvalPrioritiesBatch) -- Q doubles
      per quiz copied to the host -- and numpy's partial sort there;
  (b) PqaEngine_ListTopQuestions / PqaEngine_ListTopQuestionsBatch with maxCount = 10: the same sweep, the listing behind it on the device;
  (c) PqaEngine_NextQuestionArgmax / PqaEngine_NextQuestionArgmaxBatch: the floor, a sweep with the one pick.
The engine has no counter for the listing kernels alone: (b) - (c) bounds them from above where both calls run the same sweep (one
quiz on a Double engine); for batches (c) may take another form of the sweep than (a) and (b), which want the priorities kept.
Prints one JSON line per shape and batch size.
usage: top_questions_bench.py [Q K T [rounds=15]]   (default: 1000x5x1000 and 10000x5x10000 at 1, 64 and 256 quizzes, then
12500x5x100000 fp32 at 256 quizzes if the device has the memory)"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probqa_amd import interop

ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 15
TOP = 10
if len(sys.argv) > 3:
    SHAPES = [((int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])), [1, 64, 256], False)]
else:
    SHAPES = [((1000, 5, 1000), [1, 64, 256], False), ((10000, 5, 10000), [1, 64, 256], False), ((12500, 5, 100000), [256], True)]


def host_top(pri, n):
    """numpy's partial sort: the n largest, then ordered by (-priority, index)"""
    idx = np.flatnonzero(pri > 0)
    if len(idx) > n:
        idx = idx[np.argpartition(-pri[idx], n - 1)[:n]]
    idx = idx[np.lexsort((idx, -pri[idx]))]
    return [(int(q), float(pri[q])) for q in idx]


def prepare(eng, Q, K, n, rng):
    """n quizzes with 0..5 answered questions each"""
    quizzes = eng.start_quiz_batch(n)
    for r in range(5):
        live = [q for j, q in enumerate(quizzes) if j % 6 > r]
        if not live:
            continue
        for q in live:
            eng.set_active_question(q, int(rng.integers(0, Q)))
        eng.record_answer_batch(live, [int(x) for x in rng.integers(0, K, size=len(live))])
    return quizzes


def main():
    f = interop.PqaEngineFactory()
    for (Q, K, T), sizes, fp32 in SHAPES:
        kw = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24) if fp32 else {}
        eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **kw))
        if err is not None or eng is None:
            print(json.dumps({"shape": f"{Q}x{K}x{T}", "skipped": err.to_string(True) if err else "no engine"}), flush=True)
            continue
        eng.fill_synthetic(8.0, 0.5, 7)
        rng = np.random.default_rng(3)
        quizzes = prepare(eng, Q, K, max(sizes), rng)
        for n in sizes:
            ids = quizzes[5:5 + n] if n == 1 else quizzes[:n]   # (one quiz: one with five answers)

            if n == 1:
                def leg_a():
                    return [host_top(eng.eval_priorities(ids[0]), TOP)]

                def leg_b():
                    return [eng.list_top_questions(ids[0], TOP)]

                def leg_c():
                    eng.next_question_argmax(ids[0])
            else:
                def leg_a():
                    pri = eng.eval_priorities_batch(ids)
                    return [host_top(pri[i], TOP) for i in range(n)]

                def leg_b():
                    return eng.list_top_questions_batch(ids, TOP)

                def leg_c():
                    eng.next_question_argmax_batch(ids)

            legs = {"a_eval_and_host_sort": leg_a, "b_list_top_questions": leg_b, "c_argmax": leg_c}
            for fn in legs.values():   # warm-up: buffers, attributes, clocks
                for _ in range(3):
                    fn()
            assert leg_a() == leg_b(), "the host's sort and the device's listing disagree"
            times = {k: [] for k in legs}
            for _ in range(ROUNDS):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    fn()
                    times[k].append(time.perf_counter() - t0)
            out = {"shape": f"{Q}x{K}x{T}", "precision": "fp32" if fp32 else "fp64", "quizzes": n, "top": TOP, "rounds": ROUNDS,
                   "host_bytes_a": 8 * Q * n, "host_bytes_b": 16 * TOP * n}
            for k, ts in times.items():
                out[k] = {"ms_median": round(statistics.median(ts) * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)}
            print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
