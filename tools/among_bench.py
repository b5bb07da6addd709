"""What choosing among a LIST of questions costs (a tool, not a test).  One process, one engine per shape; per batch size and list
length three legs, interleaved round by round after a warm-up, medians with the spread (min..max) of the rounds:
  (a) PqaEngine_NextQuestionArgmaxAmongBatch: one launch over the (quiz, question) pairs, the argmax per quiz behind it;
  (b) today's way to the same pick: PqaEngine_ListTopQuestionsBatch(256) and a filter on the host where every quiz finds a listed
      question among its 256 records, else PqaEngine_EvalPrioritiesBatch and an argmax over the list on the host;
  (c) PqaEngine_NextQuestionArgmaxBatch: the full sweep, the floor of a selection over the whole axis.
All legs go through the C ABI with their buffers built beforehand (a ctypes array of 2.5 million ids takes Python longer than any leg).
The same seeded list serves every leg; each line says whether (a) and (b) named the same questions before the timing.
Prints one JSON line per engine, batch size and list length.
usage: among_bench.py [rounds=9]   (Double engines at 1000x5x1000 and 10000x5x10000, a Float engine at 10000x5x10000; batches of
1, 64 and 256 quizzes; lists of 16, 256, Q/4 and Q questions per quiz)"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probqa_amd import interop

ROUNDS = max(9, int(sys.argv[1])) if len(sys.argv) > 1 else 9
WARMUP = 2
SHAPES = [((1000, 5, 1000), False), ((10000, 5, 10000), False), ((10000, 5, 10000), True)]
BATCHES = [1, 64, 256]
RECORD = np.dtype([("q", "<i8"), ("p", "<f8")])


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


def check(err):
    if err:
        raise RuntimeError(interop.PqaError(err).to_string(True))


def main():
    lib = interop.load_library()
    f = interop.PqaEngineFactory()
    p64, pd = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    for (Q, K, T), fp32 in SHAPES:
        kw = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24) if fp32 else {}
        eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **kw))
        if err is not None or eng is None:
            print(json.dumps({"shape": f"{Q}x{K}x{T}", "skipped": err.to_string(True) if err else "no engine"}), flush=True)
            continue
        eng.fill_synthetic(8.0, 0.5, 7)
        rng = np.random.default_rng(3)
        quizzes = prepare(eng, Q, K, max(BATCHES), rng)
        for n in BATCHES:
            ids = quizzes[5:5 + n] if n == 1 else quizzes[:n]   # (one quiz: one with five answers)
            c_quiz = (ctypes.c_int64 * n)(*ids)
            picked = np.zeros(n, dtype=np.int64)
            full = np.zeros((n, Q), dtype=np.float64)
            recs = np.zeros((n, 256), dtype=RECORD)
            rec_counts = np.zeros(n, dtype=np.int64)
            for length in sorted({min(16, Q), min(256, Q), Q // 4, Q}):
                lrng = np.random.default_rng(1000 + length)
                lists = np.stack([np.sort(lrng.permutation(Q)[:length]) for _ in range(n)]).astype(np.int64)
                counts = np.full(n, length, dtype=np.int64)
                member = np.zeros((n, Q), dtype=bool)
                member[np.arange(n)[:, None], lists] = True

                def leg_a():
                    check(lib.PqaEngine_NextQuestionArgmaxAmongBatch(eng.c_engine, n, c_quiz, counts.ctypes.data_as(p64), lists.ctypes.data_as(p64),
                                                                     picked.ctypes.data_as(p64)))
                    return picked.copy()

                def leg_b_top():
                    check(lib.PqaEngine_ListTopQuestionsBatch(eng.c_engine, n, c_quiz, 256, recs.ctypes.data_as(ctypes.POINTER(interop.CiRatedQuestion)),
                                                              rec_counts.ctypes.data_as(p64)))
                    out = np.full(n, -2, dtype=np.int64)            # -2: no listed question among the records
                    for i in range(n):
                        q = recs["q"][i, :rec_counts[i]]
                        hit = np.flatnonzero(member[i, q])
                        if len(hit):
                            out[i] = q[hit[0]]
                        elif rec_counts[i] < 256:
                            out[i] = -1                             # (the whole listing was seen)
                    return out

                def leg_b_eval():
                    check(lib.PqaEngine_EvalPrioritiesBatch(eng.c_engine, n, c_quiz, full.ctypes.data_as(pd)))
                    sub = np.take_along_axis(full, lists, axis=1)
                    best = sub.argmax(axis=1)                       # (lists ascending: the first of equal values is the lowest id)
                    return np.where(sub[np.arange(n), best] > 0, lists[np.arange(n), best], -1)

                def leg_c():
                    check(lib.PqaEngine_NextQuestionArgmaxBatch(eng.c_engine, n, c_quiz, picked.ctypes.data_as(p64)))

                top_suffices = bool((leg_b_top() != -2).all())
                leg_b = leg_b_top if top_suffices else leg_b_eval
                legs = {"a_among": leg_a, "b_today": leg_b, "c_full_sweep": leg_c}
                for fn in legs.values():   # warm-up: buffers, attributes, clocks
                    for _ in range(WARMUP):
                        fn()
                same = bool((leg_a() == leg_b()).all())            # (a Float engine's listing ranks by its fp32 sweep: may differ)
                times = {k: [] for k in legs}
                for _ in range(ROUNDS):
                    for k, fn in legs.items():
                        t0 = time.perf_counter()
                        fn()
                        times[k].append(time.perf_counter() - t0)
                out = {"shape": f"{Q}x{K}x{T}", "precision": "fp32" if fp32 else "fp64", "quizzes": n, "list": length, "rounds": ROUNDS,
                       "b_way": "list_top_256" if top_suffices else "eval_and_host_argmax", "a_equals_b": same}
                for k, ts in times.items():
                    out[k] = {"ms_median": round(statistics.median(ts) * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)}
                print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
