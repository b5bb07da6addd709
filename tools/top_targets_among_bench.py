"""What listing a quiz's best targets WITHIN A LISTED SET costs (a tool, not a test).  One process, one engine per shape; 256 quizzes
sharing one list; per list length two legs, interleaved round by round after a warm-up, medians with the spread (min..max):
  (a) PqaEngine_ListTopTargetsAmongBatch: the list staged once, level 0 gathers through it, records + count + mass per quiz come back;
  (b) today's way to the same listing: PqaEngine_ListTopTargetsBatch(quizzes, T) -- every posterior copied to the host -- and a filter
      on the host that keeps the listed targets, takes the first `top` and sums the listed probabilities.
Both legs go through the C ABI with their buffers built beforehand.  Before the timing the two listings are compared: the same
targets and probability bits wherever the listed probabilities differ from their neighbours (leg (b) lists equal probabilities in the
reference's heap order, leg (a) by ascending target), and masses within n * 2^-52 relative of each other.
Prints one JSON line per shape and list length.
usage: top_targets_among_bench.py [rounds=9]                    the two shapes 1000x5x1000 and 64x5x100000, lists of 16, 1000, 10000
       top_targets_among_bench.py Q K T rounds quizzes len...   one shape of your own (what the suite runs, tiny)"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probqa_amd import interop

WARMUP = 2
TOP = 10
RECORD = np.dtype([("t", "<i8"), ("p", "<f8")])


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


def run_shape(lib, f, Q, K, T, rounds, n, lengths):
    p64, pd, prec = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(interop.CiRatedTarget)
    eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
    if err is not None or eng is None:
        print(json.dumps({"shape": f"{Q}x{K}x{T}", "skipped": err.to_string(True) if err else "no engine"}), flush=True)
        return
    eng.fill_synthetic(8.0, 0.5, 7)
    eng.set_option("top_exact", 0)        # leg (b) in the order of leg (a): probability descending, target ascending
    quizzes = prepare(eng, Q, K, n, np.random.default_rng(3))
    c_quiz = (ctypes.c_int64 * n)(*quizzes)
    list_of = np.zeros(n, dtype=np.int64)
    got = np.zeros((n, TOP), dtype=RECORD)
    got_counts, mass = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64)
    full = np.zeros((n, T), dtype=RECORD)
    full_counts = np.zeros(n, dtype=np.int64)
    for length in lengths:
        if length > T:
            continue
        ids = np.ascontiguousarray(np.random.default_rng(1000 + length).permutation(T)[:length], dtype=np.int64)
        counts = np.array([length], dtype=np.int64)
        member = np.zeros(T, dtype=bool)
        member[ids] = True

        def leg_a():
            check(lib.PqaEngine_ListTopTargetsAmongBatch(eng.c_engine, n, c_quiz, list_of.ctypes.data_as(p64), 1, counts.ctypes.data_as(p64),
                                                         ids.ctypes.data_as(p64), TOP, got.ctypes.data_as(prec), got_counts.ctypes.data_as(p64),
                                                         mass.ctypes.data_as(pd)))
            return [got[i, :got_counts[i]].copy() for i in range(n)], mass.copy()

        def leg_b():
            check(lib.PqaEngine_ListTopTargetsBatch(eng.c_engine, n, c_quiz, T, full.ctypes.data_as(prec), full_counts.ctypes.data_as(p64)))
            lists, masses = [], np.zeros(n)
            for i in range(n):
                rec = full[i, :full_counts[i]]
                rec = rec[member[rec["t"]]]
                lists.append(rec[:TOP].copy())
                masses[i] = rec["p"].sum()
            return lists, masses

        la, ma = leg_a()
        lb, mb = leg_b()
        same = all(np.array_equal(x, y) for x, y in zip(la, lb))
        mass_ok = bool((np.abs(ma - mb) <= length * 2.0 ** -52 * np.maximum(ma, mb)).all())
        legs = {"a_among": leg_a, "b_today": leg_b}
        for fn in legs.values():
            for _ in range(WARMUP):
                fn()
        times = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t0)
        out = {"shape": f"{Q}x{K}x{T}", "quizzes": n, "list": length, "top": TOP, "rounds": rounds, "a_equals_b": same, "mass_agrees": mass_ok}
        for k, ts in times.items():
            out[k] = {"ms_median": round(statistics.median(ts) * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)}
        print(json.dumps(out), flush=True)
    eng.close()


def main():
    lib = interop.load_library()
    f = interop.PqaEngineFactory()
    if len(sys.argv) > 5:
        Q, K, T, rounds, n = (int(x) for x in sys.argv[1:6])
        run_shape(lib, f, Q, K, T, rounds, n, [int(x) for x in sys.argv[6:]])
        return
    rounds = max(9, int(sys.argv[1])) if len(sys.argv) > 1 else 9
    for Q, K, T in ((1000, 5, 1000), (64, 5, 100000)):
        run_shape(lib, f, Q, K, T, rounds, 256, [16, 1000, 10000])


if __name__ == "__main__":
    main()
