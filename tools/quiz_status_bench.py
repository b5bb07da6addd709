"""What asking where a quiz stands costs (a tool, not a test).  One process, one Double engine per shape; per load three legs, interleaved
round by round after a warm-up, min / median / max:
  (a) the new call: PqaEngine_QuizStatusBatch with 4 levels (status loads), PqaEngine_RankTargetsBatch (the rank load);
  (b) today's best from calls that were there before: PqaHip_GetPriors per quiz -- T doubles to the host -- and numpy for entropy, mass,
      best target, candidates and the levels (status), or for the rank of each named target (ranks; one copy per distinct quiz);
  (c) PqaEngine_ListTopTargetsBatch(1) over the same quizzes: the floor of a launch that reads every posterior once.
Legs (a) and (c) are timed through the C ABI with their buffers built beforehand, as a C client pays for them; leg (b) through the
Python methods (its host work is part of what it costs).  Before the timing the legs are compared: counts, best targets, level counts
and ranks must be equal, entropies within 2 (T + 16) 2^-52 max(1, H) bits of each other -- reported as legs_agree.
Loads: 1, 64 and 256 quizzes (resumed from 1 .. 5 answers each) for the status; 256 ranks of 16 quizzes x 16 targets.
Shapes: 1000x5x1000 and 2000x5x100000 (questions x answers x targets).  Prints one JSON line per shape and load, then the table.
usage: quiz_status_bench.py [--quick] [rounds=9]      --quick: one small shape, 40x5x1300, for the suite"""
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
P64, PD = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)


def numpy_status(p, levels):
    c = p[p > 0]
    top = int(np.argmax(p)) if len(c) else -1
    return (float(-(c * np.log2(c)).sum()), float(c.sum()), float(p[top]) if len(c) else 0.0, top, len(c), [int((c >= lv).sum()) for lv in levels],
            [float(c[c >= lv].sum()) for lv in levels])


def numpy_ranks(p, targets):
    ids = np.arange(len(p))
    ok = p > 0
    rank = np.full(len(p), -1, dtype=np.int64)
    rank[ids[ok][np.lexsort((ids[ok], -p[ok]))]] = np.arange(int(ok.sum()))
    return [int(rank[t]) for t in targets]


def checked(err):
    if err:
        raise RuntimeError(interop.PqaError(err).to_string(True))


def raw_status(eng, quizzes, levels):
    lib = interop.load_library()
    qs, lv = np.array(quizzes, dtype=np.int64), np.array(levels, dtype=np.float64)
    status = (interop.CiHipQuizStatus * len(qs))()
    counts, mass = np.zeros(len(qs) * len(lv), dtype=np.int64), np.zeros(len(qs) * len(lv))
    return lambda: checked(lib.PqaEngine_QuizStatusBatch(eng.c_engine, len(qs), qs.ctypes.data_as(P64), len(lv), lv.ctypes.data_as(PD), status,
                                                         counts.ctypes.data_as(P64), mass.ctypes.data_as(PD)))


def raw_rank(eng, pairs):
    lib = interop.load_library()
    qs, ts = np.array([z for z, _ in pairs], dtype=np.int64), np.array([t for _, t in pairs], dtype=np.int64)
    prob, rank = np.zeros(len(qs)), np.zeros(len(qs), dtype=np.int64)
    return lambda: checked(lib.PqaEngine_RankTargetsBatch(eng.c_engine, len(qs), qs.ctypes.data_as(P64), ts.ctypes.data_as(P64), prob.ctypes.data_as(PD),
                                                          rank.ctypes.data_as(P64)))


def raw_top1(eng, quizzes):
    lib = interop.load_library()
    qs = np.array(quizzes, dtype=np.int64)
    records, counts = (interop.CiRatedTarget * len(qs))(), np.zeros(len(qs), dtype=np.int64)
    return lambda: checked(lib.PqaEngine_ListTopTargetsBatch(eng.c_engine, len(qs), qs.ctypes.data_as(P64), 1, records, counts.ctypes.data_as(P64)))


def timed(legs, rounds):
    for fn in legs.values():
        for _ in range(WARMUP):
            fn()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    return times


def report(out, times, rows):
    med = {k: statistics.median(ts) for k, ts in times.items()}
    for k, ts in times.items():
        out[k] = {"ms_min": round(min(ts) * 1e3, 4), "ms_median": round(med[k] * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)}
    out["b_over_a"] = round(med["b_get_priors_numpy"] / med["a_new_call"], 2)
    out["a_over_c"] = round(med["a_new_call"] / med["c_top1_floor"], 2)
    print(json.dumps(out), flush=True)
    rows.append("| %s | %s | %.3f | %.3f | %.3f | %.1f | %.2f |" % (out["shape"], out["load"], med["a_new_call"] * 1e3, med["b_get_priors_numpy"] * 1e3,
                                                                 med["c_top1_floor"] * 1e3, out["b_over_a"], out["a_over_c"]))


def run(f, Q, K, T, rounds, rows):
    eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
    if err is not None or eng is None:
        print(json.dumps({"shape": f"{Q}x{K}x{T}", "skipped": err.to_string(True) if err else "no engine"}), flush=True)
        return
    eng.fill_synthetic(8.0, 0.5, 7)
    eng.set_option("top_exact", 0)
    rng = np.random.default_rng(3)
    seqs = [[interop.AnsweredQuestion(int(q), int(rng.integers(K))) for q in rng.permutation(Q)[:1 + j % 5]] for j in range(256)]
    live = eng.resume_quiz_batch(seqs)
    levels = [0.5, 0.1, 1.0 / T, 0.0]
    bar = 2 * (T + 16) * 2.0 ** -52
    for n in (1, 64, 256):
        quizzes = live[:n]
        got = eng.quiz_status_batch(quizzes, levels)
        want = [numpy_status(eng.get_priors(z), levels) for z in quizzes]
        agree = all(abs(g.entropy - w[0]) <= bar * max(1.0, w[0]) and abs(g.mass - w[1]) <= bar * w[1] and g.top_prob == w[2] and
                    (g.i_top_target, g.n_candidates, g.level_counts) == (w[3], w[4], w[5]) for g, w in zip(got, want))
        legs = {"a_new_call": raw_status(eng, quizzes, levels), "b_get_priors_numpy": lambda: [numpy_status(eng.get_priors(z), levels) for z in quizzes],
                "c_top1_floor": raw_top1(eng, quizzes)}
        report({"shape": f"{Q}x{K}x{T}", "load": "status_%d_quizzes" % n, "entries": n, "levels": len(levels), "rounds": rounds, "legs_agree": bool(agree)},
               timed(legs, rounds), rows)
    pairs = [(z, int(t)) for z in live[:16] for t in rng.permutation(T)[:16]]
    got = eng.rank_targets_batch(pairs)
    want = [r for z in live[:16] for r in numpy_ranks(eng.get_priors(z), [t for zz, t in pairs if zz == z])]
    legs = {"a_new_call": raw_rank(eng, pairs),
            "b_get_priors_numpy": lambda: [numpy_ranks(eng.get_priors(z), [t for zz, t in pairs if zz == z]) for z in live[:16]],
            "c_top1_floor": raw_top1(eng, live[:16])}
    report({"shape": f"{Q}x{K}x{T}", "load": "rank_256_pairs_16_quizzes_x_16_targets", "entries": len(pairs), "levels": 0, "rounds": rounds,
            "legs_agree": bool([r for r, _ in got] == want)}, timed(legs, rounds), rows)
    eng.close()


def main():
    args = [a for a in sys.argv[1:] if a != "--quick"]
    quick = len(args) != len(sys.argv) - 1
    rounds = int(args[0]) if args else 9
    f = interop.PqaEngineFactory()
    rows = []
    for Q, K, T in ([(40, 5, 1300)] if quick else [(1000, 5, 1000), (2000, 5, 100000)]):
        run(f, Q, K, T, rounds, rows)
    print("| shape | load | (a) new call ms | (b) get_priors + numpy ms | (c) ListTopTargetsBatch(1) ms | b / a | a / c |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(r)


if __name__ == "__main__":
    main()
