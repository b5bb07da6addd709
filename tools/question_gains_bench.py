"""What the information gain of every question costs (a tool, not a test).  One process, one engine per shape; per batch of quizzes four
legs, interleaved round by round after a warm-up, min / median / max:
  (eval)  PqaEngine_EvalQuestionGainsBatch: a row of gains per quiz;
  (list)  PqaEngine_ListInformativeQuestionsBatch(10): the sweep and the listing kernels;
  (a)     the route to the same numbers from calls that were there before: PqaEngine_QuizStatusBatch plus PqaEngine_PreviewAnswersBatch
          (maxCount 0) over the questions of every quiz, composed on the host as H_now - sum_k likelihood_k H_k.  Where a shape has more
          than SAMPLE questions, SAMPLE of them are previewed and the time is SCALED by Q / SAMPLE: the row says so;
  (b)     PqaEngine_EvalPrioritiesBatch for the same quizzes: the floor of a launch that reads the same cube.
All legs go through the C ABI with their buffers built beforehand.  Before the timing eval is compared with leg (a) on the previewed
questions (eval_minus_a_max_bits; legs_agree: within 1e-9 bits on a Double engine, whose synthetic cube has D == sum_k A exactly; a Float
cube rounds D and A apart, so there the identity holds to fp32 rounding only and the difference is reported without a verdict).
Per shape the tool also derives what a pass over the cube makes of the device from the one-quiz eval: cube bytes / time and fp64
logarithms / time -- a Float engine reads half the bytes for the same logarithms, so the Float : Double ratio at equal shape says which of
the two binds.
Shapes: 1000x5x1000, 10000x5x10000, and a Float engine at the latter (questions x answers x targets); batches of 1 / 8 / 64 / 256 quizzes
(resumed from 1 .. 5 answers each).  Prints one JSON line per shape and batch, then the table.
usage: question_gains_bench.py [--quick] [rounds=9]      --quick: one small shape, 40x5x1300"""
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
SAMPLE = 1000     # questions per quiz that leg (a) previews at most
P64, PD = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)


def checked(err):
    if err:
        raise RuntimeError(interop.PqaError(err).to_string(True))


def raw_eval(eng, quizzes, Q):
    lib = interop.load_library()
    qs, out = np.array(quizzes, dtype=np.int64), np.zeros((len(quizzes), Q))
    return (lambda: checked(lib.PqaEngine_EvalQuestionGainsBatch(eng.c_engine, len(qs), qs.ctypes.data_as(P64), out.ctypes.data_as(PD), Q))), out


def raw_list(eng, quizzes, max_count):
    lib = interop.load_library()
    qs = np.array(quizzes, dtype=np.int64)
    records, counts = (interop.CiRatedQuestion * (len(qs) * max_count))(), np.zeros(len(qs), dtype=np.int64)
    return lambda: checked(lib.PqaEngine_ListInformativeQuestionsBatch(eng.c_engine, len(qs), qs.ctypes.data_as(P64), max_count, records, counts.ctypes.data_as(P64)))


def raw_status_preview(eng, quizzes, questions, K):
    """QuizStatusBatch + PreviewAnswersBatch(0) over `questions` of every quiz, composed into out[quiz][question of the sample]"""
    lib = interop.load_library()
    qs = np.array(quizzes, dtype=np.int64)
    status = (interop.CiHipQuizStatus * len(qs))()
    pq = np.repeat(qs, len(questions))
    pj = np.tile(np.array(questions, dtype=np.int64), len(qs))
    lik, ent = np.zeros(len(pq) * K), np.zeros(len(pq) * K)
    counts = np.zeros(len(pq) * K, dtype=np.int64)
    out = np.zeros((len(qs), len(questions)))

    def call():
        checked(lib.PqaEngine_QuizStatusBatch(eng.c_engine, len(qs), qs.ctypes.data_as(P64), 0, None, status, None, None))
        checked(lib.PqaEngine_PreviewAnswersBatch(eng.c_engine, len(pq), pq.ctypes.data_as(P64), pj.ctypes.data_as(P64), 0, lik.ctypes.data_as(PD),
                                                  ent.ctypes.data_as(PD), None, counts.ctypes.data_as(P64)))
        h = np.array([s.entropy for s in status])
        out[:] = h[:, None] - np.nansum((lik * ent).reshape(len(qs), len(questions), K), axis=2)

    return call, out


def raw_priorities(eng, quizzes, Q):
    lib = interop.load_library()
    qs, out = np.array(quizzes, dtype=np.int64), np.zeros((len(quizzes), Q))
    return lambda: checked(lib.PqaEngine_EvalPrioritiesBatch(eng.c_engine, len(qs), qs.ctypes.data_as(P64), out.ctypes.data_as(PD)))


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


def run(f, Q, K, T, f32, rounds, rows, derived):
    shape = "%dx%dx%d%s" % (Q, K, T, " float" if f32 else "")
    eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **(F32 if f32 else {})))
    if err is not None or eng is None:
        print(json.dumps({"shape": shape, "skipped": err.to_string(True) if err else "no engine"}), flush=True)
        return
    eng.fill_synthetic(8.0, 0.5, 7)
    rng = np.random.default_rng(3)
    seqs = [[interop.AnsweredQuestion(int(q), int(rng.integers(K))) for q in rng.permutation(Q)[:1 + j % 5]] for j in range(256)]
    live = eng.resume_quiz_batch(seqs)
    sample = sorted(int(q) for q in rng.permutation(Q)[:min(Q, SAMPLE)])
    scale = Q / len(sample)
    for n in (1, 8, 64, 256):
        quizzes = live[:n]
        ev, rows_out = raw_eval(eng, quizzes, Q)
        old, old_out = raw_status_preview(eng, quizzes, sample, K)
        ev()
        old()
        differ = float(np.abs(rows_out[:, sample] - old_out).max())
        agree = None if f32 else bool(differ <= 1e-9)   # (a Float cube rounds D and A apart: D == sum_k A holds to 2^-24 only, and so does the identity)
        legs = {"eval": ev, "list10": raw_list(eng, quizzes, 10), "a_status_preview": old, "b_priorities_floor": raw_priorities(eng, quizzes, Q)}
        times = timed(legs, rounds)
        med = {k: statistics.median(ts) for k, ts in times.items()}
        out = {"shape": shape, "quizzes": n, "rounds": rounds, "legs_agree": agree, "eval_minus_a_max_bits": differ, "a_sampled_questions": len(sample), "a_scaled_by": round(scale, 3)}
        for k, ts in times.items():
            out[k] = {"ms_min": round(min(ts) * 1e3, 4), "ms_median": round(med[k] * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)}
        a_ms = med["a_status_preview"] * 1e3 * scale
        out["a_scaled_ms_median"] = round(a_ms, 3)
        out["a_over_eval"] = round(a_ms / (med["eval"] * 1e3), 2)
        out["eval_over_b"] = round(med["eval"] / med["b_priorities_floor"], 2)
        print(json.dumps(out), flush=True)
        spread = lambda k: "%.3f (%.3f .. %.3f)" % (med[k] * 1e3, min(times[k]) * 1e3, max(times[k]) * 1e3)
        rows.append("| %s | %d | %s | %s | %.3f%s | %s | %.1f | %.2f |" % (shape, n, spread("eval"), spread("list10"), a_ms, " (scaled x%.0f)" % scale if scale > 1 else "",
                                                                        spread("b_priorities_floor"), out["a_over_eval"], out["eval_over_b"]))
        if n == 1:
            elem = 4 if f32 else 8
            derived.append({"shape": shape, "one_quiz_eval_ms": round(med["eval"] * 1e3, 4), "cube_GB": round(Q * (K + 1) * T * elem / 1e9, 4),
                            "cube_GB_per_s": round(Q * (K + 1) * T * elem / 1e9 / med["eval"], 1), "Glog2_per_s": round(Q * (K + 1) * T / 1e9 / med["eval"], 2)})
    eng.close()


def main():
    args = [a for a in sys.argv[1:] if a != "--quick"]
    quick = len(args) != len(sys.argv) - 1
    rounds = int(args[0]) if args else 9
    f = interop.PqaEngineFactory()
    rows, derived = [], []
    for Q, K, T, f32 in ([(40, 5, 1300, False)] if quick else [(1000, 5, 1000, False), (10000, 5, 10000, False), (10000, 5, 10000, True)]):
        run(f, Q, K, T, f32, rounds, rows, derived)
    print("| shape | quizzes | Eval ms median (min .. max) | List(10) ms | (a) status + previews ms | (b) EvalPrioritiesBatch ms | a / Eval | Eval / b |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(r)
    for d in derived:
        print(json.dumps(d))


if __name__ == "__main__":
    main()
