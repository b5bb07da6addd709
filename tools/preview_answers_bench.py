"""What previewing every answer of a question costs (a tool, not a test).  One process, one engine per precision; per load two legs,
interleaved round by round after a warm-up, min / median / max:
  (a) PqaEngine_PreviewAnswersBatch: one call, K would-be posteriors per pair reduced on the device to likelihood, entropy and top 10;
  (b) today's best from calls that were there before: per pair K scratch quizzes by PqaEngine_ResumeQuizBatch, PqaEngine_SetActiveQuestion
      on each, PqaEngine_RecordAnswerBatch, PqaEngine_ListTopTargetsBatch, the posteriors copied out (get_priors) for the entropy on the
      host, and the scratch quizzes released.
The live quizzes are themselves resumed from their answer sequences, so leg (b)'s scratch quizzes start from the live quizzes' bits.
Leg (a) is timed through the C ABI with its buffers built beforehand, as a C client pays for it; leg (b) through the Python methods (its
host work -- the entropy of K copied posteriors per pair -- is part of what it costs).  Before the timing the legs are compared: the
records must be equal, the entropies within 2 (T + 16) 2^-52 max(1, H) bits of each other (each leg is held to (T + 16) 2^-52
max(1, H) of the model) -- reported as legs_agree.
Loads: 1 pair; 64 pairs of distinct quizzes; 256 pairs of 16 quizzes x 16 questions.  Top 10.  Double and Float engines.
Prints one JSON line per precision and load, with the bytes the rows kernel must touch -- per pair K + 2 rows read (the K answer rows and
the denominator row in the engine's element type, the posterior in fp64) and K rows written -- and their fraction of 8 TB/s at leg (a)'s
median.
usage: preview_answers_bench.py [Q K T [rounds=9]]      default 1000 5 1000"""
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
CHUNK = 256
PEAK = 8e12
F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)


def entropy_bits(p):
    v = p[p > 0]
    return float(-(v * np.log2(v)).sum())


def leg_today(eng, pairs, histories, K):
    """[(entropy, records)] per row, through scratch quizzes."""
    lists, questions, answers = [], [], []
    for quiz, q in pairs:
        for k in range(K):
            lists.append(histories[quiz])
            questions.append(q)
            answers.append(k)
    out = []
    for first in range(0, len(lists), CHUNK):
        scratch = eng.resume_quiz_batch(lists[first:first + CHUNK])
        for z, q in zip(scratch, questions[first:first + CHUNK]):
            eng.set_active_question(z, q)
        eng.record_answer_batch(scratch, answers[first:first + CHUNK])
        listed = eng.list_top_targets_batch(scratch, TOP)
        for z, lst in zip(scratch, listed):
            out.append((entropy_bits(eng.get_priors(z)), [(t.i_target, t.prob) for t in lst]))
        for z in scratch:
            eng.release_quiz(z)
    return out


def leg_preview(eng, pairs):
    return [(p.entropy, [(t.i_target, t.prob) for t in p.targets]) for previews in eng.preview_answers_batch(pairs, TOP) for p in previews]


def raw_preview(eng, pairs, K):
    """Leg (a) as a C client pays for it: the call through the C ABI with its buffers built beforehand."""
    import ctypes

    p64, pd = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    lib = interop.load_library()
    n = len(pairs)
    quizzes, questions = np.array([z for z, _ in pairs], dtype=np.int64), np.array([q for _, q in pairs], dtype=np.int64)
    likelihood, entropy, counts = np.zeros(n * K), np.zeros(n * K), np.zeros(n * K, dtype=np.int64)
    records = (interop.CiRatedTarget * (n * K * TOP))()

    def call():
        err = lib.PqaEngine_PreviewAnswersBatch(eng.c_engine, n, quizzes.ctypes.data_as(p64), questions.ctypes.data_as(p64), TOP, likelihood.ctypes.data_as(pd),
                                                entropy.ctypes.data_as(pd), records, counts.ctypes.data_as(p64))
        if err:
            raise RuntimeError(interop.PqaError(err).to_string(True))

    return call


def run(f, Q, K, T, rounds, f32):
    eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **(F32 if f32 else {})))
    precision = "float" if f32 else "double"
    if err is not None or eng is None:
        print(json.dumps({"shape": f"{Q}x{K}x{T}", "precision": precision, "skipped": err.to_string(True) if err else "no engine"}), flush=True)
        return
    eng.fill_synthetic(8.0, 0.5, 7)
    eng.set_option("top_exact", 0)        # leg (b) in the order of leg (a): probability descending, target ascending
    rng = np.random.default_rng(3)
    # 64 live quizzes, resumed from 1 .. 5 answers each
    seqs = [[interop.AnsweredQuestion(int(q), int(rng.integers(K))) for q in rng.permutation(Q)[:1 + j % 5]] for j in range(64)]
    live = eng.resume_quiz_batch(seqs)
    histories = dict(zip(live, seqs))
    nq = min(16, Q)
    loads = {
        "1_pair": [(live[0], int(rng.integers(Q)))],
        "64_pairs_distinct_quizzes": [(z, int(rng.integers(Q))) for z in live],
        "256_pairs_16_quizzes_x_16_questions": [(z, int(q)) for z in live[:16] for q in rng.permutation(Q)[:nq]],
    }
    elem = 4 if f32 else 8
    for name, pairs in loads.items():
        a, b = leg_preview(eng, pairs), leg_today(eng, pairs, histories, K)
        agree = len(a) == len(b) and all(ra == rb and abs(ha - hb) <= 2 * (T + 16) * 2.0 ** -52 * max(1.0, hb) for (ha, ra), (hb, rb) in zip(a, b))
        legs = {"a_preview": raw_preview(eng, pairs, K), "b_today": lambda: leg_today(eng, pairs, histories, K)}
        for fn in legs.values():
            for _ in range(WARMUP):
                fn()
        times = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t0)
        touched = len(pairs) * T * ((K + 1) * elem + 8 + K * 8)
        med = {k: statistics.median(ts) for k, ts in times.items()}
        out = {"shape": f"{Q}x{K}x{T}", "precision": precision, "load": name, "pairs": len(pairs), "rows": len(pairs) * K, "top": TOP, "rounds": rounds,
               "legs_agree": bool(agree)}
        for k, ts in times.items():
            out[k] = {"ms_min": round(min(ts) * 1e3, 4), "ms_median": round(med[k] * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)}
        out["b_over_a"] = round(med["b_today"] / med["a_preview"], 2)
        out["rows_kernel_bytes"] = touched
        out["fraction_of_8TBps"] = touched / med["a_preview"] / PEAK
        print(json.dumps(out), flush=True)
    eng.close()


def main():
    Q, K, T = (int(x) for x in sys.argv[1:4]) if len(sys.argv) > 3 else (1000, 5, 1000)
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 9
    f = interop.PqaEngineFactory()
    for f32 in (False, True):
        run(f, Q, K, T, rounds, f32)


if __name__ == "__main__":
    main()
