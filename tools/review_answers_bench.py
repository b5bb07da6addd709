"""What reviewing the answers of a quiz costs (a tool, not a test).  One process, one engine per precision; per load two legs, interleaved
round by round after a warm-up, min / median / max:
  (a) PqaEngine_ReviewAnswersBatch: one call, every (quiz, position) reduced on the device to the left-out answer's likelihood, the
      entropy of the others' posterior and its top 10;
  (b) today's best from calls that were there before, per position: a scratch quiz by PqaEngine_ResumeQuizBatch from the other answers,
      PqaEngine_SetActiveQuestion of the left-out question, PqaEngine_PreviewAnswersBatch for the left-out answer's likelihood,
      PqaEngine_ListTopTargetsBatch, the posterior copied out (get_priors) for the entropy on the host, PqaEngine_ReleaseQuiz -- each of
      them batched over the positions, 256 scratch quizzes at a time.
Leg (a) is timed through the C ABI with its buffers built beforehand, as a C client pays for it; leg (b) through the Python methods (its
host work -- the entropy of a copied posterior per position -- is part of what it costs).  Before the timing the legs are compared: the
records and the likelihoods must be equal, the entropies within 2 (T + 16) 2^-52 max(1, H) bits of each other -- reported as legs_agree.
Loads: one quiz of 8, 20 and 50 answers; 16 quizzes of 20 answers; all positions; top 10.  Double and Float engines.
Prints one JSON line per precision and load.
usage: review_answers_bench.py [Q K T [rounds=9 [answers,answers,...]]]      default 1000 5 1000 9 8,20,50"""
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
CHUNK = 256
F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)


def entropy_bits(p):
    v = p[p > 0]
    return float(-(v * np.log2(v)).sum())


def leg_today(eng, pairs, histories):
    """[(likelihood, entropy, records)] per pair, through scratch quizzes."""
    out = []
    for first in range(0, len(pairs), CHUNK):
        part = pairs[first:first + CHUNK]
        scratch = eng.resume_quiz_batch([[aq for j, aq in enumerate(histories[z]) if j != i] for z, i in part])
        left = [histories[z][i] for z, i in part]
        for s, aq in zip(scratch, left):
            eng.set_active_question(s, aq.i_question)
        previews = eng.preview_answers_batch([(s, aq.i_question) for s, aq in zip(scratch, left)], 0)
        listed = eng.list_top_targets_batch(scratch, TOP)
        for s, aq, pv, lst in zip(scratch, left, previews, listed):
            out.append((pv[aq.i_answer].likelihood, entropy_bits(eng.get_priors(s)), [(t.i_target, t.prob) for t in lst]))
        for s in scratch:
            eng.release_quiz(s)
    return out


def leg_review(eng, pairs):
    return [(p.likelihood, p.entropy, [(t.i_target, t.prob) for t in p.targets]) for p in eng.review_answers_batch(pairs, TOP)]


def raw_review(eng, pairs):
    """Leg (a) as a C client pays for it: the call through the C ABI with its buffers built beforehand."""
    p64, pd = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    lib = interop.load_library()
    n = len(pairs)
    quizzes, positions = np.array([z for z, _ in pairs], dtype=np.int64), np.array([i for _, i in pairs], dtype=np.int64)
    likelihood, entropy, counts = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    records = (interop.CiRatedTarget * (n * TOP))()

    def call():
        err = lib.PqaEngine_ReviewAnswersBatch(eng.c_engine, n, quizzes.ctypes.data_as(p64), positions.ctypes.data_as(p64), TOP, likelihood.ctypes.data_as(pd),
                                               entropy.ctypes.data_as(pd), records, counts.ctypes.data_as(p64))
        if err:
            raise RuntimeError(interop.PqaError(err).to_string(True))

    return call


def run(f, Q, K, T, rounds, depths, f32):
    eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **(F32 if f32 else {})))
    precision = "float" if f32 else "double"
    if err is not None or eng is None:
        print(json.dumps({"shape": f"{Q}x{K}x{T}", "precision": precision, "skipped": err.to_string(True) if err else "no engine"}), flush=True)
        return
    eng.fill_synthetic(8.0, 0.5, 7)
    eng.set_option("top_exact", 0)        # leg (b) in the order of leg (a): probability descending, target ascending
    rng = np.random.default_rng(3)

    def sequence(n):
        perm = rng.permutation(Q)
        return [interop.AnsweredQuestion(int(perm[j % Q]), int(rng.integers(K))) for j in range(n)]

    many = depths[len(depths) // 2]
    loads = [("1_quiz_%d_answers" % n, [sequence(n)]) for n in depths] + [("16_quizzes_%d_answers" % many, [sequence(many) for _ in range(16)])]
    for name, seqs in loads:
        live = eng.resume_quiz_batch(seqs)
        histories = dict(zip(live, seqs))
        pairs = [(z, i) for z in live for i in range(len(histories[z]))]
        a, b = leg_review(eng, pairs), leg_today(eng, pairs, histories)
        agree = len(a) == len(b) and all(la == lb and ra == rb and abs(ha - hb) <= 2 * (T + 16) * 2.0 ** -52 * max(1.0, hb) for (la, ha, ra), (lb, hb, rb) in zip(a, b))
        legs = {"a_review": raw_review(eng, pairs), "b_today": lambda: leg_today(eng, pairs, histories)}
        for fn in legs.values():
            for _ in range(WARMUP):
                fn()
        times = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t0)
        med = {k: statistics.median(ts) for k, ts in times.items()}
        out = {"shape": f"{Q}x{K}x{T}", "precision": precision, "load": name, "quizzes": len(live), "rows": len(pairs), "top": TOP, "rounds": rounds,
               "legs_agree": bool(agree)}
        for k, ts in times.items():
            out[k] = {"ms_min": round(min(ts) * 1e3, 4), "ms_median": round(med[k] * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)}
        out["b_over_a"] = round(med["b_today"] / med["a_review"], 2)
        print(json.dumps(out), flush=True)
        for z in live:
            eng.release_quiz(z)
    eng.close()


def main():
    Q, K, T = (int(x) for x in sys.argv[1:4]) if len(sys.argv) > 3 else (1000, 5, 1000)
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 9
    depths = [int(x) for x in sys.argv[5].split(",")] if len(sys.argv) > 5 else [8, 20, 50]
    f = interop.PqaEngineFactory()
    for f32 in (False, True):
        run(f, Q, K, T, rounds, depths, f32)


if __name__ == "__main__":
    main()
