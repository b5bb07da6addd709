"""What a greedy page of questions costs (a tool, not a test).  One process, one engine per shape; per batch of quizzes and page size
three legs, interleaved round by round after a warm-up, min / median / max:
  (page)  PqaEngine_ListQuestionPageBatch: the branch rows, the gain sweeps, the combines and the picks on the device, one wait;
  (a)     the route to the same page from calls that were there before, step by step on the host: per step PqaEngine_EvalQuestionGainsBatch
          over scratch quizzes, one per answer combination of the prefix, combined with the combinations' probabilities and picked on the
          host; then PqaEngine_PreviewAnswersBatch(0) for the likelihoods of the pick's answers under every scratch quiz (a resumed quiz
          is normalised: its QuizStatusBatch mass is 1 and carries no weight, so the weights are chained from the likelihoods) and
          PqaEngine_ResumeQuizBatch of K times as many scratch quizzes; at the end every scratch quiz is released;
  (b)     PqaEngine_ListInformativeQuestionsBatch(pageSize): the naive page -- the best questions by marginal gain -- and the floor.
Before the timing the page of leg (a) is compared with the new call's (legs_agree: the same questions in the same order, every value
within 1e-9 bits).  As information only the tool reports the joint information I(A_page ; T) in bits of the greedy and of the naive page
of the batch's first quiz: the sum of the greedy page's values by the chain rule, and the same sum for the naive page's questions taken
in their listed order (PqaEngine_EvalConditionalGainsBatch given the prefix).
Shapes: 1000x5x1000 with pages of 2 / 3 / 4 for 1 / 8 / 64 quizzes, 10000x5x10000 with pages of 2 / 3 (questions x answers x targets;
quizzes resumed from 1 .. 5 answers each).  Prints one JSON line per shape, batch and page size, then the table.
usage: question_page_bench.py [--quick] [rounds=5]      --quick: one small shape, 40x5x1300, pages of 2 / 3 for 1 / 8 quizzes"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probqa_amd import interop

WARMUP = 1
P64 = ctypes.POINTER(ctypes.c_int64)
AQ = interop.AnsweredQuestion


def checked(err):
    if err:
        raise RuntimeError(interop.PqaError(err).to_string(True))


def raw_page(eng, quizzes, size):
    lib = interop.load_library()
    qs = np.array(quizzes, dtype=np.int64)
    records, counts = (interop.CiRatedQuestion * (len(qs) * size))(), np.zeros(len(qs), dtype=np.int64)

    def call():
        checked(lib.PqaEngine_ListQuestionPageBatch(eng.c_engine, len(qs), qs.ctypes.data_as(P64), None, None, size, records, counts.ctypes.data_as(P64)))

    def pages():
        return [[(records[i * size + j].iQuestion, records[i * size + j].priority) for j in range(counts[i])] for i in range(len(qs))]

    return call, pages


def raw_naive(eng, quizzes, size):
    lib = interop.load_library()
    qs = np.array(quizzes, dtype=np.int64)
    records, counts = (interop.CiRatedQuestion * (len(qs) * size))(), np.zeros(len(qs), dtype=np.int64)
    return lambda: checked(lib.PqaEngine_ListInformativeQuestionsBatch(eng.c_engine, len(qs), qs.ctypes.data_as(P64), size, records, counts.ctypes.data_as(P64)))


def todays_route(eng, quizzes, seqs, size, K):
    """the page of every quiz from EvalQuestionGainsBatch over scratch quizzes, PreviewAnswersBatch and ResumeQuizBatch"""
    n = len(quizzes)
    asked = [{a.i_question for a in s} for s in seqs]
    branches = [[(quizzes[i], 1.0, list(seqs[i]))] for i in range(n)]   # (quiz id, probability of the combination, its answers)
    pages, scratch = [[] for _ in range(n)], []
    for step in range(size):
        flat = [b[0] for bs in branches for b in bs]
        rows = eng.eval_question_gains_batch(flat)
        at, picks = 0, []
        for i in range(n):
            w = np.array([b[1] for b in branches[i]])
            cg = (w[:, None] * rows[at:at + len(w)]).sum(axis=0) / w.sum()
            at += len(w)
            cg[sorted(asked[i] | {q for q, _ in pages[i]})] = 0.0
            best = int(np.argmax(cg))
            picks.append(best)
            pages[i].append((best, float(cg[best])))
        if step + 1 == size:
            break
        previews = eng.preview_answers_batch([(b[0], picks[i]) for i in range(n) for b in branches[i]], 0)
        at, lists, grown = 0, [], []
        for i in range(n):
            new = []
            for quiz, weight, answers in branches[i]:
                for k in range(K):
                    new.append((None, weight * previews[at][k].likelihood, answers + [AQ(picks[i], k)]))
                at += 1
            grown.append(new)
            lists += [b[2] for b in new]
        ids = eng.resume_quiz_batch(lists)
        scratch += ids
        at = 0
        for i in range(n):
            branches[i] = [(ids[at + j], b[1], b[2]) for j, b in enumerate(grown[i])]
            at += len(grown[i])
    for quiz in scratch:
        eng.release_quiz(quiz)
    return pages


def joint_bits(eng, quiz, questions):
    """I(A_questions ; T) by the chain rule over the listed order"""
    return float(sum(eng.eval_conditional_gains_batch([quiz], [questions[:j]])[0][q] for j, q in enumerate(questions)))


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


def run(f, Q, K, T, batches, sizes, rounds, rows):
    shape = "%dx%dx%d" % (Q, K, T)
    eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
    if err is not None or eng is None:
        print(json.dumps({"shape": shape, "skipped": err.to_string(True) if err else "no engine"}), flush=True)
        return
    eng.fill_synthetic(8.0, 0.5, 7)
    rng = np.random.default_rng(3)
    seqs = [[AQ(int(q), int(rng.integers(K))) for q in rng.permutation(Q)[:1 + j % 5]] for j in range(max(batches))]
    live = eng.resume_quiz_batch(seqs)
    for n in batches:
        for size in sizes:
            quizzes = live[:n]
            page, pages_of = raw_page(eng, quizzes, size)
            page()
            new = pages_of()
            old = todays_route(eng, quizzes, seqs[:n], size, K)
            same = all([q for q, _ in a] == [q for q, _ in b] for a, b in zip(new, old))
            differ = max((abs(x[1] - y[1]) for a, b in zip(new, old) for x, y in zip(a, b)), default=0.0)
            legs = {"page": page, "a_todays_route": lambda: todays_route(eng, quizzes, seqs[:n], size, K), "b_naive_floor": raw_naive(eng, quizzes, size)}
            times = timed(legs, rounds)
            med = {k: statistics.median(ts) for k, ts in times.items()}
            naive = [q for q, _ in eng.list_informative_questions(quizzes[0], size)]
            out = {"shape": shape, "quizzes": n, "page_size": size, "rounds": rounds, "legs_agree": bool(same and differ <= 1e-9), "page_minus_a_max_bits": differ,
                   "greedy_joint_bits": round(sum(v for _, v in new[0]), 6), "naive_joint_bits": round(joint_bits(eng, quizzes[0], naive), 6)}
            for k, ts in times.items():
                out[k] = {"ms_min": round(min(ts) * 1e3, 4), "ms_median": round(med[k] * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)}
            out["a_over_page"] = round(med["a_todays_route"] / med["page"], 2)
            out["page_over_b"] = round(med["page"] / med["b_naive_floor"], 2)
            print(json.dumps(out), flush=True)
            spread = lambda k: "%.3f (%.3f .. %.3f)" % (med[k] * 1e3, min(times[k]) * 1e3, max(times[k]) * 1e3)
            rows.append("| %s | %d | %d | %s | %s | %s | %.1f | %.2f | %.4f | %.4f |" % (shape, n, size, spread("page"), spread("a_todays_route"), spread("b_naive_floor"),
                                                                                     out["a_over_page"], out["page_over_b"], out["greedy_joint_bits"], out["naive_joint_bits"]))
    eng.close()


def main():
    args = [a for a in sys.argv[1:] if a != "--quick"]
    quick = len(args) != len(sys.argv) - 1
    rounds = int(args[0]) if args else 5
    f = interop.PqaEngineFactory()
    rows = []
    plan = [(40, 5, 1300, (1, 8), (2, 3))] if quick else [(1000, 5, 1000, (1, 8, 64), (2, 3, 4)), (10000, 5, 10000, (1, 8, 64), (2, 3))]
    for Q, K, T, batches, sizes in plan:
        run(f, Q, K, T, batches, sizes, rounds, rows)
    print("| shape | quizzes | page | Page ms median (min .. max) | (a) today's route ms | (b) ListInformative ms | a / Page | Page / b | greedy page bits | naive page bits |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(r)


if __name__ == "__main__":
    main()
