"""What recording a page of answers costs (a tool, not a test).  One process, one engine per shape; per batch of quizzes and page
size three legs, interleaved round by round after a warm-up round, median / min / max over the rounds:
  (page)  PqaEngine_RecordAnswerPageBatch: one call, one launch per 256 quizzes;
  (a)     today's route to the same posteriors: per position PqaEngine_SetActiveQuestion for every quiz, then PqaEngine_RecordAnswerBatch;
  (b)     the floor: ONE PqaEngine_RecordAnswerBatch of one answer per quiz (active questions set outside the timed region).
Every round gets fresh quizzes for each leg (PqaEngine_StartQuizBatch, outside the timed region, the stream synchronised before the
clock starts), and every timing ends in a synchronisation of the engine's stream.  In the warm-up round the posteriors of (page) and
(a) are compared for equality (legs_agree).
Shapes: 1000x5x1000, 10000x5x10000 and 2000x5x100000 (questions x answers x targets) for 1 / 64 / 256 quizzes and pages of 3 / 5 / 10.
Prints one JSON line per shape, batch and page size, then the table.
usage: record_page_bench.py [rounds=9]   (at least 9)      record_page_bench.py --quick ROUNDS: one small shape, 60x5x1300, 1 / 8 quizzes, pages of 3 / 5"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probqa_amd import interop

AQ = interop.AnsweredQuestion


def leg_page(eng, quizzes, pages):
    eng.record_answer_page_batch(quizzes, pages)


def leg_todays_route(eng, quizzes, pages):
    for p in range(len(pages[0])):
        for quiz, page in zip(quizzes, pages):
            eng.set_active_question(quiz, page[p].i_question)
        eng.record_answer_batch(quizzes, [page[p].i_answer for page in pages])


def leg_floor(eng, quizzes, pages):
    eng.record_answer_batch(quizzes, [page[0].i_answer for page in pages])


def one_round(eng, n, pages, times, check=False):
    """fresh quizzes for each leg, each leg timed to a synchronisation -> legs_agree if `check`"""
    sets = {k: eng.start_quiz_batch(n) for k in ("page", "a_todays_route", "b_floor")}
    for quiz, page in zip(sets["b_floor"], pages):
        eng.set_active_question(quiz, page[0].i_question)
    legs = {"page": leg_page, "a_todays_route": leg_todays_route, "b_floor": leg_floor}
    for k, fn in legs.items():
        eng.synchronize()
        t0 = time.perf_counter()
        fn(eng, sets[k], pages)
        eng.synchronize()
        if times is not None:
            times[k].append(time.perf_counter() - t0)
    agree = None
    if check:
        agree = all(np.array_equal(eng.get_priors(x), eng.get_priors(y)) for x, y in zip(sets["page"], sets["a_todays_route"]))
    for ids in sets.values():
        for quiz in ids:
            eng.release_quiz(quiz)
    return agree


def run(f, Q, K, T, batches, sizes, rounds, rows):
    shape = "%dx%dx%d" % (Q, K, T)
    eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
    if err is not None or eng is None:
        print(json.dumps({"shape": shape, "skipped": err.to_string(True) if err else "no engine"}), flush=True)
        return
    eng.fill_synthetic(8.0, 0.5, 7)
    rng = np.random.default_rng(3)
    for n in batches:
        for size in sizes:
            pages = [[AQ(int(q), int(rng.integers(K))) for q in rng.permutation(Q)[:size]] for _ in range(n)]
            agree = one_round(eng, n, pages, None, check=True)       # the warm-up round
            times = {k: [] for k in ("page", "a_todays_route", "b_floor")}
            for _ in range(rounds):
                one_round(eng, n, pages, times)
            med = {k: statistics.median(ts) for k, ts in times.items()}
            out = {"shape": shape, "quizzes": n, "page_size": size, "rounds": rounds, "legs_agree": bool(agree)}
            for k, ts in times.items():
                out[k] = {"ms_median": round(med[k] * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)}
            out["page_over_a"] = round(med["page"] / med["a_todays_route"], 3)
            out["page_over_b"] = round(med["page"] / med["b_floor"], 2)
            print(json.dumps(out), flush=True)
            spread = lambda k: "%.3f (%.3f .. %.3f)" % (med[k] * 1e3, min(times[k]) * 1e3, max(times[k]) * 1e3)
            rows.append("| %s | %d | %d | %s | %s | %s | %.3f | %.2f |" % (shape, n, size, spread("page"), spread("a_todays_route"), spread("b_floor"),
                                                                          out["page_over_a"], out["page_over_b"]))
    eng.close()


def main():
    args = sys.argv[1:]
    quick = "--quick" in args
    numbers = [int(a) for a in args if a != "--quick"]
    rounds = numbers[0] if numbers else 9
    if not quick:
        rounds = max(rounds, 9)
    f = interop.PqaEngineFactory()
    rows = []
    plan = [(60, 5, 1300, (1, 8), (3, 5))] if quick else [(1000, 5, 1000, (1, 64, 256), (3, 5, 10)), (10000, 5, 10000, (1, 64, 256), (3, 5, 10)),
                                                          (2000, 5, 100000, (1, 64, 256), (3, 5, 10))]
    for Q, K, T, batches, sizes in plan:
        run(f, Q, K, T, batches, sizes, rounds, rows)
    print("| shape | quizzes | page | Page ms median (min .. max) | (a) today's route ms | (b) one RecordAnswerBatch ms | Page / a | Page / b |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(r)


if __name__ == "__main__":
    main()
