"""PqaEngine_RecordAnswerPageBatch on a real MI355X: a page of answers per quiz in one launch.  The baseline is a TWIN quiz on the same
engine, driven by set_active_question + record_answer once per answer; every posterior comparison is bit for bit (np.array_equal),
nothing is compared within a tolerance.  Row lengths: the 256-thread form, an odd tail, the 1024-thread staged form, a row that does
not fit the LDS stage, a row beyond 16384 targets; Double and Float engines; `workers` 1, 16 and 64."""
import ctypes
import json
import os
import sys
import threading

import numpy as np
import pytest

import cases
import orclib
from probqa_amd import interop
from test_gpu_resume_batch import aq_list, synthetic

pytestmark = pytest.mark.gpu

GDIR = os.path.join(os.path.dirname(__file__), "golden")
K, Q = 5, 300
N_QUIZZES = 24
COUNTERS = ("record_page_calls", "page_answers", "page_launches")
NEG, NULL, RANGE, MODE = "The count is negative", "Expected non-null argument", "Index is out of range", "An attempt to execute an operation in a wrong mode"


def make_pages(rng, n, n_questions, n_answers, asked_before, qgaps=()):
    """Pages of 0, 1, ... 12 answers (cycled): from three answers on a question is repeated within the page, from two on the page
    holds the question the quiz had asked before."""
    valid = np.array([q for q in range(n_questions) if q not in set(qgaps)])
    pages = []
    for i in range(n):
        m = i % 13
        qs = [int(q) for q in rng.choice(valid, size=m, replace=True)]
        if m >= 3:
            qs[m // 2] = qs[0]
        if m >= 2:
            qs[1] = int(asked_before[i])
        pages.append([(q, int((i + j) % n_answers)) for j, q in enumerate(qs)])
    return pages


def answers_of(eng, quiz):
    return [(a.i_question, a.i_answer) for a in eng.get_quiz_answers(quiz)]


def listing(eng, quiz, n=10):
    return [(t.i_target, t.prob) for t in eng.list_top_targets(quiz, n)]


def step_by_step(eng, quiz, page):
    for q, a in page:
        eng.set_active_question(quiz, q)
        eng.record_answer(quiz, a)


def assert_same_quiz(eng, quiz, twin, what, select=True):
    assert np.array_equal(eng.get_priors(quiz), eng.get_priors(twin)), what
    assert np.array_equal(eng.eval_priorities(quiz), eng.eval_priorities(twin)), what      # (the asked sets)
    assert answers_of(eng, quiz) == answers_of(eng, twin), what
    assert listing(eng, quiz) == listing(eng, twin), what
    if select:
        assert eng.next_question_argmax(quiz) == eng.next_question_argmax(twin), what


def started_pairs(eng, n, rng):
    """n quizzes and their twins, each with one answer recorded the usual way; -> quizzes, twins, the questions asked."""
    quizzes, twins = eng.start_quiz_batch(n), eng.start_quiz_batch(n)
    dims = eng.copy_dims()
    before = [int(q) for q in rng.choice(dims.n_questions, size=n)]
    for i in range(n):
        for z in (quizzes[i], twins[i]):
            eng.set_active_question(z, before[i])
            eng.record_answer(z, i % dims.n_answers)
    return quizzes, twins, before


# ---- 1. row-length edges -------------------------------------------------------------------------------------------------------------
EDGES = [(1000, 16, False), (1003, 16, False), (1500, 16, False), (9000, 16, False), (20000, 16, False),
         (1000, 1, False), (1000, 64, False), (1003, 1, False), (1003, 64, False), (1000, 16, True), (9000, 16, True)]


@pytest.mark.parametrize("T,workers,f32", EDGES, ids=["%dx%d%s" % (t, w, "f" if f else "") for t, w, f in EDGES])
def test_pages_equal_the_consecutive_calls(T, workers, f32, factory):
    eng = synthetic(factory, K, Q, T, 5, (3, 17, T - 1), f32)
    eng.set_option("workers", workers)
    rng = np.random.default_rng(T + workers)
    quizzes, twins, before = started_pairs(eng, N_QUIZZES, rng)
    pages = make_pages(rng, N_QUIZZES, Q, K, before)
    assert [len(p) for p in pages[:13]] == list(range(13))
    for z in (quizzes[0], twins[0], quizzes[13], twins[13]):                    # the quizzes with an empty page: their active question stays
        eng.set_active_question(z, 7)
    assert eng.record_answer_page_batch(quizzes, [aq_list(p) for p in pages]) is None
    for twin, page in zip(twins, pages):
        step_by_step(eng, twin, page)
    for i, (quiz, twin) in enumerate(zip(quizzes, twins)):
        assert eng.get_active_question_id(quiz) == (-1 if pages[i] else 7), i
        assert_same_quiz(eng, quiz, twin, (T, workers, f32, i))
    # one more answer on both (to the question next_question_argmax has just made active): still equal
    for i, (quiz, twin) in enumerate(zip(quizzes, twins)):
        for z in (quiz, twin):
            eng.record_answer(z, (i + 1) % K)
    for i, (quiz, twin) in enumerate(zip(quizzes, twins)):
        assert_same_quiz(eng, quiz, twin, ("one more", T, workers, f32, i), select=False)
    eng.close()


# ---- 2. the CPU oracle ---------------------------------------------------------------------------------------------------------------
def _golden_names():
    return sorted(f[:-5] for f in os.listdir(GDIR) if f.endswith(".json"))


@pytest.mark.parametrize("name", _golden_names())
def test_pages_match_the_oracle_on_golden_cases(name, factory):
    """(gaps_37x5x101 at 64 workers: 26 vectors over 63 subtasks, the quot == 0 branch of the split)"""
    sys.path.insert(0, GDIR)
    import make_golden

    case = make_golden.case_from_meta(json.load(open(os.path.join(GDIR, name + ".json"))))
    eng, orc = case.make_engine(factory), case.make_oracle()
    rng = np.random.default_rng(3)
    valid = [q for q in range(case.Q) if q not in set(case.qgaps)]
    for workers in (1, 16, 64):
        eng.set_option("workers", workers)
        qs = [int(q) for q in rng.choice(valid, size=8)]
        qs[5] = qs[1]
        page = [(q, int((j + workers) % case.K)) for j, q in enumerate(qs)]
        quiz = eng.start_quiz()
        orc.start_quiz(workers)
        assert np.array_equal(eng.get_priors(quiz), orc.priors())
        eng.record_answer_page(quiz, aq_list(page))
        for q, a in page:
            orc.record_answer(q, a, max(1, workers - 1))
        assert np.array_equal(eng.get_priors(quiz), orc.priors()), (name, workers)
    eng.close()


# ---- 3. likelihoods ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,f32", [(1000, False), (9000, False), (1000, True), (9000, True)], ids=["1000", "9000", "1000f", "9000f"])
def test_likelihoods_are_the_previews(T, f32, factory):
    eng = synthetic(factory, K, 60, T, 9, (3, 17, T - 1), f32)
    rng = np.random.default_rng(T)
    quizzes, twins, before = started_pairs(eng, 6, rng)
    pages = [p for p in make_pages(rng, 13, 60, K, before * 3) if len(p) in (0, 1, 2, 5, 9, 12)]
    got = eng.record_answer_page_batch(quizzes, [aq_list(p) for p in pages], likelihoods=True)
    assert [len(g) for g in got] == [len(p) for p in pages]
    for i, (twin, page) in enumerate(zip(twins, pages)):
        for j, (q, a) in enumerate(page):
            want = eng.preview_answers(twin, q, 0)[a].likelihood            # the twin just before this step
            assert np.float64(got[i][j]).tobytes() == np.float64(want).tobytes(), (i, j, got[i][j], want)
            eng.set_active_question(twin, q)
            eng.record_answer(twin, a)
        assert np.array_equal(eng.get_priors(quizzes[i]), eng.get_priors(twin)), i
    single, twin = eng.start_quiz(), eng.start_quiz()
    lik = eng.record_answer_page(single, aq_list([(4, 1), (9, 0)]), likelihoods=True)
    assert lik[0] == eng.preview_answers(twin, 4, 0)[1].likelihood and len(lik) == 2
    eng.close()


# ---- 4. a dead answer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
def test_dead_answer(f32, factory):
    """After a dead answer the update kernels leave 0 / NaN = NaN at a target gap too; RecordAnswer's OTHER route, the update fused
    into the speculative sweep (option "fuse_update", rows of up to 1024 targets, a client alone in the engine), writes the gap-masked
    value back and leaves 0.0 there -- the two routes of the consecutive calls differ in that one element, and only in this case.  The
    page runs the update kernels' code, so the twin is driven through them: fuse_update 0."""
    k, nq, T = 3, 8, 130
    eng = synthetic(factory, k, nq, T, 7, (5,), f32)
    eng.set_option("fuse_update", 0)
    A, D, B = eng.get_kb()
    q, dead = 2, 1
    A[q][dead][:] = 0.0
    D[q] = A[q][0] + A[q][2]
    eng.set_kb(A, D, B)
    page = [(0, 1), (q, dead), (4, 2), (6, 0)]
    quiz, twin = eng.start_quiz(), eng.start_quiz()
    lik = eng.record_answer_page(quiz, aq_list(page), likelihoods=True)
    step_by_step(eng, twin, page)
    got, want = eng.get_priors(quiz), eng.get_priors(twin)
    assert lik[1] == 0.0 and np.isnan(lik[2]) and np.isnan(got).any()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got, want, equal_nan=True)
    assert answers_of(eng, quiz) == page and eng.get_active_question_id(quiz) == -1
    eng.close()


# ---- 5. engine state -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("server", [0, 1], ids=["launched", "server"])
def test_speculation_and_selection(server, factory):
    eng = synthetic(factory, K, 120, 1000, 3, (3, 17))
    eng.set_option("select", 1)
    eng.set_option("server", server)
    page = [(11, 2), (40, 0), (11, 3), (77, 1)]
    quiz = eng.start_quiz()                                          # (alone in the engine: a speculative sweep goes out behind it)
    first = eng.next_question(quiz)
    eng.record_answer(quiz, 1)                                       # ... and behind this
    eng.record_answer_page(quiz, aq_list(page))
    picks = [eng.next_question_argmax(quiz), eng.next_question(quiz)]
    twin = eng.start_quiz()
    assert eng.next_question(twin) == first
    eng.record_answer(twin, 1)
    step_by_step(eng, twin, page)
    assert [eng.next_question_argmax(twin), eng.next_question(twin)] == picks
    assert np.array_equal(eng.get_priors(quiz), eng.get_priors(twin)) and listing(eng, quiz) == listing(eng, twin)
    eng.close()


def test_a_deferred_answer_is_applied_first(factory):
    eng = synthetic(factory, K, 120, 1003, 3, (3, 17))
    page = [(11, 2), (40, 0), (5, 4)]
    quiz, twin = eng.start_quiz(), eng.start_quiz()
    eng.set_option("post_always", 1)                                 # the posted form of RecordAnswer: its update stays deferred
    flushed0 = eng.get_option("updates_flushed")
    eng.set_active_question(quiz, 33)
    eng.record_answer(quiz, 2)
    deferred = eng.get_option("updates_flushed") == flushed0
    eng.record_answer_page(quiz, aq_list(page))
    assert eng.get_option("updates_flushed") == flushed0 + 1
    eng.set_option("post_always", 0)
    step_by_step(eng, twin, [(33, 2)] + page)
    assert_same_quiz(eng, quiz, twin, ("deferred", deferred))
    eng.close()


# ---- 6. chunks and counters ----------------------------------------------------------------------------------------------------------
def test_three_hundred_quizzes_take_two_launches(factory):
    eng = synthetic(factory, K, 40, 1000, 4, (3,))
    n = 300
    rng = np.random.default_rng(1)
    pages = [[(int(q), int(a)) for q, a in zip(rng.choice(40, size=1 + i % 3), rng.integers(0, K, size=1 + i % 3))] for i in range(n)]
    quizzes, twins = eng.start_quiz_batch(n), eng.start_quiz_batch(n)
    c0 = [eng.get_option(c) for c in COUNTERS]
    eng.set_option("time_sweeps", 1)
    ns0 = eng.get_option("record_page_device_ns")
    eng.record_answer_page_batch(quizzes, [aq_list(p) for p in pages])
    assert [eng.get_option(c) for c in COUNTERS] == [c0[0] + 1, c0[1] + sum(len(p) for p in pages), c0[2] + 2]
    assert eng.get_option("record_page_device_ns") > ns0
    eng.set_option("time_sweeps", 0)
    for p in range(3):                                                # today's route, position by position
        live = [i for i in range(n) if len(pages[i]) > p]
        for i in live:
            eng.set_active_question(twins[i], pages[i][p][0])
        for first in range(0, len(live), 256):
            part = live[first:first + 256]
            eng.record_answer_batch([twins[i] for i in part], [pages[i][p][1] for i in part])
    for i in range(n):
        assert np.array_equal(eng.get_priors(quizzes[i]), eng.get_priors(twins[i])), i
    assert answers_of(eng, quizzes[299]) == pages[299] and listing(eng, quizzes[299]) == listing(eng, twins[299])
    assert eng.record_answer_page_batch([], []) is None                # an empty call is a call
    assert eng.get_option("record_page_calls") == c0[0] + 2 and eng.get_option("page_launches") == c0[2] + 2
    eng.close()


# ---- 7. refusals, in the header's order, the offending entry LAST among valid ones ---------------------------------------------------
P64, PD, PAQ = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(interop.CiAnsweredQuestion)


def raw_page(eng, quizzes, pages, n=None, counts=None, null=()):
    """The C call itself -> the error's text ('' for success)."""
    lib = interop.load_library()
    qs = (ctypes.c_int64 * max(len(quizzes), 1))(*quizzes)
    cs = (ctypes.c_int64 * max(len(quizzes), 1))(*(counts if counts is not None else [len(p) for p in pages]))
    flat = [aq for p in pages for aq in p]
    arr = (interop.CiAnsweredQuestion * max(len(flat), 1))()
    for i, (q, a) in enumerate(flat):
        arr[i].iQuestion, arr[i].iAnswer = q, a
    lik = (ctypes.c_double * max(len(flat), 1))(*([-7.0] * max(len(flat), 1)))
    err = lib.PqaEngine_RecordAnswerPageBatch(eng.c_engine, len(quizzes) if n is None else n, None if "quizzes" in null else qs,
                                              None if "counts" in null else cs, None if "aqs" in null else ctypes.cast(arr, PAQ), lik)
    assert all(v == -7.0 for v in lik) or not err
    return interop.PqaError(err).to_string(True) if err else ""


def test_refusals_change_nothing(factory):
    k, nq, T = 3, 8, 13
    eng = synthetic(factory, k, nq, T, 7)
    eng.set_question_gaps([5])
    a, b, c = eng.start_quiz_batch(3)
    step_by_step(eng, a, [(1, 1)])
    for z, q in ((a, 2), (b, 3), (c, 4)):
        eng.set_active_question(z, q)
    good = [[(1, 0)], [(2, 1), (3, 2)]]

    def state():
        return [(eng.get_priors(z).tobytes(), answers_of(eng, z), eng.get_active_question_id(z)) for z in (a, b, c)] + [eng.get_option(n) for n in COUNTERS]

    state0 = state()

    def refused(text, code, *parts):
        assert text.startswith("[" + code + "]") and all(p in text for p in parts), text
        assert state() == state0, text

    refused(raw_page(eng, [a, b, c], good + [[(0, 0)]], n=-1), NEG, "count=-1")
    refused(raw_page(eng, [a, b, c], good + [[]], counts=[1, 2, -3]), NEG, "entry=2", "count=-3")
    refused(raw_page(eng, [a, b, c], good + [[(0, 0)]], null=("quizzes",)), NULL)
    refused(raw_page(eng, [a, b, c], good + [[(0, 0)]], null=("counts",)), NULL)
    refused(raw_page(eng, [a, b, c], good + [[(0, 0)]], null=("aqs",)), NULL)
    refused(raw_page(eng, [a, b, c], good + [[(0, 0)] * 4097]), RANGE, "entry=2", "subjIndex=4097", "4096")
    refused(raw_page(eng, [a, b, 99], good + [[(0, 0)]]), RANGE, "entry=2", "quizId=99")
    refused(raw_page(eng, [a, b, a], good + [[(0, 0)]]), RANGE, "entry=2", "twice")
    refused(raw_page(eng, [a, b, c], good + [[(0, 0), (nq, 0)]]), RANGE, "entry=2", "position=1", "questionId=%d" % nq)
    refused(raw_page(eng, [a, b, c], good + [[(-1, 0)]]), RANGE, "entry=2", "position=0", "questionId=-1")
    refused(raw_page(eng, [a, b, c], good + [[(0, 0), (0, 1), (5, 0)]]), RANGE, "entry=2", "position=2", "questionId=5", "gap")
    refused(raw_page(eng, [a, b, c], good + [[(0, k)]]), RANGE, "entry=2", "position=0", "subjIndex=%d" % k)
    refused(raw_page(eng, [a, b, c], good + [[(0, 0), (0, -1)]]), RANGE, "entry=2", "position=1", "subjIndex=-1")
    # the order: a count before a NULL, the limit before the quiz, the quiz before its repeat, the question before the answer
    refused(raw_page(eng, [a, b, c], good + [[]], counts=[1, 2, -3], null=("aqs",)), NEG, "entry=2")
    refused(raw_page(eng, [99, b, c], [[(0, 0)] * 4097, [], []]), RANGE, "entry=0", "subjIndex=4097")
    refused(raw_page(eng, [a, 99, a], [[(0, k)], [], []]), RANGE, "entry=1", "quizId=99")
    refused(raw_page(eng, [a, b, a], [[(nq, k)], [], []]), RANGE, "entry=2", "twice")
    refused(raw_page(eng, [a, b], [[(0, k)], [(nq, 0)]]), RANGE, "entry=1", "questionId=%d" % nq)
    # the next good call is correct, and an empty page leaves its quiz alone
    assert raw_page(eng, [a, b, c], good + [[]]) == ""
    twin = eng.start_quiz()
    step_by_step(eng, twin, [(1, 1), (1, 0)])
    assert np.array_equal(eng.get_priors(a), eng.get_priors(twin)) and eng.get_active_question_id(c) == 4 and answers_of(eng, c) == []
    assert [eng.get_option(n) for n in COUNTERS] == [state0[3] + 1, state0[4] + 3, state0[5] + 1]
    # maintenance mode and shutdown, as RecordAnswerBatch answers them: behind a NULL, in front of the limit and the quiz
    eng.start_maintenance(True)
    text = raw_page(eng, [99], [[(0, 0)] * 4097])
    assert text.startswith("[" + MODE + "]") and "record an answer" in text, text
    assert raw_page(eng, [99], [[(0, 0)]], null=("aqs",)).startswith("[" + NULL + "]")
    eng.finish_maintenance()
    eng.shutdown()
    assert raw_page(eng, [a], [[(0, 0)]]).startswith("[" + MODE + "]")
    eng.close()


# ---- 8. client threads ---------------------------------------------------------------------------------------------------------------
def test_eight_client_threads(factory):
    n_threads, rounds, nq = 8, 5, 90
    engines = [synthetic(factory, K, nq, 1000, 6, (3, 17)) for _ in range(2)]

    def pages_of(t):
        return [[((11 * t + 2 * r) % nq, (t + r) % K), ((11 * t + 2 * r + 1) % nq, (t + 2 * r) % K)] for r in range(rounds)]

    def run(eng, quiz, t, out):
        picks = []
        for page in pages_of(t):
            eng.record_answer_page(quiz, aq_list(page))
            picks.append(eng.next_question_argmax(quiz))
        out[t] = picks

    shared, alone = engines
    quizzes = shared.start_quiz_batch(n_threads)
    got, want = {}, {}
    threads = [threading.Thread(target=run, args=(shared, quizzes[t], t, got)) for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
    assert not any(th.is_alive() for th in threads) and sorted(got) == list(range(n_threads))
    twins = alone.start_quiz_batch(n_threads)
    for t in range(n_threads):
        run(alone, twins[t], t, want)
    assert got == want
    for t in range(n_threads):
        assert np.array_equal(shared.get_priors(quizzes[t]), alone.get_priors(twins[t])), t
        assert answers_of(shared, quizzes[t]) == answers_of(alone, twins[t])
    for e in engines:
        e.close()
