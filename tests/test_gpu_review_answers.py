"""PqaHip_GetQuizAnswers and PqaEngine_ReviewAnswersBatch on the GPU (include/PqaHipExt.h; review_kernels.hip; hip_engine_review.cpp):
a quiz with each of its answers left out -- the left-out answer's likelihood, the entropy and the best targets of the others' posterior
-- without changing the quiz.

The truth of a row (quiz, position i) is a TWIN quiz: resume_quiz_batch of the remaining answers in their order, then get_priors.  On
Double engines the twin is held to orclib.Oracle.resume_quiz as well, bit for bit (start_quiz where nothing remains).

Records must EQUAL numpy's listing of the twin's posterior by (-p, id) over the non-gap p > 0, id and probability bits; maxCount is 256,
so for T <= 256 every bit of the posterior is checked.  The likelihood must carry the bits of preview_answers(twin, q)[a].likelihood for
the left-out (q, a).  The entropy's bar is derived, not measured: |H - H_ref| <= (T + 16) 2^-52 max(1, H_ref) bits, H_ref =
-math.fsum(p log2 p) over the twin's posterior -- every term is >= 0, so the sum of the terms' magnitudes is H itself.  The worst seen
is printed in units of the bar."""
import ctypes
import math

import numpy as np
import pytest

import cases
import orclib
from probqa_amd import interop
from probqa_amd.interop import AnsweredQuestion as AQ

pytestmark = pytest.mark.gpu

F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)
P64, PD, PREC = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(interop.CiRatedTarget)
EPS = 2.0 ** -52
MAX = 256

# K, Q, T, target gaps: PreviewAnswersBatch's table (tests/test_gpu_preview_answers.py)
SHAPES = {
    "min_2x1x2": (2, 1, 2, ()),
    "gaps_3x8x12": (3, 8, 12, (2, 11)),
    "padded_3x8x13": (3, 8, 13, (2, 11)),
    "ragged_5x17x67": (5, 17, 67, ()),
    "small_5x12x1024": (5, 12, 1024, (1023,)),
    "large_5x12x1025": (5, 12, 1025, ()),
    "oddk_7x9x130": (7, 9, 130, (0,)),
    "nolds_3x6x9000": (3, 6, 9000, (4500,)),
    "long_2x4x16400": (2, 4, 16400, ()),
}
DEEP = ("ragged_5x17x67", "small_5x12x1024")   # ... also 100 answers deep, where the exponent surgery decides bits
WORST = {"entropy": 0.0}


def make_engine(factory, K, Q, T, tgaps=(), f32=False, seed=7, init=0.1, workers=cases.WORKERS):
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=init, **(F32 if f32 else {})))
    assert err is None and eng is not None, err
    eng.fill_synthetic(8.0, 0.5, seed)
    eng.set_option("workers", workers)
    if tgaps:
        eng.set_target_gaps(list(tgaps))
    return eng


def history(Q, K, n, seed):
    """n answers; the questions cycle through a permutation, so some are answered again."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(Q)
    return [(int(perm[i % Q]), int(rng.integers(K))) for i in range(n)]


def resume(eng, hist):
    return eng.resume_quiz([AQ(q, a) for q, a in hist])


def answers_of(eng, quiz):
    return [(a.i_question, a.i_answer) for a in eng.get_quiz_answers(quiz)]


def listing(p, tgaps, max_count):
    ids = np.arange(len(p))
    ok = (p > 0) & ~np.isin(ids, list(tgaps))
    c, pc = ids[ok], p[ok]
    take = np.lexsort((c, -pc))[:max_count]
    return [(int(t), float(x)) for t, x in zip(c[take], pc[take])]


def records(review):
    return [(t.i_target, t.prob) for t in review.targets]


def bits(x):
    return np.float64(x).tobytes()


def same(a, b):
    return records(a) == records(b) and bits(a.likelihood) == bits(b.likelihood) and bits(a.entropy) == bits(b.entropy)


def entropy_of(p, tgaps):
    v = np.delete(p, list(tgaps)) if len(tgaps) else p
    v = v[v > 0]
    return -math.fsum((v * np.log2(v)).tolist())


def twins_of(eng, hist, positions):
    """Per position the twin's posterior and the likelihood a preview of the twin gives the left-out answer."""
    lists = [[AQ(q, a) for j, (q, a) in enumerate(hist) if j != i] for i in positions]
    quizzes = eng.resume_quiz_batch(lists)
    previews = eng.preview_answers_batch([(z, hist[i][0]) for z, i in zip(quizzes, positions)], 0)
    out = []
    for z, i, pv in zip(quizzes, positions, previews):
        out.append((eng.get_priors(z), pv[hist[i][1]].likelihood))
        eng.release_quiz(z)
    return out


def check_rows(name, eng, hist, positions, got, tgaps, T, oracle=None):
    workers, bug_compat = eng.get_option("workers"), bool(eng.get_option("bug_compat"))   # (the oracle runs under the engine's options)
    for i, row, (twin, like) in zip(positions, got, twins_of(eng, hist, positions)):
        assert np.isfinite(twin).all()
        assert records(row) == listing(twin, tgaps, MAX), (name, i, records(row)[:3], listing(twin, tgaps, MAX)[:3])
        assert bits(row.likelihood) == bits(like), (name, i, row.likelihood, like)
        h_ref = entropy_of(twin, tgaps)
        dh = abs(row.entropy - h_ref) / ((T + 16) * EPS * max(1.0, h_ref))
        WORST["entropy"] = max(WORST["entropy"], dh)
        assert dh <= 1.0, (name, i, row.entropy, h_ref)
        if oracle is not None:
            rest = [aq for j, aq in enumerate(hist) if j != i]
            if rest:
                assert oracle.resume_quiz(rest, workers, bug_compat) == 0
            else:
                oracle.start_quiz(workers)
            assert oracle.priors().tobytes() == twin.tobytes(), (name, i)


def make_oracle(eng, K, Q, T, tgaps, init=0.1):
    o = orclib.Oracle(K, Q, T, init)
    o.set_kb(*eng.get_kb())
    o.set_target_gaps(list(tgaps))
    return o


# ---- 1. every shape, both precisions, every answer count, every position, one call --------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_rows_are_the_twins(factory, shape, f32):
    K, Q, T, tgaps = SHAPES[shape]
    eng = make_engine(factory, K, Q, T, tgaps, f32)
    spill = eng.get_option("review_lds_answers") + 1   # one past where the ratios leave LDS
    assert spill == 25
    counts = [1, 2, 3, 17, spill] + ([100] if shape in DEEP else [])
    hists = [history(Q, K, n, 31 + n) for n in counts]
    quizzes = [resume(eng, h) for h in hists]
    # the long shapes review a spread of the deep quizzes' positions, the others every position
    spread = lambda n: list(range(n)) if n <= 17 or T <= 1100 else sorted({0, 1, n // 2, n - 2, n - 1})
    pairs = [(z, i) for z, h in zip(quizzes, hists) for i in spread(len(h))]
    got = eng.review_answers_batch(pairs, MAX)
    assert len(got) == len(pairs)
    oracle = None if f32 else make_oracle(eng, K, Q, T, tgaps)
    at = 0
    for z, h in zip(quizzes, hists):
        positions = spread(len(h))
        check_rows((shape, f32, len(h)), eng, h, positions, got[at:at + len(positions)], tgaps, T, oracle)
        at += len(positions)
    if oracle is not None:
        oracle.close()
    one = eng.review_answers(quizzes[2], MAX)          # every position of one quiz
    assert len(one) == 3 and all(same(a, b) for a, b in zip(one, [g for g, p in zip(got, pairs) if p[0] == quizzes[2]]))
    print("worst entropy so far, in units of the bar:", WORST["entropy"])
    eng.close()


# ---- 2. order and chunk independence ----------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch(factory):
    K, Q, T = 5, 17, 67
    eng = make_engine(factory, K, Q, T, (3, 66))
    hists = [history(Q, K, n, 50 + n) for n in (3, 17, 30)]
    quizzes = [resume(eng, h) for h in hists]
    base = [(z, i) for z, h in zip(quizzes, hists) for i in range(len(h))]
    alone = {p: eng.review_answers_batch([p], 10)[0] for p in base}
    rng = np.random.default_rng(3)
    shuffled = [base[i] for i in rng.permutation(len(base))]
    interleaved = [p for i in range(30) for p in [(quizzes[k], i) for k in range(3) if i < len(hists[k])]]
    repeated = base[:5] * 3 + [base[7]] * 4
    big = [base[i % len(base)] for i in rng.integers(0, len(base), 600)]        # more than 256 rows: chunks, and the 30-answer quiz split
    for name, pairs in (("shuffled", shuffled), ("interleaved", interleaved), ("repeated", repeated), ("big", big)):
        got = eng.review_answers_batch(pairs, 10)
        assert len(got) == len(pairs)
        for p, g in zip(pairs, got):
            assert same(g, alone[p]) and len(g.targets) == 10, (name, p)
    eng.close()


# ---- 3. options: the twin's bits under the same option --------------------------------------------------------------------------------------
@pytest.mark.parametrize("workers,bug_compat", [(1, 0), (2, 0), (15, 0), (cases.WORKERS, 1), (32, 0)])
def test_workers_and_bug_compat(factory, workers, bug_compat):
    K, Q, T = 5, 17, 67                                                        # 17 vectors: workers 32 splits into fewer subtasks than workers (quot == 0)
    eng = make_engine(factory, K, Q, T, (5,), workers=workers)
    eng.set_option("bug_compat", bug_compat)
    hist = history(Q, K, 6, 11)
    quiz = resume(eng, hist)
    oracle = make_oracle(eng, K, Q, T, (5,))
    check_rows((workers, bug_compat), eng, hist, list(range(6)), eng.review_answers(quiz, MAX), (5,), T, oracle)
    oracle.close()
    eng.close()


# ---- 4. get_quiz_answers ---------------------------------------------------------------------------------------------------------------
def test_get_quiz_answers(factory):
    K, Q, T = 3, 8, 13
    eng = make_engine(factory, K, Q, T)
    lib = interop.load_library()
    fresh = eng.start_quiz()
    assert eng.get_quiz_answers(fresh) == []
    hist = history(Q, K, 4, 2)
    quiz = resume(eng, hist)
    eng.set_active_question(quiz, 6)
    eng.record_answer(quiz, 2)
    want = hist + [(6, 2)]
    assert answers_of(eng, quiz) == want
    n = len(want)
    for capacity in (0, n - 1, n, n + 3):
        arr = (interop.CiAnsweredQuestion * (n + 3))()
        for x in arr:
            x.iQuestion, x.iAnswer = -7, -7
        c_err = ctypes.c_void_p()
        assert lib.PqaHip_GetQuizAnswers(eng.c_engine, ctypes.byref(c_err), quiz, arr if capacity else None, capacity) == n and not c_err.value
        assert [(x.iQuestion, x.iAnswer) for x in arr] == want[:capacity] + [(-7, -7)] * (n + 3 - min(capacity, n))
    for bad_quiz, capacity, code, text in ((99, 0, "Index is out of range", "subjIndex=99"), (quiz, -1, "The count is negative", "count=-1")):
        c_err = ctypes.c_void_p()
        assert lib.PqaHip_GetQuizAnswers(eng.c_engine, ctypes.byref(c_err), bad_quiz, None, capacity) == -1 and c_err.value
        s = interop.PqaError(c_err.value).to_string(True)
        assert s.startswith("[" + code + "]") and text in s, s
    eng.close()


def test_one_process_sharded_engine(factory, monkeypatch):
    monkeypatch.setenv("PQA_DEVICES", "0,0")        # two shards side by side on the one device
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(5, 37, 101, init_amount=0.1))
    assert err is None and eng.get_option("shards") == 2
    hist = history(37, 5, 4, 1)
    quiz = resume(eng, hist)
    eng.set_active_question(quiz, 30)
    eng.record_answer(quiz, 1)
    assert answers_of(eng, quiz) == hist + [(30, 1)]
    err, L, H, R, C = raw_review(eng, [(quiz, 1)], 3)
    s = interop.PqaError(err).to_string(True) if err else ""
    assert s.startswith("[Not implemented]") and "Answer reviews are for whole engines" in s, s
    assert (L == -7.0).all() and (C == -7).all()
    eng.close()


# ---- 5. maxCount and NULL buffers, a dead row -----------------------------------------------------------------------------------------------
def raw_review(eng, pairs, max_count, lik=True, ent=True, dest=True, counts=True, fill=-7.0, n=None):
    """The C call on sentinel-filled buffers -> (error pointer, likelihood, entropy, records as float64 pairs, counts)."""
    pr = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    n = len(pr) if n is None else n
    quizzes, positions = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
    rows = max(len(pr), 1)
    L, H = np.full(rows, fill), np.full(rows, fill)
    C = np.full(rows, int(fill), dtype=np.int64)
    R = np.full((rows * max(max_count, 1), 2), fill)
    err = interop.load_library().PqaEngine_ReviewAnswersBatch(
        eng.c_engine, n, quizzes.ctypes.data_as(P64), positions.ctypes.data_as(P64), max_count, L.ctypes.data_as(PD) if lik else None,
        H.ctypes.data_as(PD) if ent else None, R.ctypes.data_as(PREC) if dest else None, C.ctypes.data_as(P64) if counts else None)
    return err, L, H, R, C


def test_max_counts_and_null_buffers(factory):
    K, Q, T, tgaps = 3, 8, 13, (2, 11)
    eng = make_engine(factory, K, Q, T, tgaps)
    hist = history(Q, K, 3, 9)
    quiz = resume(eng, hist)
    full = eng.review_answers(quiz, MAX)
    pairs = [(quiz, i) for i in range(3)]
    for max_count in (1, 10, T + 5):
        got = eng.review_answers_batch(pairs, max_count)
        for g, f in zip(got, full):
            assert records(g) == records(f)[:max_count] and (g.likelihood, g.entropy) == (f.likelihood, f.entropy)
    err, L, H, R, C = raw_review(eng, pairs, 0, dest=False, counts=False)
    assert not err and L.tolist() == [p.likelihood for p in full] and H.tolist() == [p.entropy for p in full]
    err, L, H, R, C = raw_review(eng, pairs, 4, lik=False)
    assert not err and (L == -7.0).all() and H.tolist() == [p.entropy for p in full] and C.tolist() == [4] * 3
    err, L, H, R, C = raw_review(eng, pairs, 4, ent=False)
    assert not err and (H == -7.0).all() and L.tolist() == [p.likelihood for p in full]
    err, L, H, R, C = raw_review(eng, pairs, 4, lik=False, ent=False)
    rec = np.frombuffer(R.tobytes(), dtype=[("id", "<i8"), ("value", "<f8")])
    assert not err and [(int(r["id"]), float(r["value"])) for r in rec[4:8]] == records(full[1])[:4]
    assert not raw_review(eng, [], 4)[0]                                       # no pairs: no error, nothing written
    eng.close()


@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
def test_dead_rows(factory, f32):
    """Every target a gap: ResumeQuiz over any remaining answers fails with I64Underflow, and StartQuiz's total is 0."""
    K, Q, T = 3, 8, 13
    eng = make_engine(factory, K, Q, T, (), f32)
    quizzes = [resume(eng, history(Q, K, n, 4)) for n in (1, 3)]
    eng.set_target_gaps(list(range(T)))
    with pytest.raises(interop.PqaException) as e:
        resume(eng, history(Q, K, 2, 4))
    assert "I64" in str(e.value) or "exponent" in str(e.value), str(e.value)
    got = eng.review_answers_batch([(quizzes[0], 0)] + [(quizzes[1], i) for i in range(3)], 10)
    for g in got:
        assert math.isnan(g.likelihood) and math.isnan(g.entropy) and g.targets == []
    eng.close()


# ---- 6. state ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("server", [0, 1])
def test_nothing_changes(factory, server):
    K, Q, T = 5, 37, 1000
    eng = make_engine(factory, K, Q, T, (7,))
    eng.set_option("server", server)
    hist = history(Q, K, 4, 21)
    quiz, mirror = resume(eng, hist), resume(eng, hist)                        # the mirror quiz is never reviewed
    for z in (quiz, mirror):
        eng.set_active_question(z, 11)
    eng.record_answer_batch([quiz, mirror], [3, 3])                            # (a deferred RecordAnswerBatch in front)
    for z in (quiz, mirror):
        eng.set_active_question(z, 12)
    calls0, rows0 = eng.get_option("review_calls"), eng.get_option("review_rows")
    got = eng.review_answers(quiz, 10)
    assert len(got) == 5 and (eng.get_option("review_calls"), eng.get_option("review_rows")) == (calls0 + 1, rows0 + 5)
    check_rows(("state", server), eng, hist + [(11, 3)], list(range(5)), eng.review_answers(quiz, MAX), (7,), T)
    assert answers_of(eng, quiz) == hist + [(11, 3)] == answers_of(eng, mirror)
    assert eng.get_active_question_id(quiz) == 12
    assert eng.get_priors(quiz).tobytes() == eng.get_priors(mirror).tobytes()
    assert eng.next_question_argmax(quiz) == eng.next_question_argmax(mirror)
    eng.set_option("time_sweeps", 1)
    ns0 = eng.get_option("review_device_ns")
    eng.review_answers(quiz, 5)
    assert eng.get_option("review_device_ns") > ns0
    eng.close()


# ---- 7. refusals, in the header's order ---------------------------------------------------------------------------------------------------
def test_refusals(factory):
    K, Q, T = 3, 8, 13
    eng = make_engine(factory, K, Q, T)
    quiz, empty = resume(eng, history(Q, K, 3, 1)), eng.start_quiz()
    calls0, rows0 = eng.get_option("review_calls"), eng.get_option("review_rows")
    NEG, NULL, RANGE, MODE = "The count is negative", "Expected non-null argument", "Index is out of range", "An attempt to execute an operation in a wrong mode"
    ok = [(quiz, 1), (quiz, 2)]

    def refused(result, code, *texts):
        err, L, H, R, C = result
        assert err, texts
        s = interop.PqaError(err).to_string(True)
        assert s.startswith("[" + code + "]") and all(t in s for t in texts), s
        assert (L == -7.0).all() and (H == -7.0).all() and (R == -7.0).all() and (C == -7).all()
        assert (eng.get_option("review_calls"), eng.get_option("review_rows")) == (calls0, rows0)

    refused(raw_review(eng, ok, 4, n=-1), NEG, "count=-1", "nPairs")
    refused(raw_review(eng, ok, -2), NEG, "count=-2", "maxCount")
    refused(raw_review(eng, ok, 257), RANGE, "subjIndex=257", "256")
    refused(raw_review(eng, ok, 4, dest=False), NULL)
    refused(raw_review(eng, ok, 4, counts=False), NULL)
    refused(raw_review(eng, [(99, 1)], 4), RANGE, "entry=0", "quizId=99")
    refused(raw_review(eng, ok + [(1 << 40, 1)], 4), RANGE, "entry=2")
    refused(raw_review(eng, ok + [(quiz, 3)], 4), RANGE, "entry=2", "position=3")
    refused(raw_review(eng, [(quiz, -1)] + ok, 4), RANGE, "entry=0", "position=-1")
    refused(raw_review(eng, ok + [(empty, 0)], 4), RANGE, "entry=2", "position=0")   # a quiz without answers refuses every position
    # the order: the counts, the limit, a NULL, the mode, the quiz, the position
    refused(raw_review(eng, ok, -2, n=-1), NEG, "count=-1")
    refused(raw_review(eng, [(99, 9)], 257, dest=False), RANGE, "subjIndex=257")
    refused(raw_review(eng, [(99, 9)], 4, dest=False), NULL)
    refused(raw_review(eng, [(quiz, 9), (99, 1)], 4), RANGE, "entry=1", "quizId=99")
    eng.start_maintenance(True)
    refused(raw_review(eng, [(99, 9)], 4), MODE)
    refused(raw_review(eng, [(99, 9)], 4, counts=False), NULL)
    eng.finish_maintenance()
    quiz = resume(eng, history(Q, K, 3, 1))
    got = eng.review_answers(quiz, 4)                                          # the next good call is correct
    assert [len(p.targets) for p in got] == [4] * 3 and (eng.get_option("review_calls"), eng.get_option("review_rows")) == (calls0 + 1, rows0 + 3)
    calls0, rows0 = calls0 + 1, rows0 + 3
    eng.shutdown()
    refused(raw_review(eng, [(quiz, 1)], 4), MODE)
    eng.close()
