"""PqaEngine_PreviewAnswersBatch on the GPU (include/PqaHipExt.h; preview_kernels.hip; hip_engine_preview.cpp): what each answer would do
to a quiz -- likelihood, entropy and best targets of every would-be posterior -- without changing the quiz.

The truth of a row (quiz, question q, answer k) comes from a TWIN quiz: the live quiz's record_answer sequence, then
set_active_question(q), record_answer(k), get_priors.  The twin is held to orclib.Oracle.record_answer as well, bit for bit (an engine
with option "workers" = cases.WORKERS runs RecordAnswer's sum over cases.WORKERS - 1 subtasks, reference PqaCore/CEQuiz.h:98 -- the count
the oracle is given, as tests/golden/make_golden.py gives it).

Records must EQUAL numpy's listing of the twin's posterior by (-p, id) over the non-gap p > 0, id and probability bits.
The bars of the two numbers are derived, not measured:
  likelihood: within (T + 16) 2^-52 relative of math.fsum(prior (A / D)) in numpy fp64 over get_priors / get_kb -- every term is
    non-negative and carries two roundings, and any summation order of n non-negative terms stays within n 2^-53 relative;
  entropy: |H - H_ref| <= (T + 16) 2^-52 max(1, H_ref) bits, H_ref = -math.fsum(p log2 p) over the twin's posterior: every term is >= 0,
    so the sum of the terms' magnitudes is H itself.
The worst seen of either is printed (in units of its bar)."""
import ctypes
import math

import numpy as np
import pytest

import cases
import orclib
from probqa_amd import interop

pytestmark = pytest.mark.gpu

F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)
P64, PD, PREC = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(interop.CiRatedTarget)
EPS = 2.0 ** -52

# K, Q, T, target gaps: the smallest shapes that reach each edge of the kernels
SHAPES = {
    "min_2x1x2": (2, 1, 2, ()),
    "gaps_3x8x12": (3, 8, 12, (2, 11)),                     # target gaps
    "padded_3x8x13": (3, 8, 13, (2, 11)),                   # ... and T mod 4 != 0: the padded last vector
    "ragged_5x17x67": (5, 17, 67, ()),                      # 17 vectors over 15 subtasks: chains of one and two (quot == 0: test_quot_zero_split)
    "small_5x12x1024": (5, 12, 1024, (1023,)),              # the two thread shapes of the update kernels
    "large_5x12x1025": (5, 12, 1025, ()),
    "oddk_7x9x130": (7, 9, 130, (0,)),
    "nolds_3x6x9000": (3, 6, 9000, (4500,)),                # the stage does not fit LDS
    "long_2x4x16400": (2, 4, 16400, ()),                    # beyond 16384: the twin's RecordAnswer runs the long-row launches
}
WORST = {"likelihood": 0.0, "entropy": 0.0}


def make_engine(factory, K, Q, T, tgaps=(), f32=False, seed=7, init=0.1, fill=True, workers=cases.WORKERS):
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=init, **(F32 if f32 else {})))
    assert err is None and eng is not None, err
    if fill:
        eng.fill_synthetic(8.0, 0.5, seed)
    eng.set_option("workers", workers)
    if tgaps:
        eng.set_target_gaps(list(tgaps))
    return eng


def history(Q, K, n, seed):
    """n answers; the questions cycle through a permutation, so a knowledge base of few questions answers some again."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(Q)
    return [(int(perm[i % Q]), int(rng.integers(K))) for i in range(n)]


def play(eng, hist):
    quiz = eng.start_quiz()
    for q, a in hist:
        eng.set_active_question(quiz, q)
        eng.record_answer(quiz, a)
    return quiz


def twin_posterior(eng, hist, q, k):
    quiz = play(eng, list(hist) + [(q, k)])
    pri = eng.get_priors(quiz)
    eng.release_quiz(quiz)
    return pri


def listing(p, tgaps, max_count):
    ids = np.arange(len(p))
    ok = (p > 0) & ~np.isin(ids, list(tgaps))
    c, pc = ids[ok], p[ok]
    take = np.lexsort((c, -pc))[:max_count]
    return [(int(t), float(x)) for t, x in zip(c[take], pc[take])]


def records(preview):
    return [(t.i_target, t.prob) for t in preview.targets]


def entropy_of(p, tgaps):
    v = np.delete(p, list(tgaps)) if len(tgaps) else p
    v = v[v > 0]
    return -math.fsum((v * np.log2(v)).tolist())


def check_row(name, got, eng_kb, prior, twin, tgaps, q, k, max_count, T):
    A, D, _ = eng_kb
    assert records(got) == listing(twin, tgaps, max_count), (name, records(got)[:4], listing(twin, tgaps, max_count)[:4])
    valid = np.ones(T, dtype=bool)
    valid[list(tgaps)] = False
    want = math.fsum((prior[valid] * (A[q][k][valid] / D[q][valid])).tolist())
    dl = abs(got.likelihood - want) / ((T + 16) * EPS * want)
    h_ref = entropy_of(twin, tgaps)
    dh = abs(got.entropy - h_ref) / ((T + 16) * EPS * max(1.0, h_ref))
    WORST["likelihood"], WORST["entropy"] = max(WORST["likelihood"], dl), max(WORST["entropy"], dh)
    print("%s: likelihood %.17g want %.17g (%.3f of the bar); entropy %.17g want %.17g (%.3f of the bar)" % (name, got.likelihood, want, dl, got.entropy, h_ref, dh))
    assert dl <= 1.0, (name, got.likelihood, want)
    assert dh <= 1.0, (name, got.entropy, h_ref)


def oracle_posterior(eng, K, Q, T, init, tgaps, hist, q, k):
    o = orclib.Oracle(K, Q, T, init)
    o.set_kb(*eng.get_kb())
    o.set_target_gaps(list(tgaps))
    o.start_quiz(cases.WORKERS)
    for qq, aa in list(hist) + [(q, k)]:
        o.record_answer(qq, aa, cases.WORKERS - 1)
    pri = o.priors()
    o.close()
    return pri


# ---- 1. every shape, both precisions, three quiz states, one call ------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_rows_are_the_twins(factory, shape, f32):
    K, Q, T, tgaps = SHAPES[shape]
    eng = make_engine(factory, K, Q, T, tgaps, f32)
    kb = eng.get_kb()
    hists = [history(Q, K, n, 31 + n) for n in sorted({0, 3, min(Q - 1, 12)})]   # fresh, after 3 answers, after min(Q - 1, 12)
    quizzes = [play(eng, h) for h in hists]
    pairs, meta = [], []
    for quiz, hist in zip(quizzes, hists):
        asked = [q for q, _ in hist]
        qs = sorted({0, Q - 1, Q // 2} | set(asked[:1]))                         # one quiz under several questions, an asked one among them
        for q in qs:
            pairs.append((quiz, q))
            meta.append((quiz, hist, q))
    max_count = 10
    got = eng.preview_answers_batch(pairs, max_count)
    assert len(got) == len(pairs) and all(len(g) == K for g in got)
    priors = {quiz: eng.get_priors(quiz) for quiz in quizzes}
    for (quiz, hist, q), previews in zip(meta, got):
        for k in range(K):
            twin = twin_posterior(eng, hist, q, k)
            assert np.isfinite(twin).all()
            check_row((shape, f32, len(hist), q, k), previews[k], kb, priors[quiz], twin, tgaps, q, k, max_count, T)
            if len(hist) == 3 or Q == 1:   # the twin itself, held to the oracle
                assert twin.tobytes() == oracle_posterior(eng, K, Q, T, 0.1, tgaps, hist, q, k).tobytes(), (shape, f32, q, k)
    print("worst so far, in units of the bar:", WORST)
    eng.close()


def test_quot_zero_split(factory):
    """Fewer vectors than subtasks (quot == 0): T = 67 is 17 vectors, option "workers" 32 makes RecordAnswer's split 31 subtasks."""
    K, Q, T = 5, 17, 67
    eng = make_engine(factory, K, Q, T, workers=32)
    hist = history(Q, K, 3, 5)
    quiz = play(eng, hist)
    got = eng.preview_answers(quiz, 4, 10)
    for k in range(K):
        twin = twin_posterior(eng, hist, 4, k)
        assert records(got[k]) == listing(twin, (), 10), k
    eng.close()


# ---- 2. ties: a fresh init_amount-only KB ------------------------------------------------------------------------------------------------
def test_order_among_ties(factory):
    K, Q, T = 3, 8, 301
    eng = make_engine(factory, K, Q, T, fill=False, init=1.0)
    quiz = eng.start_quiz()
    for max_count in (10, 256):
        got = eng.preview_answers(quiz, 5, max_count)
        for k in range(K):
            twin = twin_posterior(eng, [], 5, k)
            assert len(set(twin.tolist())) == 1
            assert [t.i_target for t in got[k].targets] == list(range(max_count)), (max_count, k)
            assert records(got[k]) == listing(twin, (), max_count)
            assert abs(got[k].likelihood - 1.0 / K) <= (T + 16) * EPS / K
            assert abs(got[k].entropy - math.log2(T)) <= (T + 16) * EPS * math.log2(T)
    eng.close()


# ---- 3. 300 rows across the 256-row chunk, a repeated pair, every row equal to the row previewed alone -----------------------------------
def test_rows_do_not_depend_on_the_batch(factory):
    K, Q, T = 5, 17, 67
    eng = make_engine(factory, K, Q, T, (3, 66))
    quizzes = [play(eng, history(Q, K, n, 50 + n)) for n in (0, 3, 12)]
    pairs = [(quizzes[i % 3], (7 * i) % Q) for i in range(58)] + [(quizzes[1], 4), (quizzes[1], 4)]   # 60 pairs x 5 = 300 rows; pair 51 straddles the chunk
    assert len(pairs) * K == 300
    got = eng.preview_answers_batch(pairs, 10)
    alone = {}
    for pair, previews in zip(pairs, got):
        if pair not in alone:
            alone[pair] = eng.preview_answers(pair[0], pair[1], 10)
        for a, b in zip(previews, alone[pair]):
            assert records(a) == records(b) and len(a.targets) == 10
            assert np.float64(a.likelihood).tobytes() == np.float64(b.likelihood).tobytes()
            assert np.float64(a.entropy).tobytes() == np.float64(b.entropy).tobytes()
    eng.close()


# ---- 4. maxCount and NULL buffers -----------------------------------------------------------------------------------------------------------
def raw_preview(eng, pairs, max_count, K, lik=True, ent=True, dest=True, counts=True, fill=-7.0):
    """The C call on sentinel-filled buffers -> (error pointer, likelihood, entropy, records as float64 pairs, counts)."""
    pr = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    n = len(pr)
    quizzes, questions = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
    rows = max(n * K, 1)
    L, H = np.full(rows, fill), np.full(rows, fill)
    C = np.full(rows, int(fill), dtype=np.int64)
    R = np.full((rows * max(max_count, 1), 2), fill)
    err = interop.load_library().PqaEngine_PreviewAnswersBatch(
        eng.c_engine, n, quizzes.ctypes.data_as(P64), questions.ctypes.data_as(P64), max_count, L.ctypes.data_as(PD) if lik else None,
        H.ctypes.data_as(PD) if ent else None, R.ctypes.data_as(PREC) if dest else None, C.ctypes.data_as(P64) if counts else None)
    return err, L, H, R, C


def test_max_counts_and_null_buffers(factory):
    K, Q, T, tgaps = 3, 8, 13, (2, 11)
    eng = make_engine(factory, K, Q, T, tgaps)
    hist = history(Q, K, 3, 9)
    quiz = play(eng, hist)
    twins = [twin_posterior(eng, hist, 6, k) for k in range(K)]
    full = eng.preview_answers(quiz, 6, 256)
    candidates = [int(((tw > 0) & ~np.isin(np.arange(T), tgaps)).sum()) for tw in twins]
    for max_count in (1, 10, 256, T + 5):                                      # 10 of 11 candidates; 256 and T + 5: more than there are
        got = eng.preview_answers(quiz, 6, max_count)
        for k in range(K):
            assert records(got[k]) == listing(twins[k], tgaps, max_count) and len(got[k].targets) == min(max_count, candidates[k])
            assert (got[k].likelihood, got[k].entropy) == (full[k].likelihood, full[k].entropy)
    # maxCount 0: no records, and neither their buffer nor the counts are needed
    err, L, H, R, C = raw_preview(eng, [(quiz, 6)], 0, K, dest=False, counts=False)
    assert not err and L.tolist() == [p.likelihood for p in full] and H.tolist() == [p.entropy for p in full]
    err, L, H, R, C = raw_preview(eng, [(quiz, 6)], 0, K, dest=False)
    assert not err and (C == 0).all() and L.tolist() == [p.likelihood for p in full]
    # either number may be left out
    err, L, H, R, C = raw_preview(eng, [(quiz, 6)], 4, K, lik=False)
    assert not err and (L == -7.0).all() and H.tolist() == [p.entropy for p in full] and C.tolist() == [4] * K
    err, L, H, R, C = raw_preview(eng, [(quiz, 6)], 4, K, ent=False)
    assert not err and (H == -7.0).all() and L.tolist() == [p.likelihood for p in full]
    err, L, H, R, C = raw_preview(eng, [(quiz, 6)], 4, K, lik=False, ent=False)
    assert not err and C.tolist() == [4] * K
    rec = np.frombuffer(R.tobytes(), dtype=[("id", "<i8"), ("value", "<f8")])
    for k in range(K):
        assert [(int(r["id"]), float(r["value"])) for r in rec[4 * k:4 * k + 4]] == listing(twins[k], tgaps, 4)
    assert not raw_preview(eng, [], 4, K)[0]                                   # no pairs: no error, nothing written
    eng.close()


# ---- 5. a dead answer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
def test_dead_answer(factory, f32):
    K, Q, T = 3, 8, 130
    eng = make_engine(factory, K, Q, T, (5,), f32)
    A, D, B = eng.get_kb()
    q, dead = 2, 1
    A[q][dead][:] = 0.0
    D[q] = A[q][0] + A[q][2]
    eng.set_kb(A, D, B)
    hist = [(h, a) for h, a in history(Q, K, 3, 3) if h != q]
    quiz = play(eng, hist)
    before = eng.get_priors(quiz)
    got = eng.preview_answers_batch([(quiz, q), (quiz, 4)], 10)
    assert got[0][dead].likelihood == 0.0 and math.isnan(got[0][dead].entropy) and got[0][dead].targets == []
    kb = eng.get_kb()
    for qq, previews in ((q, got[0]), (4, got[1])):
        for k in range(K):
            if (qq, k) != (q, dead):                                           # the other answers are unaffected
                check_row(("dead", f32, qq, k), previews[k], kb, before, twin_posterior(eng, hist, qq, k), (5,), qq, k, 10, T)
    assert eng.get_priors(quiz).tobytes() == before.tobytes()
    eng.close()


# ---- 6. state, counters, the recorded answer -------------------------------------------------------------------------------------------------
def test_nothing_changes_and_the_recorded_answer_lists_the_preview(factory):
    K, Q, T = 5, 37, 1025
    eng = make_engine(factory, K, Q, T, (7,))
    eng.set_option("top_exact", 0)
    hist = history(Q, K, 4, 21)
    quiz, mirror = play(eng, hist), play(eng, hist)                            # the mirror quiz is never previewed
    for z in (quiz, mirror):
        eng.set_active_question(z, 11)
    pri0, act0, ev0 = eng.get_priors(quiz), eng.get_active_question_id(quiz), eng.eval_priorities(quiz)
    calls0, pairs0 = eng.get_option("preview_calls"), eng.get_option("preview_pairs")
    pairs = [(quiz, 11), (quiz, hist[0][0]), (quiz, 30)]
    got = eng.preview_answers_batch(pairs, 10)
    assert (eng.get_option("preview_calls"), eng.get_option("preview_pairs")) == (calls0 + 1, pairs0 + len(pairs))
    assert eng.get_priors(quiz).tobytes() == pri0.tobytes() and eng.get_active_question_id(quiz) == act0 == 11
    assert eng.eval_priorities(quiz).tobytes() == ev0.tobytes()
    assert eng.next_question_argmax(quiz) == eng.next_question_argmax(mirror)
    # a deferred answer is applied first: record, preview at once, and the preview is of the updated quiz
    eng.set_active_question(quiz, 11)
    eng.record_answer(quiz, 3)
    assert [(t.i_target, t.prob) for t in eng.list_top_targets(quiz, 10)] == records(got[0][3])   # the previewed records are the recorded answer's
    eng.set_active_question(quiz, 20)
    eng.record_answer(quiz, 1)
    after = eng.preview_answers(quiz, 30, 5)                                   # (no call in between: the answer to 20 may still be pending)
    twin = twin_posterior(eng, hist + [(11, 3), (20, 1)], 30, 2)
    assert records(after[2]) == listing(twin, (7,), 5)
    eng.set_option("time_sweeps", 1)
    ns0 = eng.get_option("preview_device_ns")
    eng.preview_answers(quiz, 30, 5)
    assert eng.get_option("preview_device_ns") > ns0
    eng.close()


# ---- 7. refusals, in the header's order ---------------------------------------------------------------------------------------------------
def test_refusals(factory):
    K, Q, T = 3, 8, 13
    eng = make_engine(factory, K, Q, T)
    eng.set_question_gaps([5])
    quiz = eng.start_quiz()
    calls0, pairs0 = eng.get_option("preview_calls"), eng.get_option("preview_pairs")
    NEG, NULL, RANGE, MODE = "The count is negative", "Expected non-null argument", "Index is out of range", "An attempt to execute an operation in a wrong mode"
    lib = interop.load_library()
    ok = [(quiz, 1), (quiz, 2)]

    def refused(result, code, *texts):
        err, L, H, R, C = result
        assert err, texts
        s = interop.PqaError(err).to_string(True)
        assert s.startswith("[" + code + "]") and all(t in s for t in texts), s
        assert (L == -7.0).all() and (H == -7.0).all() and (R == -7.0).all() and (C == -7).all()
        assert (eng.get_option("preview_calls"), eng.get_option("preview_pairs")) == (calls0, pairs0)

    def negative_pairs(max_count):
        L, H, C, R = np.full(4, -7.0), np.full(4, -7.0), np.full(4, -7, dtype=np.int64), np.full((4, 2), -7.0)
        return lib.PqaEngine_PreviewAnswersBatch(eng.c_engine, -1, None, None, max_count, L.ctypes.data_as(PD), H.ctypes.data_as(PD), R.ctypes.data_as(PREC), C.ctypes.data_as(P64)), L, H, R, C

    refused(negative_pairs(4), NEG, "count=-1", "nPairs")
    refused(raw_preview(eng, ok, -2, K), NEG, "count=-2", "maxCount")
    refused(raw_preview(eng, ok, 257, K), RANGE, "subjIndex=257", "256")
    refused(raw_preview(eng, ok, 4, K, dest=False), NULL)
    refused(raw_preview(eng, ok, 4, K, counts=False), NULL)
    refused(raw_preview(eng, [(99, 1)], 4, K), RANGE, "entry=0")
    refused(raw_preview(eng, ok + [(1 << 40, 1)], 4, K), RANGE, "entry=2")
    refused(raw_preview(eng, ok + [(quiz, Q)], 4, K), RANGE, "entry=2", "questionId=%d" % Q)
    refused(raw_preview(eng, [(quiz, -1)] + ok, 4, K), RANGE, "entry=0", "questionId=-1")
    refused(raw_preview(eng, ok + [(quiz, 5)], 4, K), RANGE, "entry=2", "questionId=5", "gap")
    # the order: the counts, the limit, a NULL, the quiz, the question
    refused(negative_pairs(-2), NEG, "count=-1")
    refused(raw_preview(eng, [(99, Q)], 257, K, dest=False), RANGE, "subjIndex=257")
    refused(raw_preview(eng, [(99, Q)], 4, K, dest=False), NULL)
    refused(raw_preview(eng, [(quiz, Q), (99, 1)], 4, K), RANGE, "entry=1", "quizId=99")
    # maintenance mode and shutdown, as ListTopTargetsBatch answers them -- in front of the quiz and the question, behind a NULL
    eng.start_maintenance(True)
    refused(raw_preview(eng, [(99, Q)], 4, K), MODE)
    refused(raw_preview(eng, [(99, Q)], 4, K, counts=False), NULL)
    eng.finish_maintenance()
    quiz = eng.start_quiz()
    got = eng.preview_answers(quiz, 1, 4)                                      # the next good call is correct
    assert [len(p.targets) for p in got] == [4] * K and (eng.get_option("preview_calls"), eng.get_option("preview_pairs")) == (calls0 + 1, pairs0 + 1)
    calls0, pairs0 = calls0 + 1, pairs0 + 1
    eng.shutdown()
    refused(raw_preview(eng, [(quiz, 1)], 4, K), MODE)
    eng.close()


def test_one_process_sharded_engine_refuses(factory, monkeypatch):
    monkeypatch.setenv("PQA_DEVICES", "0,0")        # two shards side by side on the one device
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(5, 37, 101, init_amount=0.1))
    assert err is None and eng.get_option("shards") == 2
    quiz = eng.start_quiz()
    err, L, H, R, C = raw_preview(eng, [(quiz, 1)], 3, 5)
    s = interop.PqaError(err).to_string(True) if err else ""
    assert s.startswith("[Not implemented]") and "Answer previews are for whole engines" in s, s
    assert (L == -7.0).all() and (C == -7).all()
    eng.close()
