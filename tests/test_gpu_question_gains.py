"""The information gain of every question of a quiz on the GPU (include/PqaHipExt.h: PqaEngine_EvalQuestionGainsBatch,
PqaEngine_ListInformativeQuestionsBatch; gain_kernels.hip; hip_engine_gain.cpp).

The model works over one get_kb() and get_priors(): r = A * (1.0 / D) in numpy fp64 -- the kernel's own product, its reciprocal
(pqa_device.h: div_nr) being IEEE division's -- and p the posterior with zeros at the target gaps and where it is not > 0.  It evaluates the
TABLE definition, not the kernel's algebra: with J[k][t] = p_t r_k(t), W_k the row totals, c_t the column totals and Z the total,
    gain = sum over J > 0 of (J / Z) log2(J Z / (W_k c_t))
in Python floats with math.log2 and math.fsum.  The bar is derived, not measured, and ABSOLUTE (a gain may be near 0):
    |gpu - model| <= (T + 16) (K + 8) 2^-52 bits
-- the target sums carry up to T accumulations of non-negative terms whose total is at most Z log2 K; each element carries K + 1 one-ulp
logarithms and about two roundings per product of magnitude <= 0.54, plus the reciprocal's allowance.  A wrong term shows as 1e-3 bits or
more.  Worst seen on an MI355X over every case of this file: see README.md.
Listings are held to the engine's own Eval rows record for record, bit for bit."""
import ctypes
import math

import numpy as np
import pytest

import cases
from probqa_amd import interop

pytestmark = pytest.mark.gpu

F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)
AQ = interop.AnsweredQuestion
P64, PD, PREC = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(interop.CiRatedQuestion)
TILE = {2: 16, 3: 12, 4: 8, 5: 8}    # quizzes of a tile of the sweep (pqa_kernels.h: GainTileWidth); other answer counts go quiz by quiz
CHUNK = 256                           # quizzes of a chunk of the host's loop (kTopBatchQuizzes)
EPS = 2.0 ** -52


def bar(T, K):
    return (T + 16) * (K + 8) * EPS


class Plant:
    """what set_kb planted among the questions that are no gaps: a question with a run of exact zeros under answer `kz` (answering it
    leaves exact zeros in the posterior) and nothing at all under answer `kd` (answering that kills the quiz), a question every target
    answers alike, a question block copied bitwise to another id"""

    def __init__(self, Q, K, T, qgaps):
        free = [q for q in range(Q) if q not in qgaps]
        self.qz, self.kz, self.kd = free[0], 0, K - 1
        self.zeros = range(T // 5, T // 5 + max(2, T // 10))
        self.alike = free[1] if len(free) >= 2 else None
        self.copy = (free[2], free[-1]) if len(free) >= 4 else None


def make_engine(factory, K, Q, T, tgaps=(), qgaps=(), seed=7, trains=3, plant=True, **kw):
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **kw))
    assert err is None and eng is not None, err
    eng.fill_synthetic(8.0, 0.5, seed)
    eng.set_option("workers", cases.WORKERS)
    rng = np.random.default_rng(seed)
    free_t = [t for t in range(T) if t not in tgaps]
    for _ in range(trains):
        qs = rng.permutation(Q)[:min(3, Q)]
        eng.train([AQ(int(q), int(rng.integers(K))) for q in qs], int(rng.choice(free_t)), 1.5)
    pl = Plant(Q, K, T, qgaps) if plant else None
    if pl:
        A, D, B = eng.get_kb()
        A[pl.qz, pl.kz, pl.zeros.start:pl.zeros.stop] = 0.0
        A[pl.qz, pl.kd, :] = 0.0
        if pl.alike is not None:   # r_k = (k + 1) / 8 at every target, exact in either precision
            D[pl.alike, :] = 8.0
            for k in range(K):
                A[pl.alike, k, :] = k + 1.0
        if pl.copy:
            A[pl.copy[1]], D[pl.copy[1]] = A[pl.copy[0]], D[pl.copy[0]]
        eng.set_kb(A, D, B)
    if tgaps:
        eng.set_target_gaps(list(tgaps))
    if qgaps:
        eng.set_question_gaps(list(qgaps))
    return eng, pl


def history(Q, K, n, seed, avoid=()):
    """n answers to distinct questions where the knowledge base has as many; the questions cycle through a permutation"""
    rng = np.random.default_rng(seed)
    perm = [int(q) for q in rng.permutation(Q) if int(q) not in avoid]
    return [(perm[i % len(perm)], int(rng.integers(K))) for i in range(n)]


def play(eng, hist):
    quiz = eng.start_quiz()
    for q, a in hist:
        eng.set_active_question(quiz, q)
        eng.record_answer(quiz, a)
    return quiz


def clean_posterior(eng, quiz, tgaps):
    p = eng.get_priors(quiz).copy()
    p[list(tgaps)] = 0.0
    p[~(p > 0)] = 0.0
    return p


class Model:
    """gain(quiz, q) by the table definition over one get_kb()"""

    def __init__(self, A, D, tgaps, qgaps):
        self.Q, self.K, self.T = A.shape
        self.qgaps = set(qgaps)
        with np.errstate(all="ignore"):
            self.r = A * (1.0 / D)[:, None, :]
        self.r[:, :, list(tgaps)] = 0.0

    def gain(self, p, q):
        if q in self.qgaps:
            return 0.0
        J = (p[None, :] * self.r[q]).tolist()
        W = [math.fsum(row) for row in J]
        Z = math.fsum(W)
        if not Z > 0 or not math.isfinite(Z):
            return 0.0
        c = [math.fsum(col) for col in zip(*J)]
        log2 = math.log2
        return max(0.0, math.fsum((j / Z) * log2(j * Z / (W[k] * c[t])) for k, row in enumerate(J) for t, j in enumerate(row) if j > 0))

    def row(self, p):
        return np.array([self.gain(p, q) for q in range(self.Q)])


WORST = {"bits": 0.0, "of_bar": 0.0}


def within_bar(name, got_row, ref_row, T, K):
    err = float(np.abs(got_row - ref_row).max())
    WORST["bits"], WORST["of_bar"] = max(WORST["bits"], err), max(WORST["of_bar"], err / bar(T, K))
    print("%s: worst deviation %.3g bits, bar %.3g (worst so far %.3g bits, %.3g of its bar)" % (name, err, bar(T, K), WORST["bits"], WORST["of_bar"]))
    assert err <= bar(T, K), (name, err, bar(T, K))


def listing_of_row(row, max_count, asked=(), q_first=0):
    """what the listing must be, from the engine's own Eval row: value > 0 (gaps are 0), not asked (GLOBAL ids), by (-value, id)"""
    ids = np.array([q for q in range(len(row)) if row[q] > 0 and q_first + q not in asked], dtype=np.int64)
    if len(ids) == 0:
        return []
    take = np.lexsort((ids, -row[ids]))[:max_count]
    return [(int(q_first + q), float(row[q])) for q in ids[take]]


def asked_of(eng, quiz):
    return {a.i_question for a in eng.get_quiz_answers(quiz)}


# ---- rows against the model, listings against the rows --------------------------------------------------------------------------------
SHAPES = {
    "q8_k3_t12": dict(Q=8, K=3, T=12),
    "q37_k5_t101_gaps": dict(Q=37, K=5, T=101, tgaps=(3, 17, 100), qgaps=(0, 5, 36)),
    "q33_k7_t130_generic": dict(Q=33, K=7, T=130),
    "q50_k4_t67": dict(Q=50, K=4, T=67),
    "q20_k2_t257": dict(Q=20, K=2, T=257),
    "q12_k5_t1000": dict(Q=12, K=5, T=1000),
    "q12_k5_t1025": dict(Q=12, K=5, T=1025),
    "q6_k5_t4099_long_row": dict(Q=6, K=5, T=4099),
    "q3_k2_t16400_long_row": dict(Q=3, K=2, T=16400),
    "f32_q37_k5_t101_gaps": dict(Q=37, K=5, T=101, tgaps=(3, 17, 100), qgaps=(0, 5, 36), f32=True),
    "f32_q20_k2_t257": dict(Q=20, K=2, T=257, f32=True),
    "f32_q6_k5_t4099_long_row": dict(Q=6, K=5, T=4099, f32=True),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rows_and_listings(factory, name):
    sh = dict(SHAPES[name])
    K, Q, T, tgaps, qgaps = sh["K"], sh["Q"], sh["T"], sh.get("tgaps", ()), sh.get("qgaps", ())
    eng, pl = make_engine(factory, K, Q, T, tgaps, qgaps, **(F32 if sh.get("f32") else {}))
    A, D, B = eng.get_kb()
    model = Model(A, D, tgaps, qgaps)
    # fresh, after 1, 3 and 8 answers (never the planted answers), one with exact zeros in its posterior, one dead
    hists = [history(Q, K, n, 31 + n, avoid=set(qgaps) | {pl.qz}) for n in (0, 1, 3, 8)]
    quizzes = [play(eng, h) for h in hists]
    zq = play(eng, hists[1] + [(pl.qz, pl.kz)])
    quizzes.append(zq)
    pz = eng.get_priors(zq)
    assert (pz[pl.zeros.start:pl.zeros.stop] == 0.0).all() and (pz > 0).sum() >= 2     # the zeros are there, exact
    dead = play(eng, [(pl.qz, pl.kd)])
    pd = eng.get_priors(dead)
    assert not (pd > 0).any(), pd[:8]                                                   # nothing is > 0: Z == 0
    posteriors = [clean_posterior(eng, z, tgaps) for z in quizzes]
    calls0, n0 = eng.get_option("gain_calls"), eng.get_option("gain_quizzes")
    got = eng.eval_question_gains_batch(quizzes + [dead])
    assert got.shape == (len(quizzes) + 1, Q)
    assert eng.get_option("gain_calls") == calls0 + 1 and eng.get_option("gain_quizzes") == n0 + len(quizzes) + 1
    assert eng.eval_question_gains_batch(quizzes + [dead]).tobytes() == got.tobytes()    # the same call, the same bytes
    assert not got[-1].any() and eng.list_informative_questions(dead, 10) == []         # a dead quiz: a row of zeros, nothing listed
    for i, z in enumerate(quizzes):
        want = model.row(posteriors[i])
        within_bar((name, i), got[i], want, T, K)
        assert (got[i] >= 0).all() and (got[i] <= math.log2(K) + bar(T, K)).all()
        for q in asked_of(eng, z):                                                       # an asked question is evaluated like any other
            if want[q] > bar(T, K):
                assert got[i, q] > 0, (name, i, q, got[i, q], want[q])
        assert clean_posterior(eng, z, tgaps).tobytes() == posteriors[i].tobytes()       # the posterior is as it was
    if qgaps:
        assert not got[:, list(qgaps)].any()
    live = [q for q in range(Q) if q not in qgaps and q not in (pl.alike, pl.qz)]
    assert (got[:len(quizzes)][:, live] > 1e-6).sum() >= len(quizzes) * len(live) // 2  # the cube informs: nothing hides under the absolute bar
    # the planted structure
    if pl.alike is not None:
        assert (got[:, pl.alike] <= bar(T, K)).all(), got[:, pl.alike]
    if pl.copy:
        assert got[:, pl.copy[0]].tobytes() == got[:, pl.copy[1]].tobytes()              # a copied block, the same bits for every quiz
        assert (got[:, pl.copy[0]] > 0).any()
    # every quiz alone (a tile of one), the batch in reverse order, a quiz listed twice
    for i, z in enumerate(quizzes):
        assert eng.eval_question_gains_batch([z])[0].tobytes() == got[i].tobytes(), (name, i)
    assert eng.eval_question_gains_batch((quizzes + [dead])[::-1])[::-1].tobytes() == got.tobytes()
    twice = eng.eval_question_gains_batch([quizzes[2], quizzes[3], quizzes[2]])
    assert twice[0].tobytes() == twice[2].tobytes() == got[2].tobytes()
    # listings: the engine's own rows, record for record
    for max_count in (0, 1, 10, 300):
        listed = eng.list_informative_questions_batch(quizzes + [dead], max_count)
        assert len(listed) == len(quizzes) + 1
        for i, z in enumerate(quizzes):
            assert listed[i] == listing_of_row(got[i], max_count, asked_of(eng, z)), (name, max_count, i)
        assert listed[-1] == []
        assert not {q for lst in listed for q, _ in lst} & set(qgaps)
    assert eng.list_informative_questions(quizzes[3], 3) == listing_of_row(got[3], 3, asked_of(eng, quizzes[3]))
    assert eng.eval_question_gains_batch([]).shape == (0, Q) and eng.list_informative_questions_batch([], 5) == []
    print("worst so far:", WORST)
    eng.close()


# ---- the gain is what the status and preview calls compose ------------------------------------------------------------------------------
@pytest.mark.parametrize("K,Q,T", [(5, 12, 101), (2, 9, 1025), (7, 6, 130)])
def test_gain_is_entropy_now_minus_expected_entropy(factory, K, Q, T):
    """On a knowledge base of integer counts with D == sum_k A bit for bit, the gain equals _entropy of QuizStatusBatch minus
    sum_k likelihood_k entropy_k of PreviewAnswersBatch within this call's bar plus the status bar plus K preview bars (each
    (T + 16) 2^-52 max(1, H)); dead answers are left out."""
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=1.0))
    assert err is None
    eng.set_option("workers", cases.WORKERS)
    rng = np.random.default_rng(3)
    A = rng.integers(1, 40, size=(Q, K, T)).astype(np.float64)
    A[1, 0, : T // 3] = 0.0                      # an answer some targets never give
    D = A.sum(axis=1)
    B = rng.integers(1, 9, size=T).astype(np.float64)
    eng.set_kb(A, D, B)
    A2, D2, _ = eng.get_kb()
    assert A2.tobytes() == A.tobytes() and D2.tobytes() == D.tobytes() and (A2.sum(axis=1) == D2).all()
    quizzes = [play(eng, history(Q, K, n, 70 + n)) for n in (0, 3)]
    got = eng.eval_question_gains_batch(quizzes)
    status = eng.quiz_status_batch(quizzes)
    worst = 0.0
    for i, z in enumerate(quizzes):
        previews = eng.preview_answers_batch([(z, q) for q in range(Q)], 0)
        for q in range(Q):
            live = [p for p in previews[q] if p.likelihood > 0 and not math.isnan(p.entropy)]
            composed = status[i].entropy - math.fsum(p.likelihood * p.entropy for p in live)
            allowed = bar(T, K) + (T + 16) * EPS * max(1.0, status[i].entropy) + sum((T + 16) * EPS * max(1.0, p.entropy) for p in live) \
                + (K - len(live)) * (T + 16) * EPS
            worst = max(worst, abs(got[i, q] - composed) / allowed)
            assert abs(got[i, q] - composed) <= allowed, (i, q, got[i, q], composed, allowed)
    print("gain against status - preview: worst %.3g of the allowed difference" % worst)
    eng.close()


# ---- tiles and chunks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,f32", [(5, False), (2, False), (3, True), (7, False)])
def test_a_row_does_not_depend_on_the_batch(factory, K, f32):
    """A quiz evaluated alone, at positions 0 / 3 / last of batches of 2, a tile, a tile and one, and 257 quizzes (two chunks), and
    listed twice in one call has a byte-identical row; so has every other quiz of those batches."""
    Q, T = 37, 101
    eng, pl = make_engine(factory, K, Q, T, tgaps=(3, 17, 100), qgaps=(0, 5, 36), **(F32 if f32 else {}))
    pool = [play(eng, history(Q, K, n, 90 + n, avoid={0, 5, 36, pl.qz})) for n in (0, 1, 2, 3, 5, 8, 13)]
    probe = pool[3]
    alone = {z: eng.eval_question_gains_batch([z])[0].tobytes() for z in pool}
    assert len(set(alone.values())) == len(pool)
    nq = TILE.get(K, 1)
    for size in sorted({2, max(nq, 2), nq + 1, CHUNK + 1}):
        for pos in sorted({0, min(3, size - 1), size - 1}):
            batch = [pool[(i * 5 + size) % len(pool)] for i in range(size)]
            batch[pos] = probe
            got = eng.eval_question_gains_batch(batch)
            assert got[pos].tobytes() == alone[probe], (K, size, pos)
            for i, z in enumerate(batch):
                assert got[i].tobytes() == alone[z], (K, size, pos, i)
            listed = eng.list_informative_questions_batch(batch, 4)
            for i in (0, pos, size - 1):
                assert listed[i] == listing_of_row(got[i], 4, asked_of(eng, batch[i])), (K, size, pos, i)
    twice = eng.eval_question_gains_batch([probe, pool[0], probe])
    assert twice[0].tobytes() == twice[2].tobytes() == alone[probe]
    eng.close()


def test_a_copied_block_differs_only_by_its_asked_state_in_the_listing(factory):
    K, Q, T = 5, 37, 101
    eng, pl = make_engine(factory, K, Q, T)
    src, dst = pl.copy
    quiz = play(eng, [(src, 1), (7, 2)])                      # the original is asked, the copy is not
    row = eng.eval_question_gains_batch([quiz])[0]
    assert row[src].tobytes() == row[dst].tobytes() and row[src] > 0
    ids = [q for q, _ in eng.list_informative_questions(quiz, Q)]
    assert dst in ids and src not in ids and 7 not in ids
    fresh = eng.start_quiz()
    ids = [q for q, _ in eng.list_informative_questions(fresh, Q)]
    assert ids[ids.index(src) + 1] == dst                     # ties by ascending id: the copy stands right behind its original
    eng.close()


def test_host_prefix_beyond_256_records(factory):
    """More than 256 questions and maxCount beyond 256: the rows are copied and the prefix is taken on the host, in the listing kernels' order."""
    K, Q, T = 2, 300, 33
    eng, pl = make_engine(factory, K, Q, T, tgaps=(6,), qgaps=(7, 299))
    A, D, B = eng.get_kb()
    quizzes = [play(eng, history(Q, K, n, 11 + n, avoid={7, 299, pl.qz})) for n in (0, 3, 8)]
    got = eng.eval_question_gains_batch(quizzes)
    model = Model(A, D, (6,), (7, 299))
    within_bar("q300", got[1], model.row(clean_posterior(eng, quizzes[1], (6,))), T, K)
    for max_count in (256, 257, 300, Q + 5):
        listed = eng.list_informative_questions_batch(quizzes, max_count)
        for i, z in enumerate(quizzes):
            assert listed[i] == listing_of_row(got[i], max_count, asked_of(eng, z)), (max_count, i)
    assert len(eng.list_informative_questions(quizzes[0], 300)) > 256
    eng.close()


# ---- nothing changes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("server", [0, 1])
def test_the_calls_change_no_quiz_state(factory, server):
    """One engine makes the calls between the steps of a quiz loop -- also directly behind record_answer, when its update is deferred --,
    its twin makes none."""
    K, Q, T, tgaps = 5, 40, 1000, (3, 700)
    (a, _), (b, _) = (make_engine(factory, K, Q, T, tgaps, plant=False) for _ in range(2))
    for e in (a, b):
        e.set_option("server", server)
    qa, qb = a.start_quiz(), b.start_quiz()
    calls0, n0 = a.get_option("gain_calls"), a.get_option("gain_quizzes")
    A, D, B = a.get_kb()
    model = Model(A, D, tgaps, ())
    rng = np.random.default_rng(12)
    for step in range(4):
        pa, pb = a.next_question_argmax(qa), b.next_question_argmax(qb)
        assert pa == pb and a.get_active_question_id(qa) == pa, (step, pa, pb)
        before = (a.get_priors(qa).tobytes(), [(x.i_question, x.i_answer) for x in a.get_quiz_answers(qa)], a.get_active_question_id(qa))
        rows = a.eval_question_gains_batch([qa, qa])
        listed = a.list_informative_questions(qa, 5)
        assert (a.get_priors(qa).tobytes(), [(x.i_question, x.i_answer) for x in a.get_quiz_answers(qa)], a.get_active_question_id(qa)) == before
        assert listed == listing_of_row(rows[0], 5, asked_of(a, qa))
        ans = int(rng.integers(K))
        a.record_answer(qa, ans)
        b.record_answer(qb, ans)
        row = a.eval_question_gains_batch([qa])[0]                                   # (directly behind record_answer)
        if step == 1:
            within_bar(("loop", server, step), row, model.row(clean_posterior(b, qb, tgaps)), T, K)
    assert a.next_question_argmax(qa) == b.next_question_argmax(qb)
    assert a.get_priors(qa).tobytes() == b.get_priors(qb).tobytes()
    assert a.get_total_questions_asked() == b.get_total_questions_asked()
    assert a.get_option("gain_calls") == calls0 + 12 and a.get_option("gain_quizzes") == n0 + 16
    a.set_option("time_sweeps", 1)
    ns0 = a.get_option("gain_device_ns")
    a.eval_question_gains_batch([qa])
    ns1 = a.get_option("gain_device_ns")
    a.list_informative_questions(qa, 3)
    assert a.get_option("gain_device_ns") > ns1 > ns0
    a.close()
    b.close()


# ---- refusals, in the header's order --------------------------------------------------------------------------------------------------
SENT = -7.0


def raw_eval(eng, quizzes, n, count=None, null=()):
    """The C call on a sentinel-filled buffer -> (error pointer, the buffers)."""
    qs = np.ascontiguousarray(list(quizzes) or [0], dtype=np.int64)
    out = np.full(max(len(quizzes), 1) * max(n, 1), SENT)
    err = interop.load_library().PqaEngine_EvalQuestionGainsBatch(
        eng.c_engine, len(quizzes) if count is None else count, None if "quizzes" in null else qs.ctypes.data_as(P64), None if "out" in null else out.ctypes.data_as(PD), n)
    return err, (out,)


def raw_list(eng, quizzes, max_count, count=None, null=()):
    qs = np.ascontiguousarray(list(quizzes) or [0], dtype=np.int64)
    rec = np.full(max(len(quizzes), 1) * max(max_count, 1) * 2, SENT)
    counts = np.full(max(len(quizzes), 1), int(SENT), dtype=np.int64)
    err = interop.load_library().PqaEngine_ListInformativeQuestionsBatch(
        eng.c_engine, len(quizzes) if count is None else count, None if "quizzes" in null else qs.ctypes.data_as(P64), max_count,
        None if "dest" in null else ctypes.cast(rec.ctypes.data, PREC), None if "counts" in null else counts.ctypes.data_as(P64))
    return err, (rec, counts)


def test_refusals(factory):
    K, Q, T = 3, 8, 13
    eng, _ = make_engine(factory, K, Q, T, plant=False)
    quiz = eng.start_quiz()
    counters = ("gain_calls", "gain_quizzes")
    before = [eng.get_option(c) for c in counters]
    NEG, NULL, RANGE, MODE = "The count is negative", "Expected non-null argument", "Index is out of range", "An attempt to execute an operation in a wrong mode"
    ok = [quiz, quiz]

    def refused(result, code, *texts):
        err, buffers = result
        assert err, texts
        s = interop.PqaError(err).to_string(True)
        assert s.startswith("[" + code + "]") and all(t in s for t in texts), s
        assert all((b == SENT).all() for b in buffers), s
        assert [eng.get_option(c) for c in counters] == before

    refused(raw_eval(eng, ok, Q, count=-1), NEG, "count=-1", "nQuizzes")
    refused(raw_eval(eng, ok, Q, null=("quizzes",)), NULL)
    refused(raw_eval(eng, ok, Q, null=("out",)), NULL)
    refused(raw_eval(eng, ok, Q - 1), RANGE, "subjIndex=%d" % (Q - 1))
    refused(raw_eval(eng, ok, Q + 1), RANGE, "subjIndex=%d" % (Q + 1))
    refused(raw_eval(eng, [99], Q), RANGE, "entry=0", "quizId=99")
    refused(raw_eval(eng, ok + [1 << 40], Q), RANGE, "entry=2", "quizId=%d" % (1 << 40))
    refused(raw_list(eng, ok, 4, count=-2), NEG, "count=-2", "nQuizzes")
    refused(raw_list(eng, ok, -4), NEG, "count=-4", "maxCount")
    refused(raw_list(eng, ok, 4, null=("quizzes",)), NULL)
    refused(raw_list(eng, ok, 4, null=("dest",)), NULL)
    refused(raw_list(eng, ok, 4, null=("counts",)), NULL)
    refused(raw_list(eng, ok + [77], 4), RANGE, "entry=2", "quizId=77")
    # the order: a count, a NULL, the row length, the mode, the quiz
    refused(raw_eval(eng, [99], Q - 1, count=-1, null=("quizzes", "out")), NEG, "count=-1")
    refused(raw_eval(eng, [99], Q - 1, null=("out",)), NULL)
    refused(raw_eval(eng, [99], Q - 1), RANGE, "subjIndex=%d" % (Q - 1))
    refused(raw_list(eng, [99], -1, count=-1, null=("quizzes", "dest", "counts")), NEG, "count=-1")
    refused(raw_list(eng, [99], -1, null=("dest",)), NEG, "count=-1")
    refused(raw_list(eng, [99], 3, null=("dest",)), NULL)
    # maxCount 0 lists nothing and is no error, without a destination; no quizzes is no error without any buffer
    err, (rec, counts) = raw_list(eng, ok, 0, null=("dest",))
    assert not err and (counts == 0).all()
    assert not raw_eval(eng, [], Q, null=("quizzes", "out"))[0] and not raw_list(eng, [], 3, null=("quizzes", "dest", "counts"))[0]
    assert [eng.get_option(c) for c in counters] == [before[0] + 1, before[1] + 2]   # (an empty call moves no counter)
    # maintenance mode and shutdown, as QuizStatusBatch answers them: behind the row length, in front of the quiz
    before = [eng.get_option(c) for c in counters]
    eng.start_maintenance(True)
    refused(raw_eval(eng, [99], Q), MODE)
    refused(raw_eval(eng, ok, Q), MODE)
    refused(raw_eval(eng, [99], Q - 1), RANGE, "subjIndex=%d" % (Q - 1))
    refused(raw_eval(eng, [99], Q, null=("out",)), NULL)
    refused(raw_list(eng, [99], 3), MODE)
    refused(raw_list(eng, ok, 3), MODE)
    eng.finish_maintenance()
    quiz = eng.start_quiz()
    row = eng.eval_question_gains_batch([quiz])[0]                                  # the next good call is correct
    A, D, B = eng.get_kb()
    within_bar("after", row, Model(A, D, (), ()).row(clean_posterior(eng, quiz, ())), T, K)
    assert eng.list_informative_questions(quiz, 3) == listing_of_row(row, 3)
    before = [eng.get_option(c) for c in counters]
    eng.shutdown()
    refused(raw_eval(eng, [quiz], Q), MODE)
    refused(raw_list(eng, [quiz], 3), MODE)
    eng.close()


def test_one_process_sharded_engine_refuses(factory, monkeypatch):
    monkeypatch.setenv("PQA_DEVICES", "0,0")        # two shards side by side on the one device
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(5, 37, 101, init_amount=0.1))
    assert err is None and eng.get_option("shards") == 2
    quiz = eng.start_quiz()
    for err, _ in (raw_eval(eng, [quiz], 37), raw_list(eng, [quiz], 3)):
        s = interop.PqaError(err).to_string(True) if err else ""
        assert "Question gains are for whole engines" in s, s
    eng.close()
