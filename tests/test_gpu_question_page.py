"""Conditional gains and greedy question pages on the GPU (include/PqaHipExt.h: PqaEngine_EvalConditionalGainsBatch,
PqaEngine_ListQuestionPageBatch; page_kernels.hip; hip_engine_page.cpp).

The model works over one get_kb() and get_priors(), as tests/test_gpu_question_gains.py does.  The BRANCH rows of a set S = (q_1 .. q_j)
are built in numpy fp64 with the kernel's own products -- w_b = ((p r_k1^q1) r_k2^q2) ..., b = ((k_1 K + k_2) K + ...) + k_j, each
product rounded to a double --, their masses and the weights m_b / M with math.fsum, and
    CG(q | S) = fsum over the branches with m_b > 0 of (m_b / M) gain_table(w_b, q)
with that file's table definition of the gain (math.log2, math.fsum).  The bar is derived, not measured, and ABSOLUTE:
    |gpu - model| <= ((T + 16) (K + 8) + (2 (T + 16) + B + 2) log2 K) 2^-52 bits,   B = K^|S|
-- each branch's own gain bar (the weights sum to 1), the weights' relative error (a mass and the total are sums of up to T + 16
roundings each) times the bound log2 K of a gain, and the fma chain over the B branches.  A wrong weighting or a missing branch shows
at 1e-3 bits or more.  The model costs K T logarithms per (branch, question) in Python, so beyond a budget of elements per set the deeper
sets are held to the model at a few columns -- the copied block, the planted questions and the first free ones --; the device forms
every column by the same code.  Worst seen on an MI355X over every case of this file: see README.md.
Pages are held to a host greedy over the engine's own Eval rows record for record, bit for bit."""
import ctypes
import math

import numpy as np
import pytest

import cases
from probqa_amd import interop
from test_gpu_question_gains import F32, Model, asked_of, clean_posterior, history, make_engine, play

pytestmark = pytest.mark.gpu

P64, PD, PREC = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(interop.CiRatedQuestion)
EPS = 2.0 ** -52
BUDGET = 800_000   # table elements of the model per (quiz, set)


def bar(T, K, n_set):
    return ((T + 16) * (K + 8) + (2 * (T + 16) + K ** n_set + 2) * math.log2(K)) * EPS


def branch_rows(model, p, given):
    """the set's branch rows in branch order, the device's products"""
    rows = [p]
    for q in given:
        rows = [row * model.r[q][k] for row in rows for k in range(model.K)]
    return rows


def conditional_gain(model, rows, q):
    masses = [math.fsum(row.tolist()) for row in rows]
    M = math.fsum(masses)
    if not M > 0 or not math.isfinite(M):
        return 0.0
    return math.fsum((m / M) * model.gain(row, q) for m, row in zip(masses, rows) if m > 0)


WORST = {"bits": 0.0, "of_bar": 0.0}


def within_bar(name, got, want, T, K, n_set):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    b = bar(T, K, n_set)
    WORST["bits"], WORST["of_bar"] = max(WORST["bits"], err), max(WORST["of_bar"], err / b)
    print("%s: worst deviation %.3g bits, bar %.3g (worst so far %.3g bits, %.3g of its bar)" % (name, err, b, WORST["bits"], WORST["of_bar"]))
    assert err <= b, (name, err, b)


def host_page(eng, quiz, page_size, given, qgaps=()):
    """the page a host would fill from the engine's own Eval rows: the largest CG > 0 among the questions that are no gaps, not asked
    and not in the set so far, the lowest id among equals"""
    asked, prefix, page = asked_of(eng, quiz), list(given), []
    for _ in range(page_size):
        row = eng.eval_conditional_gains_batch([quiz], [prefix])[0]
        cand = [q for q in range(len(row)) if row[q] > 0 and q not in asked and q not in prefix and q not in qgaps]
        if not cand:
            break
        best = min(cand, key=lambda q: (-row[q], q))
        page.append((best, float(row[best])))
        prefix.append(best)
    return page


SHAPES = {
    "q8_k3_t12": dict(Q=8, K=3, T=12),
    "q37_k5_t101_gaps": dict(Q=37, K=5, T=101, tgaps=(3, 17, 100), qgaps=(0, 5, 36)),
    "q33_k7_t130_generic": dict(Q=33, K=7, T=130),
    "q50_k4_t67": dict(Q=50, K=4, T=67),
    "q20_k2_t257": dict(Q=20, K=2, T=257),
    "q12_k5_t1025": dict(Q=12, K=5, T=1025),
    "q6_k5_t4099_long_row": dict(Q=6, K=5, T=4099),
    "f32_q37_k5_t101_gaps": dict(Q=37, K=5, T=101, tgaps=(3, 17, 100), qgaps=(0, 5, 36), f32=True),
    "f32_q20_k2_t257": dict(Q=20, K=2, T=257, f32=True),
    "f32_q6_k5_t4099_long_row": dict(Q=6, K=5, T=4099, f32=True),
}


# ---- 1, 2, 6: rows against the model, the empty set, a planted dead answer among the branches ---------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rows_against_the_model(factory, name):
    sh = dict(SHAPES[name])
    K, Q, T, tgaps, qgaps = sh["K"], sh["Q"], sh["T"], sh.get("tgaps", ()), sh.get("qgaps", ())
    eng, pl = make_engine(factory, K, Q, T, tgaps, qgaps, **(F32 if sh.get("f32") else {}))
    A, D, B = eng.get_kb()
    model = Model(A, D, tgaps, qgaps)
    free = [q for q in range(Q) if q not in qgaps]
    quizzes = [play(eng, history(Q, K, n, 41 + n, avoid=set(qgaps) | {pl.qz})) for n in (0, 6)]
    posteriors = [clean_posterior(eng, z, tgaps) for z in quizzes]
    plain = eng.eval_question_gains_batch(quizzes)
    calls0, n0 = eng.get_option("page_calls"), eng.get_option("page_quizzes")
    # the empty set, as NULL pointers and as empty lists: EvalQuestionGainsBatch's rows bit for bit
    assert eng.eval_conditional_gains_batch(quizzes).tobytes() == plain.tobytes()
    assert eng.eval_conditional_gains_batch(quizzes, [[], []]).tobytes() == plain.tobytes()
    assert eng.get_option("page_calls") == calls0 + 2 and eng.get_option("page_quizzes") == n0 + 4
    pages = eng.list_question_page_batch(quizzes, 2)
    informative = eng.list_informative_questions_batch(quizzes, 1)
    for i in range(2):
        assert pages[i][:1] == informative[i] and pages[i] == host_page(eng, quizzes[i], 2, [], qgaps), (name, i, pages[i], informative[i])
    # sets of 1, 2, 3 questions: the planted question first (exact zeros under one answer, a DEAD answer: a branch of mass 0), then an
    # asked question of the second quiz, then the original of the copied block
    asked = sorted(asked_of(eng, quizzes[1]))
    members = [pl.qz, asked[0], pl.copy[0] if pl.copy else free[-1]]
    columns = [q for q in dict.fromkeys(([pl.copy[1]] if pl.copy else []) + [pl.qz, pl.alike] + free) if q is not None]
    for n_set in (0, 1, 2, 3):
        if K ** n_set > 256:
            continue
        given = members[:n_set]
        got = eng.eval_conditional_gains_batch(quizzes, [given, given])
        assert got.shape == (2, Q)
        if qgaps:
            assert not got[:, list(qgaps)].any()
        assert (got >= 0).all() and (got <= math.log2(K) + bar(T, K, n_set)).all()
        take = columns[:max(1, BUDGET // (K ** n_set * K * T))]
        for i in range(2):
            rows = branch_rows(model, posteriors[i], given)
            if n_set >= 1:
                masses = [math.fsum(r.tolist()) for r in rows]
                assert masses[pl.kd * K ** (n_set - 1)] == 0.0 and any(m > 0 for m in masses)              # the dead answer's branches are there, and others live
            want = [conditional_gain(model, rows, q) for q in take]
            within_bar((name, n_set, i), got[i, take], want, T, K, n_set)
        if pl.copy:
            assert got[:, pl.copy[0]].tobytes() == got[:, pl.copy[1]].tobytes()       # a copied block, the same bits
    assert (clean_posterior(eng, quizzes[1], tgaps) == posteriors[1]).all()
    print("worst so far:", WORST)
    eng.close()


# ---- 3: the chain rule ------------------------------------------------------------------------------------------------------------------
def joint_information(p, blocks):
    """I(A_page ; T) from the joint K^m x T table, in math.fsum"""
    J = [p.tolist()]
    for r in blocks:
        J = [[x * y for x, y in zip(row, rk.tolist())] for row in J for rk in r]
    W = [math.fsum(row) for row in J]
    Z = math.fsum(W)
    c = [math.fsum(col) for col in zip(*J)]
    return math.fsum((j / Z) * math.log2(j * Z / (W[k] * c[t])) for k, row in enumerate(J) for t, j in enumerate(row) if j > 0)


@pytest.mark.parametrize("Q,K,T,m", [(8, 3, 12, 4), (10, 5, 101, 3), (9, 4, 67, 4), (6, 2, 257, 3)])
def test_a_pages_gains_add_up_to_its_joint_information(factory, Q, K, T, m):
    """Integer counts with D == sum_k A bit for bit: the page's _priority values sum to I(A_page ; T) within the sum of the steps' bars
    plus 4 m (K + 2) 2^-52 for s_q(t) being 1 only to rounding."""
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=1.0))
    assert err is None
    eng.set_option("workers", cases.WORKERS)
    rng = np.random.default_rng(3)
    A = rng.integers(1, 40, size=(Q, K, T)).astype(np.float64)
    A[1, 0, : T // 3] = 0.0
    D = A.sum(axis=1)
    eng.set_kb(A, D, rng.integers(1, 9, size=T).astype(np.float64))
    A2, D2, _ = eng.get_kb()
    assert A2.tobytes() == A.tobytes() and D2.tobytes() == D.tobytes()
    model = Model(A2, D2, (), ())
    quizzes = [play(eng, history(Q, K, n, 70 + n)) for n in (0, 3)]
    pages = eng.list_question_page_batch(quizzes, m)
    worst = 0.0
    for z, page in zip(quizzes, pages):
        assert len(page) == m and len({q for q, _ in page}) == m and not {q for q, _ in page} & asked_of(eng, z), page
        joint = joint_information(clean_posterior(eng, z, ()), [model.r[q] for q, _ in page])
        allowed = sum(bar(T, K, s) for s in range(m)) + 4 * m * (K + 2) * EPS
        total = math.fsum(v for _, v in page)
        worst = max(worst, abs(total - joint) / allowed)
        assert abs(total - joint) <= allowed, (page, total, joint, allowed)
    print("chain rule %dx%dx%d, page of %d: worst %.3g of the allowed difference" % (Q, K, T, m, worst))
    eng.close()


# ---- 4: the picks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q37_k5_t101_gaps", "q50_k4_t67", "q20_k2_t257", "f32_q37_k5_t101_gaps", "q33_k7_t130_generic"])
def test_pages_are_a_greedy_over_the_engines_own_rows(factory, name):
    sh = dict(SHAPES[name])
    K, Q, T, tgaps, qgaps = sh["K"], sh["Q"], sh["T"], sh.get("tgaps", ()), sh.get("qgaps", ())
    eng, pl = make_engine(factory, K, Q, T, tgaps, qgaps, **(F32 if sh.get("f32") else {}))
    src, dst = pl.copy
    quizzes = [eng.start_quiz(), play(eng, history(Q, K, 6, 47, avoid=set(qgaps) | {pl.qz})), play(eng, [(src, 1)])]
    size = {2: 5, 4: 3, 5: 3, 7: 2}[K]
    sets = [[], [pl.qz], [dst]]
    pages = eng.list_question_page_batch(quizzes, size, sets)
    for z, given, page in zip(quizzes, sets, pages):
        assert page == host_page(eng, z, size, given, qgaps), (name, z, given)
        ids = [q for q, _ in page]
        assert len(ids) == size and not set(ids) & (set(qgaps) | asked_of(eng, z) | set(given)), (ids, given)
        assert eng.list_question_page(z, size, given) == page
    # the copied block: equal bits, the lowest id wins
    fresh = eng.start_quiz()
    row = eng.eval_conditional_gains_batch([fresh], [[pl.qz]])[0]
    assert row[src].tobytes() == row[dst].tobytes()
    page = eng.list_question_page(fresh, 2, [pl.qz])
    order = sorted((q for q in range(Q) if row[q] > 0 and q != pl.qz and q not in qgaps), key=lambda q: (-row[q], q))
    assert page[0] == (order[0], float(row[order[0]]))
    if src in order:
        assert order.index(dst) == order.index(src) + 1
    after = eng.eval_conditional_gains_batch([fresh], [[src]])[0]               # (a repeated question is a draw of its own: a chain like any other)
    assert after[dst].tobytes() == after[src].tobytes()
    assert eng.list_question_page_batch(quizzes, 0, sets) == [[], [], []] and eng.list_question_page_batch([], 3) == []
    eng.close()


def test_a_page_larger_than_the_candidates_stops_early(factory):
    K, Q, T = 2, 7, 33
    eng, pl = make_engine(factory, K, Q, T, qgaps=(4,))
    quiz = play(eng, [(1, 0), (6, 1)])
    page = eng.list_question_page(quiz, 8)               # 2^7 branches at the last step; 4 candidates at most
    want = host_page(eng, quiz, 8, [], (4,))
    assert page == want and 1 <= len(page) <= 4, (page, want)
    assert not {q for q, _ in page} & {1, 6, 4}
    pages = eng.list_question_page_batch([quiz, eng.start_quiz()], 3, [[0, 2, 3], [5]])
    assert pages[0] == host_page(eng, quiz, 3, [0, 2, 3], (4,)) and len(pages[0]) <= 1
    assert len(pages[1]) == 3
    eng.close()


# ---- 5: independence --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,f32", [(5, False), (2, True), (7, False)])
def test_a_value_does_not_depend_on_the_call(factory, K, f32):
    Q, T, tgaps, qgaps = 37, 101, (3, 17, 100), (0, 5, 36)
    eng, pl = make_engine(factory, K, Q, T, tgaps, qgaps, **(F32 if f32 else {}))
    pool = [play(eng, history(Q, K, n, 90 + n, avoid=set(qgaps) | {pl.qz})) for n in (0, 1, 2, 3, 5, 8, 13)]
    depth = 3 if K <= 5 else 2
    probe, given = pool[3], [pl.qz, 9, 20][:depth]
    alone = eng.eval_conditional_gains_batch([probe], [given])[0]
    size = 3 if K ** 3 <= 256 else 2
    page = eng.list_question_page(probe, size, given[:1])
    assert eng.eval_conditional_gains_batch([probe], [given])[0].tobytes() == alone.tobytes()
    others = [[], [7], [8, 9], [pl.qz], [10, 11, 12][:depth], [2]]
    batch, sets = pool[:3] + [probe] + pool[4:], others[:3] + [given] + others[3:]
    got = eng.eval_conditional_gains_batch(batch, sets)
    assert got[3].tobytes() == alone.tobytes()
    for i in (0, 2, 6):
        assert got[i].tobytes() == eng.eval_conditional_gains_batch([batch[i]], [sets[i]])[0].tobytes(), i
    twice = eng.eval_conditional_gains_batch([probe, pool[0], probe], [given, [], given])
    assert twice[0].tobytes() == twice[2].tobytes() == alone.tobytes()
    paged = eng.list_question_page_batch(batch, size, [s[:1] for s in sets])
    assert paged[3] == page and paged[0] == eng.list_question_page(batch[0], size, sets[0][:1])
    # the call's branch rows cross the 256-row edge of a chunk: 3 quizzes x K^depth rows
    if K == 5:
        three = eng.eval_conditional_gains_batch([pool[1], probe, probe], [given, given, given])
        assert three[1].tobytes() == three[2].tobytes() == alone.tobytes()
        assert three[0].tobytes() == eng.eval_conditional_gains_batch([pool[1]], [given])[0].tobytes()
        pages = eng.list_question_page_batch([pool[1], probe, probe], 1, [given] * 3)
        assert pages[1] == pages[2] == eng.list_question_page(probe, 1, given)
    # another order of the set: the same number to rounding, not to the bit
    permuted = eng.eval_conditional_gains_batch([probe], [given[::-1]])[0]
    print("permuted set: %.3g of the bar" % (np.abs(permuted - alone).max() / bar(T, K, len(given))))
    assert np.abs(permuted - alone).max() <= bar(T, K, len(given))
    # a duplicate id is a chain like any other
    dup = eng.eval_conditional_gains_batch([probe], [[9, 9]])[0]
    A, D, B = eng.get_kb()
    model = Model(A, D, tgaps, qgaps)
    rows = branch_rows(model, clean_posterior(eng, probe, tgaps), [9, 9])
    within_bar(("duplicate", K), dup[[9, 10, 20]], [conditional_gain(model, rows, q) for q in (9, 10, 20)], T, K, 2)
    eng.close()


# ---- 6: dead sets -----------------------------------------------------------------------------------------------------------------------
def test_a_set_with_every_branch_dead(factory):
    K, Q, T = 5, 37, 101
    eng, pl = make_engine(factory, K, Q, T)
    dead = play(eng, [(pl.qz, pl.kd)])
    assert not (eng.get_priors(dead) > 0).any()
    live = eng.start_quiz()
    got = eng.eval_conditional_gains_batch([dead, live, dead], [[7, 8], [7, 8], []])
    assert not got[0].any() and not got[2].any() and got[1].any()
    pages = eng.list_question_page_batch([dead, live, dead], 2, [[7], [7], []])
    assert pages[0] == [] and pages[2] == [] and len(pages[1]) == 2
    assert pages[1] == host_page(eng, live, 2, [7])
    eng.close()


# ---- 7: nothing changes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("server", [0, 1])
def test_the_calls_change_no_quiz_state(factory, server):
    K, Q, T, tgaps = 5, 40, 1000, (3, 700)
    (a, _), (b, _) = (make_engine(factory, K, Q, T, tgaps, plant=False) for _ in range(2))
    for e in (a, b):
        e.set_option("server", server)
    qa, qb = a.start_quiz(), b.start_quiz()
    rng = np.random.default_rng(12)

    def state():
        return (a.get_priors(qa).tobytes(), [(x.i_question, x.i_answer) for x in a.get_quiz_answers(qa)], a.get_active_question_id(qa))

    for step in range(3):
        pa, pb = a.next_question_argmax(qa), b.next_question_argmax(qb)
        assert pa == pb and a.get_active_question_id(qa) == pa, (step, pa, pb)
        before = state()
        rows = a.eval_conditional_gains_batch([qa, qa], [[4, 11], []])
        page = a.list_question_page(qa, 3, [4])
        assert state() == before
        assert len(page) == 3 and page == host_page(a, qa, 3, [4])
        assert rows[1].tobytes() == a.eval_question_gains_batch([qa])[0].tobytes()
        ans = int(rng.integers(K))
        a.record_answer(qa, ans)
        b.record_answer(qb, ans)
        a.list_question_page(qa, 2)                                                 # (directly behind record_answer)
    assert a.next_question_argmax(qa) == b.next_question_argmax(qb)
    assert a.get_priors(qa).tobytes() == b.get_priors(qb).tobytes()
    assert a.get_total_questions_asked() == b.get_total_questions_asked()
    a.set_option("time_sweeps", 1)
    ns0 = a.get_option("page_device_ns")
    a.eval_conditional_gains_batch([qa], [[4]])
    ns1 = a.get_option("page_device_ns")
    a.list_question_page(qa, 2)
    assert a.get_option("page_device_ns") > ns1 > ns0
    a.close()
    b.close()


# ---- 8: refusals, in the header's order -------------------------------------------------------------------------------------------------
SENT = -7.0


def given_args(given, n, null):
    if given is None:
        return None, None, ()
    counts = np.ascontiguousarray([len(g) if not isinstance(g, int) else g for g in given] + [0], dtype=np.int64)
    ids = np.ascontiguousarray([q for g in given if not isinstance(g, int) for q in g] + [0], dtype=np.int64)
    return counts.ctypes.data_as(P64), None if "given" in null else ids.ctypes.data_as(P64), (counts, ids)


def raw_eval(eng, quizzes, n, given=None, count=None, null=()):
    qs = np.ascontiguousarray(list(quizzes) or [0], dtype=np.int64)
    out = np.full(max(len(quizzes), 1) * max(n, 1), SENT)
    c, g, keep = given_args(given, len(quizzes), null)
    err = interop.load_library().PqaEngine_EvalConditionalGainsBatch(
        eng.c_engine, len(quizzes) if count is None else count, None if "quizzes" in null else qs.ctypes.data_as(P64), c, g,
        None if "out" in null else out.ctypes.data_as(PD), n)
    return err, (out,)


def raw_page(eng, quizzes, page_size, given=None, count=None, null=()):
    qs = np.ascontiguousarray(list(quizzes) or [0], dtype=np.int64)
    rec = np.full(max(len(quizzes), 1) * max(min(page_size, 16), 1) * 2, SENT)   # (a page beyond 9 is refused before anything is written)
    counts = np.full(max(len(quizzes), 1), int(SENT), dtype=np.int64)
    c, g, keep = given_args(given, len(quizzes), null)
    err = interop.load_library().PqaEngine_ListQuestionPageBatch(
        eng.c_engine, len(quizzes) if count is None else count, None if "quizzes" in null else qs.ctypes.data_as(P64), c, g, page_size,
        None if "dest" in null else ctypes.cast(rec.ctypes.data, PREC), None if "counts" in null else counts.ctypes.data_as(P64))
    return err, (rec, counts)


def test_refusals(factory):
    K, Q, T = 3, 8, 13
    eng, _ = make_engine(factory, K, Q, T, qgaps=(6,), plant=False)
    quiz = eng.start_quiz()
    counters = ("page_calls", "page_quizzes")
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
    refused(raw_eval(eng, ok, Q, given=[[1], -2]), NEG, "entry=1", "count=-2")
    refused(raw_eval(eng, ok, Q, null=("quizzes",)), NULL)
    refused(raw_eval(eng, ok, Q, null=("out",)), NULL)
    refused(raw_eval(eng, ok, Q, given=[[], [1]], null=("given",)), NULL)
    refused(raw_eval(eng, ok, Q - 1), RANGE, "subjIndex=%d" % (Q - 1))
    refused(raw_eval(eng, [99], Q), RANGE, "entry=0", "quizId=99")
    refused(raw_eval(eng, ok, Q, given=[[1], [2, Q]]), RANGE, "entry=1", "questionId=%d" % Q)
    refused(raw_eval(eng, ok, Q, given=[[-1], [2]]), RANGE, "entry=0", "questionId=-1")
    refused(raw_eval(eng, ok, Q, given=[[1], [2, 6]]), RANGE, "entry=1", "questionId=6", "gap")
    refused(raw_eval(eng, ok, Q, given=[[1], [1, 2, 3, 4, 5, 7]]), RANGE, "entry=1", "branches=")          # 3^6 = 729
    refused(raw_page(eng, ok, 2, count=-2), NEG, "count=-2", "nQuizzes")
    refused(raw_page(eng, ok, -4), NEG, "count=-4", "pageSize")
    refused(raw_page(eng, ok, 2, given=[-1, [1]]), NEG, "entry=0", "count=-1")
    refused(raw_page(eng, ok, 2, null=("quizzes",)), NULL)
    refused(raw_page(eng, ok, 2, null=("dest",)), NULL)
    refused(raw_page(eng, ok, 2, null=("counts",)), NULL)
    refused(raw_page(eng, ok, 2, given=[[1], []], null=("given",)), NULL)
    refused(raw_page(eng, ok + [77], 2), RANGE, "entry=2", "quizId=77")
    refused(raw_page(eng, ok, 2, given=[[6], []]), RANGE, "entry=0", "questionId=6")
    refused(raw_page(eng, ok, 7), RANGE, "entry=0", "branches=")                                           # 3^6 at the last step
    refused(raw_page(eng, ok, 3, given=[[1], [1, 2, 3, 4]]), RANGE, "entry=1", "branches=")                # 3^(4 + 2)
    refused(raw_page(eng, ok, 1 << 40), RANGE, "entry=0", "branches=")
    # the order: a count, a NULL, the row length, the quiz, the given question, the limits
    refused(raw_eval(eng, [99], Q - 1, given=[-1], count=-1, null=("quizzes", "out")), NEG, "count=-1", "nQuizzes")
    refused(raw_eval(eng, [99], Q - 1, given=[-1], null=("out",)), NEG, "count=-1", "entry=0")
    refused(raw_eval(eng, [99], Q - 1, given=[[Q]], null=("out",)), NULL)
    refused(raw_eval(eng, [99], Q - 1, given=[[Q]]), RANGE, "subjIndex=%d" % (Q - 1))
    refused(raw_eval(eng, [99], Q, given=[[Q]]), RANGE, "quizId=99")
    refused(raw_eval(eng, ok, Q, given=[[1, 2, 3, 4, 5, 7], [Q]]), RANGE, "entry=1", "questionId=%d" % Q)
    refused(raw_page(eng, [99], -1, count=-1, null=("quizzes", "dest", "counts")), NEG, "count=-1", "nQuizzes")
    refused(raw_page(eng, [99], 3, null=("dest",)), NULL)
    refused(raw_page(eng, [99], 9, given=[[Q]]), RANGE, "quizId=99")
    refused(raw_page(eng, ok, 9, given=[[], [Q]]), RANGE, "entry=1", "questionId=%d" % Q)
    # the limits at their edges: 3^5 = 243 rows pass
    err, (out,) = raw_eval(eng, [quiz], Q, given=[[1, 2, 3, 4, 5]])
    assert not err and (out != SENT).all()
    err, (rec, counts) = raw_page(eng, [quiz], 6)
    assert not err and 1 <= counts[0] <= 6
    # a page of 0 lists nothing and is no error, without a destination; no quizzes is no error without any buffer
    err, (rec, counts) = raw_page(eng, ok, 0, null=("dest",))
    assert not err and (counts == 0).all()
    assert not raw_eval(eng, [], Q, null=("quizzes", "out"))[0] and not raw_page(eng, [], 3, null=("quizzes", "dest", "counts"))[0]
    assert [eng.get_option(c) for c in counters] == [before[0] + 3, before[1] + 4]   # (an empty call moves no counter)
    # maintenance mode and shutdown: behind the row length, in front of the quiz
    before = [eng.get_option(c) for c in counters]
    eng.start_maintenance(True)
    refused(raw_eval(eng, [99], Q), MODE)
    refused(raw_eval(eng, ok, Q, given=[[Q], []]), MODE)
    refused(raw_eval(eng, [99], Q - 1), RANGE, "subjIndex=%d" % (Q - 1))
    refused(raw_page(eng, [99], 3), MODE)
    refused(raw_page(eng, ok, 9), MODE)
    eng.finish_maintenance()
    quiz = eng.start_quiz()
    assert eng.list_question_page(quiz, 2, [1]) == host_page(eng, quiz, 2, [1], (6,))   # the next good call is correct
    before = [eng.get_option(c) for c in counters]
    eng.shutdown()
    refused(raw_eval(eng, [quiz], Q), MODE)
    refused(raw_page(eng, [quiz], 3), MODE)
    eng.close()


def test_a_row_too_long_for_the_scratch_is_refused(factory):
    """2^8 branch rows of 40000 targets would be 78 MiB: refused; 2^7 of them pass."""
    K, Q, T = 2, 9, 40000
    eng, _ = make_engine(factory, K, Q, T, plant=False, trains=0)
    quiz = eng.start_quiz()
    err, _ = raw_eval(eng, [quiz], Q, given=[list(range(8))])
    s = interop.PqaError(err).to_string(True) if err else ""
    assert s.startswith("[Index is out of range]") and "entry=0" in s and "branches=256" in s, s
    got = eng.eval_conditional_gains_batch([quiz], [list(range(7))])
    assert got.shape == (1, Q) and got[0, 7] > 0 and got[0, 8] > 0
    eng.close()


def test_sharded_engines_refuse(factory, monkeypatch):
    shard = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(5, 18, 101, init_amount=0.1), 0, 37, 0)
    quiz = shard.start_quiz()
    for err, _ in (raw_eval(shard, [quiz], 18), raw_page(shard, [quiz], 3)):
        s = interop.PqaError(err).to_string(True) if err else ""
        assert "Question pages need the given questions' blocks" in s and "Feature=" in s, s
    shard.close()
    monkeypatch.setenv("PQA_DEVICES", "0,0")        # two shards side by side on the one device
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(5, 37, 101, init_amount=0.1))
    assert err is None and eng.get_option("shards") == 2
    quiz = eng.start_quiz()
    for err, _ in (raw_eval(eng, [quiz], 37), raw_page(eng, [quiz], 3)):
        s = interop.PqaError(err).to_string(True) if err else ""
        assert "Question pages need the given questions' blocks" in s, s
    eng.close()
