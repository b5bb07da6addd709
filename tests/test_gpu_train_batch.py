"""PqaEngine_TrainBatch and PqaEngine_RecordQuizTargetBatch on a real MI355X: the KB (A, D, vB) bit-identical to the CPU
oracle's consecutive trainings and to consecutive single calls on a twin engine -- fp64 and Float, chunk edges everywhere, skewed
targets, long rows, gaps --, all or none, the sweep reading the trained cube, the sharded engine."""
import ctypes
import math
import os

import numpy as np
import pytest

import cases
from probqa_amd import interop

pytestmark = pytest.mark.gpu


def kb_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.get_kb(), b.get_kb()))


def oracle_equal(eng, orc, Q, T):
    A, D, B = eng.get_kb(Q)
    return np.array_equal(A, orc.A[:, :, :T]) and np.array_equal(D, orc.D[:, :T]) and np.array_equal(B, orc.B[:T])


def random_records(rng, n, Q, K, T, lo=8, hi=24, qgaps=(), tgaps=(), skew=0.0, repeat=True):
    """counts, aqs [sum, 2], targets, amounts: 8-24 answers per record, repeated questions, shared targets, amounts 0.3-2.0;
    `skew` of the records share one target."""
    qs_ok = np.setdiff1d(np.arange(Q), np.array(list(qgaps), dtype=np.int64))
    ts_ok = np.setdiff1d(np.arange(T), np.array(list(tgaps), dtype=np.int64))
    counts = rng.integers(lo, hi + 1, size=n).astype(np.int64)
    total = int(counts.sum())
    aqs = np.empty((total, 2), dtype=np.int64)
    aqs[:, 0] = rng.choice(qs_ok, size=total)
    aqs[:, 1] = rng.integers(0, K, size=total)
    if repeat:   # a repeated question in most records, with the same or another answer
        at = 0
        for c in counts:
            if c >= 3 and rng.random() < 0.7:
                aqs[at + c - 1, 0] = aqs[at, 0]
                if rng.random() < 0.5:
                    aqs[at + c - 1, 1] = aqs[at, 1]
            at += c
    targets = rng.choice(ts_ok, size=n).astype(np.int64)
    if skew > 0:
        targets[rng.random(n) < skew] = ts_ok[len(ts_ok) // 3]
    amounts = rng.uniform(0.3, 2.0, size=n)
    return counts, aqs, targets, amounts


def train_single(eng, counts, aqs, targets, amounts):
    """Consecutive PqaEngine_Train calls, one per record."""
    lib = interop.load_library()
    aqs = np.ascontiguousarray(aqs, dtype=np.int64)
    base = aqs.ctypes.data
    at = 0
    for c, t, a in zip(counts.tolist(), targets.tolist(), amounts.tolist()):
        p = ctypes.cast(base + 16 * at, ctypes.POINTER(interop.CiAnsweredQuestion))
        interop._check(lib.PqaEngine_Train(eng.c_engine, c, p, t, a))
        at += c
    return aqs


def oracle_train(orc, counts, aqs, targets, amounts, workers):
    at = 0
    for c, t, a in zip(counts.tolist(), targets.tolist(), amounts.tolist()):
        orc.train([(int(q), int(x)) for q, x in aqs[at:at + c]], t, a, workers)
        at += c


SCRIPTS = [   # tests/test_gpu_kb.py: Perform2's three cases in the reference's pairing order, and an empty record
    ([(7, 1), (7, 1)], 3, 0.8),
    ([(7, 1), (7, 2)], 3, 1.0),
    ([(7, 1), (8, 0), (7, 1)], 5, 0.5),
    ([(1, 0), (17, 1), (33, 2), (1, 0), (17, 3), (29, 1), (1, 2)], 9, 1.7),
    ([], 2, 2.0),
]


def synthetic(factory, K, Q, T, seed, f32=False, tgaps=(), qgaps=()):
    d = (interop.EngineDefinition(K, Q, T, init_amount=0.1, prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)
         if f32 else interop.EngineDefinition(K, Q, T, init_amount=0.1))
    eng, err = factory.create_cpu_engine(d)
    assert err is None and eng is not None, err
    eng.fill_synthetic(8.0, 0.5, seed)
    if tgaps:
        eng.set_target_gaps(list(tgaps))
    if qgaps:
        eng.set_question_gaps(list(qgaps))
    return eng


@pytest.mark.parametrize("ci", [2, 3])          # ragged_50x4x67 (ldT padding), k7_33x7x130
@pytest.mark.parametrize("workers", [1, 16, 24])
def test_train_batch_bit_identical_to_oracle(ci, workers, factory):
    case = cases.small_cases()[ci]
    K, Q, T = case.K, case.Q, case.T
    eng = case.make_engine(factory)
    eng.set_option("workers", workers)
    orc = case.make_oracle()
    rng = np.random.default_rng(100 * ci + workers)
    counts, aqs, targets, amounts = random_records(rng, 2000, Q, K, T, lo=0, hi=12)
    s_counts = np.array([len(s[0]) for s in SCRIPTS], dtype=np.int64)
    s_aqs = np.array([p for s in SCRIPTS for p in s[0]], dtype=np.int64).reshape(-1, 2) % [Q, K]
    counts = np.concatenate([s_counts, counts])
    aqs = np.concatenate([s_aqs, aqs])
    targets = np.concatenate([np.array([s[1] for s in SCRIPTS], dtype=np.int64), targets])
    amounts = np.concatenate([np.array([s[2] for s in SCRIPTS]), amounts])
    asked0 = eng.get_total_questions_asked()
    calls0 = eng.get_option("train_bulk_calls")
    eng.train_batch_arrays(counts, aqs, targets, amounts)
    oracle_train(orc, counts, aqs, targets, amounts, workers)
    assert oracle_equal(eng, orc, Q, T)
    assert eng.get_total_questions_asked() == asked0 + int(counts.sum())
    assert eng.get_option("train_bulk_calls") == calls0 + 1
    # the tuple form, and RecordQuizTargetBatch over quizzes with a re-asked question, against the oracle's RecordQuizTarget
    recs = [([interop.AnsweredQuestion(q % Q, a % K) for q, a in s[0]], s[1], s[2]) for s in SCRIPTS]
    eng.train_batch(recs)
    for s in SCRIPTS:
        orc.train([(q % Q, a % K) for q, a in s[0]], s[1], s[2], workers)
    assert oracle_equal(eng, orc, Q, T)
    answers = [[(12, 1), (12, 1), (30, 0)], [(12, 1), (30, 0), (12, 3)], [(5, 2), (5, 0)], [(20, 3)], []]
    quizzes = []
    for ans in answers:
        qz = eng.start_quiz()
        for q, a in ans:
            eng.set_active_question(qz, q % Q)
            eng.record_answer(qz, a % K)
        quizzes.append(qz)
    tq = [20, 21, 20, 3, 4, 20]
    am = [0.9, 1.3, 0.4, 2.0, 0.7, 1.1]
    quizzes.append(quizzes[0])
    answers.append(answers[0])
    before = eng.get_total_questions_asked()
    eng.record_quiz_target_batch(quizzes, tq, am)
    for ans, t, a in zip(answers, tq, am):
        orc.record_quiz_target(t, a, [(q % Q, x % K) for q, x in ans])
    assert oracle_equal(eng, orc, Q, T)
    assert eng.get_total_questions_asked() == before
    eng.close()
    orc.close()


@pytest.mark.parametrize("f32", [False, True])
def test_train_batch_equals_consecutive_calls_across_chunk_edges(f32, factory):
    K, Q, T = 5, 1000, 1000
    rng = np.random.default_rng(7 + f32)
    counts, aqs, targets, amounts = random_records(rng, 20000, Q, K, T)
    twin = synthetic(factory, K, Q, T, 3, f32)
    train_single(twin, counts, aqs, targets, amounts)
    head = 1500   # (chunks of one step: a launch per step -- on the first records only, the rest in one default batch)
    for chunk in (1, 7, None):
        eng = synthetic(factory, K, Q, T, 3, f32)
        asked0 = eng.get_total_questions_asked()
        if chunk is not None:
            eng.set_option("train_chunk_steps", chunk)
        if chunk == 1:
            at = int(counts[:head].sum())
            eng.train_batch_arrays(counts[:head], aqs[:at], targets[:head], amounts[:head])
            eng.set_option("train_chunk_steps", 1 << 22)
            eng.train_batch_arrays(counts[head:], aqs[at:], targets[head:], amounts[head:])
        else:
            eng.train_batch_arrays(counts, aqs, targets, amounts)
        assert kb_equal(eng, twin), f"chunk {chunk}"
        assert eng.get_total_questions_asked() == asked0 + int(counts.sum())
        eng.close()
    twin.close()


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape", ["skewed", "long_row", "gaps"])
def test_train_batch_equals_consecutive_calls_shapes(shape, f32, factory):
    rng = np.random.default_rng(11)
    if shape == "skewed":        # one target holds 30 % of the records
        K, Q, T, n, tg, qg, skew = 5, 1000, 1000, 6000, (), (), 0.3
    elif shape == "long_row":    # a row of 20000 targets
        K, Q, T, n, tg, qg, skew = 5, 200, 20000, 4000, (), (), 0.0
    else:                        # target and question gaps present, never trained
        K, Q, T, n, tg, qg, skew = 5, 300, 1000, 4000, tuple(range(5, 1000, 37)), (3, 150, 299), 0.0
    counts, aqs, targets, amounts = random_records(rng, n, Q, K, T, qgaps=qg, tgaps=tg, skew=skew)
    eng = synthetic(factory, K, Q, T, 5, f32, tg, qg)
    twin = synthetic(factory, K, Q, T, 5, f32, tg, qg)
    eng.train_batch_arrays(counts, aqs, targets, amounts)
    train_single(twin, counts, aqs, targets, amounts)
    assert kb_equal(eng, twin)
    assert eng.get_total_questions_asked() == twin.get_total_questions_asked()
    eng.close()
    twin.close()


def test_counters_and_launches_per_chunk(factory):
    K, Q, T = 5, 1000, 1000
    eng = synthetic(factory, K, Q, T, 9)
    rng = np.random.default_rng(2)
    n = 300
    counts = rng.integers(1, 9, size=n).astype(np.int64)
    # distinct questions within a record: every answered question is one step
    aqs = np.concatenate([np.stack([rng.choice(Q, size=c, replace=False), rng.integers(0, K, size=c)], axis=1) for c in counts])
    targets = rng.integers(0, T, size=n).astype(np.int64)
    amounts = rng.uniform(0.3, 2.0, size=n)
    eng.set_option("train_chunk_steps", 7)
    assert eng.get_option("train_chunk_steps") == 7
    c0, r0, l0 = (eng.get_option(x) for x in ("train_bulk_calls", "train_bulk_records", "train_bulk_launches"))
    eng.train_batch_arrays(counts, aqs, targets, amounts)
    assert eng.get_option("train_bulk_calls") == c0 + 1
    assert eng.get_option("train_bulk_records") == r0 + n
    assert eng.get_option("train_bulk_launches") == l0 + math.ceil(int(counts.sum()) / 7)
    assert eng.get_option("train_bulk_device_ns") > 0 and eng.get_option("train_bulk_host_ns") > 0
    eng.train_batch_arrays(np.zeros(0, np.int64), np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.zeros(0))   # n == 0
    assert eng.get_option("train_bulk_calls") == c0 + 1
    eng.close()


def make_quizzes(eng, rng, n, Q, K, qgaps=()):
    """n quizzes of 0-11 answers each, the last question of a quiz repeating its first."""
    valid = np.setdiff1d(np.arange(Q), np.array(list(qgaps), dtype=np.int64))
    ids = []
    for i in range(n):
        qz = eng.start_quiz()
        m = int(rng.integers(0, 12))
        qs = rng.choice(valid, size=m)
        if m >= 3:
            qs[-1] = qs[0]
        for j, q in enumerate(qs.tolist()):
            eng.set_active_question(qz, q)
            eng.record_answer(qz, (i + j) % K)
        ids.append(qz)
    return ids


@pytest.mark.parametrize("combine", [0, 1])
def test_record_quiz_target_batch_equals_consecutive_calls(combine, factory):
    K, Q, T = 5, 300, 1000
    eng = synthetic(factory, K, Q, T, 21)
    twin = synthetic(factory, K, Q, T, 21)
    ids = []
    for e in (eng, twin):
        e.set_option("combine", combine)
        ids.append(make_quizzes(e, np.random.default_rng(8), 64, Q, K))
    assert ids[0] == ids[1]
    rng = np.random.default_rng(9)
    quizzes = ids[0] + [ids[0][5]]                 # a quiz listed twice
    targets = rng.integers(0, T, size=len(quizzes))
    targets[:10] = 17                              # shared targets
    amounts = rng.uniform(0.3, 2.0, size=len(quizzes))
    asked = eng.get_total_questions_asked()
    eng.record_quiz_target_batch(quizzes, targets, amounts)
    for qz, t, a in zip(quizzes, targets.tolist(), amounts.tolist()):
        twin.record_quiz_target(qz, t, a)
    assert kb_equal(eng, twin)
    assert eng.get_total_questions_asked() == asked
    eng.close()
    twin.close()


def test_all_or_none(factory):
    case = cases.small_cases()[1]                  # gaps_37x5x101: question gaps 3, 20; target gaps
    K, Q, T = case.K, case.Q, case.T
    eng = case.make_engine(factory)
    rng = np.random.default_rng(3)
    counts, aqs, targets, amounts = random_records(rng, 6, Q, K, T, lo=2, hi=5, qgaps=case.qgaps, tgaps=case.tgaps)
    eng.train_batch_arrays(counts, aqs, targets, amounts)   # (valid as it stands)
    e3 = int(counts[:3].sum())
    gap_t = case.tgaps[0]

    def bad(what):
        c, x, t, a = counts.copy(), aqs.copy(), targets.copy(), amounts.copy()
        if what == "question":
            x[e3, 0] = Q
        elif what == "answer":
            x[e3 + 1, 1] = K
        elif what == "gap question":
            x[e3, 0] = case.qgaps[1]
        elif what == "gap target":
            t[3] = gap_t
        elif what == "amount":
            a[3] = 0.0
        elif what == "negative count":
            c[3] = -1
        return c, x, t, a

    def snapshot():
        return (eng.get_kb(), eng.get_total_questions_asked(),
                [eng.get_option(n) for n in ("train_bulk_calls", "train_bulk_records", "train_bulk_launches")])

    def same(s0, s1):
        return all(np.array_equal(x, y) for x, y in zip(s0[0], s1[0])) and s0[1:] == s1[1:]

    s0 = snapshot()
    for what in ("question", "answer", "gap question", "gap target", "amount", "negative count"):
        err = eng.train_batch_arrays(*bad(what), throw=False)
        assert err is not None and "Batch entry 3: " in err.to_string(True), what
        assert same(s0, snapshot()), what
    # null answered questions where entry 3 is the first with a count
    lib = interop.load_library()
    c = np.array([0, 0, 0, 2, 0, 0], dtype=np.int64)
    err = interop._check(lib.PqaEngine_TrainBatch(eng.c_engine, 6, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None,
                                                  targets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                  amounts.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), False)
    assert err is not None and "Batch entry 3: " in err.to_string(True)
    err = interop._check(lib.PqaEngine_TrainBatch(eng.c_engine, 6, None, None, None, None), False)
    assert err is not None and "Nullptr" in err.to_string(True)
    assert same(s0, snapshot())
    # RecordQuizTargetBatch: a released quiz, a gap target, a zero amount in entry 3
    quizzes = make_quizzes(eng, np.random.default_rng(4), 6, Q, K, case.qgaps)
    s0 = snapshot()
    ok_t = np.array([t for t in range(T) if t not in case.tgaps][:6], dtype=np.int64)
    for what in ("released", "gap target", "amount"):
        qz, t, a = list(quizzes), ok_t.copy(), np.ones(6)
        if what == "released":
            qz[3] = eng.start_quiz()
            eng.release_quiz(qz[3])
        elif what == "gap target":
            t[3] = gap_t
        else:
            a[3] = -1.0
        err = eng.record_quiz_target_batch(qz, t, a, throw=False)
        assert err is not None and "Batch entry 3: " in err.to_string(True), what
        assert same(s0, snapshot()), what
    eng.record_quiz_target_batch(quizzes, ok_t, np.ones(6))
    assert not same(s0, snapshot())
    eng.close()


@pytest.mark.parametrize("server", [0, 1])
def test_sweep_sees_the_batch(server, factory):
    case = cases.small_cases()[4]                  # 300 x 5 x 1000: the resident sweep serves rows of <= 1024 targets
    K, Q, T = case.K, case.Q, case.T
    eng, twin = case.make_engine(factory), case.make_engine(factory)
    orc = case.make_oracle()
    quizzes = []
    for e in (eng, twin):
        e.set_option("server", server)
        qz = e.start_quiz()
        e.set_active_question(qz, 10)
        e.record_answer(qz, 2)                     # leaves a speculative sweep in flight
        quizzes.append(qz)
    orc.start_quiz(cases.WORKERS)
    orc.record_answer(10, 2, cases.WORKERS - 1)
    counts, aqs, targets, amounts = random_records(np.random.default_rng(6), 500, Q, K, T)
    eng.train_batch_arrays(counts, aqs, targets, amounts)
    train_single(twin, counts, aqs, targets, amounts)
    oracle_train(orc, counts, aqs, targets, amounts, cases.WORKERS)
    assert kb_equal(eng, twin)
    pe, pt = eng.eval_priorities(quizzes[0]), twin.eval_priorities(quizzes[1])
    assert np.array_equal(pe, pt)
    assert eng.next_question_argmax(quizzes[0]) == twin.next_question_argmax(quizzes[1])
    _, opri = orc.eval(1)
    assert cases.rel_err(pe, opri).max() < 1e-9
    eng.close()
    twin.close()
    orc.close()


class devices:
    def __init__(self, spec):
        self.spec = spec

    def __enter__(self):
        self.saved = os.environ.get("PQA_DEVICES")
        os.environ["PQA_DEVICES"] = self.spec

    def __exit__(self, *a):
        if self.saved is None:
            os.environ.pop("PQA_DEVICES", None)
        else:
            os.environ["PQA_DEVICES"] = self.saved


@pytest.mark.parametrize("T", [1000, 20000])
def test_sharded_batch_equals_whole_engine(T, factory):
    K, Q = 5, 120
    with devices("0,0,0,0"):
        sh = synthetic(factory, K, Q, T, 13, qgaps=(70,))
    assert sh.get_option("shards") == 4
    whole = synthetic(factory, K, Q, T, 13, qgaps=(70,))
    counts, aqs, targets, amounts = random_records(np.random.default_rng(5), 2000, Q, K, T, qgaps=(70,))
    for e in (sh, whole):
        e.set_option("workers", 16)
        e.train_batch_arrays(counts, aqs, targets, amounts)
    assert kb_equal(sh, whole)
    assert sh.get_total_questions_asked() == whole.get_total_questions_asked()
    ids = [make_quizzes(e, np.random.default_rng(1), 20, Q, K, (70,)) for e in (sh, whole)]
    assert ids[0] == ids[1]
    qt = np.random.default_rng(2).integers(0, T, size=20)
    for e, qz in zip((sh, whole), ids):
        e.record_quiz_target_batch(qz, qt, np.full(20, 0.7))
    assert kb_equal(sh, whole)
    # question 70 is at a gap and owned by shard 2: no shard trains
    before = sh.get_kb()
    c, x = counts[:6].copy(), aqs[:int(counts[:6].sum())].copy()
    x[int(c[:3].sum()), 0] = 70
    with pytest.raises(interop.PqaException, match="Batch entry 3"):
        sh.train_batch_arrays(c, x, targets[:6], amounts[:6])
    assert all(np.array_equal(a, b) for a, b in zip(before, sh.get_kb()))
    sh.close()
    whole.close()
