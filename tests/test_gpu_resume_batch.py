"""PqaEngine_ResumeQuizBatch, the long-row ResumeQuiz and combined ResumeQuiz calls on a real MI355X: every posterior bit-identical
to the CPU oracle's resume_quiz and to a single ResumeQuiz of the same list; ids, all-or-none, combining, the sharded engine."""
import json
import os
import sys
import threading

import numpy as np
import pytest

import cases
import orclib
from probqa_amd import interop

pytestmark = pytest.mark.gpu

GDIR = os.path.join(os.path.dirname(__file__), "golden")


def aq_list(pairs):
    return [interop.AnsweredQuestion(int(q), int(a)) for q, a in pairs]


def ragged_lists(rng, n, Q, K, max_len=40, qgaps=()):
    """n answer lists with counts 0, 1, 2 ... max_len (cycled, then shuffled), repeated questions and every answer value."""
    valid = np.array([q for q in range(Q) if q not in set(qgaps)])
    out = []
    for i in range(n):
        m = i % (max_len + 1)
        qs = rng.choice(valid, size=m, replace=True)
        if m >= 3:
            qs[m // 2] = qs[0]                     # a repeated question
        out.append([(int(q), int((i + j) % K)) for j, q in enumerate(qs)])
    order = rng.permutation(n)
    return [out[i] for i in order]


def oracle_resume(orc, pairs, workers, bug):
    if not pairs:
        orc.start_quiz(workers)
    else:
        assert orc.resume_quiz(pairs, workers, bool(bug)) == 0
    return orc.priors().copy()


def synthetic(factory, K, Q, T, seed, tgaps=(), f32=False):
    d = (interop.EngineDefinition(K, Q, T, init_amount=0.1, prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)
         if f32 else interop.EngineDefinition(K, Q, T, init_amount=0.1))
    eng, err = factory.create_cpu_engine(d)
    assert err is None and eng is not None, err
    eng.fill_synthetic(8.0, 0.5, seed)
    if tgaps:
        eng.set_target_gaps(list(tgaps))
    return eng


def oracle_of(eng, K, Q, T, tgaps=()):
    orc = orclib.Oracle(K, Q, T, 0.1)
    orc.set_kb(*eng.get_kb())
    orc.set_target_gaps(list(tgaps))
    return orc


def check_batch_against_oracle(eng, orc, lists, workers, bug):
    eng.set_option("workers", workers)
    eng.set_option("bug_compat", bug)
    ids = eng.resume_quiz_batch([aq_list(l) for l in lists])
    assert len(ids) == len(lists) and len(set(ids)) == len(ids)
    for i, (quiz, l) in enumerate(zip(ids, lists)):
        want = oracle_resume(orc, l, workers, bug)
        got = eng.get_priors(quiz)
        assert np.array_equal(got, want), f"entry {i} ({len(l)} answers, workers {workers}, bug {bug}): max rel {cases.rel_err(got, want).max():g}"
    for quiz in ids:
        eng.release_quiz(quiz)


def _golden_names():
    return sorted(f[:-5] for f in os.listdir(GDIR) if f.endswith(".json"))


@pytest.mark.parametrize("name", _golden_names())
def test_batch_matches_oracle_on_golden_cases(name, factory):
    sys.path.insert(0, GDIR)
    import make_golden

    case = make_golden.case_from_meta(json.load(open(os.path.join(GDIR, name + ".json"))))
    eng, orc = case.make_engine(factory), case.make_oracle()
    rng = np.random.default_rng(11)
    lists = ragged_lists(rng, 64, case.Q, case.K, qgaps=case.qgaps)
    lists[0] = list(case.answers)
    for workers in (1, 16, 64):
        for bug in (0, 1):
            check_batch_against_oracle(eng, orc, lists, workers, bug)
    eng.close()


@pytest.mark.parametrize("shape,runs,n", [
    ((5, 1000, 1000), [(16, 1), (64, 0), (1, 1)], 300),
    ((5, 2000, 10000), [(16, 0), (64, 1)], 96),
    ((5, 40, 20000), [(16, 1), (64, 0)], 64),      # long rows: the multi-workgroup resume
    ((3, 20, 100000), [(16, 0), (1, 1)], 64),
], ids=["1000x5x1000", "2000x5x10000", "40x5x20000", "20x3x100000"])
def test_batch_matches_oracle_on_synthetic_cubes(shape, runs, n, factory):
    K, Q, T = shape
    tgaps = (3, 17, T - 1)
    eng = synthetic(factory, K, Q, T, 5, tgaps)
    orc = oracle_of(eng, K, Q, T, tgaps)
    lists = ragged_lists(np.random.default_rng(T), n, Q, K)
    for workers, bug in runs:
        check_batch_against_oracle(eng, orc, lists, workers, bug)
    eng.close()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("T", [1000, 20000])
def test_batch_quiz_is_the_single_call_quiz(f32, T, factory):
    K, Q = 5, 300
    eng = synthetic(factory, K, Q, T, 9, f32=f32)
    eng.set_option("workers", 16)
    lists = ragged_lists(np.random.default_rng(2), 24, Q, K, max_len=12)
    lists = [l for l in lists if l] + [[]]
    batch = eng.resume_quiz_batch([aq_list(l) for l in lists])
    single = [eng.resume_quiz(aq_list(l)) for l in lists]
    for i, (qb, qs) in enumerate(zip(batch, single)):
        assert np.array_equal(eng.get_priors(qb), eng.get_priors(qs)), f"entry {i}: posterior"
        assert np.array_equal(eng.eval_priorities(qb), eng.eval_priorities(qs)), f"entry {i}: priorities (asked sets)"
        assert eng.next_question_argmax(qb) == eng.next_question_argmax(qs)
        assert eng.next_question_sampled(qb, 0x9E3779B97F4A7C15) == eng.next_question_sampled(qs, 0x9E3779B97F4A7C15)
        for q in (qb, qs):
            eng.set_active_question(q, eng.next_question_argmax(q))
            eng.record_answer(q, i % K)
        assert np.array_equal(eng.get_priors(qb), eng.get_priors(qs)), f"entry {i}: posterior after RecordAnswer"
        tb, ts = eng.list_top_targets(qb, 10), eng.list_top_targets(qs, 10)
        assert [(t.i_target, t.prob) for t in tb] == [(t.i_target, t.prob) for t in ts]
    # RecordQuizTarget of a batch-resumed quiz trains exactly what the single-resumed twin's would (twin engines, same history)
    twin = synthetic(factory, K, Q, T, 9) if not f32 else None
    if twin is not None:
        twin.set_option("workers", 16)
        l = lists[0]
        qb = eng.resume_quiz_batch([aq_list(l)])[0]
        qs = twin.resume_quiz(aq_list(l))
        eng.record_quiz_target(qb, 7, 1.5)
        twin.record_quiz_target(qs, 7, 1.5)
        for a, b in zip(eng.get_kb(), twin.get_kb()):
            assert np.array_equal(a, b)
        twin.close()
    eng.close()


def test_ids_and_all_or_none(factory):
    K, Q, T = 5, 200, 1000
    a, b = synthetic(factory, K, Q, T, 4), synthetic(factory, K, Q, T, 4)
    for e in (a, b):   # the same history: ids handed out and given back
        qs = [e.start_quiz() for _ in range(6)]
        e.release_quiz(qs[1])
        e.release_quiz(qs[4])
    lists = ragged_lists(np.random.default_rng(8), 12, Q, K, max_len=6)
    assert a.resume_quiz_batch([aq_list(l) for l in lists]) == [b.resume_quiz(aq_list(l)) for l in lists]
    nxt = a.start_quiz()
    a.release_quiz(nxt)
    good = [aq_list(l) for l in lists]
    for bad, what in (([interop.AnsweredQuestion(Q, 0)], "Question index"), ([interop.AnsweredQuestion(3, K)], "Answer index"),
                      ([interop.AnsweredQuestion(-1, 0)], "Question index")):
        with pytest.raises(interop.PqaException, match="Batch entry 5: " + what):
            a.resume_quiz_batch(good[:5] + [bad] + good[5:])
        assert a.start_quiz() == nxt
        a.release_quiz(nxt)
    lib = interop.load_library()
    counts = (interop.ctypes.c_int64 * 3)(1, -2, 1)
    aqs = (interop.CiAnsweredQuestion * 2)()
    out = (interop.ctypes.c_int64 * 3)()
    with pytest.raises(interop.PqaException, match="non-negative"):
        interop._check(lib.PqaEngine_ResumeQuizBatch(a.c_engine, 3, counts, aqs, out))
    counts = (interop.ctypes.c_int64 * 3)(1, 2, 1)
    with pytest.raises(interop.PqaException, match="Nullptr"):
        interop._check(lib.PqaEngine_ResumeQuizBatch(a.c_engine, 3, counts, None, out))
    with pytest.raises(interop.PqaException, match="Nullptr"):
        interop._check(lib.PqaEngine_ResumeQuizBatch(a.c_engine, 3, None, aqs, out))
    with pytest.raises(interop.PqaException, match="non-negative"):
        interop._check(lib.PqaEngine_ResumeQuizBatch(a.c_engine, -1, counts, aqs, out))
    assert a.start_quiz() == nxt
    a.release_quiz(nxt)
    # every target in a gap: I64Underflow, nothing created
    a.set_target_gaps(list(range(T)))
    with pytest.raises(interop.PqaException, match="Max exponent"):
        a.resume_quiz_batch(good[1:4])
    assert a.start_quiz() == nxt
    a.close()
    b.close()
    # a 1000-quiz batch crosses chunk boundaries
    c, d = synthetic(factory, K, Q, T, 4), synthetic(factory, K, Q, T, 4)
    lists = ragged_lists(np.random.default_rng(9), 1000, Q, K, max_len=8)
    ids = c.resume_quiz_batch([aq_list(l) for l in lists])
    assert ids == list(range(1000))
    for i in (0, 255, 256, 257, 511, 512, 999):
        assert np.array_equal(c.get_priors(ids[i]), d.get_priors(d.resume_quiz(aq_list(lists[i])))), i
    c.close()
    d.close()


@pytest.mark.parametrize("form", [1, 0], ids=["long_row_form", "one_workgroup"])
def test_long_row_single_resume_matches_oracle(form, factory):
    K, Q, T = 5, 200, 100000
    tgaps = (0, 50000, T - 1)
    eng = synthetic(factory, K, Q, T, 12, tgaps)
    eng.set_option("workers", 16)
    eng.set_option("long_row_form", form)
    orc = oracle_of(eng, K, Q, T, tgaps)
    rng = np.random.default_rng(5)
    lists = [[(int(q), int(rng.integers(K))) for q in rng.choice(Q, 16, replace=False)], [(7, 2)],
             [(11, 0)] * 1000]                         # the same answer 1000 times: some elements flush to 0
    for bug in (1, 0):
        eng.set_option("bug_compat", bug)
        for l in lists:
            want = oracle_resume(orc, l, 16, bug)
            quiz = eng.resume_quiz(aq_list(l))
            assert np.array_equal(eng.get_priors(quiz), want), f"{len(l)} answers, bug {bug}"
            eng.release_quiz(quiz)
    mask = np.ones(T, bool)
    mask[list(tgaps)] = False
    assert (want[mask] == 0).any() and (want[mask] > 0).any()   # the flush case did flush
    eng.close()


@pytest.mark.parametrize("mode", ["post_always", "contention"])
def test_combined_resumes(mode, factory):
    K, Q, T = 5, 300, 1000
    eng = synthetic(factory, K, Q, T, 6)
    ref = synthetic(factory, K, Q, T, 6)
    for e in (eng, ref):
        e.set_option("workers", 16)
    eng.set_option("combine", 1)
    if mode == "post_always":
        eng.set_option("post_always", 1)
    rng = np.random.default_rng(21)
    lists = [ragged_lists(rng, 8, Q, K, max_len=10) for _ in range(32)]
    lists[5][3] = [(2, 1), (Q + 7, 0)]                 # the one failing call
    want = {}
    for t in range(32):
        for k in range(8):
            if (t, k) != (5, 3):
                want[(t, k)] = ref.get_priors(ref.resume_quiz(aq_list(lists[t][k])))
    posted0, batches0 = eng.get_option("resumes_batched"), eng.get_option("resume_batches")
    got, errors = {}, {}
    barrier = threading.Barrier(32)

    def client(t):
        barrier.wait()
        for k in range(8):
            try:
                got[(t, k)] = eng.resume_quiz(aq_list(lists[t][k]))
            except interop.PqaException as ex:
                errors[(t, k)] = str(ex)

    threads = [threading.Thread(target=client, args=(t,)) for t in range(32)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert list(errors) == [(5, 3)] and "Question index" in errors[(5, 3)]
    assert len(set(got.values())) == len(got) == 255
    for key, quiz in got.items():
        assert np.array_equal(eng.get_priors(quiz), want[key]), key
    posted = eng.get_option("resumes_batched") - posted0
    batches = eng.get_option("resume_batches") - batches0
    if mode == "post_always":
        assert posted == 256
    assert 0 <= batches <= posted <= 256
    assert (posted == 0) == (batches == 0)
    eng.close()
    ref.close()


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
        sh = synthetic(factory, K, Q, T, 13)
    assert sh.get_option("shards") == 4
    whole = synthetic(factory, K, Q, T, 13)
    for e in (sh, whole):
        e.set_option("workers", 16)
        e.start_quiz()
    lists = ragged_lists(np.random.default_rng(4), 40, Q, K, max_len=20)
    ids_s = sh.resume_quiz_batch([aq_list(l) for l in lists])
    ids_w = whole.resume_quiz_batch([aq_list(l) for l in lists])
    assert ids_s == ids_w
    for qs, qw in zip(ids_s, ids_w):
        assert np.array_equal(sh.get_priors(qs), whole.get_priors(qw))
    nxt = sh.start_quiz()
    sh.release_quiz(nxt)
    with pytest.raises(interop.PqaException, match="Batch entry 2"):
        sh.resume_quiz_batch([aq_list(lists[0]), aq_list(lists[1]), [interop.AnsweredQuestion(Q, 0)]])
    assert sh.start_quiz() == nxt
    sh.close()
    whole.close()
