"""PqaEngine_NextQuestionSampledBatch / PqaEngine_NextQuestionBatch through the C ABI: the reference's sampled selector
(PqaCore/CpuEngine.cpp:362-400) for many quizzes, one batched sweep and one selector launch behind it (select_kernels.hip).

Held to: the host's selector over the same priority bits (option sampled_batch_host on a twin engine -- no exemption), the oracle,
consecutive single calls on a twin engine, a plain-Python restatement of the selector (Float engines) and the whole engine (sharded).
Random draws compared with another sweep's priorities are guarded on the INPUT side (sampled_batch_common.boundary_distance, from the
oracle's run lengths alone; tests/test_sampled_batch_abi.py checks the seeds without a GPU), so every comparison is exact equality."""
import os

import numpy as np
import pytest

import cases
import sampled_batch_common as sb
from probqa_amd import interop

pytestmark = pytest.mark.gpu

BATCH_SIZES = [1, 2, 7, 8, 31, 32, 33, 64, 65, 200, 256]
FIXED_RNDS = [0, 1, 2**63, 2**64 - 1]


def plain_engine(factory, K, Q, T, seed, qgaps=(), float_engine=False):
    kw = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24) if float_engine else {}
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **kw))
    assert err is None and eng is not None, err
    eng.fill_synthetic(8.0, 0.5, seed)
    eng.set_option("workers", cases.WORKERS)
    if qgaps:
        eng.set_question_gaps(list(qgaps))
    return eng


def quiz_scripts(Q, K, n, qgaps, seed, exhaust):
    """Per quiz a list of (question, answer): 0 to 20 answers (as many as the cube has questions); quiz `exhaust` answers every
    question.  The last question is never asked, except by the exhausted quiz."""
    rng = np.random.default_rng(seed)
    free = [q for q in range(Q) if q not in qgaps]
    scripts = []
    for j in range(n):
        depth = len(free) if j == exhaust else min(j % 21, max(len(free) - 1, 0))
        pool = free if j == exhaust else free[:-1]
        qs = rng.permutation(pool)[:depth] if depth else []
        scripts.append([(int(q), int(rng.integers(0, K))) for q in qs])
    return scripts


def play(eng, scripts):
    quizzes = eng.start_quiz_batch(len(scripts))
    for r in range(max(len(s) for s in scripts)):
        live = [j for j, s in enumerate(scripts) if len(s) > r]
        for j in live:
            eng.set_active_question(quizzes[j], scripts[j][r][0])
        eng.record_answer_batch([quizzes[j] for j in live], [scripts[j][r][1] for j in live])
    return quizzes


@pytest.mark.parametrize("Q", [1, 5, 37, 127, 1000, 1001, 9000, 30000])
def test_device_selector_equals_host_selector(Q, factory):
    """Same engine state, same random numbers, sampled_batch_host 0 and 1 on twin engines: identical picks for every quiz, whichever
    priority layout the sweep leaves (batch_form 1 / 2 / 3) and however many subtasks split the question axis."""
    K, T = 5, 40
    qgaps = [3, Q // 2] if Q > 5 else []
    exhaust = 5 if Q <= 1001 else -1
    scripts = quiz_scripts(Q, K, 256, qgaps, 1000 + Q, exhaust)
    dev, host = (plain_engine(factory, K, Q, T, 77, qgaps) for _ in range(2))
    host.set_option("sampled_batch_host", 1)
    qd, qh = play(dev, scripts), play(host, scripts)
    assert qd == qh
    rng = np.random.default_rng(Q)
    calls = 0
    for subtasks in (1, 3, 0):
        for form in (1, 2, 3):
            for eng in (dev, host):
                eng.set_option("eval_subtasks", subtasks)
                eng.set_option("batch_form", form)
            for n in BATCH_SIZES:
                first = int(rng.integers(0, 257 - n))
                ids = qd[first:first + n]
                if exhaust >= 0 and n >= 7 and qd[exhaust] not in ids:
                    ids = ids[:-1] + [qd[exhaust]]
                pool = FIXED_RNDS + [int(x) for x in rng.integers(0, 2**64, size=n, dtype=np.uint64)]
                rnds = pool[calls % 5:][:n]   # (small batches meet every fixed number over the calls)
                a, b = dev.next_question_sampled_batch(ids, rnds), host.next_question_sampled_batch(ids, rnds)
                assert a == b, f"Q={Q} subtasks={subtasks} form={form} n={n}: {[(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:8]}"
                if exhaust >= 0 and qd[exhaust] in ids:
                    assert a[ids.index(qd[exhaust])] == -1
                assert all(0 <= x < Q and x not in qgaps for i, x in zip(ids, a) if exhaust < 0 or i != qd[exhaust])
                calls += 1
    assert dev.get_option("sampled_batches") == calls and host.get_option("sampled_batches") == calls
    assert dev.get_option("priority_host_bytes") == 0 and host.get_option("priority_host_bytes") > 0
    dev.close()
    host.close()


def scenario_engines(case, factory, n_engines):
    out = []
    for _ in range(n_engines):
        eng = case.make_engine(factory)
        quizzes = eng.start_quiz_batch(len(case.answers) + 1)
        for i, quiz in enumerate(quizzes):
            for q, a in case.answers[:i]:
                eng.set_active_question(quiz, q)
                eng.record_answer(quiz, a)
        out.append((eng, quizzes))
    return out


def assert_guarded(case, steps, rnds):
    for i, r in enumerate(rnds):
        d = sb.boundary_distance(steps[i][0], sb.SUBTASKS, r)
        assert d > sb.GUARD, f"{case.name}: draw {r:#x} of quiz {i} lies {d:g} from a run-length boundary: choose another seed"


@pytest.mark.parametrize("case", sb.scenarios(), ids=lambda c: c.name)
def test_batch_against_oracle_and_single_calls(case, factory):
    """Quizzes at different steps of a script in one batch: every pick is the oracle's (orc.select_sampled over orc.eval's run
    lengths) and the single call's on a twin engine; then the same active questions, the same counter, and bit-identical posteriors
    after the next RecordAnswerBatch."""
    steps = sb.oracle_steps(case)
    (eb, qb), (es, qs) = scenario_engines(case, factory, 2)
    assert eb.get_option("eval_subtasks") == sb.SUBTASKS
    asked0 = eb.get_total_questions_asked(), es.get_total_questions_asked()
    served = 0
    for rnds, guarded in sb.batches(case):
        if guarded:
            assert_guarded(case, steps, rnds)
        want = [steps[i][1][r] for i, r in enumerate(rnds)]
        got = eb.next_question_sampled_batch(qb, rnds)
        exhausted = [w < 0 for w in want]
        assert got == [-1 if x else w for x, w in zip(exhausted, want)], f"{case.name} rnds={[hex(r) for r in rnds]}: {got} != {want}"
        single = []
        for quiz, r, x in zip(qs, rnds, exhausted):
            if x:
                with pytest.raises(interop.PqaException, match="run out of questions"):
                    es.next_question_sampled(quiz, r)
                single.append(-1)
            else:
                single.append(es.next_question_sampled(quiz, r))
        assert got == single
        served += sum(not x for x in exhausted)
        assert [eb.get_active_question_id(q) for q, x in zip(qb, exhausted) if not x] == [es.get_active_question_id(q) for q, x in zip(qs, exhausted) if not x]
        assert eb.get_total_questions_asked() - asked0[0] == served == es.get_total_questions_asked() - asked0[1]
    live = [i for i, g in enumerate(got) if g >= 0]
    answers = [(g + i) % case.K for i, g in enumerate(got) if g >= 0]
    eb.record_answer_batch([qb[i] for i in live], answers)
    es.record_answer_batch([qs[i] for i in live], answers)
    for i in live:
        assert np.array_equal(eb.get_priors(qb[i]), es.get_priors(qs[i])), f"{case.name} quiz {i}: posterior after the batch"
    eb.close()
    es.close()


def test_next_question_batch_follows_the_engine_generator(factory):
    """select = 0 and a seeded generator: one NextQuestionBatch equals consecutive NextQuestion calls in batch order, over 20 rounds
    of answer + select; select = 1: the argmax batch."""
    K, Q, T, n = 5, 300, 200, 24
    a, b = (plain_engine(factory, K, Q, T, 5) for _ in range(2))
    for eng in (a, b):
        eng.set_option("select", 0)
        eng.set_option("seed", 4242)
    qa, qb = a.start_quiz_batch(n), b.start_quiz_batch(n)
    for rnd in range(20):
        got = a.next_question_batch(qa)
        want = [b.next_question(q) for q in qb]
        assert got == want, f"round {rnd}"
        answers = [(g + rnd) % K for g in got]
        a.record_answer_batch(qa, answers)
        b.record_answer_batch(qb, answers)
    assert a.get_option("sampled_batches") == 20
    for eng in (a, b):
        eng.set_option("select", 1)
    assert a.next_question_batch(qa) == b.next_question_argmax_batch(qb)
    assert a.get_option("sampled_batches") == 20
    assert a.next_question_batch([]) == [] and a.next_question_sampled_batch([], []) == []
    a.close()
    b.close()


def test_errors_change_nothing(factory):
    K, Q, T = 5, 200, 100
    a, b = (plain_engine(factory, K, Q, T, 9) for _ in range(2))
    for eng in (a, b):
        eng.set_option("select", 0)
        eng.set_option("seed", 17)
    qa, qb = a.start_quiz_batch(300), b.start_quiz_batch(300)
    first = a.next_question_sampled_batch(qa[:10], list(range(1, 11)))
    assert first == b.next_question_sampled_batch(qb[:10], list(range(1, 11)))
    before = [a.get_active_question_id(q) for q in qa[:10]], a.get_total_questions_asked(), a.get_option("sampled_batches")
    unknown = max(qa) + 1000
    lib = interop.load_library()
    import ctypes

    def raw(fn, n, ids, rnds, out):
        e = fn(a.c_engine, n, ids, *(([rnds] if rnds is not False else []) + [out]))
        assert e, "the call must be refused"
        msg = interop.PqaError(e).to_string(True)
        return msg

    for call in ("sampled", "plain"):
        def go(ids):
            return a.next_question_sampled_batch(ids, [5] * len(ids)) if call == "sampled" else a.next_question_batch(ids)
        with pytest.raises(interop.PqaException, match=r"quizId=%d\b.*twice|twice.*quizId=%d\b" % (qa[3], qa[3])):
            go(qa[:5] + [qa[3]])
        with pytest.raises(interop.PqaException, match=str(unknown)):
            go(qa[:5] + [unknown])
        with pytest.raises(interop.PqaException, match="257"):
            go(qa[:257])
    ids = (ctypes.c_int64 * 4)(*qa[:4])
    rn = (ctypes.c_uint64 * 4)(1, 2, 3, 4)
    out = (ctypes.c_int64 * 4)()
    null64, nullu = ctypes.POINTER(ctypes.c_int64)(), ctypes.POINTER(ctypes.c_uint64)()
    for args in ((null64, rn, out), (ids, nullu, out), (ids, rn, null64)):
        assert "Nullptr" in raw(lib.PqaEngine_NextQuestionSampledBatch, 4, args[0], args[1], args[2])
    for args in ((null64, out), (ids, null64)):
        assert "Nullptr" in raw(lib.PqaEngine_NextQuestionBatch, 4, args[0], False, args[1])
    assert ([a.get_active_question_id(q) for q in qa[:10]], a.get_total_questions_asked(), a.get_option("sampled_batches")) == before
    # the generator: the twin never made a failing call and draws the same questions
    assert [a.next_question(q) for q in qa[:6]] == [b.next_question(q) for q in qb[:6]]
    assert a.next_question_batch(qa[6:40]) == b.next_question_batch(qb[6:40])
    a.close()
    b.close()


@pytest.mark.parametrize("Q,T", [(300, 200), (1000, 64)])
def test_float_engine_equals_the_python_selector(Q, T, factory):
    """Float engines: both EvalPrioritiesBatch and the sampled batch take the row-sharing sweep, so the selector restated in plain
    Python over eval_priorities_batch of the same quizzes must give the same picks exactly."""
    K, n = 5, 70
    qgaps = [2, Q // 3]
    eng = plain_engine(factory, K, Q, T, 31, qgaps, float_engine=True)
    assert eng.get_option("precision") == 1
    scripts = quiz_scripts(Q, K, n, qgaps, 55, -1)
    quizzes = play(eng, scripts)
    pri = eng.eval_priorities_batch(quizzes, Q)
    rng = np.random.default_rng(8)
    rnds = (FIXED_RNDS + [int(x) for x in rng.integers(0, 2**64, size=n, dtype=np.uint64)])[:n]
    got = eng.next_question_sampled_batch(quizzes, rnds)
    for i in range(n):
        skip = [False] * Q
        for q in qgaps + [q for q, _ in scripts[i]]:
            skip[q] = True
        assert got[i] == sb.select_py(pri[i], skip, sb.SUBTASKS, rnds[i]), f"quiz {i} rnd {rnds[i]:#x}"
    eng.close()


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


@pytest.mark.parametrize("case", [sb.scenarios()[1], sb.scenarios()[4]], ids=lambda c: c.name)
def test_sharded_engine_equals_the_whole_engine(case, factory):
    steps = sb.oracle_steps(case)
    with devices("0,0,0"):
        (sh, qsh), (sh2, qsh2) = scenario_engines(case, factory, 2)
    assert sh.get_option("shards") == 3
    ((whole, qw),) = scenario_engines(case, factory, 1)
    for rnds, guarded in sb.batches(case):
        if guarded:
            assert_guarded(case, steps, rnds)
        got = sh.next_question_sampled_batch(qsh, rnds)
        assert got == whole.next_question_sampled_batch(qw, rnds)
        assert got == [steps[i][1][r] if steps[i][1][r] >= 0 else -1 for i, r in enumerate(rnds)]
        assert [sh.get_active_question_id(q) for q, g in zip(qsh, got) if g >= 0] == [g for g in got if g >= 0]
    with pytest.raises(interop.PqaException, match="twice"):
        sh.next_question_sampled_batch(qsh[:2] + [qsh[0]], [1, 2, 3])
    # the sharded engine's own generator: a batch equals consecutive calls on a twin
    live = [i for i in range(len(qsh)) if steps[i][1][0] >= 0]
    for eng in (sh, sh2):
        eng.set_option("select", 0)
        eng.set_option("seed", 99)
    assert sh.next_question_batch([qsh[i] for i in live]) == [sh2.next_question(qsh2[i]) for i in live]
    for eng in (sh, sh2, whole):
        eng.close()
