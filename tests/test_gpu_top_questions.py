"""PqaEngine_ListTopQuestions / PqaEngine_ListTopQuestionsBatch through the C ABI: the best next questions of a quiz, listed on the
device (kb_kernels.hip: top_questions_chunks_kernel, top_questions_tile_kernel, top_merge_kernel).

The reference of every comparison is the engine's own PqaEngine_EvalPriorities / PqaEngine_EvalPrioritiesBatch output, sorted in numpy
by (-priority, index) with the non-positive entries dropped.  Equality is exact: indices equal, priorities bit-equal, counts equal."""
import ctypes

import numpy as np
import pytest

import cases
from probqa_amd import dist as pdist
from probqa_amd import interop, synth

pytestmark = pytest.mark.gpu


def reference(pri, max_count, q_first=0):
    pri = np.asarray(pri, dtype=np.float64)
    idx = np.flatnonzero(pri > 0)
    order = idx[np.lexsort((idx, -pri[idx]))][:max(max_count, 0)]
    return [(int(q) + q_first, float(pri[q])) for q in order]


def same(got, want):
    """Record for record: indices equal, priorities bit-equal."""
    return len(got) == len(want) and all(a[0] == b[0] and np.float64(a[1]).view(np.int64) == np.float64(b[1]).view(np.int64) for a, b in zip(got, want))


def synth_engine(factory, K, Q, T, seed=7, qgaps=(), float_engine=False):
    kw = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24) if float_engine else {}
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **kw))
    assert err is None and eng is not None, err
    eng.fill_synthetic(8.0, 0.5, seed)
    eng.set_option("workers", cases.WORKERS)
    if qgaps:
        eng.set_question_gaps(list(qgaps))
    return eng


def answer(eng, quiz, pairs):
    for q, a in pairs:
        eng.set_active_question(quiz, q)
        eng.record_answer(quiz, a)


def err_class(text):
    return str(text).split("]")[0].lstrip("[")


# ---- sizes at which the kernels can go wrong ------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,counts", [(1000, (1, 10, 256)), (1024, (10, 256)), (1025, (1, 10, 256)), (5000, (1, 10, 256)), (70000, (256, 1, 10))],
                         ids=lambda v: str(v) if isinstance(v, int) else "")
def test_sizes(Q, counts, factory):
    """One wave list partly filled; the wave boundary; two workgroups and one merge; 69 wave lists, fan-in 64 and two merge levels."""
    eng = synth_engine(factory, 2, Q, 16)
    quiz = eng.start_quiz()
    for state in range(2):
        pri = eng.eval_priorities(quiz)
        for n in counts:
            got = eng.list_top_questions(quiz, n)
            assert same(got, reference(pri, n)), (Q, state, n, got[:4], reference(pri, n)[:4])
        answer(eng, quiz, [(Q - 1, 1)])
    eng.close()


# ---- real rows ----------------------------------------------------------------------------------------------------------------
def real_cases():
    big = cases.Case("synth_1000x5x1000", 5, 1000, 1000, seed=21, answers=cases.consistent_answers(1000, 1000) + [(100, 2), (900, 4)])
    return cases.small_cases() + [big]


@pytest.mark.parametrize("case", real_cases(), ids=lambda c: c.name)
def test_real_rows_and_argmax(case, factory):
    """The fixture cubes fresh and after each of their recorded answers: the listing is the sorted EvalPriorities, and its first entry
    is the question NextQuestionArgmax selects on a second, identical engine (the quiz under test is not advanced)."""
    eng, twin = case.make_engine(factory), case.make_engine(factory)
    quiz, tquiz = eng.start_quiz(), twin.start_quiz()
    for step in range(len(case.answers) + 1):
        before = eng.get_active_question_id(quiz)
        pri = eng.eval_priorities(quiz)
        for n in (1, 5, 32, 256):
            assert same(eng.list_top_questions(quiz, n), reference(pri, n)), (case.name, step, n)
        assert eng.get_active_question_id(quiz) == before
        top = eng.list_top_questions(quiz, 1)
        assert top and top[0][0] == twin.next_question_argmax(tquiz), (case.name, step)
        if step < len(case.answers):
            answer(eng, quiz, [case.answers[step]])
            answer(twin, tquiz, [case.answers[step]])
    eng.close()
    twin.close()


# ---- eligibility ----------------------------------------------------------------------------------------------------------------
def test_asked_and_gap_questions_are_never_listed(factory):
    Q, gaps = 2100, [0, 1023, 1024, 2047, 2048]
    eng = synth_engine(factory, 2, Q, 16, qgaps=gaps)
    quiz = eng.start_quiz()
    rng = np.random.default_rng(3)
    free = [q for q in range(Q) if q not in gaps]
    script = [(int(q), int(rng.integers(0, 2))) for q in rng.permutation(free)[:40]]
    script[0] = (1, 0)
    script[1] = (1022, 1)
    script[2] = (1025, 0)
    asked = set()
    for depth in (0, 1, 40):
        answer(eng, quiz, script[len(asked):depth])
        asked = {q for q, _ in script[:depth]}
        pri = eng.eval_priorities(quiz)
        for n in (256, Q):   # (Q: everything eligible, through the host's listing)
            got = eng.list_top_questions(quiz, n)
            assert same(got, reference(pri, n)), (depth, n)
            assert not ({q for q, _ in got} & (asked | set(gaps))), (depth, n)
        assert len(eng.list_top_questions(quiz, Q)) == int((pri > 0).sum())
    eng.close()


def test_short_and_empty_listings(factory):
    """max_count beyond the eligible questions lists them all; a quiz with every question asked lists nothing and is no error."""
    Q = 40
    eng = synth_engine(factory, 3, Q, 50, qgaps=[5])
    quiz = eng.start_quiz()
    pri = eng.eval_priorities(quiz)
    got = eng.list_top_questions(quiz, 256)
    assert same(got, reference(pri, 256)) and len(got) == int((pri > 0).sum()) <= Q - 1
    answer(eng, quiz, [(q, q % 3) for q in range(Q) if q != 5])
    assert eng.list_top_questions(quiz, 10) == []
    assert eng.list_top_questions_batch([quiz], 10) == [[]]
    assert eng.list_top_questions(quiz, 0) == []
    eng.close()


# ---- ties -----------------------------------------------------------------------------------------------------------------------
def test_equal_priorities_list_by_ascending_question(factory):
    """Questions 3, 700, 1023, 1024 and 4999 are copies of the cube's best question: they (and it) tie for the top, across waves,
    workgroups and merge inputs, and appear in ascending index wherever the list ends."""
    K, Q, T = 2, 5000, 16
    A, D, B = synth.synthetic_kb(K, Q, T, 0.1, 8.0, 0.5, 9)
    probe, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
    assert err is None
    probe.set_kb(A, D, B)
    best = int(np.argmax(probe.eval_priorities(probe.start_quiz())))
    probe.close()
    copies = [3, 700, 1023, 1024, 4999]
    for c in copies:
        A[c], D[c] = A[best], D[best]
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
    assert err is None
    eng.set_kb(A, D, B)
    quiz = eng.start_quiz()
    pri = eng.eval_priorities(quiz)
    tied = sorted(set(copies + [best]))
    assert len({pri[q] for q in tied}) == 1 and [q for q, _ in reference(pri, len(tied))] == tied
    for n in range(1, len(tied) + 3):
        got = eng.list_top_questions(quiz, n)
        assert same(got, reference(pri, n)), n
        assert [q for q, _ in got][:len(tied)] == tied[:n]
    assert same(eng.list_top_questions(quiz, 256), reference(pri, 256))
    assert same(eng.list_top_questions_batch([quiz], 4)[0], reference(eng.eval_priorities_batch([quiz])[0], 4))
    eng.close()


# ---- the host's listing and the Float engine ------------------------------------------------------------------------------------
def test_long_lists_on_the_host(factory):
    eng = synth_engine(factory, 2, 1000, 16)
    quiz = eng.start_quiz()
    answer(eng, quiz, [(10, 1)])
    pri = eng.eval_priorities(quiz)
    assert same(eng.list_top_questions(quiz, 300), reference(pri, 300))
    assert same(eng.list_top_questions_batch([quiz], 300)[0], reference(eng.eval_priorities_batch([quiz])[0], 300))
    eng.close()


def test_float_engine_lists_by_its_own_priorities(factory):
    eng = synth_engine(factory, 5, 5000, 40, float_engine=True)
    quiz = eng.start_quiz()
    answer(eng, quiz, [(17, 2), (4000, 0)])
    pri = eng.eval_priorities(quiz)
    for n in (1, 10, 256):
        assert same(eng.list_top_questions(quiz, n), reference(pri, n)), n
    eng.close()


# ---- batches --------------------------------------------------------------------------------------------------------------------
def play(eng, n, Q, K, seed, qgaps=()):
    """n quizzes after 0..6 answers each."""
    rng = np.random.default_rng(seed)
    free = [q for q in range(Q) if q not in qgaps]
    quizzes = eng.start_quiz_batch(n)
    for j, quiz in enumerate(quizzes):
        answer(eng, quiz, [(int(q), int(rng.integers(0, K))) for q in rng.permutation(free)[:j % 7]])
    return quizzes


@pytest.mark.parametrize("float_engine", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("Q", [37, 1025, 5000])
def test_batch_equals_sorted_eval_priorities_batch(Q, float_engine, factory):
    """Every quiz's list is the reference made from EvalPrioritiesBatch of the same batch at the same batch_form (1: the quizzes' own
    vectors; 2 and 3: the quiz-minor matrix, which the tile kernel turns in LDS).  At Q = 37 max_count exceeds the candidates."""
    K, T = 5, 40
    eng = synth_engine(factory, K, Q, T, qgaps=[3, Q // 2], float_engine=float_engine)
    quizzes = play(eng, 256, Q, K, Q, [3, Q // 2])
    rng = np.random.default_rng(Q + 1)
    for form in (1, 2, 3):
        eng.set_option("batch_form", form)
        for n in (1, 3, 8, 9, 64, 65, 256):
            first = int(rng.integers(0, 257 - n))
            ids = quizzes[first:first + n]
            pri = eng.eval_priorities_batch(ids)
            for max_count in ((64,) if Q == 37 else (10,) if n > 9 else (1, 10, 256)):
                got = eng.list_top_questions_batch(ids, max_count)
                assert len(got) == n
                for i in range(n):
                    want = reference(pri[i], max_count)
                    assert same(got[i], want), (Q, form, n, i, max_count, got[i][:3], want[:3])
                    if Q == 37:
                        assert len(got[i]) == int((pri[i] > 0).sum()) < max_count
    eng.close()


def test_batch_refusals_leave_the_destination_untouched(factory):
    eng = synth_engine(factory, 5, 200, 40)
    quizzes = eng.start_quiz_batch(4)
    lib = interop.load_library()
    twin_codes = {}
    for name, ids in (("repeated", [quizzes[0], quizzes[1], quizzes[0]]), ("unknown", [quizzes[0], 999]), ("too many", list(range(257)))):
        n = len(ids)
        qs = (ctypes.c_int64 * n)(*ids)
        counts = (ctypes.c_int64 * n)(*([-7] * n))
        arr = (interop.CiRatedQuestion * (n * 5))()
        for r in arr:
            r.iQuestion, r.priority = -7, -7.0
        e = interop.PqaError.factor(lib.PqaEngine_ListTopQuestionsBatch(eng.c_engine, n, qs, 5, arr, counts))
        assert e is not None, name
        text = e.to_string(True)
        pri = np.zeros((n, 200))
        t = interop.PqaError.factor(lib.PqaEngine_EvalPrioritiesBatch(eng.c_engine, n, qs, pri.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        assert t is not None and err_class(text) == err_class(t.to_string(True)), (name, text)
        twin_codes[name] = err_class(text)
        assert all(r.iQuestion == -7 and r.priority == -7.0 for r in arr) and all(c == -7 for c in counts), name
        if name == "repeated":
            assert "quizId=%d" % quizzes[0] in text
        if name == "unknown":
            assert "999" in text
        if name == "too many":
            assert "257" in text
    assert twin_codes["too many"] == "Index is out of range"
    eng.close()


# ---- no side effects ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("server", [0, 1], ids=["launched", "server"])
def test_listing_changes_nothing(server, factory):
    """Two engines with the same seed run the same 30-step quiz loop, speculation and fuse_update on; one lists between every
    RecordAnswer and NextQuestion.  Same questions, same final posterior, the active question untouched by the listing.
    server = 1: the resident sweep serves the (argmax) selections of the 1000-target shape; the listing sends it away as
    EvalPriorities does and the next selection brings it back."""
    K, Q, T = 5, 300, 1000
    engines = []
    for _ in range(2):
        eng = synth_engine(factory, K, Q, T, seed=5)
        eng.set_option("seed", 1234)
        eng.set_option("speculate", 1)
        eng.set_option("fuse_update", 1)
        if server:
            eng.set_option("select", 1)
            eng.set_option("server", 1)
        engines.append(eng)
    plain, listing = engines
    rng = np.random.default_rng(8)
    answers = [int(a) for a in rng.integers(0, K, size=30)]
    transcripts = []
    for eng in engines:
        quiz = eng.start_quiz()
        asked = []
        for a in answers:
            if eng is listing:
                before = eng.get_active_question_id(quiz)
                got = eng.list_top_questions(quiz, 10)
                assert eng.get_active_question_id(quiz) == before
                assert len(got) == 10 and not ({q for q, _ in got} & set(asked))
            q = eng.next_question(quiz)
            asked.append(q)
            eng.record_answer(quiz, a)
        if eng is listing:
            assert same(eng.list_top_questions(quiz, 10), reference(eng.eval_priorities(quiz), 10))
        transcripts.append((asked, eng.get_priors(quiz), eng.get_total_questions_asked()))
    assert transcripts[0][0] == transcripts[1][0]
    assert np.array_equal(transcripts[0][1], transcripts[1][1])
    assert transcripts[0][2] == transcripts[1][2]
    for eng in engines:
        eng.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_are_the_twin_calls(factory):
    eng = synth_engine(factory, 5, 200, 40)
    quiz = eng.start_quiz()
    lib = interop.load_library()
    dest = (interop.CiRatedQuestion * 8)()
    tdest = (interop.CiRatedTarget * 8)()
    counts = (ctypes.c_int64 * 1)()
    one = (ctypes.c_int64 * 1)(quiz)

    def single(i_quiz, max_count, buf):
        c_err = ctypes.c_void_p()
        n = lib.PqaEngine_ListTopQuestions(eng.c_engine, ctypes.byref(c_err), i_quiz, max_count, buf)
        e = interop.PqaError.factor(c_err.value)
        assert (n == -1) == (e is not None)
        return n, (err_class(e.to_string(True)) if e else None)

    def targets(i_quiz, max_count):
        c_err = ctypes.c_void_p()
        lib.PqaEngine_ListTopTargets(eng.c_engine, ctypes.byref(c_err), i_quiz, max_count, tdest)
        e = interop.PqaError.factor(c_err.value)
        return err_class(e.to_string(True)) if e else None

    def batch(fn, buf, max_count, cnt=counts, ids=one):
        e = interop.PqaError.factor(fn(eng.c_engine, 1, ids, max_count, buf, cnt))
        return err_class(e.to_string(True)) if e else None

    lq, lt = lib.PqaEngine_ListTopQuestionsBatch, lib.PqaEngine_ListTopTargetsBatch
    # unknown quiz
    assert single(777, 5, dest)[1] == targets(777, 5) is not None
    assert batch(lq, dest, 5, ids=(ctypes.c_int64 * 1)(777)) == batch(lt, tdest, 5, ids=(ctypes.c_int64 * 1)(777)) is not None
    # maxCount < 0, missing buffers with maxCount > 0: ListTopTargetsBatch's codes
    assert single(quiz, -1, dest)[1] == batch(lq, dest, -1) == batch(lt, tdest, -1) == "The count is negative"
    assert single(quiz, 5, None)[1] == batch(lq, None, 5) == batch(lt, None, 5) == "Expected non-null argument"
    assert batch(lq, dest, 5, cnt=None) == batch(lt, tdest, 5, cnt=None) == "Expected non-null argument"
    # maxCount == 0 lists nothing and is no error, with or without a buffer
    assert single(quiz, 0, None) == (0, None) and batch(lq, None, 0) is None and counts[0] == 0
    # maintenance mode
    eng.start_maintenance(True)
    assert single(quiz, 5, dest)[1] == targets(quiz, 5) is not None
    assert batch(lq, dest, 5) == batch(lt, tdest, 5) is not None
    pri = np.zeros(200)
    e = interop.PqaError.factor(lib.PqaEngine_EvalPriorities(eng.c_engine, quiz, pri.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 200))
    assert e is not None and err_class(e.to_string(True)) == single(quiz, 5, dest)[1]
    eng.finish_maintenance()
    eng.close()


# ---- shards ---------------------------------------------------------------------------------------------------------------------
def test_one_process_sharded_engine_equals_the_whole(factory, monkeypatch):
    """PQA_DEVICES=0,0,0: three shards on the one device; single and batch listings equal the whole engine's, record for record."""
    K, Q, T = 5, 5000, 40
    whole = synth_engine(factory, K, Q, T, qgaps=[7, 1700, 4999])
    monkeypatch.setenv("PQA_DEVICES", "0,0,0")
    sharded = synth_engine(factory, K, Q, T, qgaps=[7, 1700, 4999])
    monkeypatch.delenv("PQA_DEVICES")
    assert sharded.get_option("shards") == 3
    qw, qs = play(whole, 9, Q, K, 4, [7, 1700, 4999]), play(sharded, 9, Q, K, 4, [7, 1700, 4999])
    assert qw == qs
    for quiz in (qw[0], qw[6]):
        for n in (1, 10, 256, 300):
            assert same(sharded.list_top_questions(quiz, n), whole.list_top_questions(quiz, n)), (quiz, n)
    assert sharded.get_option("shards_in_flight_max") == 3
    for n in (10, 256):
        a, b = sharded.list_top_questions_batch(qs, n), whole.list_top_questions_batch(qw, n)
        assert all(same(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 9, n
    assert sharded.get_option("shards_in_flight_max") == 3
    whole.close()
    sharded.close()


@pytest.mark.parametrize("world", [2, 3])
def test_shard_engines_list_their_own_global_ids(world, factory):
    """Engines from PqaEngineFactory_CreateHipEngineSharded in one process: each lists only its own GLOBAL ids, and
    dist.merge_top_questions over the shards' lists is the whole engine's listing."""
    K, Q, T = 5, 3001, 40
    whole = synth_engine(factory, K, Q, T)
    quiz = whole.start_quiz()
    shards = []
    for r in range(world):
        first, limit = pdist.shard_range(Q, world, r)
        eng = factory.create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1), first, Q, 0)
        eng.fill_synthetic(8.0, 0.5, 7)
        eng.set_option("workers", cases.WORKERS)
        assert eng.start_quiz() == quiz
        shards.append((eng, first, limit))
    for n in (1, 10, 256):
        lists = []
        for eng, first, limit in shards:
            got = eng.list_top_questions(quiz, n)
            assert same(got, reference(eng.eval_priorities(quiz, limit - first), n, first))
            assert all(first <= q < limit for q, _ in got) and len(got) == min(n, limit - first)
            lists.append(got)
        assert same(pdist.merge_top_questions(lists, n), whole.list_top_questions(quiz, n)), n
        per = [eng.list_top_questions_batch([quiz], n)[0] for eng, _, _ in shards]
        assert same(pdist.merge_top_questions(per, n), whole.list_top_questions_batch([quiz], n)[0]), n
    for eng, _, _ in shards:
        eng.close()
    whole.close()
