"""The Among calls on the GPU (include/PqaHipExt.h; among_kernels.hip: eval_listed_kernel; hip_engine_among.cpp): evaluate and select
over a listed set of questions per quiz -- for the call, every question outside the list counts as asked.

Bars, the project's own: priorities rel < 1e-9 against the oracle (cases / test_gpu_batch: PRIORITY_RTOL, oracle_priorities, rel_vec);
argmax picks equal the oracle's wherever its top-2 margin among the listed, eligible questions exceeds 1e-8 (the convention of
tests/test_gpu_late.py: batched_states); sampled draws are the plain-Python selector's (sampled_batch_common.select_py) over the call's
own priorities scattered into a zero vector with skip = gaps | asked | not listed -- the seeded draws guarded by
boundary_distance > GUARD, the edge numbers unguarded.

Float engines: the listed questions are evaluated in fp64 on the engine's fp32 rows, so the oracle is fed the engine's own cube
(PqaHip_GetKB) and the engine's own posterior (PqaHip_GetPriors) and the bar stays 1e-9.  There is no pole fix on a Float engine: a
Float state that misses the bar is dropped from the Float leg only if the same state misses it on a Double engine with pole_fix = 0
(float_state_is_at_the_pole) -- it is at the pole of the lack term then.  None of the states below needed that."""
import ctypes

import numpy as np
import pytest

import cases
import sampled_batch_common as sb
import test_gpu_batch as tb
from probqa_amd import dist as pdist
from probqa_amd import interop
from test_gpu_late import late_case

pytestmark = pytest.mark.gpu

RTOL = tb.PRIORITY_RTOL
F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)
WORST = {"rel": 0.0}     # the worst relative error of legs 1-3, printed by the last of them


def make_engine(case, factory, f32=False, pole_fix=None):
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(case.K, case.Q, case.T, init_amount=case.init, **(F32 if f32 else {})))
    assert err is None and eng is not None, err
    eng.set_kb(*case.kb())
    eng.set_option("workers", cases.WORKERS)
    if pole_fix is not None:
        eng.set_option("pole_fix", pole_fix)
    if case.tgaps:
        eng.set_target_gaps(case.tgaps)
    if case.qgaps:
        eng.set_question_gaps(case.qgaps)
    return eng


def make_oracle(case, eng, f32):
    orc = case.make_oracle()
    if f32:
        orc.set_kb(*eng.get_kb())    # the cube the engine holds: rounded to fp32
    return orc


def play(eng, hist):
    quiz = eng.start_quiz()
    for q, a in hist:
        eng.set_active_question(quiz, q)
        eng.record_answer(quiz, a)
    return quiz


def oracle_state(orc, hist, eng=None, quiz=None):
    """The oracle's priorities of the state after `hist`; with eng / quiz given (Float engines): over the engine's own posterior."""
    orc.start_quiz(cases.WORKERS)
    for q, a in hist:
        orc.record_answer(q, a, cases.WORKERS - 1)
    if eng is not None:
        orc.mants[: orc.T] = eng.get_priors(quiz)
    _, pri = orc.eval(1)
    return pri


def three_answers(case, seed):
    """The case's script, extended to three answers by seeded questions that are neither gaps nor answered."""
    rng = np.random.default_rng(seed)
    hist = list(case.answers[:3])
    free = [q for q in range(case.Q) if q not in case.qgaps and q not in [h[0] for h in hist]]
    for q in rng.permutation(free)[: 3 - len(hist)]:
        hist.append((int(q), int(rng.integers(case.K))))
    return hist


def check_priorities(name, got, opri, ids):
    """got parallel to ids against the oracle's vector: zeros exactly where the oracle has them, 1e-9 elsewhere."""
    got, want = np.asarray(got), opri[list(ids)] if len(ids) else np.zeros(0)
    rel = tb.rel_vec(got, want) if len(ids) else np.zeros(0)
    worst = float(rel.max()) if len(ids) else 0.0
    WORST["rel"] = max(WORST["rel"], worst)
    assert worst < RTOL, (name, worst, int(rel.argmax()))
    return worst


def check_pick(name, pick, opri, ids):
    """The argmax among the list by the margin rule: -1 where no listed question is eligible; always a listed, eligible question."""
    elig = sorted(q for q in ids if opri[q] != 0)
    if not elig:
        assert pick == -1, (name, pick)
        return
    assert pick in elig, (name, pick)
    top = np.sort(opri[elig])[::-1]
    margin = (top[0] - top[1]) / top[0] if len(top) > 1 and top[0] > 0 else 1.0
    if margin > 1e-8:
        want = min(q for q in elig if opri[q] == top[0])
        assert pick == want, (name, pick, want, margin)


def float_state_is_at_the_pole(case, factory, hist, ids):
    """The same state on a Double engine without the pole fix: does it miss the bar too?"""
    eng = make_engine(case, factory, pole_fix=0)
    quiz = play(eng, hist)
    got = eng.eval_priorities_among(quiz, ids)
    opri = oracle_state(case.make_oracle(), hist)
    eng.close()
    return float(tb.rel_vec(got, opri[list(ids)]).max()) >= RTOL


# ---- 1. fixtures: every small case, fresh and three answers deep, Double and Float, every kind of list in ONE call ------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("case", cases.small_cases(), ids=lambda c: c.name)
def test_lists_against_the_oracle(case, f32, factory):
    eng = make_engine(case, factory, f32)
    orc = make_oracle(case, eng, f32)
    Q = case.Q
    quizzes, lists, states = [], [], []
    for hist in ([], three_answers(case, 7)):
        dead = sorted(set(case.qgaps) | {q for q, _ in hist})
        kinds = [list(range(Q)), list(range(0, Q, 3)), [Q - 1 if Q - 1 not in dead else Q - 2], dead, [], list(range(Q - 1, -1, -2))]
        for ids in kinds:
            quizzes.append(play(eng, hist))
            lists.append(ids)
            states.append(hist)
    opris = [oracle_state(orc, h, eng if f32 else None, q) for h, q in zip(states, quizzes)]
    before = eng.get_option("priority_host_bytes"), eng.get_option("among_calls"), eng.get_option("among_pairs")
    got = eng.eval_priorities_among_batch(quizzes, lists)
    n_pairs = sum(len(x) for x in lists)
    assert eng.get_option("priority_host_bytes") - before[0] == 8 * n_pairs            # nothing of size Q crosses
    assert (eng.get_option("among_calls") - before[1], eng.get_option("among_pairs") - before[2]) == (1, n_pairs)
    for j, (ids, opri) in enumerate(zip(lists, opris)):
        name = (case.name, "float" if f32 else "double", j)
        if f32 and len(ids) and float(tb.rel_vec(got[j], opri[ids]).max()) >= RTOL and float_state_is_at_the_pole(case, factory, states[j], ids):
            continue    # (at the pole of the lack term: no Float path has the fix)
        check_priorities(name, got[j], opri, ids)
    # the picks, the active questions afterwards, the counter: one question asked per quiz that got one
    asked0, active0 = eng.get_total_questions_asked(), [eng.get_active_question_id(q) for q in quizzes]
    bytes0 = eng.get_option("priority_host_bytes")
    sel = eng.select_argmax_among_batch(quizzes, lists)
    assert [eng.get_active_question_id(q) for q in quizzes] == active0 and eng.get_total_questions_asked() == asked0   # (no bookkeeping)
    picks = eng.next_question_argmax_among_batch(quizzes, lists)
    assert eng.get_option("priority_host_bytes") == bytes0
    for j, (ids, opri) in enumerate(zip(lists, opris)):
        check_pick((case.name, f32, j), picks[j], opri, ids)
        assert int(sel[j, 1]) == picks[j]
        if picks[j] >= 0:
            assert sel[j, 0] == got[j][ids.index(picks[j])]
        assert eng.get_active_question_id(quizzes[j]) == (picks[j] if picks[j] >= 0 else active0[j])
    assert eng.get_total_questions_asked() - asked0 == sum(p >= 0 for p in picks)
    # a single quiz is a batch of one
    assert eng.next_question_argmax_among(quizzes[1], lists[1]) == picks[1]
    assert np.array_equal(eng.eval_priorities_among(quizzes[1], lists[1]), got[1])
    assert eng.eval_priorities_among_batch([], []) == [] and eng.next_question_argmax_among_batch([], []) == []
    eng.close()


# ---- 2. the row-length edges of the kernel: the strided loops and their tails, the padding columns, rows beyond 16384 targets ----------------
@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("T", [2, 30, 511, 513, 1025, 16400])
def test_row_length_edges(T, f32, factory):
    Q = 6
    for K in (2, 5, 7):
        case = cases.Case("edge_%dx%dx%d" % (Q, K, T), K, Q, T, seed=40 + K)
        eng = make_engine(case, factory, f32)
        orc = make_oracle(case, eng, f32)
        hists = [[], [(1, K - 1), (4, 0)]]
        quizzes, lists, states = [], [], []
        for hist in hists:
            for ids in (list(range(Q)), [5, 0, 2]):
                quizzes.append(play(eng, hist))
                lists.append(ids)
                states.append(hist)
        got = eng.eval_priorities_among_batch(quizzes, lists)
        picks = eng.next_question_argmax_among_batch(quizzes, lists)
        for j, ids in enumerate(lists):
            opri = oracle_state(orc, states[j], eng if f32 else None, quizzes[j])
            check_priorities((case.name, f32, j), got[j], opri, ids)
            check_pick((case.name, f32, j), picks[j], opri, ids)
        eng.close()


# ---- 3. late states: the listed sweep's pole watch and the fix behind it ---------------------------------------------------------------------
LATE = [0, 3, 4, 6, 9]    # the register, streaming, cluster, short and grid.y legs' shapes (their engine options are not applied)


def late_states(i, factory, pole_fix):
    """One quiz per prefix of the answer script in ONE batched call: list = all unanswered questions, then a seeded half of them.
    Returns (case, worst relative error, [(pick, oracle vector, list)])."""
    _, case, _ = late_case(i)
    eng, orc = make_engine(case, factory, pole_fix=pole_fix), case.make_oracle()
    rng = np.random.default_rng(900 + i)
    quizzes, hists = [], []
    for j in range(len(case.answers) + 1):
        hists.append(case.answers[:j])
        quizzes.append(play(eng, hists[-1]))
    opris = [oracle_state(orc, h) for h in hists]
    worst, picked = 0.0, []
    for half in (False, True):
        lists = []
        for h in hists:
            free = [q for q in range(case.Q) if q not in [x[0] for x in h]]
            lists.append(sorted(int(q) for q in rng.permutation(free)[: (len(free) + 1) // 2]) if half else free)
        got = eng.eval_priorities_among_batch(quizzes, lists)
        picks = eng.next_question_argmax_among_batch(quizzes, lists)
        for j, ids in enumerate(lists):
            worst = max(worst, float(tb.rel_vec(got[j], opris[j][ids]).max()))
            picked.append((picks[j], opris[j], ids))
    eng.close()
    return case, worst, picked


@pytest.mark.parametrize("i", LATE)
def test_late_states(i, factory):
    case, worst, picked = late_states(i, factory, None)
    WORST["rel"] = max(WORST["rel"], worst)
    print("%s: worst relative error %.3g (legs 1-3 so far: %.3g)" % (case.name, worst, WORST["rel"]))
    assert worst < RTOL, (case.name, worst)
    for pick, opri, ids in picked:
        check_pick(case.name, pick, opri, ids)


def test_late_states_need_the_fix(factory):
    """The guard of the late cases: without the fix (pole_fix = 0) at least one of them misses the bar -- else they would say nothing
    about the watch and the fix behind the listed sweep."""
    worst = {}
    for i in LATE:
        case, w, _ = late_states(i, factory, 0)
        worst[case.name] = w
    print("pole_fix = 0:", {k: "%.3g" % v for k, v in worst.items()})
    assert max(worst.values()) >= RTOL, worst


# ---- 4. sampled ---------------------------------------------------------------------------------------------------------------------------------
def run_lengths(pri, skip, n_workers):
    """select_py's per-subtask run lengths (what boundary_distance takes)."""
    quot, rem, ns = sb.split(len(pri), n_workers)
    run = [0.0] * len(pri)
    for s in range(ns):
        first, limit = (0 if s == 0 else sb.bound(s - 1, quot, rem)), sb.bound(s, quot, rem)
        st = (0.0, 0.0)
        for i in range(first, limit):
            if not skip[i]:
                st = sb.kahan_add(st, float(pri[i]))
            run[i] = st[0] - st[1]
    return run


def among_vectors(eng, case, quizzes, hists, lists):
    """Per quiz: the call's own priorities scattered into a zero vector, and skip = gaps | asked | not listed."""
    got = eng.eval_priorities_among_batch(quizzes, lists)
    out = []
    for j, ids in enumerate(lists):
        pri = np.zeros(case.Q)
        pri[ids] = got[j]
        skip = [True] * case.Q
        for q in ids:
            skip[q] = q in case.qgaps or q in [x[0] for x in hists[j]]
        out.append((pri, skip))
    return out


@pytest.mark.parametrize("case", sb.scenarios(), ids=lambda c: c.name)
def test_sampled_among_equals_the_python_selector(case, factory):
    """Quiz i = the case after i answers, each with a seeded list that leaves the last question out -- so the edge number 2^64 - 1,
    whose pick is the last question, makes the reference's fallback run: its result lies in the list."""
    eng = make_engine(case, factory)
    rng = np.random.default_rng(case.seed)
    hists = [case.answers[:i] for i in range(len(case.answers) + 1)]
    quizzes = [play(eng, h) for h in hists]
    lists = [sorted(int(q) for q in rng.permutation(case.Q - 1)[: max(2, (2 * case.Q) // 3)]) for _ in hists]
    vectors = among_vectors(eng, case, quizzes, hists, lists)
    asked0, fell_back = eng.get_total_questions_asked(), 0
    bytes0 = eng.get_option("priority_host_bytes")
    for rnds, guarded in sb.batches(case):
        got = eng.next_question_sampled_among_batch(quizzes, rnds, lists)
        for j, (pri, skip) in enumerate(vectors):
            if guarded:
                d = sb.boundary_distance(run_lengths(pri, skip, sb.SUBTASKS), sb.SUBTASKS, rnds[j])
                assert d > sb.GUARD, f"{case.name}: draw {rnds[j]:#x} of quiz {j} lies {d:g} from a run-length boundary: choose another seed"
            pick = sb.select_py(pri, skip, sb.SUBTASKS, rnds[j])
            if skip[pick]:       # the fallback: the nearest free question under the same bits -- never outside the list
                fell_back += 1
                assert got[j] in lists[j] and not skip[got[j]], (case.name, j, rnds[j], got[j])
            else:
                assert got[j] == pick, (case.name, j, hex(rnds[j]), got[j], pick)
            assert eng.get_active_question_id(quizzes[j]) == got[j]
    assert fell_back >= len(quizzes)      # (the edge number 2^64 - 1 of every quiz)
    assert eng.get_total_questions_asked() - asked0 == len(quizzes) * len(sb.batches(case))
    assert eng.get_option("priority_host_bytes") == bytes0
    # a list of gaps and asked questions only, and an empty one: no pick, no change
    dead = sorted(set(case.qgaps) | {q for q, _ in hists[-1]})
    active = eng.get_active_question_id(quizzes[-1]), eng.get_active_question_id(quizzes[0])
    assert eng.next_question_sampled_among_batch([quizzes[-1], quizzes[0]], [5, 6], [dead, []]) == [-1, -1]
    assert (eng.get_active_question_id(quizzes[-1]), eng.get_active_question_id(quizzes[0])) == active
    eng.close()


class SelectorRng:
    """The engine's generator restated (engine_options.h: xorshift128+ seeded by SplitMix64); held to the engine itself below."""
    M = (1 << 64) - 1

    def __init__(self, seed):
        self.s, x = [], seed & self.M
        for _ in range(2):
            x = (x + 0x9E3779B97F4A7C15) & self.M
            z = x
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & self.M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & self.M
            self.s.append(z ^ (z >> 31))

    def next(self):
        s1, s0 = self.s
        self.s[0] = s0
        s1 ^= (s1 << 23) & self.M
        self.s[1] = s1 ^ s0 ^ (s1 >> 18) ^ (s0 >> 5)
        return (self.s[1] + s0) & self.M


def test_next_question_among_batch_obeys_select(factory):
    case = sb.scenarios()[4]
    a, b, c = (make_engine(case, factory) for _ in range(3))
    n, Q = 12, case.Q
    rng = np.random.default_rng(3)
    qa, qb, qc = (e.start_quiz_batch(n) for e in (a, b, c))
    lists = [sorted(int(q) for q in rng.permutation(Q)[: Q // 2]) for _ in range(n)]
    # select = 1: the argmax form
    for e in (a, b, c):
        e.set_option("select", 1)
    assert a.next_question_among_batch(qa, lists) == b.next_question_argmax_among_batch(qb, lists)
    # select = 0 and a seed.  Full lists: nothing is "not listed", so the batch equals consecutive NextQuestion calls on a twin with the
    # same seed -- one number per quiz in batch order -- and the restated generator gives the sampled form the same numbers.
    for e in (a, b, c):
        e.set_option("select", 0)
        e.set_option("seed", 4242)
    gen = SelectorRng(4242)
    full = [list(range(Q))] * n
    got = a.next_question_among_batch(qa, full)
    assert got == [b.next_question(q) for q in qb]
    assert got == c.next_question_sampled_among_batch(qc, [gen.next() for _ in range(n)], full)
    # ... and partial lists: the sampled form for the numbers the generator draws next
    got = a.next_question_among_batch(qa, lists)
    assert got == c.next_question_sampled_among_batch(qc, [gen.next() for _ in range(n)], lists)
    assert all(g in ids for g, ids in zip(got, lists))
    for e in (a, b, c):
        e.close()


# ---- 5. refusals change nothing -----------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(factory):
    case = sb.scenarios()[4]
    a, b = (make_engine(case, factory) for _ in range(2))
    for e in (a, b):
        e.set_option("select", 0)
        e.set_option("seed", 17)
    Q = case.Q
    qa, qb = a.start_quiz_batch(300), b.start_quiz_batch(300)
    ok = [list(range(0, Q, 2))] * 4
    assert a.next_question_among_batch(qa[:4], ok) == b.next_question_among_batch(qb[:4], ok)

    def state():
        return ([a.get_active_question_id(q) for q in qa[:6]], a.get_total_questions_asked(), a.get_option("among_calls"),
                a.get_option("among_pairs"), a.get_option("priority_host_bytes"))

    before = state()
    unknown = max(qa) + 1000
    calls = {
        "eval": lambda qs, ls: a.eval_priorities_among_batch(qs, ls),
        "select": lambda qs, ls: a.select_argmax_among_batch(qs, ls),
        "argmax": lambda qs, ls: a.next_question_argmax_among_batch(qs, ls),
        "sampled": lambda qs, ls: a.next_question_sampled_among_batch(qs, [5] * len(qs), ls),
        "plain": lambda qs, ls: a.next_question_among_batch(qs, ls),
    }
    for name, go in calls.items():
        with pytest.raises(interop.PqaException, match=r"entry=2 position=1 questionId=-1\b"):
            go(qa[:4], [[1, 2], [3], [4, -1], [5]])
        with pytest.raises(interop.PqaException, match=r"entry=1 position=0 questionId=%d\b" % Q):
            go(qa[:4], [[1, 2], [Q], [4], [5]])
        with pytest.raises(interop.PqaException, match=r"entry=3 position=2 questionId=7\b.*twice|twice.*entry=3 position=2 questionId=7\b"):
            go(qa[:4], [[7], [7], [7], [7, 8, 7]])
        with pytest.raises(interop.PqaException, match=r"quizId=%d\b.*twice|twice.*quizId=%d\b" % (qa[1], qa[1])):
            go(qa[:3] + [qa[1]], [[1]] * 4)
        with pytest.raises(interop.PqaException, match=str(unknown)):
            go(qa[:3] + [unknown], [[1]] * 4)
        with pytest.raises(interop.PqaException, match="257"):
            go(qa[:257], [[1]] * 257)
    # null buffers, through the library itself
    lib = interop.load_library()
    ids = (ctypes.c_int64 * 2)(*qa[:2])
    counts = (ctypes.c_int64 * 2)(1, 1)
    qs = (ctypes.c_int64 * 2)(3, 4)
    rn = (ctypes.c_uint64 * 2)(1, 2)
    out = (ctypes.c_int64 * 2)()
    outd = (ctypes.c_double * 2)()
    outs = (interop.CiHipSelection * 2)()
    n64, nu, nd, ns = ctypes.POINTER(ctypes.c_int64)(), ctypes.POINTER(ctypes.c_uint64)(), ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(interop.CiHipSelection)()

    def refused(fn, *args):
        e = fn(a.c_engine, 2, *args)
        assert e, "the call must be refused"
        return interop.PqaError(e).to_string(True)

    for fn, good, null in ((lib.PqaEngine_EvalPrioritiesAmongBatch, outd, nd), (lib.PqaHip_SelectArgmaxAmongBatch, outs, ns),
                           (lib.PqaEngine_NextQuestionArgmaxAmongBatch, out, n64), (lib.PqaEngine_NextQuestionAmongBatch, out, n64)):
        for args in ((n64, counts, qs, good), (ids, n64, qs, good), (ids, counts, n64, good), (ids, counts, qs, null)):
            assert "Nullptr" in refused(fn, *args)
    for args in ((n64, counts, qs, rn, out), (ids, n64, qs, rn, out), (ids, counts, n64, rn, out), (ids, counts, qs, nu, out), (ids, counts, qs, rn, n64)):
        assert "Nullptr" in refused(lib.PqaEngine_NextQuestionSampledAmongBatch, *args)
    assert state() == before
    # maintenance mode (entering it releases the quizzes: an engine of its own)
    m = make_engine(case, factory)
    qm = m.start_quiz_batch(2)
    m.start_maintenance(True)
    for go in (lambda: m.eval_priorities_among_batch(qm, [[1], [2]]), lambda: m.select_argmax_among_batch(qm, [[1], [2]]),
               lambda: m.next_question_argmax_among_batch(qm, [[1], [2]]), lambda: m.next_question_sampled_among_batch(qm, [1, 2], [[1], [2]]),
               lambda: m.next_question_among_batch(qm, [[1], [2]])):
        with pytest.raises(interop.PqaException, match="current mode is not regular"):
            go()
    assert m.get_option("among_calls") == 0 and m.get_total_questions_asked() == 0
    m.finish_maintenance()
    m.close()
    # the next valid call succeeds, and the generator has drawn nothing for the refused ones: the twin made none
    assert a.next_question_among_batch(qa[4:9], [list(range(1, Q, 3))] * 5) == b.next_question_among_batch(qb[4:9], [list(range(1, Q, 3))] * 5)
    assert [a.next_question(q) for q in qa[9:12]] == [b.next_question(q) for q in qb[9:12]]
    assert a.get_option("among_calls") == before[2] + 1
    a.close()
    b.close()


# ---- 6. no interference with a quiz's own selections ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speculate", [0, 1])
def test_among_calls_leave_the_quiz_loop_alone(speculate, factory):
    """One engine makes Among calls between the steps of a quiz loop -- also directly behind record_answer, when a speculative sweep
    may be in flight --, its twin makes none: eval_priorities, next_question_argmax and list_top_targets agree bit for bit."""
    case = sb.synthetic_case()
    a, b = (make_engine(case, factory) for _ in range(2))
    for e in (a, b):
        e.set_option("speculate", speculate)
    qa, qb = a.start_quiz(), b.start_quiz()
    other = a.start_quiz_batch(3)
    b.start_quiz_batch(3)
    rng = np.random.default_rng(11)
    for step in range(6):
        ids = sorted(int(q) for q in rng.permutation(case.Q)[:40])
        a.eval_priorities_among(qa, ids)
        pa, pb = a.next_question_argmax(qa), b.next_question_argmax(qb)
        assert pa == pb, step
        a.select_argmax_among_batch([qa] + other, [ids] * 4)
        ans = int(rng.integers(case.K))
        a.record_answer(qa, ans)
        b.record_answer(qb, ans)
        a.next_question_sampled_among_batch(other + [qa], [1, 2, 3, 4], [ids[:7]] * 4)    # (directly behind record_answer)
        if step % 2:
            assert np.array_equal(a.eval_priorities(qa), b.eval_priorities(qb)), step
        ta, tb_ = a.list_top_targets(qa, 5), b.list_top_targets(qb, 5)
        assert [(t.i_target, t.prob) for t in ta] == [(t.i_target, t.prob) for t in tb_], step
    assert a.next_question_argmax(qa) == b.next_question_argmax(qb)
    a.close()
    b.close()


# ---- 8. shards: engines made for a part of the question axis, side by side on one device --------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_shards_merge_to_the_whole_engines_pick(world, factory):
    case = sb.scenarios()[4]
    K, Q, T = case.K, case.Q, case.T
    A, D, B = case.kb()
    bounds = pdist.shard_bounds(Q, world)
    firsts = [0] + bounds[:-1]
    whole = make_engine(case, factory)
    shards = []
    for first, limit in zip(firsts, bounds):
        sh = factory.create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=case.init), first, Q, 0)
        sh.set_kb(A[first:limit], D[first:limit], B)
        sh.set_option("workers", cases.WORKERS)
        shards.append(sh)
    n = 4
    qw = whole.start_quiz_batch(n)
    qs = [sh.start_quiz_batch(n) for sh in shards]
    rng = np.random.default_rng(world)
    lists = [list(range(firsts[1] + 3, bounds[1], 2)),                   # on one shard only
             list(range(2, firsts[1], 5)),                                # ... on the first
             sorted(int(q) for q in rng.permutation(Q)[: Q // 3]),        # straddling the shards
             list(range(bounds[0] - 4, bounds[0] + 4))]                  # ... around a bound
    want = whole.select_argmax_among_batch(qw, lists)
    pairs0 = [sh.get_option("among_pairs") for sh in shards]
    local = np.stack([sh.select_argmax_among_batch(q, lists) for sh, q in zip(shards, qs)])
    picks = pdist.pick_batch(local)
    assert picks == [int(x) for x in want[:, 1]]
    assert picks == whole.next_question_argmax_among_batch(qw, lists)
    for r, sh in enumerate(shards):     # the pairs this engine holds
        held = sum(firsts[r] <= q < bounds[r] for ids in lists for q in ids)
        assert sh.get_option("among_pairs") - pairs0[r] == held
    # another shard's ids: priority 0 here; this shard's: the whole engine's value
    wpri = whole.eval_priorities_among(qw[2], lists[2])
    for r, sh in enumerate(shards):
        got = sh.eval_priorities_among(qs[r][2], lists[2])
        mine = np.array([firsts[r] <= q < bounds[r] for q in lists[2]])
        assert (got[~mine] == 0).all() and np.array_equal(got[mine], wpri[mine]), r
    # an id beyond the whole knowledge base is refused on a shard as on the whole engine
    with pytest.raises(interop.PqaException, match=r"entry=0 position=0 questionId=%d\b" % Q):
        shards[0].select_argmax_among_batch(qs[0][:1], [[Q]])
    for e in [whole] + shards:
        e.close()


def test_one_process_sharded_engine_answers_not_implemented(factory):
    from test_gpu_sampled_batch import devices

    case = sb.scenarios()[1]
    with devices("0,0"):
        sh = case.make_engine(factory)
    assert sh.get_option("shards") == 2
    quiz = sh.start_quiz()
    for go in (lambda: sh.eval_priorities_among(quiz, [1, 2]), lambda: sh.select_argmax_among_batch([quiz], [[1, 2]]),
               lambda: sh.next_question_argmax_among(quiz, [1, 2]), lambda: sh.next_question_sampled_among(quiz, 5, [1, 2]),
               lambda: sh.next_question_among_batch([quiz], [[1, 2]])):
        with pytest.raises(interop.PqaException, match="Among calls are for whole engines"):
            go()
    sh.close()
