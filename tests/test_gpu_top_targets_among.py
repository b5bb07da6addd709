"""PqaEngine_ListTopTargetsAmongBatch on the GPU (include/PqaHipExt.h; kb_kernels.hip: top_among_chunks_kernel;
hip_engine_top_among.cpp): a quiz's best targets within a listed set, and the posterior's total over the set.

The expected values need no oracle: the posterior is read back with get_priors (held to the oracle elsewhere).  The expected listing is
numpy's -- the list's entries with p > 0 and no gap, sorted by (-p, id), cut at max_count -- and records must be EQUAL, id and
probability bits.  The expected mass is math.fsum of the same entries; the device's value must be within n * 2^-52 relative of it, n the
list's length: any summation order of n non-negative doubles stays within (n - 1) * 2^-53 relative of the exact sum to first order, and
fsum is the exact sum rounded once -- the bound is derived, not tuned."""
import ctypes
import math

import numpy as np
import pytest

import cases
from probqa_amd import dist as pdist
from probqa_amd import interop, synth

pytestmark = pytest.mark.gpu

F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)
TGAPS = [3, 700, 4096, 5002]
LENGTHS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5003]
MAX_COUNTS = [1, 10, 256, 257, 6000]


def synth_engine(factory, K, Q, T, seed=7, tgaps=(), **kw):
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **kw))
    assert err is None and eng is not None, err
    eng.fill_synthetic(8.0, 0.5, seed)
    eng.set_option("workers", cases.WORKERS)
    if tgaps:
        eng.set_target_gaps(list(tgaps))
    return eng


def play(eng, hist):
    quiz = eng.start_quiz()
    for q, a in hist:
        eng.set_active_question(quiz, q)
        eng.record_answer(quiz, a)
    return quiz


def history(Q, K, n, seed):
    rng = np.random.default_rng(seed)
    return [(int(q), int(rng.integers(K))) for q in rng.permutation(Q)[:n]]


def expected(pri, tgaps, ids, max_count):
    """([(id, p)], mass) by the header's points (a), (b), (c), (e)."""
    ids = np.asarray(ids, dtype=np.int64)
    if len(ids) == 0:
        return [], 0.0
    p = pri[ids]
    ok = (p > 0) & ~np.isin(ids, list(tgaps))
    c, pc = ids[ok], p[ok]
    take = np.lexsort((c, -pc))[:max_count]
    return [(int(t), float(x)) for t, x in zip(c[take], pc[take])], math.fsum(pc)


def records(listing):
    return [(t.i_target, t.prob) for t in listing]


def check(name, got, mass, pri, tgaps, ids, max_count):
    want, wmass = expected(pri, tgaps, ids, max_count)
    assert records(got) == want, (name, records(got)[:5], want[:5])
    print("%s: mass %.17g expected %.17g" % (name, mass, wmass))
    assert abs(mass - wmass) <= len(ids) * 2.0 ** -52 * wmass, (name, mass, wmass)


def seeded_lists(T, lengths, seed, forced=()):
    """Per length a shuffled list; the ids in `forced` are put in front of the lists long enough to hold them and more."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        ids = [int(t) for t in rng.permutation(T)[:n]]
        if n > 2 * len(forced):
            rest = [t for t in ids if t not in forced]
            ids = list(forced) + rest[: n - len(forced)]
            ids = [ids[i] for i in rng.permutation(n)]
        assert len(ids) == n == len(set(ids))
        out.append(ids)
    return out


# ---- 1. order among ties: a fresh engine, a uniform posterior ------------------------------------------------------------------------------
def test_order_among_ties(factory):
    K, Q, T = 3, 8, 301
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=1.0))
    assert err is None
    quiz = eng.start_quiz()
    pri = eng.get_priors(quiz)
    assert len(set(pri)) == 1
    ids = [int(t) for t in np.random.default_rng(1).permutation(T)[:150]]
    for max_count in (10, 150):
        for order in (ids, ids[::-1], sorted(ids)):
            got, mass = eng.list_top_targets_among(quiz, order, max_count)
            assert [t.i_target for t in got] == sorted(ids)[:max_count], (max_count, [t.i_target for t in got][:12])
            assert all(t.prob == pri[0] for t in got)
            assert abs(mass - 150 / T) <= 150 * 2.0 ** -52 * (150 / T), mass
            check(("ties", max_count), got, mass, pri, [], order, max_count)
    eng.close()


def test_order_among_ties_across_waves(factory):
    """The same over 4500 shuffled ids of 5003: the equal probabilities lie in five waves' lists of two workgroups, and in the merge a
    lane holds candidates of several lists whose ids do not ascend -- what the rounds' unordered form (pqa_device.h: lane_best) is for."""
    K, Q, T = 3, 8, 5003
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=1.0))
    assert err is None
    quiz = eng.start_quiz()
    pri = eng.get_priors(quiz)
    assert len(set(pri)) == 1
    ids = [int(t) for t in np.random.default_rng(2).permutation(T)[:4500]]
    for max_count in (10, 200, 256, 300):
        got, mass = eng.list_top_targets_among(quiz, ids, max_count)
        assert [t.i_target for t in got] == sorted(ids)[:max_count], (max_count, [t.i_target for t in got][:12])
        check(("ties across waves", max_count), got, mass, pri, [], ids, max_count)
    eng.close()


# ---- 2. a trained engine, a late-ish state: list lengths across a lane, a wave's 1024 and a workgroup's 4096; both paths --------------------------
@pytest.fixture(scope="module")
def trained(factory):
    K, Q, T = 4, 12, 5003
    eng = synth_engine(factory, K, Q, T, tgaps=TGAPS)
    quiz = play(eng, history(Q, K, 6, 5))
    pri = eng.get_priors(quiz)
    pri.setflags(write=False)
    yield eng, quiz, pri
    eng.close()


@pytest.mark.parametrize("max_count", MAX_COUNTS)
def test_trained_engine_list_lengths(trained, max_count):
    eng, quiz, pri = trained
    T = len(pri)
    lists = seeded_lists(T, LENGTHS, 11, TGAPS)
    assert all(set(TGAPS) <= set(x) for x in lists if len(x) > 8)          # the gaps are listed too
    both = lists + [sorted(x) for x in lists]
    got, mass = eng.list_top_targets_among_batch([quiz] * len(both), both, max_count)       # (one quiz under 24 lists)
    for j, ids in enumerate(both):
        check((max_count, len(ids), j), got[j], mass[j], pri, TGAPS, ids, max_count)
        assert all(t.i_target not in TGAPS for t in got[j])
    for j in range(len(lists)):       # shuffled and sorted: the same listing
        assert records(got[j]) == records(got[j + len(lists)]), (max_count, len(lists[j]))
    # one list alone, as the single-quiz method gives it
    j = LENGTHS.index(1025)
    one, m1 = eng.list_top_targets_among(quiz, lists[j], max_count)
    assert records(one) == records(got[j]) and m1 == mass[j]


# ---- 3. sharing and repetition ---------------------------------------------------------------------------------------------------------------------
def test_sharing_and_repetition(factory):
    K, Q, T = 4, 12, 5003
    eng = synth_engine(factory, K, Q, T, tgaps=TGAPS)
    quizzes = [play(eng, history(Q, K, j % 5, 30 + j)) for j in range(9)]
    pris = [eng.get_priors(q) for q in quizzes]
    lists = seeded_lists(T, [40, 1500, 4500, 77], 3, TGAPS)       # (list 3: no quiz uses it)
    batch = quizzes + [quizzes[2]]
    list_of = [0, 1, 2, 0, 1, 2, 0, 1, 2, 0]                       # quiz 2: under list 2 and under list 0
    for max_count in (10, 300):      # (300: quizzes under lists 1 and 2 take the host selection, under list 0 the device's -- in one call)
        got, mass = eng.list_top_targets_among_batch(batch, lists, max_count, list_of)
        again, mass2 = eng.list_top_targets_among_batch(batch, lists, max_count, list_of)
        assert [records(x) for x in got] == [records(x) for x in again] and mass == mass2           # the same call: the same bits
        for i, (q, l) in enumerate(zip(batch, list_of)):
            check((max_count, i), got[i], mass[i], pris[quizzes.index(q)], TGAPS, lists[l], max_count)
            alone, m1 = eng.list_top_targets_among(q, lists[l], max_count)
            assert records(alone) == records(got[i]) and m1 == mass[i], (max_count, i)             # ... alone: the same bits
        # list_of = None: quiz i takes list i
        got3, mass3 = eng.list_top_targets_among_batch(quizzes[:4], lists, max_count)
        for i in range(4):
            check((max_count, "none", i), got3[i], mass3[i], pris[i], TGAPS, lists[i], max_count)
    assert eng.list_top_targets_among_batch([], [], 5) == ([], [])
    got, mass = eng.list_top_targets_among_batch(quizzes[:2], [lists[0]], 0, [0, 0])     # max_count 0: nothing listed, the mass all the same
    assert got == [[], []] and mass[0] == eng.list_top_targets_among(quizzes[0], lists[0], 10)[1]
    eng.close()


# ---- 4. more than 256 quizzes ------------------------------------------------------------------------------------------------------------------------
def test_more_than_256_quizzes(factory):
    K, Q, T = 3, 8, 301
    eng = synth_engine(factory, K, Q, T, tgaps=[5])
    quizzes = eng.start_quiz_batch(300)
    for r in range(3):
        live = [q for j, q in enumerate(quizzes) if j % 4 > r]
        for q in live:
            eng.set_active_question(q, (q + r) % Q)
        eng.record_answer_batch(live, [(q * 7 + r) % K for q in live])
    lists = seeded_lists(T, [120, 301], 9)
    list_of = [j % 2 for j in range(300)]
    got, mass = eng.list_top_targets_among_batch(quizzes, lists, 7, list_of)
    for j in (0, 1, 2, 3, 130, 255, 256, 257, 298, 299):
        check(("300", j), got[j], mass[j], eng.get_priors(quizzes[j]), [5], lists[list_of[j]], 7)
    tail, tail_mass = eng.list_top_targets_among_batch(quizzes[256:], lists, 7, list_of[256:])      # the second group as a call of its own
    assert [records(x) for x in tail] == [records(x) for x in got[256:]] and tail_mass == mass[256:]
    eng.close()


# ---- 5. two merge levels: more wave lists than one merge workgroup takes -----------------------------------------------------------------------------
def test_two_merge_levels(factory):
    """T = 66001: 17 chunks of 4096 = 68 wave lists; at max_count = 256 a merge workgroup takes 16384 / 256 = 64 of them
    (kb_kernels.hip: TopFanIn), so a second level runs; at 10 one level does."""
    K, Q, T = 2, 8, 66001
    eng = synth_engine(factory, K, Q, T, tgaps=[0, 65999])
    quiz = play(eng, history(Q, K, 3, 2))
    pri = eng.get_priors(quiz)
    ids = [int(t) for t in np.random.default_rng(4).permutation(T)]
    for max_count in (256, 10):
        got, mass = eng.list_top_targets_among(quiz, ids, max_count)
        check(("levels", max_count), got, mass, pri, [0, 65999], ids, max_count)
    eng.close()


# ---- 6. precision and shards -----------------------------------------------------------------------------------------------------------------------------
def test_float_engine(factory):
    K, Q, T = 4, 12, 5003
    eng = synth_engine(factory, K, Q, T, tgaps=TGAPS, **F32)
    quiz = play(eng, history(Q, K, 6, 5))
    pri = eng.get_priors(quiz)
    lists = seeded_lists(T, [65, 1025, 5003], 11, TGAPS)
    for max_count in (10, 257):
        got, mass = eng.list_top_targets_among_batch([quiz] * 3, lists, max_count)
        for j, ids in enumerate(lists):
            check(("float", max_count, j), got[j], mass[j], pri, TGAPS, ids, max_count)
    eng.close()


def test_shard_engines_list_what_the_whole_engine_lists(factory):
    """Engines made for parts of the question axis, side by side on one device: the posterior is replicated, the call needs nothing more."""
    K, Q, T = 4, 30, 1300
    A, D, B = synth.synthetic_kb(K, Q, T, 0.1, 8.0, 0.5, 4)
    whole, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
    assert err is None
    whole.set_kb(A, D, B)
    bounds = pdist.shard_bounds(Q, 2)
    firsts = [0] + bounds[:-1]
    shards = []
    for first, limit in zip(firsts, bounds):
        sh = factory.create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1), first, Q, 0)
        sh.set_kb(A[first:limit], D[first:limit], B)
        shards.append(sh)
    lists = seeded_lists(T, [50, 1100], 6)
    qw = whole.start_quiz_batch(2)
    want, wmass = whole.list_top_targets_among_batch(qw, lists, 12)
    pri = whole.get_priors(qw[0])
    assert len(set(pri)) > T // 2
    check("whole", want[1], wmass[1], pri, [], lists[1], 12)
    for sh in shards:
        qs = sh.start_quiz_batch(2)
        assert np.array_equal(sh.get_priors(qs[0]), pri)
        got, mass = sh.list_top_targets_among_batch(qs, lists, 12)
        assert [records(x) for x in got] == [records(x) for x in want] and mass == wmass
        with pytest.raises(interop.PqaException, match=r"list=0 position=0 targetId=%d\b" % T):
            sh.list_top_targets_among(qs[0], [T], 3)
    for e in [whole] + shards:
        e.close()


def test_one_process_sharded_engine_lists_what_the_whole_engine_lists(factory):
    from test_gpu_sampled_batch import devices

    K, Q, T = 4, 30, 1300
    A, D, B = synth.synthetic_kb(K, Q, T, 0.1, 8.0, 0.5, 4)
    engines = []
    for spec in ("0,0", None):
        if spec:
            with devices(spec):
                eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
        else:
            eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
        assert err is None
        eng.set_kb(A, D, B)
        engines.append(eng)
    sh, whole = engines
    assert sh.get_option("shards") == 2
    lists = seeded_lists(T, [50, 1100, 0], 6)
    hists = [history(Q, K, j, 60 + j) for j in range(3)]
    out = []
    for eng in engines:
        quizzes = [play(eng, h) for h in hists]
        out.append([eng.list_top_targets_among_batch(quizzes, lists, m) for m in (12, 300)])
        if eng is whole:
            check("whole", out[-1][0][0][1], out[-1][0][1][1], eng.get_priors(quizzes[1]), [], lists[1], 12)
        with pytest.raises(interop.PqaException, match=r"entry=1 "):
            eng.list_top_targets_among_batch([quizzes[0], 12345], lists[:2], 3)
    for (ga, ma), (gb, mb) in zip(*out):
        assert [records(x) for x in ga] == [records(x) for x in gb] and ma == mb
    sh.close()
    whole.close()


# ---- 7. nothing changes -----------------------------------------------------------------------------------------------------------------------------------
def test_the_calls_change_no_quiz_state(factory):
    """One engine makes the calls between the steps of a quiz loop -- also directly behind record_answer, when its update is deferred --,
    its twin makes none."""
    K, Q, T = 4, 12, 5003
    a, b = (synth_engine(factory, K, Q, T, tgaps=TGAPS) for _ in range(2))
    qa, qb = a.start_quiz(), b.start_quiz()
    lists = seeded_lists(T, [300, 4200], 8, TGAPS)
    rng = np.random.default_rng(12)
    for step in range(4):
        pa, pb = a.next_question_argmax(qa), b.next_question_argmax(qb)
        assert pa == pb and a.get_active_question_id(qa) == pa
        a.list_top_targets_among_batch([qa, qa], lists, 10)
        assert a.get_active_question_id(qa) == pa
        ans = int(rng.integers(K))
        a.record_answer(qa, ans)
        b.record_answer(qb, ans)
        got, mass = a.list_top_targets_among_batch([qa, qa], lists, 300)      # (directly behind record_answer)
        pri = b.get_priors(qb)
        assert np.array_equal(a.get_priors(qa), pri), step
        for j in range(2):
            check(("loop", step, j), got[j], mass[j], pri, TGAPS, lists[j], 300)
        assert records(a.list_top_targets(qa, 5)) == records(b.list_top_targets(qb, 5)), step
    assert a.next_question_argmax(qa) == b.next_question_argmax(qb)
    assert a.get_total_questions_asked() == b.get_total_questions_asked()
    a.close()
    b.close()


# ---- 8. refusals: decided before anything is launched or written ------------------------------------------------------------------------------------------------
def test_refusals(factory):
    K, Q, T = 3, 8, 301
    eng = synth_engine(factory, K, Q, T)
    quizzes = eng.start_quiz_batch(3)
    pri = eng.get_priors(quizzes[0])
    lib = interop.load_library()
    p64, pd, prec = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(interop.CiRatedTarget)
    SENT = -77

    def call(n=3, qs=tuple(quizzes), list_of=(0, 1, 1), n_lists=2, counts=(2, 3), targets=(5, 6, 7, 8, 9), max_count=4, null=()):
        """The call through the library itself; returns the error's text ('' for success).  A refused call must have written nothing."""
        arr = lambda v: np.array(list(v) + [0], dtype=np.int64)
        a_qs, a_lof, a_counts, a_targets = arr(qs), (None if list_of is None else arr(list_of)), arr(counts), arr(targets)
        dest = np.full(2 * max(n, 1) * max(max_count, 1), float(SENT))
        out_counts, mass = np.full(max(n, 1), SENT, dtype=np.int64), np.full(max(n, 1), float(SENT))
        ptr = lambda name, a, t: None if (a is None or name in null) else a.ctypes.data_as(t)
        e = lib.PqaEngine_ListTopTargetsAmongBatch(eng.c_engine, n, ptr("quizzes", a_qs, p64), ptr("list_of", a_lof, p64), n_lists, ptr("counts", a_counts, p64),
                                                   ptr("targets", a_targets, p64), max_count, ptr("dest", dest, prec), ptr("out_counts", out_counts, p64),
                                                   ptr("mass", mass, pd))
        if not e:
            return ""
        assert (dest == SENT).all() and (out_counts == SENT).all() and (mass == SENT).all()
        return interop.PqaError(e).to_string(True)

    assert call() == ""
    assert call(null=("mass",)) == ""                                  # (the mass is optional)
    for kw in (dict(n=-1), dict(n_lists=-2), dict(max_count=-3)):
        assert "must be non-negative" in call(**kw), kw
    msg = call(counts=(2, -3))
    assert "list=1" in msg and "non-negative" in msg
    for name in ("quizzes", "counts", "targets", "dest", "out_counts"):
        assert "Nullptr" in call(null=(name,)), name
    assert "as many lists as quizzes" in call(list_of=None)                 # 2 lists, 3 quizzes
    assert call(list_of=None, n_lists=3, counts=(2, 2, 1)) == ""
    for bad in (2, -1):
        msg = call(list_of=(0, 1, bad))
        assert "entry=2" in msg and "list index" in msg, msg
    msg = call(qs=(quizzes[0], 99999, quizzes[2]))
    assert "entry=1" in msg and "99999" in msg, msg
    for bad in (-1, T):
        msg = call(targets=(5, 6, 7, bad, 9))
        assert "list=1 position=1 targetId=%d " % bad in msg and "out of range" in msg, msg
    msg = call(targets=(5, 6, 7, 8, 7))
    assert "list=1 position=2 targetId=7" in msg and "twice" in msg, msg
    assert call(targets=(5, 6, 5, 6, 7)) == ""                              # (the same target in two lists is no repetition)
    assert "targetId=%d" % T in call(list_of=(0, 0, 0), targets=(5, 6, 7, T, 9))   # a list no quiz points at is validated all the same
    # maintenance mode (entering it releases the quizzes: an engine of its own)
    m = synth_engine(factory, K, Q, T)
    qm = m.start_quiz_batch(1)
    m.start_maintenance(True)
    with pytest.raises(interop.PqaException, match="current mode is not regular"):
        m.list_top_targets_among(qm[0], [1, 2], 2)
    m.finish_maintenance()
    m.close()
    # after the refused calls the next good one is correct
    ids = [int(t) for t in np.random.default_rng(2).permutation(T)[:200]]
    got, mass = eng.list_top_targets_among(quizzes[0], ids, 9)
    check("after refusals", got, mass, pri, [], ids, 9)
    eng.close()
