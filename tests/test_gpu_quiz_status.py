"""PqaEngine_QuizStatusBatch and PqaEngine_RankTargetsBatch on the GPU (include/PqaHipExt.h; status_kernels.hip; hip_engine_status.cpp):
where a quiz stands -- entropy, mass, best target, candidates, candidates above levels -- and where named targets stand in it.

The expected values need no oracle: the posterior is read back with get_priors (held to the oracle elsewhere).  A candidate is a target
that is no gap with p > 0.  Counts, the best target, the bits of its probability, every level count, every rank and every ranked
probability must be EQUAL to numpy's.  The bars of the sums are derived, not measured:
  entropy: |H - H_ref| <= (T + 16) 2^-52 max(1, H_ref) bits, H_ref = -math.fsum(p log2 p) over the candidates: every term is >= 0, so the
    sum of the terms' magnitudes is H itself (the bar of PreviewAnswersBatch's entropies, tests/test_gpu_preview_answers.py);
  mass and level masses: within (T + 16) 2^-52 relative of math.fsum over the same elements -- the terms are non-negative, and any
    summation order of n non-negative terms stays within n 2^-53 relative.
The worst seen of either is printed (in units of its bar).  The entropy is also held to PreviewAnswersBatch's promise bit for bit."""
import ctypes
import math
import struct

import numpy as np
import pytest

import cases
from probqa_amd import dist as pdist
from probqa_amd import interop, synth

pytestmark = pytest.mark.gpu

F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)
P64, PD, PST = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(interop.CiHipQuizStatus)
EPS = 2.0 ** -52

# K, Q, T, target gaps: the smallest shapes that reach each edge of the kernels
SHAPES = {
    "min_2x1x2": (2, 1, 2, ()),
    "gaps_3x8x12": (3, 8, 12, (2, 11)),                     # target gaps
    "padded_3x8x13": (3, 8, 13, (2, 11)),                   # ... and T mod 4 != 0
    "small_5x12x1024": (5, 12, 1024, (1023,)),              # the 256-thread shape
    "large_5x12x1025": (5, 12, 1025, ()),                   # the 1024-thread shape
    "oddk_7x9x130": (7, 9, 130, (0,)),
    "many_3x6x9000": (3, 6, 9000, (4500,)),                 # many elements per thread
    "long_2x4x16400": (2, 4, 16400, ()),                    # beyond 16384: RecordAnswer runs the long-row launches
}
WORST = {"entropy": 0.0, "mass": 0.0}


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


def bits(x):
    return struct.pack("<d", x)


def candidates(p, tgaps):
    ids = np.arange(len(p))
    ok = (p > 0) & ~np.isin(ids, list(tgaps))
    return ids[ok], p[ok]


def entropy_of(pc):
    return -math.fsum((pc * np.log2(pc)).tolist())


def ranks_of(p, tgaps):
    """rank per target by (probability descending, id ascending) over the candidates; -1 for the others"""
    c, pc = candidates(p, tgaps)
    rank = np.full(len(p), -1, dtype=np.int64)
    rank[c[np.lexsort((c, -pc))]] = np.arange(len(c))
    return rank


def kth_largest(p, tgaps, k):
    _, pc = candidates(p, tgaps)
    return float(np.sort(pc)[::-1][min(k, len(pc)) - 1]) if len(pc) else 0.5


def check_status(name, got, p, tgaps, levels, T):
    c, pc = candidates(p, tgaps)
    assert got.n_candidates == len(c), (name, got.n_candidates, len(c))
    if len(c):
        top = int(c[np.lexsort((c, -pc))[0]])
        assert got.i_top_target == top and bits(got.top_prob) == bits(float(p[top])), (name, got.i_top_target, got.top_prob, top, p[top])
    else:
        assert got.i_top_target == -1 and bits(got.top_prob) == bits(0.0), (name, got)
    h_ref, m_ref = (entropy_of(pc), math.fsum(pc.tolist())) if len(c) else (0.0, 0.0)
    dh = abs(got.entropy - h_ref) / ((T + 16) * EPS * max(1.0, h_ref))
    dm = abs(got.mass - m_ref) / ((T + 16) * EPS * m_ref) if m_ref > 0 else float(got.mass != 0.0)
    assert len(got.level_counts) == len(levels) and len(got.level_mass) == len(levels)
    for j, lv in enumerate(levels):
        above = pc[pc >= lv]
        assert got.level_counts[j] == len(above), (name, j, lv, got.level_counts[j], len(above))
        want = math.fsum(above.tolist())
        dl = abs(got.level_mass[j] - want) / ((T + 16) * EPS * want) if want > 0 else float(got.level_mass[j] != 0.0)
        dm = max(dm, dl)
        assert dl <= 1.0, (name, j, lv, got.level_mass[j], want)
    WORST["entropy"], WORST["mass"] = max(WORST["entropy"], dh), max(WORST["mass"], dm)
    print("%s: entropy %.17g want %.17g (%.3f of the bar); mass %.17g want %.17g (worst of mass and level masses %.3f of the bar)"
          % (name, got.entropy, h_ref, dh, got.mass, m_ref, dm))
    assert dh <= 1.0, (name, got.entropy, h_ref)
    assert dm <= 1.0, (name, got.mass, m_ref)


# ---- 1. every shape, both precisions, three quiz states, one call, against numpy over get_priors -----------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_status_is_numpys(factory, shape, f32):
    K, Q, T, tgaps = SHAPES[shape]
    eng = make_engine(factory, K, Q, T, tgaps, f32)
    quizzes = [play(eng, history(Q, K, n, 31 + n)) for n in (0, 3, 12)]       # fresh, after 3 answers, after 12
    priors = [eng.get_priors(z) for z in quizzes]
    # the levels are the call's: every quiz's own third-largest element among them, so >= against > is decided on equal bits for each
    levels = [0.0, 1.0 / T] + [kth_largest(p, tgaps, 3) for p in priors] + [2.0, math.inf]
    got = eng.quiz_status_batch(quizzes, levels)
    assert len(got) == 3
    for i, (st, p) in enumerate(zip(got, priors)):
        check_status((shape, f32, i), st, p, tgaps, levels, T)
        assert st.level_counts[0] == st.n_candidates and bits(st.level_mass[0]) == bits(st.mass)      # a level <= 0 counts every candidate
        assert st.level_counts[-1] == 0 and st.level_counts[-2] == 0 and st.level_mass[-1] == 0.0     # 2.0 and +inf count none
        assert st.level_counts[2 + i] >= min(3, st.n_candidates)                                       # its own third-largest: itself included
        assert eng.get_priors(quizzes[i]).tobytes() == p.tobytes()
    print("worst so far, in units of the bar:", WORST)
    eng.close()


# ---- 2. the entropy is PreviewAnswersBatch's promise, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_entropy_is_the_previewed_entropy(factory, shape, f32):
    K, Q, T, tgaps = SHAPES[shape]
    eng = make_engine(factory, K, Q, T, tgaps, f32)
    checked = 0
    for n in (0, 3):
        quiz = play(eng, history(Q, K, n, 41 + n))
        q = Q // 2
        previews = eng.preview_answers(quiz, q, 0)
        live = [k for k in range(K) if previews[k].likelihood > 0 and not math.isnan(previews[k].entropy)]
        assert live, (shape, f32, n)
        k = live[len(live) // 2]
        eng.set_active_question(quiz, q)
        eng.record_answer(quiz, k)
        got = eng.quiz_status(quiz).entropy
        assert bits(got) == bits(previews[k].entropy), (shape, f32, n, k, got, previews[k].entropy)
        checked += 1
    assert checked == 2
    eng.close()


# ---- 3. ranks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_ranks_are_numpys(factory, shape, f32):
    K, Q, T, tgaps = SHAPES[shape]
    eng = make_engine(factory, K, Q, T, tgaps, f32)
    eng.set_option("top_exact", 0)
    quizzes = [play(eng, history(Q, K, n, 51 + n)) for n in (0, 3, 12)]
    rng = np.random.default_rng(T)
    pairs = []
    for z in quizzes:   # 16 named targets per quiz, the gaps, the ends and the best targets among them (a target may repeat where T is small)
        best = [t.i_target for t in eng.list_top_targets_among(z, list(range(T)), 10)[0]]
        named = (list(tgaps) + [0, T - 1] + best + [int(t) for t in rng.integers(0, T, size=16)])[:16]
        pairs += [(z, t) for t in named]
    got = eng.rank_targets_batch(pairs)
    assert len(got) == len(pairs)
    for z in quizzes:
        p = eng.get_priors(z)
        want = ranks_of(p, tgaps)
        top10 = [t.i_target for t in eng.list_top_targets_among(z, list(range(T)), 10)[0]]
        seen_low = 0
        for (zz, t), (rank, prob) in zip(pairs, got):
            if zz != z:
                continue
            assert rank == want[t] and bits(prob) == bits(float(p[t])), (shape, f32, z, t, rank, int(want[t]), prob, p[t])
            assert (rank == -1) == (t in tgaps or not p[t] > 0)
            if 0 <= rank < 10:
                assert top10[rank] == t, (shape, f32, z, t, rank, top10)
                seen_low += 1
        assert seen_low >= min(3, len(top10))
    eng.close()


# ---- 4. ties: a fresh quiz on an engine that is not filled ---------------------------------------------------------------------------------
def test_order_among_ties(factory):
    K, Q, T, tgaps = 3, 8, 1025, (0, 64)
    eng = make_engine(factory, K, Q, T, tgaps, fill=False, init=1.0)
    quiz = eng.start_quiz()
    p = eng.get_priors(quiz)
    assert len(set(np.delete(p, list(tgaps)).tolist())) == 1
    st = eng.quiz_status(quiz, [float(p[1])])
    assert st.i_top_target == 1 and bits(st.top_prob) == bits(float(p[1])) and st.n_candidates == T - 2
    assert st.level_counts == [T - 2] and bits(st.level_mass[0]) == bits(st.mass)
    assert abs(st.entropy - math.log2(T - 2)) <= (T + 16) * EPS * math.log2(T - 2)
    named = [0, 1, 2, 62, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512, 1023, 1024]     # across lanes, waves and the last, lone element
    got = eng.rank_targets_batch([(quiz, t) for t in named])
    for t, (rank, prob) in zip(named, got):
        below = t - sum(1 for g in tgaps if g < t)
        assert rank == (-1 if t in tgaps else below), (t, rank, below)
        assert bits(prob) == bits(float(p[t]))
    eng.close()


# ---- 5. tiles and chunks ---------------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_batch(factory):
    K, Q, T, tgaps = 5, 17, 1300, (3, 1299)
    eng = make_engine(factory, K, Q, T, tgaps)
    quizzes = [play(eng, history(Q, K, n, 60 + n)) for n in (0, 3, 12)]
    levels = [0.0, 1e-3, 0.05]
    # one quiz under 70 targets, some repeated, makes three tiles; the other quizzes' pairs lie between them
    rng = np.random.default_rng(8)
    named = [int(t) for t in rng.integers(0, T, size=60)] + [3, 1299, 5, 5, 5, 7, 7, 0, T - 2, 9]
    assert len(named) == 70
    pairs = []
    for i, t in enumerate(named):
        pairs.append((quizzes[1], t))
        if i % 9 == 0:
            pairs.append((quizzes[i % 2 * 2], (31 * i) % T))
    got = eng.rank_targets_batch(pairs)
    alone = {}
    for pair, (rank, prob) in zip(pairs, got):
        if pair not in alone:
            alone[pair] = eng.rank_target(*pair)
        assert rank == alone[pair][0] and bits(prob) == bits(alone[pair][1]), pair
    want = ranks_of(eng.get_priors(quizzes[1]), tgaps)
    assert [r for (z, _), (r, _) in zip(pairs, got) if z == quizzes[1]] == [int(want[t]) for t in named]
    # 300 quizzes in one status call make two chunks; a quiz's record is the same bits wherever it stands, and alone
    order = [quizzes[i % 3] for i in range(300)]
    batch = eng.quiz_status_batch(order, levels)
    assert len(batch) == 300

    def record(s):
        return (bits(s.entropy), bits(s.mass), bits(s.top_prob), s.i_top_target, s.n_candidates, tuple(s.level_counts), tuple(bits(m) for m in s.level_mass))

    single = {z: record(eng.quiz_status(z, levels)) for z in quizzes}
    assert len(set(single.values())) == 3
    for z, s in zip(order, batch):
        assert record(s) == single[z], z
    three = eng.quiz_status_batch([quizzes[2]] * 3, levels)
    assert [record(s) for s in three] == [single[quizzes[2]]] * 3
    assert eng.quiz_status_batch([], levels) == [] and eng.rank_targets_batch([]) == []
    # without levels, and with one of the level buffers left out
    assert record(eng.quiz_status(quizzes[0]))[:5] == single[quizzes[0]][:5]
    eng.close()


# ---- 6. shard engines and the one-process sharded engine ---------------------------------------------------------------------------------------
def both(eng, quizzes, T, levels):
    def record(s):
        return (bits(s.entropy), bits(s.mass), bits(s.top_prob), s.i_top_target, s.n_candidates, tuple(s.level_counts), tuple(bits(m) for m in s.level_mass))

    pairs = [(z, t) for z in quizzes for t in (0, 1, T // 2, T - 1, 17, 17)]
    return [record(s) for s in eng.quiz_status_batch(quizzes, levels)], [(r, bits(p)) for r, p in eng.rank_targets_batch(pairs)]


def test_shard_engines_answer_like_the_whole_engine(factory):
    """Engines made for parts of the question axis, side by side on one device: the posterior is replicated, the calls need nothing more."""
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
    levels = [0.0, 1.0 / T, 0.01]
    qw = whole.start_quiz_batch(2)
    want = both(whole, qw, T, levels)
    pri = whole.get_priors(qw[0])
    check_status("whole", whole.quiz_status(qw[0], levels), pri, (), levels, T)
    for sh in shards:
        qs = sh.start_quiz_batch(2)
        assert np.array_equal(sh.get_priors(qs[0]), pri)
        assert both(sh, qs, T, levels) == want
        with pytest.raises(interop.PqaException, match=r"entry=1 targetId=%d\b" % T):
            sh.rank_targets_batch([(qs[0], 0), (qs[0], T)])
    for e in [whole] + shards:
        e.close()


def test_one_process_sharded_engine_answers_like_the_whole_engine(factory):
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
    levels = [0.0, 1.0 / T, 0.01]
    hists = [history(Q, K, j, 60 + j) for j in range(3)]
    out = []
    for eng in engines:
        quizzes = [play(eng, h) for h in hists]
        # directly behind a deferred record_answer: the answer is applied first
        eng.set_active_question(quizzes[0], 29)
        eng.record_answer(quizzes[0], 2)
        out.append(both(eng, quizzes, T, levels))
        check_status(("sharded", eng is sh), eng.quiz_status(quizzes[0], levels), eng.get_priors(quizzes[0]), (), levels, T)
        with pytest.raises(interop.PqaException, match=r"entry=1 "):
            eng.quiz_status_batch([quizzes[0], 12345], levels)
        with pytest.raises(interop.PqaException, match=r"entry=1 "):
            eng.rank_targets_batch([(quizzes[0], 3), (12345, 3)])
    assert out[0] == out[1]
    sh.close()
    whole.close()


# ---- 7. nothing changes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("server", [0, 1])
def test_the_calls_change_no_quiz_state(factory, server):
    """One engine makes the calls between the steps of a quiz loop -- also directly behind record_answer, when its update is deferred --,
    its twin makes none."""
    K, Q, T, tgaps = 5, 40, 1000, (3, 700)
    a, b = (make_engine(factory, K, Q, T, tgaps) for _ in range(2))
    for e in (a, b):
        e.set_option("server", server)
        e.set_option("seed", 5)
    qa, qb = a.start_quiz(), b.start_quiz()
    calls0, pairs0 = a.get_option("status_calls"), a.get_option("rank_pairs")
    levels = [0.0, 0.01]
    rng = np.random.default_rng(12)
    transcript = [[], []]
    for step in range(5):
        pa, pb = a.next_question(qa), b.next_question(qb)
        transcript[0].append(pa)
        transcript[1].append(pb)
        assert pa == pb and a.get_active_question_id(qa) == pa, (step, pa, pb)
        a.quiz_status_batch([qa, qa], levels)
        a.rank_targets_batch([(qa, 5), (qa, 3), (qa, 999)])
        assert a.get_active_question_id(qa) == pa
        ans = int(rng.integers(K))
        a.record_answer(qa, ans)
        b.record_answer(qb, ans)
        st = a.quiz_status(qa, levels)                                       # (directly behind record_answer)
        ranks = a.rank_targets_batch([(qa, t) for t in (0, 3, 500, 999)])
        pri = b.get_priors(qb)
        check_status(("loop", server, step), st, pri, tgaps, levels, T)
        want = ranks_of(pri, tgaps)
        assert [r for r, _ in ranks] == [int(want[t]) for t in (0, 3, 500, 999)]
    assert transcript[0] == transcript[1]
    assert a.next_question(qa) == b.next_question(qb)
    assert a.get_priors(qa).tobytes() == b.get_priors(qb).tobytes()
    assert a.get_total_questions_asked() == b.get_total_questions_asked()
    assert a.get_option("status_calls") == calls0 + 10 and a.get_option("rank_pairs") == pairs0 + 5 * 7
    assert a.get_option("status_quizzes") >= 15 and a.get_option("rank_calls") >= 10
    a.set_option("time_sweeps", 1)
    ns0 = a.get_option("status_device_ns")
    a.quiz_status(qa, levels)
    assert a.get_option("status_device_ns") > ns0
    a.close()
    b.close()


# ---- 8. refusals, in the header's order ------------------------------------------------------------------------------------------------------
SENT = -7.0


def raw_status(eng, quizzes, levels, n=None, n_levels=None, null=()):
    """The C call on sentinel-filled buffers -> (error pointer, the buffers)."""
    qs = np.ascontiguousarray(list(quizzes) or [0], dtype=np.int64)
    lv = np.ascontiguousarray(list(levels) or [0.0], dtype=np.float64)
    nq = len(quizzes) if n is None else n
    nl = len(levels) if n_levels is None else n_levels
    rows = max(len(quizzes), 1)
    S = np.full(rows * 5, SENT)
    C = np.full(rows * 16, int(SENT), dtype=np.int64)
    M = np.full(rows * 16, SENT)
    err = interop.load_library().PqaEngine_QuizStatusBatch(
        eng.c_engine, nq, None if "quizzes" in null else qs.ctypes.data_as(P64), nl, None if "levels" in null else lv.ctypes.data_as(PD),
        None if "status" in null else ctypes.cast(S.ctypes.data, PST), None if "counts" in null else C.ctypes.data_as(P64),
        None if "mass" in null else M.ctypes.data_as(PD))
    return err, (S, C, M)


def raw_rank(eng, pairs, n=None, null=()):
    pr = np.ascontiguousarray(list(pairs) or [(0, 0)], dtype=np.int64).reshape(-1, 2)
    quizzes, targets = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
    P = np.full(len(pr), SENT)
    R = np.full(len(pr), int(SENT), dtype=np.int64)
    err = interop.load_library().PqaEngine_RankTargetsBatch(
        eng.c_engine, len(pairs) if n is None else n, None if "quizzes" in null else quizzes.ctypes.data_as(P64),
        None if "targets" in null else targets.ctypes.data_as(P64), None if "prob" in null else P.ctypes.data_as(PD), None if "rank" in null else R.ctypes.data_as(P64))
    return err, (P, R)


def test_refusals(factory):
    K, Q, T = 3, 8, 13
    eng = make_engine(factory, K, Q, T)
    quiz = eng.start_quiz()
    counters = ("status_calls", "status_quizzes", "rank_calls", "rank_pairs")
    before = [eng.get_option(c) for c in counters]
    NEG, NULL, RANGE, MODE = "The count is negative", "Expected non-null argument", "Index is out of range", "An attempt to execute an operation in a wrong mode"
    ok, lv = [quiz, quiz], [0.0, 2.0]

    def refused(result, code, *texts):
        err, buffers = result
        assert err, texts
        s = interop.PqaError(err).to_string(True)
        assert s.startswith("[" + code + "]") and all(t in s for t in texts), s
        assert all((b == SENT).all() for b in buffers), s
        assert [eng.get_option(c) for c in counters] == before

    # ---- the status call
    refused(raw_status(eng, ok, lv, n=-1), NEG, "count=-1", "nQuizzes")
    refused(raw_status(eng, ok, lv, n_levels=-2), NEG, "count=-2", "nLevels")
    refused(raw_status(eng, ok, lv, n=-1, null=("quizzes", "status", "levels", "counts", "mass")), NEG, "count=-1")   # the count, not the NULL
    refused(raw_status(eng, ok, lv, n_levels=-2, null=("quizzes", "status", "levels", "counts", "mass")), NEG, "count=-2")
    refused(raw_status(eng, ok, [0.1] * 17), RANGE, "subjIndex=17", "16")
    refused(raw_status(eng, ok, lv, null=("quizzes",)), NULL)
    refused(raw_status(eng, ok, lv, null=("status",)), NULL)
    refused(raw_status(eng, ok, lv, null=("levels",)), NULL)
    refused(raw_status(eng, ok, lv, null=("counts", "mass")), NULL)
    refused(raw_status(eng, ok, [0.5, math.nan]), RANGE, "level=1")
    refused(raw_status(eng, [99], lv), RANGE, "entry=0", "quizId=99")
    refused(raw_status(eng, ok + [1 << 40], lv), RANGE, "entry=2", "quizId=%d" % (1 << 40))
    # the order: the counts, the limit, a NULL, a NaN level, the quiz
    refused(raw_status(eng, [99], [math.nan] * 17, n=-1, null=("status",)), NEG, "count=-1")
    refused(raw_status(eng, [99], [math.nan] * 17, null=("status",)), RANGE, "subjIndex=17")
    refused(raw_status(eng, [99], [math.nan], null=("status",)), NULL)
    refused(raw_status(eng, [99], [math.nan]), RANGE, "level=0")
    # either level buffer may be left out; both with no levels
    err, (S, C, M) = raw_status(eng, ok, lv, null=("counts",))
    assert not err and (C == SENT).all() and (M[:4] != SENT).all() and (M[4:] == SENT).all() and (S != SENT).all()
    err, (S, C, M) = raw_status(eng, ok, lv, null=("mass",))
    assert not err and (M == SENT).all() and C[:4].tolist() == [T, 0, T, 0]
    err, (S, C, M) = raw_status(eng, ok, [], null=("levels", "counts", "mass"))
    assert not err and (S != SENT).all()
    assert not raw_status(eng, [], lv)[0] and not raw_status(eng, [], [], null=("quizzes", "status", "levels", "counts", "mass"))[0]
    # ---- the rank call
    before = [eng.get_option(c) for c in counters]
    pairs = [(quiz, 1), (quiz, 12)]
    refused(raw_rank(eng, pairs, n=-1), NEG, "count=-1", "nPairs")
    refused(raw_rank(eng, pairs, n=-1, null=("quizzes", "targets", "prob", "rank")), NEG, "count=-1")
    for missing in ("quizzes", "targets", "prob", "rank"):
        refused(raw_rank(eng, pairs, null=(missing,)), NULL)
    refused(raw_rank(eng, [(99, 1)]), RANGE, "entry=0", "quizId=99")
    refused(raw_rank(eng, pairs + [(quiz, T)]), RANGE, "entry=2", "targetId=%d" % T)
    refused(raw_rank(eng, [(quiz, -1)] + pairs), RANGE, "entry=0", "targetId=-1")
    refused(raw_rank(eng, [(quiz, T), (99, 1)]), RANGE, "entry=1", "quizId=99")         # the quiz in front of the target
    refused(raw_rank(eng, [(99, T)], null=("prob",)), NULL)
    assert not raw_rank(eng, [])[0]
    err, (P, R) = raw_rank(eng, pairs)
    assert not err and (P != SENT).all() and (R != int(SENT)).all()
    # ---- maintenance mode and shutdown, as PreviewAnswersBatch answers them: in front of the quiz, behind a NULL and a NaN level
    before = [eng.get_option(c) for c in counters]
    eng.start_maintenance(True)
    refused(raw_status(eng, [99], lv), MODE)
    refused(raw_status(eng, [99], lv, null=("status",)), NULL)
    refused(raw_status(eng, [99], [math.nan]), RANGE, "level=0")
    refused(raw_rank(eng, [(99, T)]), MODE)
    refused(raw_rank(eng, [(99, T)], null=("rank",)), NULL)
    eng.finish_maintenance()
    quiz = eng.start_quiz()
    st = eng.quiz_status(quiz, lv)                                             # the next good call is correct
    check_status("after", st, eng.get_priors(quiz), (), lv, T)
    assert eng.rank_target(quiz, 0)[0] == int(ranks_of(eng.get_priors(quiz), ())[0])
    before = [eng.get_option(c) for c in counters]
    eng.shutdown()
    refused(raw_status(eng, [quiz], lv), MODE)
    refused(raw_rank(eng, [(quiz, 1)]), MODE)
    eng.close()
