"""Target separation on the GPU (include/PqaHipExt.h: PqaEngine_EvalTargetSeparation, PqaEngine_ListSeparatingQuestionsBatch;
separation_kernels.hip; hip_engine_sources.cpp).

The model works over one get_kb(): p = A * (1.0 / D) in numpy fp64 -- the kernel's own product, barring a difference between its
reciprocal (pqa_device.h: div_nr, a refined hardware reciprocal) and IEEE division's, which the bar's allowance of two roundings per term
covers -- and the formula
    sep(G, q) = max(0, (1 / n) sum_j sum_k f(p_k(j)) - sum_k f(m_k)),   f(x) = x log2 x,   m_k = (sum_j p_k(j)) * (1 / n)
runs in Python floats with math.log2 and math.fsum.  The bar is derived, not measured, and ABSOLUTE (sep is a difference of entropies and
may be near 0):
    |gpu - model| <= (16 + 8 n K) 2^-52 bits
-- about two roundings and a one-ulp logarithm per term of magnitude <= 0.54; the mean carries n accumulations, fed through
f' <= log2 + 1.45; the final sum has (n + 1) K terms bounded by log2 64.
Worst seen on an MI355X over every case of this file: see README.md.
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
TILE_ENTRIES, CHUNK = 256, 256   # entries of a tile of the sweep (pqa_kernels.h: kSepTileEntries); groups of a chunk of the host's loop


def bar(n, K):
    return (16 + 8 * n * K) * 2.0 ** -52


def f(x):
    return x * math.log2(x) if x > 0 else 0.0


class Plant:
    """what set_kb planted, where the cube has room for it: two identical columns, a question at which a pair's answers are disjoint,
    a question block copied bitwise to another id"""

    def __init__(self, Q, T):
        self.ident = (5, 9) if T >= 33 else None
        self.disjoint = (2, 7) if T >= 33 else (0, 1)
        self.qd = Q // 2
        self.copy = (Q // 3, Q - 2) if Q >= 17 else None


def make_engine(factory, K, Q, T, tgaps=(), qgaps=(), seed=7, trains=3, **kw):
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **kw))
    assert err is None and eng is not None, err
    eng.fill_synthetic(8.0, 0.5, seed)
    eng.set_option("workers", cases.WORKERS)
    rng = np.random.default_rng(seed)
    free_t = [t for t in range(T) if t not in tgaps]
    for _ in range(trains):
        qs = rng.permutation(Q)[:min(3, Q)]
        eng.train([AQ(int(q), int(rng.integers(K))) for q in qs], int(rng.choice(free_t)), 1.5)
    pl = Plant(Q, T)
    A, D, B = eng.get_kb()
    if pl.ident:
        A[:, :, pl.ident[1]], D[:, pl.ident[1]] = A[:, :, pl.ident[0]], D[:, pl.ident[0]]
    a, b = pl.disjoint
    A[pl.qd, :, a], A[pl.qd, :, b] = 0.0, 0.0
    A[pl.qd, 0, a], A[pl.qd, 1, b] = D[pl.qd, a], D[pl.qd, b]
    if pl.copy:
        A[pl.copy[1]], D[pl.copy[1]] = A[pl.copy[0]], D[pl.copy[0]]
    eng.set_kb(A, D, B)
    if tgaps:
        eng.set_target_gaps(list(tgaps))
    if qgaps:
        eng.set_question_gaps(list(qgaps))
    return eng, pl


class Model:
    """sep(G, q) by the definition over one get_kb(); a group's row is computed once and kept."""

    def __init__(self, A, D, tgaps, qgaps):
        self.Q, self.K, self.T = A.shape
        self.tgaps, self.qgaps = set(tgaps), set(qgaps)
        with np.errstate(all="ignore"):
            self.p = A * (1.0 / D)[:, None, :]
        self.rows = {}

    def row(self, group):
        key = tuple(group)
        if key not in self.rows:
            out = np.zeros(self.Q)
            n = len(group)
            if not self.tgaps & set(group):
                for q in range(self.Q):
                    if q in self.qgaps:
                        continue
                    pk = [[float(self.p[q, k, t]) for k in range(self.K)] for t in group]
                    s1 = math.fsum(f(x) for member in pk for x in member)
                    m = [math.fsum(pk[j][k] for j in range(n)) * (1.0 / n) for k in range(self.K)]
                    out[q] = max(0.0, (1.0 / n) * s1 - math.fsum(f(x) for x in m))
            self.rows[key] = out
        return self.rows[key]


WORST = {"bits": 0.0, "of_bar": 0.0}


def within_bar(name, got_row, ref_row, n, K):
    err = float(np.abs(got_row - ref_row).max())
    WORST["bits"], WORST["of_bar"] = max(WORST["bits"], err), max(WORST["of_bar"], err / bar(n, K))
    print("%s: worst deviation %.3g bits, bar %.3g (worst so far %.3g bits, %.3g of its bar)" % (name, err, bar(n, K), WORST["bits"], WORST["of_bar"]))
    assert err <= bar(n, K), (name, err, bar(n, K))


def listing_of_row(row, max_count, q_first=0):
    """what the listing must be, from the engine's own Eval row: value > 0 (gaps are 0), by (-value, id)"""
    ids = np.array([q for q in range(len(row)) if row[q] > 0], dtype=np.int64)
    if len(ids) == 0:
        return []
    take = np.lexsort((ids, -row[ids]))[:max_count]
    return [(int(q_first + q), float(row[q])) for q in ids[take]]


def mixed_groups(T, pl, tgaps=(), seed=11):
    """sizes 2, 3, 17 and 64 (ids repeat where T is small), the planted pairs, a group with a member listed twice, a group with a gap member"""
    rng = np.random.default_rng(seed)
    free = [t for t in range(T) if t not in tgaps]
    groups = [[int(t) for t in rng.choice(free, size=n)] for n in (2, 3, 17, 64, 2, 64, 3)]
    groups.append(list(pl.disjoint))
    if pl.ident:
        groups.append(list(pl.ident))
    a, b = pl.disjoint
    groups.append([a, a, b])
    if tgaps:
        groups.append([free[0], tgaps[0], free[-1]])
    return groups


# ---- rows against the model, listings against the rows --------------------------------------------------------------------------------
SHAPES = {
    "k2_q1_t2": dict(K=2, Q=1, T=2),
    "k3_q17_t33": dict(K=3, Q=17, T=33, tgaps=(0, 32), qgaps=(3,)),
    "k5_q70_t257": dict(K=5, Q=70, T=257, tgaps=(17, 256), qgaps=(5, 69)),
    "k7_q17_t33": dict(K=7, Q=17, T=33, tgaps=(31,), qgaps=(0,)),
    "k2_q70_t33": dict(K=2, Q=70, T=33),
    "k5_q17_t2": dict(K=5, Q=17, T=2),
    "k3_q1_t257": dict(K=3, Q=1, T=257, tgaps=(100,)),
    "k2_q3_t16400_long_row": dict(K=2, Q=3, T=16400, tgaps=(16399,)),
    "f32_k2_q17_t257": dict(K=2, Q=17, T=257, tgaps=(17,), qgaps=(1, 16), f32=True),
    "f32_k5_q1_t33": dict(K=5, Q=1, T=33, f32=True),
    "f32_k3_q70_t2": dict(K=3, Q=70, T=2, qgaps=(2,), f32=True),
    "f32_k7_q17_t257": dict(K=7, Q=17, T=257, tgaps=(254,), qgaps=(0,), f32=True),
    "f32_k5_q3_t16400_long_row": dict(K=5, Q=3, T=16400, tgaps=(16399,), f32=True),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rows_and_listings(factory, name):
    sh = dict(SHAPES[name])
    K, Q, T, tgaps, qgaps = sh["K"], sh["Q"], sh["T"], sh.get("tgaps", ()), sh.get("qgaps", ())
    eng, pl = make_engine(factory, K, Q, T, tgaps, qgaps, **(F32 if sh.get("f32") else {}))
    A, D, B = eng.get_kb()
    model = Model(A, D, tgaps, qgaps)
    groups = mixed_groups(T, pl, tgaps)
    if T > 16384:
        groups.append([0, T - 2, 16384, 16385])   # columns on both sides of the 16384th target
    calls0, swept0 = eng.get_option("separation_calls"), eng.get_option("separation_groups")
    got = eng.eval_target_separation(groups)
    assert got.shape == (len(groups), Q)
    assert eng.get_option("separation_calls") == calls0 + 1 and eng.get_option("separation_groups") == swept0 + len(groups)
    assert eng.eval_target_separation(groups).tobytes() == got.tobytes()   # the same call, the same bytes
    for i, g in enumerate(groups):
        within_bar((name, i, len(g)), got[i], model.row(g), len(g), K)
        if set(g) & set(tgaps):
            assert not got[i].any()
    if qgaps:
        assert not got[:, list(qgaps)].any()
    assert (got >= 0).all() and (got > 1e-6).sum() >= 2 * (Q - len(qgaps)), (got > 1e-6).sum()   # the cube separates (the groups of 17 and 64 at least): nothing hides under the absolute bar
    # the planted structure
    i_dis = groups.index(list(pl.disjoint))
    if pl.qd not in qgaps:
        assert abs(got[i_dis, pl.qd] - 1.0) <= bar(2, K)
        assert eng.list_separating_questions(pl.disjoint, 3)[0] == (pl.qd, got[i_dis, pl.qd])
    if pl.ident:
        i_id = groups.index(list(pl.ident))
        assert (got[i_id] <= bar(2, K)).all()
        assert all(v <= bar(2, K) for _, v in eng.list_separating_questions(pl.ident, Q + 5))
    if pl.copy:
        assert got[:, pl.copy[0]].tobytes() == got[:, pl.copy[1]].tobytes()          # invariant (c): a copied block, the same bits for every group
        assert (got[:, pl.copy[0]] > 0).any() or pl.copy[0] in qgaps
    a, b = pl.disjoint
    i_twice = groups.index([a, a, b])
    assert got[i_twice].tobytes() != eng.eval_target_separation([[a, b]])[0].tobytes()   # the repeat weighs: not the pair's values
    # invariant (a): every group alone, and the batch in reverse order
    for i, g in enumerate(groups):
        assert eng.eval_target_separation([g])[0].tobytes() == got[i].tobytes(), (name, i)
    assert eng.eval_target_separation(groups[::-1])[::-1].tobytes() == got.tobytes()
    # listings: the engine's own rows, record for record
    for max_count in (0, 1, Q + 5):
        calls0, swept0 = eng.get_option("separation_calls"), eng.get_option("separation_groups")
        listed = eng.list_separating_questions_batch(groups, max_count)
        assert eng.get_option("separation_calls") == calls0 + 1 and eng.get_option("separation_groups") == swept0 + (len(groups) if max_count else 0)
        assert len(listed) == len(groups)
        for i, g in enumerate(groups):
            assert listed[i] == listing_of_row(got[i], max_count), (name, max_count, i)
            if set(g) & set(tgaps):
                assert listed[i] == []
        assert not {q for lst in listed for q, _ in lst} & set(qgaps)
    if pl.copy and pl.copy[0] not in qgaps:   # ties by ascending id: the copied block stands right behind its original
        for lst in eng.list_separating_questions_batch(groups, Q + 5):
            ids = [q for q, _ in lst]
            if pl.copy[0] in ids:
                assert ids[ids.index(pl.copy[0]) + 1] == pl.copy[1], ids
    assert eng.eval_target_separation([]).shape == (0, Q) and eng.list_separating_questions_batch([], 5) == []
    eng.close()


# ---- tiles and chunks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
def test_tile_and_chunk_edges(factory, f32):
    """A call whose groups fill one tile exactly, one with a single entry more, and one that spans three chunks of the host's loop: every
    group's row is the bytes it has alone, wherever it stands, and within the bar of the model."""
    K, Q, T = 5, 17, 257
    eng, pl = make_engine(factory, K, Q, T, tgaps=(17,), qgaps=(5,), **(F32 if f32 else {}))
    A, D, B = eng.get_kb()
    model = Model(A, D, (17,), (5,))
    rng = np.random.default_rng(5)
    free = [t for t in range(T) if t != 17]
    pairs = [[int(t) for t in rng.choice(free, size=2)] for _ in range(2 * CHUNK + 8)]
    triple = [int(t) for t in rng.choice(free, size=3)]
    alone = {}

    def check(groups, name):
        got = eng.eval_target_separation(groups)
        for i, g in enumerate(groups):
            if tuple(g) not in alone:
                alone[tuple(g)] = eng.eval_target_separation([g])[0].tobytes()
                within_bar((name, i), got[i], model.row(g), len(g), K)
            assert got[i].tobytes() == alone[tuple(g)], (name, i)
        listed = eng.list_separating_questions_batch(groups, 4)
        for i in range(len(groups)):
            assert listed[i] == listing_of_row(got[i], 4), (name, i)

    exact = pairs[:TILE_ENTRIES // 2]
    assert sum(len(g) for g in exact) == TILE_ENTRIES
    check(exact, "one tile exactly")
    check(exact[:-1] + [triple], "a single entry more")
    check([triple] + exact, "a whole group more")
    check([[int(t) for t in rng.choice(free, size=64)] for _ in range(5)] + pairs[:3], "groups of 64 over two tiles")
    check(pairs, "three chunks")
    assert len(pairs) > 2 * CHUNK
    eng.close()


def test_host_prefix_beyond_256_records(factory):
    """More than 256 questions and maxCount beyond 256: the rows are copied and the prefix is taken on the host, in the listing kernels' order."""
    K, Q, T = 2, 300, 33
    eng, pl = make_engine(factory, K, Q, T, tgaps=(6,), qgaps=(7, 299))
    A, D, B = eng.get_kb()
    groups = mixed_groups(T, pl, (6,))
    got = eng.eval_target_separation(groups)
    model = Model(A, D, (6,), (7, 299))
    for i in (0, 2, 7):
        within_bar(("q300", i), got[i], model.row(groups[i]), len(groups[i]), K)
    for max_count in (256, 257, 300, Q + 5):
        listed = eng.list_separating_questions_batch(groups, max_count)
        for i in range(len(groups)):
            assert listed[i] == listing_of_row(got[i], max_count), (max_count, i)
    assert len(eng.list_separating_questions(groups[3], 300)) > 256
    eng.close()


# ---- gaps in regular and in maintenance mode; nothing changes -------------------------------------------------------------------------------
def test_gaps_modes_and_no_side_effects(factory):
    K, Q, T = 5, 33, 65
    eng, pl = make_engine(factory, K, Q, T, tgaps=(3,), qgaps=(4,))
    groups = [[1, 2, 60], [1, 3, 60], [10, 11], list(pl.disjoint), [20, 21, 22, 23]]
    quiz = eng.start_quiz()
    eng.record_answer(quiz, 1) if eng.next_question(quiz) >= 0 else None
    kb0, priors0 = [x.tobytes() for x in eng.get_kb()], eng.get_priors(quiz).tobytes()
    rows = eng.eval_target_separation(groups)
    listed = eng.list_separating_questions_batch(groups, Q)
    assert [x.tobytes() for x in eng.get_kb()] == kb0 and eng.get_priors(quiz).tobytes() == priors0    # no KB byte, no quiz state
    assert not rows[1].any() and listed[1] == [] and rows[0].any()         # a gap member: a row of zeros, nothing listed
    assert not rows[:, 4].any() and all(4 not in [q for q, _ in lst] for lst in listed)   # a gap question: zero, never listed
    for i in range(len(groups)):
        assert listed[i] == listing_of_row(rows[i], Q)
    A, D, B = eng.get_kb()
    model = Model(A, D, (3,), (4,))
    for i, g in enumerate(groups):
        within_bar(("regular", i), rows[i], model.row(g), len(g), K)
    # a training enqueued earlier is ordered in front
    eng.train([AQ(6, 2), AQ(7, 0)], 10, 3.0)
    after = eng.eval_target_separation(groups)
    assert after[2, 6] != rows[2, 6] and after[0].tobytes() == rows[0].tobytes()      # target 10's column of question 6, and no other group's
    A, D, B = eng.get_kb()
    within_bar("after train", after[2], Model(A, D, (3,), (4,)).row(groups[2]), 2, K)
    eng.start_maintenance(True)
    assert eng.eval_target_separation(groups).tobytes() == after.tobytes()
    assert eng.list_separating_questions_batch(groups, 10) == [listing_of_row(r, 10) for r in after]
    eng.remove_targets([21])
    eng.remove_questions([8])
    rows2 = eng.eval_target_separation(groups)
    assert not rows2[4].any() and not rows2[:, 8].any() and not rows2[1].any() and not rows2[:, 4].any()
    expect = after.copy()
    expect[4], expect[:, 8] = 0.0, 0.0
    assert rows2.tobytes() == expect.tobytes()
    listed2 = eng.list_separating_questions_batch(groups, Q)
    assert listed2[4] == [] and listed2 == [listing_of_row(r, Q) for r in rows2]
    eng.finish_maintenance()
    assert eng.eval_target_separation(groups).tobytes() == rows2.tobytes()
    eng.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffers_untouched(factory):
    K, Q, T = 5, 33, 65
    eng, pl = make_engine(factory, K, Q, T, trains=0)
    lib = interop.load_library()
    p64, pd, prec = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(interop.CiRatedQuestion)
    counts = np.array([2, 3, 2], dtype=np.int64)
    ok = np.array([1, 2, 3, 4, 5, 6, 7], dtype=np.int64)
    out = np.full((3, Q), -7.0)
    rec = np.full(3 * 4 * 2, -7.0)
    n_out = np.full(3, -7, dtype=np.int64)
    calls0 = eng.get_option("separation_calls")

    def refused(err, code, *texts):
        assert err, texts
        s = interop.PqaError(err).to_string(True)
        assert s.startswith("[" + code + "]") and all(t in s for t in texts), s
        assert (out == -7.0).all() and (rec == -7.0).all() and (n_out == -7).all()

    e = eng.c_engine
    A = lambda a: a.ctypes.data_as(p64)
    arr = lambda *v: np.array(v, dtype=np.int64)
    R = rec.ctypes.data_as(prec)
    O = out.ctypes.data_as(pd)
    NEG, NULL, RANGE, DOWN = "The count is negative", "Expected non-null argument", "Index is out of range", "Object is shut(ting) down"
    ev, ls = lib.PqaEngine_EvalTargetSeparation, lib.PqaEngine_ListSeparatingQuestionsBatch
    refused(ev(e, -1, A(counts), A(ok), O, Q), NEG, "count=-1", "nGroups")
    refused(ev(e, 3, None, A(ok), O, Q), NULL)
    refused(ev(e, 3, A(counts), None, O, Q), NULL)
    refused(ev(e, 3, A(counts), A(ok), None, Q), NULL)
    refused(ev(e, 3, A(arr(2, 1, 2)), A(ok), O, Q), RANGE, "entry=1", "count=1")
    refused(ev(e, 3, A(arr(2, 3, 65)), A(np.zeros(70, dtype=np.int64)), O, Q), RANGE, "entry=2", "count=65")
    refused(ev(e, 3, A(counts), A(arr(1, 2, 3, 4, T, 6, 7)), O, Q), RANGE, "entry=1", "member=2", "targetId=%d" % T)
    refused(ev(e, 3, A(counts), A(arr(1, 2, 3, 4, 5, -1, 7)), O, Q), RANGE, "entry=2", "member=0", "targetId=-1")
    refused(ev(e, 3, A(counts), A(ok), O, Q - 1), RANGE, "subjIndex=%d" % (Q - 1))
    refused(ev(e, 3, A(counts), A(ok), O, Q + 1), RANGE, "subjIndex=%d" % (Q + 1))
    # the one order: a count before a target before the row length; a NULL before all of them; a negative count first
    refused(ev(e, 3, A(arr(2, 1, 2)), A(arr(T, 2, 3, 4, 5)), O, Q - 1), RANGE, "entry=1", "count=1")
    refused(ev(e, 3, A(counts), A(arr(1, 2, 3, 4, T, 6, 7)), O, Q - 1), RANGE, "targetId=%d" % T)
    refused(ev(e, 3, A(arr(2, 1, 2)), A(ok), None, Q), NULL)
    refused(ev(e, -3, None, None, None, Q), NEG, "count=-3")
    refused(ls(e, -2, A(counts), A(ok), 4, R, A(n_out)), NEG, "count=-2")
    refused(ls(e, 3, A(counts), A(ok), -4, R, A(n_out)), NEG, "count=-4")
    refused(ls(e, 3, None, A(ok), 4, R, A(n_out)), NULL)
    refused(ls(e, 3, A(counts), None, 4, R, A(n_out)), NULL)
    refused(ls(e, 3, A(counts), A(ok), 4, None, A(n_out)), NULL)
    refused(ls(e, 3, A(counts), A(ok), 4, R, None), NULL)
    refused(ls(e, 3, A(arr(2, 3, 0)), A(ok), 4, R, A(n_out)), RANGE, "entry=2", "count=0")
    refused(ls(e, 3, A(counts), A(arr(1, 2, 3, -5, 5, 6, 7)), 4, R, A(n_out)), RANGE, "entry=1", "member=1", "targetId=-5")
    assert eng.get_option("separation_calls") == calls0                      # nothing was accepted
    # maxCount 0 lists nothing and is no error, without a destination; the next good call is correct
    assert not ls(e, 3, A(counts), A(ok), 0, None, A(n_out)) and (n_out == 0).all()
    n_out[:] = -7
    groups = [[1, 2], [3, 4, 5], [6, 7]]
    rows = eng.eval_target_separation(groups)
    assert eng.list_separating_questions_batch(groups, 6) == [listing_of_row(r, 6) for r in rows]
    eng.set_option("time_sweeps", 1)
    ns0 = eng.get_option("separation_device_ns")
    eng.eval_target_separation(groups)
    ns1 = eng.get_option("separation_device_ns")
    eng.list_separating_questions_batch(groups, 3)
    assert eng.get_option("separation_device_ns") > ns1 > ns0
    eng.shutdown()
    refused(ev(e, 3, A(counts), A(ok), O, Q), DOWN, "RejectedOperation=EvalTargetSeparation")
    refused(ls(e, 3, A(counts), A(ok), 4, R, A(n_out)), DOWN, "RejectedOperation=ListSeparatingQuestionsBatch")
    refused(ev(e, 3, A(counts), A(ok), O, Q - 1), RANGE)                    # ... and the row length in front of it
    eng.close()


def test_one_process_sharded_engine_refuses(factory, monkeypatch):
    monkeypatch.setenv("PQA_DEVICES", "0,0")        # two shards side by side on the one device
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(5, 37, 101, init_amount=0.1))
    assert err is None and eng.get_option("shards") == 2
    lib = interop.load_library()
    p64 = ctypes.POINTER(ctypes.c_int64)
    counts, targets = np.array([2], dtype=np.int64), np.array([1, 2], dtype=np.int64)
    out = np.zeros(37)
    rec = (interop.CiRatedQuestion * 3)()
    n_out = np.zeros(1, dtype=np.int64)
    for err in (lib.PqaEngine_EvalTargetSeparation(eng.c_engine, 1, counts.ctypes.data_as(p64), targets.ctypes.data_as(p64), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 37),
                lib.PqaEngine_ListSeparatingQuestionsBatch(eng.c_engine, 1, counts.ctypes.data_as(p64), targets.ctypes.data_as(p64), 3, rec, n_out.ctypes.data_as(p64))):
        assert err and "Target separation is for whole engines" in interop.PqaError(err).to_string(True)
    eng.close()
