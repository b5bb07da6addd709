"""Question redundancy on the GPU (include/PqaHipExt.h: PqaEngine_EvalQuestionRedundancy, PqaEngine_ListRedundantQuestionsBatch;
redundancy_kernels.hip; hip_engine_sources.cpp).

The model works over get_kb(): with w = vB (0 at a gap target) and p = A * (1 / D), numpy forms the products (w p_sk)(t) p_qk'(t), math.fsum
adds each of the K x K table entries over the targets that are no gaps, and the formula
    I = sum over J > 0 of (J / Z) log2(J Z / (r c))
runs in Python floats.  The bar is derived, not measured, and ABSOLUTE (I is a difference of entropies and may be near 0): a table entry
carries about six roundings per term and T accumulations of non-negative terms, eps = (T + 16) 2^-52 relative; the three arguments of a
logarithm carry eps each, 3 eps / ln 2 weighted by J / Z (which sums to 1); an entry's own error is weighted by |log2| times the entry,
at most about 0.53 per entry: |gpu - model| <= (8 + K^2) (T + 16) 2^-52 bits.
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
TILE = {2: 8, 3: 4, 4: 4, 5: 2}   # sources a workgroup of the sweep takes per answer count (pqa_kernels.h: RedundancyTileWidth); 1 otherwise


def bar(K, T):
    return (8 + K * K) * (T + 16) * 2.0 ** -52


def planted(Q):
    """(source, bitwise copy, copy with permuted answer rows, independent question) of a cube with room for them"""
    s = Q // 2
    return s, s + 3, s - 3, Q - 2


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
    if plant and Q >= 17:
        A, D, B = eng.get_kb()
        s, copy, perm, ind = planted(Q)
        A[copy], D[copy] = A[s], D[s]
        A[perm], D[perm] = A[s][np.roll(np.arange(K), 1)], D[s]
        A[ind] = (np.arange(K) + 1.0)[:, None] * np.ones(T)   # the same answer distribution at every target
        D[ind] = A[ind].sum(axis=0)
        eng.set_kb(A, D, B)
    if tgaps:
        eng.set_target_gaps(list(tgaps))
    if qgaps:
        eng.set_question_gaps(list(qgaps))
    return eng


def info_bits(J):
    """the formula in Python floats; Z, r, c in index order, the sum in row-major order"""
    K = len(J)
    Z = 0.0
    for k in range(K):
        for j in range(K):
            Z += J[k][j]
    if not Z > 0:
        return 0.0
    r = [0.0] * K
    c = [0.0] * K
    for k in range(K):
        for j in range(K):
            r[k] += J[k][j]
    for j in range(K):
        for k in range(K):
            c[j] += J[k][j]
    out = 0.0
    for k in range(K):
        for j in range(K):
            if J[k][j] > 0:
                out += (J[k][j] / Z) * math.log2(J[k][j] * Z / (r[k] * c[j]))
    return out


class Model:
    """I(s, q) by the definition over one get_kb(); rows are computed once per source and kept."""

    def __init__(self, A, D, B, tgaps, qgaps, questions=None):
        self.Q, self.K, self.T = A.shape
        self.qgaps = set(qgaps)
        self.live = np.array([t for t in range(self.T) if t not in tgaps], dtype=np.int64)
        with np.errstate(all="ignore"):
            self.p = (A * (1.0 / D)[:, None, :])[:, :, self.live]
        self.w = B[self.live]
        self.questions = list(range(self.Q)) if questions is None else list(questions)
        self.rows = {}

    def row(self, s):
        if s not in self.rows:
            out = np.zeros(self.Q)
            if s not in self.qgaps:
                u = self.w * self.p[s]
                for q in self.questions:
                    if q in self.qgaps:
                        continue
                    prod = u[:, None, :] * self.p[q][None, :, :]
                    out[q] = info_bits([[math.fsum(prod[k, j]) for j in range(self.K)] for k in range(self.K)])
            self.rows[s] = out
        return self.rows[s]


WORST = {"bits": 0.0, "of_bar": 0.0}


def within_bar(name, got_row, ref_row, K, T, columns=None):
    cols = slice(None) if columns is None else list(columns)
    err = float(np.abs(got_row[cols] - ref_row[cols]).max())
    WORST["bits"], WORST["of_bar"] = max(WORST["bits"], err), max(WORST["of_bar"], err / bar(K, T))
    print("%s: worst deviation %.3g bits, bar %.3g (worst so far %.3g bits, %.3g of its bar)" % (name, err, bar(K, T), WORST["bits"], WORST["of_bar"]))
    assert err <= bar(K, T), (name, err, bar(K, T))


def listing_of_row(row, source, max_count, q_first=0):
    """what the listing must be, from the engine's own Eval row: not the source, value > 0 (gaps are 0), by (-value, id)"""
    ids = np.array([q for q in range(len(row)) if q_first + q != source and row[q] > 0], dtype=np.int64)
    if len(ids) == 0:
        return []
    take = np.lexsort((ids, -row[ids]))[:max_count]
    return [(int(q_first + q), float(row[q])) for q in ids[take]]


def source_lists(K, Q, qgaps):
    """1, 2, one tile, one tile + 1 and 33 sources: both ends, a gap source where there is one, a repeated id, the planted source"""
    tile = TILE.get(K, 1)
    rng = np.random.default_rng(11)
    base = [Q // 2, 0, Q - 1] + ([qgaps[0]] if qgaps else []) + [Q // 2]
    long = base + [int(q) for q in rng.integers(0, Q, size=33)]
    return [long[:n] for n in sorted({1, 2, tile, tile + 1, 33})]


# ---- rows against the model, listings against the rows --------------------------------------------------------------------------------
SHAPES = {
    "k2_q1_t2_one_live_target": dict(K=2, Q=1, T=2, tgaps=(1,)),
    "k2_q2_t63": dict(K=2, Q=2, T=63),
    "k3_q17_t64": dict(K=3, Q=17, T=64, tgaps=(0, 63), qgaps=(3,)),
    "k5_q33_t65": dict(K=5, Q=33, T=65, tgaps=(3, 64), qgaps=(5, 32)),
    "k7_q17_t255": dict(K=7, Q=17, T=255, tgaps=(254,), qgaps=(0,)),
    "k2_q33_t257": dict(K=2, Q=33, T=257, tgaps=(17,), qgaps=(1, 30)),
    "k3_q17_t1000": dict(K=3, Q=17, T=1000),
    "k5_q17_t1025": dict(K=5, Q=17, T=1025, tgaps=(1024,), qgaps=(16,)),
    "k5_q33_t2049": dict(K=5, Q=33, T=2049, tgaps=(0, 1000), qgaps=(2,)),
    "k2_q6_t16400_long_row": dict(K=2, Q=6, T=16400, tgaps=(16399,)),
    "f32_k2_q1_t2_one_live_target": dict(K=2, Q=1, T=2, tgaps=(1,), f32=True),
    "f32_k5_q33_t65": dict(K=5, Q=33, T=65, tgaps=(3, 64), qgaps=(5, 32), f32=True),
    "f32_k7_q17_t255": dict(K=7, Q=17, T=255, tgaps=(254,), qgaps=(0,), f32=True),
    "f32_k3_q17_t1000": dict(K=3, Q=17, T=1000, f32=True),
    "f32_k2_q33_t2049": dict(K=2, Q=33, T=2049, tgaps=(0, 1000), qgaps=(2,), f32=True),
    "f32_k2_q6_t16400_long_row": dict(K=2, Q=6, T=16400, tgaps=(16399,), f32=True),
}


def test_smallest_answer_count_is_two(factory):
    """K = 2 is the smallest answer count the engine accepts (and among the shapes): one answer is refused by the engine itself."""
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(1, 4, 8, init_amount=0.1))
    assert eng is None and "nAnswers=1 of 2" in err.to_string(True)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rows_and_listings(factory, name):
    sh = dict(SHAPES[name])
    K, Q, T, tgaps, qgaps = sh["K"], sh["Q"], sh["T"], sh.get("tgaps", ()), sh.get("qgaps", ())
    eng = make_engine(factory, K, Q, T, tgaps, qgaps, **(F32 if sh.get("f32") else {}))
    A, D, B = eng.get_kb()
    model = Model(A, D, B, tgaps, qgaps)
    if Q >= 17:   # the planted structure is there, in the model: a kernel that dropped targets could not hide under the absolute bar
        s, copy, perm, ind = planted(Q)
        assert model.row(s)[copy] > 0.1 and model.row(s)[perm] > 0.1 and model.row(s)[s] > 0.1, model.row(s)
        assert abs(model.row(s)[ind]) < bar(K, T)
        every = np.array([model.row(q) for q in range(Q)])
        assert (every > 1e-6).sum() * 4 >= Q * Q, (every > 1e-6).sum()
    lists = source_lists(K, Q, qgaps)
    first_rows = {}
    for sources in lists:
        calls0, swept0 = eng.get_option("redundancy_calls"), eng.get_option("redundancy_sources")
        got = eng.eval_question_redundancy(sources)
        assert got.shape == (len(sources), Q)
        assert eng.get_option("redundancy_calls") == calls0 + 1 and eng.get_option("redundancy_sources") == swept0 + len(sources)
        assert eng.eval_question_redundancy(sources).tobytes() == got.tobytes()   # the same call, the same bytes
        for i, s in enumerate(sources):
            within_bar((name, len(sources), i), got[i], model.row(s), K, T)
            # fixed: the row of a source is the same bytes wherever it stands, in a call of any length
            assert first_rows.setdefault(s, got[i].tobytes()) == got[i].tobytes(), (name, len(sources), i, s)
            if s in qgaps:
                assert not got[i].any()
        if qgaps:
            assert not got[:, list(qgaps)].any()
        for max_count in (0, 1, 10, 256, 300):
            listed = eng.list_redundant_questions_batch(sources, max_count)
            assert len(listed) == len(sources)
            for i, s in enumerate(sources):
                assert listed[i] == listing_of_row(got[i], s, max_count), (name, len(sources), max_count, i, s)
            if max_count == 10:
                assert eng.list_redundant_questions(sources[0], 10) == listed[0]
                assert eng.list_redundant_questions_batch(sources, 10) == listed
    assert eng.eval_question_redundancy([]).shape == (0, Q) and eng.list_redundant_questions_batch([], 5) == []
    if Q >= 17:
        s, copy, perm, ind = planted(Q)
        row = np.frombuffer(first_rows[s], dtype=np.float64)
        assert row[copy] == row[s]                                              # the bits of I(s, s)
        assert abs(row[perm] - model.row(s)[perm]) <= bar(K, T)
        top = eng.list_redundant_questions(s, 3)
        assert {q for q, _ in top[:2]} == {copy, perm} and top[0][1] >= top[1][1] > top[2][1], top   # the permuted copy: second only to exact copies
        assert (copy, row[s]) in top[:2]
        for sources in ([copy, s], [0, 1, perm, s, copy, 2, 3, 4, s], [s]):   # reordered, in other tiles, alone
            rows = eng.eval_question_redundancy(sources)
            for i, x in enumerate(sources):
                if x in (s, copy):
                    assert rows[i, copy] == row[s] and rows[i, s] == row[s], (sources, i)
    eng.close()


def test_host_prefix_beyond_256_records(factory):
    """More than 256 questions and maxCount 300: the rows are copied and the prefix is taken on the host, in the listing kernels' order."""
    K, Q, T = 2, 300, 63
    eng = make_engine(factory, K, Q, T, tgaps=(5,), qgaps=(7, 299), plant=False)
    A, D, B = eng.get_kb()
    sources = [150, 7, 0, 150, 299, 42, 298, 1, 77]
    got = eng.eval_question_redundancy(sources)
    model = Model(A, D, B, (5,), (7, 299))
    for i in (0, 2, 5):
        within_bar(("q300", i), got[i], model.row(sources[i]), K, T)
    for max_count in (256, 257, 300, 1000):
        listed = eng.list_redundant_questions_batch(sources, max_count)
        for i, s in enumerate(sources):
            assert listed[i] == listing_of_row(got[i], s, max_count), (max_count, i)
    assert len(eng.list_redundant_questions(150, 300)) > 256
    eng.close()


# ---- a training changes the rows; maintenance mode ------------------------------------------------------------------------------------
def test_train_then_maintenance(factory):
    K, Q, T = 5, 33, 65
    eng = make_engine(factory, K, Q, T)
    s, copy, perm, ind = planted(Q)
    before = eng.eval_question_redundancy([s])
    assert eng.list_redundant_questions(s, 1)[0][0] in (copy, perm)
    eng.train([AQ(copy, 2), AQ(7, 0)], 40, 3.0)       # on a listed question: the call behind it sees the new block
    after = eng.eval_question_redundancy([s])
    assert after[0, copy] != before[0, copy]
    A, D, B = eng.get_kb()
    within_bar("after train", after[0], Model(A, D, B, (), ()).row(s), K, T)
    assert eng.list_redundant_questions(s, 10) == listing_of_row(after[0], s, 10)
    eng.start_maintenance(True)
    in_maintenance = eng.eval_question_redundancy([s, copy])
    assert in_maintenance[0].tobytes() == after[0].tobytes()
    assert eng.list_redundant_questions(s, 10) == listing_of_row(after[0], s, 10)
    eng.remove_questions([copy])
    rows = eng.eval_question_redundancy([s, copy])
    assert rows[0, copy] == 0 and not rows[1].any()
    listed = eng.list_redundant_questions_batch([s, copy], Q)
    assert copy not in [q for q, _ in listed[0]] and listed[1] == []
    assert listed[0] == listing_of_row(rows[0], s, Q)
    eng.finish_maintenance()
    assert eng.eval_question_redundancy([s])[0].tobytes() == rows[0].tobytes()
    eng.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffers_untouched(factory):
    K, Q, T = 5, 33, 65
    eng = make_engine(factory, K, Q, T, trains=0)
    lib = interop.load_library()
    p64, pd, prec = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(interop.CiRatedQuestion)
    src = np.array([1, 2, Q], dtype=np.int64)
    ok = np.array([1, 2, 3], dtype=np.int64)
    out = np.full((3, Q), -7.0)
    rec = np.full(3 * 4 * 2, -7.0)
    counts = np.full(3, -7, dtype=np.int64)
    calls0 = eng.get_option("redundancy_calls")

    def refused(err, code, *texts):
        assert err, texts
        s = interop.PqaError(err).to_string(True)
        assert s.startswith("[" + code + "]") and all(t in s for t in texts), s
        assert (out == -7.0).all() and (rec == -7.0).all() and (counts == -7).all()

    e = eng.c_engine
    A = lambda a: a.ctypes.data_as(p64)
    R = rec.ctypes.data_as(prec)
    O = out.ctypes.data_as(pd)
    P = ctypes.c_void_p(16)
    NEG, NULL, RANGE = "The count is negative", "Expected non-null argument", "Index is out of range"
    refused(lib.PqaEngine_EvalQuestionRedundancy(e, -1, A(ok), O, Q), NEG, "count=-1")
    refused(lib.PqaEngine_EvalQuestionRedundancy(e, 3, None, O, Q), NULL)
    refused(lib.PqaEngine_EvalQuestionRedundancy(e, 3, A(ok), None, Q), NULL)
    refused(lib.PqaEngine_EvalQuestionRedundancy(e, 3, A(ok), O, Q - 1), RANGE, "subjIndex=%d" % (Q - 1))
    refused(lib.PqaEngine_EvalQuestionRedundancy(e, 3, A(src), O, Q), RANGE, "entry=2", "questionId=%d" % Q)
    refused(lib.PqaEngine_ListRedundantQuestionsBatch(e, -2, A(ok), 4, R, A(counts)), NEG, "count=-2")
    refused(lib.PqaEngine_ListRedundantQuestionsBatch(e, 3, A(ok), -4, R, A(counts)), NEG, "count=-4")
    refused(lib.PqaEngine_ListRedundantQuestionsBatch(e, 3, A(ok), 4, None, A(counts)), NULL)
    refused(lib.PqaEngine_ListRedundantQuestionsBatch(e, 3, A(ok), 4, R, None), NULL)
    refused(lib.PqaEngine_ListRedundantQuestionsBatch(e, 3, A(np.array([1, -1, 2], dtype=np.int64)), 4, R, A(counts)), RANGE, "entry=1", "questionId=-1")
    many = np.zeros(257, dtype=np.int64)
    refused(lib.PqaHip_PackQuestionWeights(e, 257, A(many), P, None, 0), RANGE, "Batch size is out of range.")
    refused(lib.PqaHip_PackQuestionWeights(e, -1, A(ok), P, None, 0), NEG)
    refused(lib.PqaHip_PackQuestionWeights(e, 3, A(ok), None, None, 0), NULL)
    refused(lib.PqaHip_PackQuestionWeights(e, 3, A(src), P, None, 0), RANGE, "entry=2", "questionId=%d" % Q)
    refused(lib.PqaEngine_EvalQuestionRedundancyFromWeights(e, 257, A(many), P, O, Q), RANGE, "Batch size is out of range.")
    refused(lib.PqaEngine_EvalQuestionRedundancyFromWeights(e, -1, A(ok), P, O, Q), NEG)
    refused(lib.PqaEngine_EvalQuestionRedundancyFromWeights(e, 3, A(ok), None, O, Q), NULL)
    refused(lib.PqaEngine_EvalQuestionRedundancyFromWeights(e, 3, A(ok), P, None, Q), NULL)
    refused(lib.PqaEngine_EvalQuestionRedundancyFromWeights(e, 3, A(ok), P, O, Q + 1), RANGE, "subjIndex=%d" % (Q + 1))
    refused(lib.PqaEngine_EvalQuestionRedundancyFromWeights(e, 3, A(src), P, O, Q), RANGE, "entry=2", "questionId=%d" % Q)
    refused(lib.PqaEngine_ListRedundantQuestionsFromWeights(e, 257, A(many), P, 4, R, A(counts)), RANGE, "Batch size is out of range.")
    refused(lib.PqaEngine_ListRedundantQuestionsFromWeights(e, 3, A(ok), None, 4, R, A(counts)), NULL)
    refused(lib.PqaEngine_ListRedundantQuestionsFromWeights(e, 3, A(ok), P, 4, R, None), NULL)
    refused(lib.PqaEngine_ListRedundantQuestionsFromWeights(e, 3, A(src), P, 4, R, A(counts)), RANGE, "entry=2", "questionId=%d" % Q)
    refused(lib.PqaEngine_ListRedundantQuestionsFromWeights(e, 3, A(ok), P, -1, R, A(counts)), NEG)
    assert eng.get_option("redundancy_calls") == calls0                      # nothing was accepted
    assert lib.PqaHip_QuestionWeightSlotBytes(e) == K * 80 * 8               # K rows of RoundLdT(65) = 80 doubles
    # maxCount 0 lists nothing and is no error, without a destination; the next good call is correct
    assert not lib.PqaEngine_ListRedundantQuestionsBatch(e, 3, A(ok), 0, None, A(counts)) and (counts == 0).all()
    row = eng.eval_question_redundancy([2])[0]
    assert eng.list_redundant_questions(2, 6) == listing_of_row(row, 2, 6)
    eng.set_option("time_sweeps", 1)
    ns0 = eng.get_option("redundancy_device_ns")
    eng.eval_question_redundancy([2, 3])
    assert eng.get_option("redundancy_device_ns") > ns0
    eng.close()


def test_shard_engine_names_the_from_weights_pair(factory):
    """An engine made as a shard (questions [10, 20) of 37) refuses the whole-engine pair and says what to call instead."""
    sh = factory.create_hip_engine(interop.EngineDefinition(5, 10, 65, init_amount=0.1), 10, 37, 0)
    calls0 = sh.get_option("redundancy_calls")
    for call in (lambda: sh.eval_question_redundancy([12]), lambda: sh.list_redundant_questions_batch([12], 3)):
        with pytest.raises(interop.PqaException, match=r"Not implemented.*PqaHip_PackQuestionWeights.*PqaEngine_EvalQuestionRedundancyFromWeights.*"
                                                       r"PqaEngine_ListRedundantQuestionsFromWeights"):
            call()
    assert sh.get_option("redundancy_calls") == calls0 and sh.question_weight_slot_bytes() == 5 * 80 * 8
    sh.close()


def test_one_process_sharded_engine_refuses(factory, monkeypatch):
    monkeypatch.setenv("PQA_DEVICES", "0,0")        # two shards side by side on the one device
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(5, 37, 101, init_amount=0.1))
    assert err is None and eng.get_option("shards") == 2
    for call in (lambda: eng.eval_question_redundancy([1]), lambda: eng.list_redundant_questions_batch([1], 3), lambda: eng.pack_question_weights([1], 16),
                 lambda: eng.eval_question_redundancy_from_weights([1], 16), lambda: eng.list_redundant_questions_from_weights([1], 16, 3)):
        with pytest.raises(interop.PqaException, match=r"Not implemented.*Question redundancy is for whole engines"):
            call()
    assert eng.question_weight_slot_bytes() == -1
    eng.close()
