"""Question pages across separately created shards (PqaHip_PackGivenBlocks, PqaEngine_EvalConditionalGainsBatchFromBlocks,
PqaHip_SelectPageStepFromBlocks called on the shards directly).  One process: the shards of one synthetic KB sit side by side on the one
device as create_hip_engine(def, q_first, Q, 0) engines, one whole engine holds the same KB, and every engine holds the same quizzes
(the shards record through posterior packages, as tests/test_gpu_question_gains_ranks.py does).  The given questions' blocks travel
in a block package that the owners fill; a shard builds the branch rows from it and sweeps its own questions.  The shards run
exactly the whole engine's arithmetic on the same bits, so the bar is EQUALITY and there is no tolerance: the shards' Eval rows side
by side are the whole engine's bytes, and the pages driven step by step through dist.merge_page_step are the whole engine's pages
record for record, ids and bits."""
import ctypes
import mmap

import numpy as np
import pytest
import torch

from probqa_amd import dist as pdist
from probqa_amd import interop
from test_gpu_question_gains import F32

pytestmark = pytest.mark.gpu

P64, PD, PSEL = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(interop.CiHipSelection)
N_QUIZZES = 4
TGAPS, QGAPS = (3, 17, 100), (0, 5, 36)
CASES = {
    "two_k5_t101": dict(bounds=pdist.shard_bounds(37, 2), K=5, T=101),                                    # odd T, the last target a gap
    "three_k5_t101": dict(bounds=pdist.shard_bounds(37, 3), K=5, T=101),
    "three_k7_t257_one_question": dict(bounds=[18, 19, 37], K=7, T=257),        # a one-question shard; answers in pieces; 7^2 = 49 rows
    "three_k5_t101_one_gap_question": dict(bounds=[1, 20, 37], K=5, T=101),     # the first shard holds question 0 alone, a gap
    "two_k2_t257_float": dict(bounds=pdist.shard_bounds(37, 2), K=2, T=257, f32=True, depth=4),            # the four-element tail; deep sets
    "two_q6_k5_t4099": dict(bounds=[3, 6], K=5, T=4099, qgaps=(5,)),                                      # a row longer than one pass
    "two_q6_k5_t4099_float": dict(bounds=[3, 6], K=5, T=4099, qgaps=(5,), f32=True),
    "two_k5_t101_grown_to_131": dict(bounds=pdist.shard_bounds(37, 2), K=5, T=101, grow=30, tgaps=(3, 17, 130)),   # the allocation's pitch is not the slot's
}


def engine_of(first, limit, Q, K, T, f32, tgaps, qgaps, grow=0):
    eng = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1, **(F32 if f32 else {})), first, Q, 0)
    eng.fill_synthetic(8.0, 0.5, 5)       # (the same seed on every shard: each fills its part of the one cube)
    if grow:                              # replicated maintenance: every engine adds the same targets
        eng.start_maintenance(False)
        eng.add_qs_ts([], [interop.AddTargetParam(0.25 + 0.125 * (i % 3)) for i in range(grow)])
        eng.finish_maintenance()
        assert eng.copy_dims().n_targets == T + grow
    eng.set_target_gaps(list(tgaps))
    eng.set_question_gaps(list(qgaps))    # (global ids: every rank is told of all of them)
    eng.set_option("workers", 16)
    return eng


class Ranks:
    """The whole engine, the shards, and the same quizzes on all of them: quiz i has taken i of three rounds of answers."""

    def __init__(self, case, twins=False):
        c = CASES[case]
        self.bounds, self.K, self.T, self.f32 = c["bounds"], c["K"], c["T"] + c.get("grow", 0), c.get("f32", False)
        self.Q, self.qgaps, self.depth = self.bounds[-1], c.get("qgaps", QGAPS), c.get("depth", 3 if c["K"] <= 5 else 2)
        self.firsts = [0] + self.bounds[:-1]
        make = lambda f, b: engine_of(f, b, self.Q, c["K"], c["T"], self.f32, c.get("tgaps", TGAPS), self.qgaps, c.get("grow", 0))
        self.whole = make(0, self.Q)
        self.shards = [make(f, b) for f, b in zip(self.firsts, self.bounds)]
        self.twins = [make(f, b) for f, b in zip(self.firsts, self.bounds)] if twins else []
        self.slot = self.whole.question_block_slot_bytes()
        assert all(sh.question_block_slot_bytes() == self.slot for sh in self.shards)
        self.quizzes = self.whole.start_quiz_batch(N_QUIZZES)
        for sh in self.shards + self.twins:
            assert sh.start_quiz_batch(N_QUIZZES) == self.quizzes
        self.asked = [set() for _ in self.quizzes]
        for r in range(3):
            part = [i for i in range(N_QUIZZES) if i > r]
            questions = []
            for i in part:                # the questions cross the ranks; no gap, nothing a quiz has answered before
                q = (8 + 11 * i + 13 * r) % self.Q
                while q in self.qgaps or q in self.asked[i]:
                    q = (q + 1) % self.Q
                questions.append(q)
                self.asked[i].add(q)
            ids, answers = [self.quizzes[i] for i in part], [(i + r) % self.K for i in part]
            for e in [self.whole] + self.shards + self.twins:
                for quiz, q in zip(ids, questions):
                    e.set_active_question(quiz, q)
            self.whole.record_answer_batch(ids, answers)
            for group in (self.shards, self.twins):
                if not group:
                    continue
                pkg = torch.zeros(len(ids), group[0].posterior_slot_bytes() // 8, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                for sh in group:
                    sh.pack_answer_posteriors(ids, answers, pkg.data_ptr())
                for sh in group:
                    sh.synchronize()
                for sh in group:
                    sh.record_answer_batch_from_posteriors(ids, answers, pkg.data_ptr())
        self.priors = [self.whole.get_priors(quiz).tobytes() for quiz in self.quizzes]
        self.check_priors()

    def check_priors(self):
        for sh in self.shards:
            assert [sh.get_priors(quiz).tobytes() for quiz in self.quizzes] == self.priors

    def owner(self, q):
        return pdist.owner_in(self.bounds, q)

    def free(self, shard, n, taken=()):
        """up to n questions of the shard that are no gaps, cycled where it has fewer ([] where it has none)"""
        mine = [q for q in range(self.firsts[shard], self.bounds[shard]) if q not in self.qgaps and q not in taken]
        return [mine[i % len(mine)] for i in range(n)] if mine else []

    def package(self, slots):
        """a zero-filled package with the given questions' blocks, each packed by its owner: what the all-reduce hands every rank"""
        pkg = self.zeros(len(slots))
        self.pack_into(pkg, slots)
        return pkg

    def zeros(self, n_slots):
        return torch.zeros(max(n_slots, 1), self.slot // (4 if self.f32 else 8), dtype=torch.float32 if self.f32 else torch.float64, device="cuda")

    def pack_into(self, view, questions):
        torch.cuda.synchronize()
        for sh in self.shards:
            sh.pack_given_blocks(questions, view.data_ptr())
        for sh in self.shards:
            sh.synchronize()

    def poisoned(self, pkg, slots, shard):
        """the package with the slots of the shard's own questions overwritten by NaN: they must not be read"""
        bad = pkg.clone()
        for i, q in enumerate(slots):
            if self.owner(q) == shard:
                bad[i] = float("nan")
        torch.cuda.synchronize()
        return bad

    def page(self, quizzes, page_size, given, poison=False):
        """dist.list_question_page_batch's loop without a process group: the picks per quiz, and what was packed per step"""
        sets, pages, active, slots, packed = [list(s) for s in given], [[] for _ in quizzes], list(range(len(quizzes))), [], []
        pkg = self.zeros(len(pdist._distinct(sets)) + len(quizzes) * max(page_size - 1, 0))
        for _ in range(page_size):
            if not active:
                break
            new = pdist._distinct([sets[i] for i in active], slots)
            if new:
                self.pack_into(pkg[len(slots):len(slots) + len(new)], new)
                slots.extend(new)
            packed.append(new)
            records = []
            for r, sh in enumerate(self.shards):
                use = self.poisoned(pkg, slots, r) if poison else pkg
                records.append(sh.select_page_step_from_blocks([quizzes[i] for i in active], [sets[i] for i in active], slots, use.data_ptr()))
            still = []
            for i, (q, bits) in zip(active, pdist.merge_page_step(records)):
                if q >= 0:
                    pages[i].append((q, bits))
                    sets[i].append(q)
                    still.append(i)
            active = still
        return pages, packed

    def close(self):
        for e in [self.whole] + self.shards + self.twins:
            e.close()


def bits_of(pages):
    return [[(q, np.float64(b).tobytes()) for q, b in page] for page in pages]


@pytest.mark.parametrize("case", sorted(CASES))
def test_shards_return_the_whole_engines_bits(case):
    rk = Ranks(case)
    whole, shards, quizzes, depth = rk.whole, rk.shards, rk.quizzes, rk.depth
    last = len(shards) - 1
    a, z = rk.free(min(r for r in range(len(shards)) if rk.free(r, 1)), 1)[0], rk.free(last, 1)[0]
    assert rk.owner(a) != rk.owner(z)
    one_rank = rk.free(last, depth)
    # ---- Eval: sets of 0 .. depth questions -- members on different ranks, all on one rank, a duplicate member, a quiz listed twice
    batch = quizzes + [quizzes[2], quizzes[1]]
    sets = [[], [a], [a, z, rk.free(0 if rk.free(0, 1) else 1, 2)[-1]][:depth], one_rank, [z, z], ([z, a] + one_rank)[:depth]]
    assert max(len(s) for s in sets) == depth and len(sets) == len(batch)
    want = whole.eval_conditional_gains_batch(batch, sets)
    assert want.shape == (len(batch), rk.Q) and (want > 1e-9).sum() >= len(batch) * (rk.Q - len(rk.qgaps)) // 2 and not want[:, list(rk.qgaps)].any()
    slots = pdist._distinct(sets)
    pkg = rk.package(slots)
    calls0 = [sh.get_option("page_calls") for sh in shards]
    parts = [sh.eval_conditional_gains_batch_from_blocks(batch, sets, slots, pkg.data_ptr()) for sh in shards]
    assert [p.shape for p in parts] == [(len(batch), b - f) for f, b in zip(rk.firsts, rk.bounds)]
    assert np.concatenate(parts, axis=1).tobytes() == want.tobytes()
    assert [sh.get_option("page_calls") for sh in shards] == [c + 1 for c in calls0]
    # the slots a shard holds itself are not read
    for r, sh in enumerate(shards):
        bad = rk.poisoned(pkg, slots, r)
        assert sh.eval_conditional_gains_batch_from_blocks(batch, sets, slots, bad.data_ptr()).tobytes() == parts[r].tobytes(), r
    # the empty set: the shard's own gains, without a package; and a whole engine without a package: the plain call
    for sh in shards:
        assert sh.eval_conditional_gains_batch_from_blocks(batch, [[]] * len(batch)).tobytes() == sh.eval_question_gains_batch(batch).tobytes()
    assert whole.eval_conditional_gains_batch_from_blocks(batch, sets).tobytes() == want.tobytes()
    # ---- pages of 1 .. 3, step by step: fresh and advanced quizzes, empty and non-empty given sets
    limit = {2: 8, 5: 3, 7: 2}[rk.K]      # nAnswers^(|S| + page - 1) <= 256
    for page_size in (1, 2, 3):
        for given in ([[] for _ in quizzes], [[a], [], [z, a][:max(limit - page_size + 1, 0)], [z]]):
            if max(len(s) for s in given) + page_size - 1 > limit:
                given = [s[:max(limit - page_size + 1, 0)] for s in given]
            want_pages = whole.list_question_page_batch(quizzes, page_size, given)
            got, packed = rk.page(quizzes, page_size, given)
            assert bits_of(got) == bits_of(want_pages), (case, page_size, given)
            assert all(len(set(p)) == len(p) for p in packed) and len(set(q for p in packed for q in p)) == sum(len(p) for p in packed)
            if page_size == 3:
                assert bits_of(rk.page(quizzes, page_size, given, poison=True)[0]) == bits_of(want_pages)
            for i, page in enumerate(want_pages if page_size == 2 else []):   # a step's bits are the Eval form's for the prefix before it
                prefix = list(given[i])
                for q, b in page[:2]:
                    r = rk.owner(q)
                    s = pdist._distinct([prefix])
                    row = shards[r].eval_conditional_gains_batch_from_blocks([quizzes[i]], [prefix], s, rk.package(s).data_ptr())[0]
                    assert np.float64(row[q - rk.firsts[r]]).tobytes() == np.float64(b).tobytes()
                    prefix.append(q)
    if rk.Q == 6:                          # a page larger than the candidates stops at the same length
        want_pages = whole.list_question_page_batch(quizzes, 3, None)
        assert len(want_pages[3]) == rk.Q - len(rk.qgaps) - len(rk.asked[3]) < 3
        assert bits_of(rk.page(quizzes, 3, [[] for _ in quizzes])[0]) == bits_of(want_pages)
    rk.check_priors()
    rk.close()


@pytest.mark.parametrize("server", [0, 1])
def test_the_calls_change_no_quiz_state(server):
    rk = Ranks("two_k5_t101", twins=True)
    for e in rk.shards + rk.twins:
        e.set_option("server", server)
    quizzes = rk.quizzes
    everything = [list(range(rk.Q)) for _ in quizzes]

    def state(sh):
        return ([sh.get_priors(z).tobytes() for z in quizzes], [[(x.i_question, x.i_answer) for x in sh.get_quiz_answers(z)] for z in quizzes],
                [sh.get_active_question_id(z) for z in quizzes], sh.select_argmax_among_batch(quizzes, everything).tobytes())

    before = [state(sh) for sh in rk.shards]
    assert before == [state(sh) for sh in rk.twins]
    sets = [[30], [2, 30], [], [20, 2]]
    slots = pdist._distinct(sets)
    pkg = rk.package(slots)
    for sh in rk.shards:
        sh.eval_conditional_gains_batch_from_blocks(quizzes, sets, slots, pkg.data_ptr())
    rk.page(quizzes, 2, sets[:2] + [[], []])
    assert [state(sh) for sh in rk.shards] == before
    for sh, twin in zip(rk.shards, rk.twins):        # the next selection is what it would have been
        for z in quizzes:
            assert sh.next_question_argmax(z) == twin.next_question_argmax(z)
    # the package in registered host memory is staged (option rows_stage), the needed slots only, and gives the same bits
    sh = rk.shards[0]
    want = sh.eval_conditional_gains_batch_from_blocks(quizzes, sets, slots, pkg.data_ptr())
    image = pkg.cpu().numpy().tobytes()
    seg = mmap.mmap(-1, len(image))
    seg.write(image)
    address = ctypes.addressof(ctypes.c_char.from_buffer(seg))
    dev = interop.host_register(address, len(image))
    try:
        for stage in (1, 0):
            sh.set_option("rows_stage", stage)
            staged0 = sh.get_option("rows_staged")
            assert sh.eval_conditional_gains_batch_from_blocks(quizzes, sets, slots, dev).tobytes() == want.tobytes()
            assert sh.get_option("rows_staged") - staged0 == stage
    finally:
        sh.synchronize()
        interop.host_unregister(address)
    # the counters: the new calls count as page calls, the pack as a pack
    sh.set_option("time_sweeps", 1)
    c0, z0, ns0, head0, p0, b0 = (sh.get_option(n) for n in ("page_calls", "page_quizzes", "page_device_ns", "page_head_ns", "pack_calls", "pack_bytes"))
    sh.select_page_step_from_blocks(quizzes, sets, slots, pkg.data_ptr())
    sh.pack_given_blocks([2, 30], pkg.data_ptr())    # (question 2 is this shard's, question 30 is not)
    sh.synchronize()
    assert sh.get_option("page_calls") == c0 + 1 and sh.get_option("page_quizzes") == z0 + len(quizzes)
    assert sh.get_option("page_device_ns") - ns0 > sh.get_option("page_head_ns") - head0 > 0
    assert sh.get_option("pack_calls") == p0 + 1 and sh.get_option("pack_bytes") == b0 + rk.slot
    rk.close()


# ---- refusals, each through the raw call so that the text is seen -------------------------------------------------------------------
def raw(eng, call, quizzes, given, named, blocks, slot_bytes, n=None):
    lib = interop.load_library()
    qs = np.ascontiguousarray(list(quizzes), dtype=np.int64)
    counts = np.ascontiguousarray([len(s) for s in given] + [0], dtype=np.int64)
    ids = np.ascontiguousarray([q for s in given for q in s] + [0], dtype=np.int64)
    names = np.ascontiguousarray(list(named) + [0], dtype=np.int64)
    head = (eng.c_engine, len(qs), qs.ctypes.data_as(P64), counts.ctypes.data_as(P64), ids.ctypes.data_as(P64), len(named), names.ctypes.data_as(P64),
            ctypes.c_void_p(blocks or None), slot_bytes)
    if call == "eval":
        n = eng.get_option("local_questions") if n is None else n
        out = np.zeros((len(qs), max(n, 1)))
        err = lib.PqaEngine_EvalConditionalGainsBatchFromBlocks(*head, out.ctypes.data_as(PD), n)
    else:
        out = (interop.CiHipSelection * max(len(qs), 1))()
        err = lib.PqaHip_SelectPageStepFromBlocks(*head, out)
    return interop.PqaError(err).to_string(True) if err else None


@pytest.mark.parametrize("call", ["eval", "step"])
def test_refusals(call):
    rk = Ranks("two_k5_t101")
    sh, quizzes, slot = rk.shards[0], rk.quizzes, rk.slot     # questions [0, 19) of 37
    slots = [30, 2, 25]
    pkg = rk.package(slots)
    ptr = pkg.data_ptr()
    before = [sh.get_option(n) for n in ("page_calls", "page_quizzes")]
    assert raw(sh, call, quizzes[:2], [[30], [2]], slots, ptr, slot) is None
    before[0], before[1] = before[0] + 1, before[1] + 2
    text = raw(sh, call, quizzes[:2], [[30], [2]], slots, ptr, slot + 128)
    assert text and "Index is out of range" in text and "slotBytes=%d of %d" % (slot + 128, slot) in text, text
    text = raw(sh, call, quizzes[:3], [[2], [30, 31], []], slots, ptr, slot)                     # question 31 is another shard's and not named
    assert text and "Index is out of range" in text and "entry=1" in text and "questionId=31" in text and "block package" in text, text
    text = raw(sh, call, quizzes[:2], [[2], [30]], slots, 0, slot)
    assert text and "Expected non-null argument" in text, text
    assert raw(sh, call, quizzes[:2], [[2], [7]], slots, 0, slot) is None                        # its own questions alone need no package
    before[0], before[1] = before[0] + 1, before[1] + 2
    for gap in (5, 36):                                                                          # its own gap, and another shard's
        text = raw(sh, call, quizzes[:2], [[2], [gap]], slots + [36], ptr, slot)
        assert text and "Index is out of range" in text and "entry=1 questionId=%d" % gap in text and "gap" in text, text
    text = raw(sh, call, quizzes[:2], [[2], [37]], slots, ptr, slot)
    assert text and "entry=1 questionId=37" in text and "out of range" in text, text
    text = raw(sh, call, quizzes[:2], [[2], [2, 30, 25, 2]], slots, ptr, slot)                   # 5^4 rows
    assert text and "Index is out of range" in text and "entry=1 branches=>256" in text, text
    # the plain call's refusals come first: a wrong slot size behind too many branches is not reached
    text = raw(sh, call, quizzes[:2], [[2], [2, 30, 25, 2]], slots, ptr, slot + 128)
    assert text and "branches=" in text and "slotBytes" not in text, text
    text = raw(sh, call, [quizzes[0], 12345], [[2], [30]], slots, ptr, slot)
    assert text and "entry=1 quizId=12345" in text, text
    if call == "eval":
        text = raw(sh, call, quizzes[:1], [[2]], slots, ptr, slot, n=37)                         # the row length is the LOCAL question count
        assert text and "Index is out of range" in text, text
    # the plain calls still refuse a shard
    for plain in (lambda: sh.eval_conditional_gains_batch(quizzes[:1], [[2]]), lambda: sh.list_question_page_batch(quizzes[:1], 2)):
        with pytest.raises(interop.PqaException, match="Question pages need the given questions' blocks"):
            plain()
    assert [sh.get_option(n) for n in ("page_calls", "page_quizzes")] == before                  # a refused call counts nothing
    # PqaHip_PackGivenBlocks: a gap -- this shard's or another's --, out of range, and maintenance mode
    for gap in (5, 36):
        with pytest.raises(interop.PqaException, match=r"questionId=%d" % gap):
            sh.pack_given_blocks([2, gap], ptr)
    with pytest.raises(interop.PqaException, match=r"questionId=40"):
        sh.pack_given_blocks([2, 40], ptr)
    # a whole engine with NULL blocks is the plain call
    sets = [[30, 2], [25]]
    assert rk.whole.eval_conditional_gains_batch_from_blocks(quizzes[:2], sets).tobytes() == rk.whole.eval_conditional_gains_batch(quizzes[:2], sets).tobytes()
    step = rk.whole.select_page_step_from_blocks(quizzes[:2], sets)
    want = rk.whole.list_question_page_batch(quizzes[:2], 1, sets)
    assert [(int(q), np.float64(b).tobytes()) for b, q in step] == [(p[0][0], np.float64(p[0][1]).tobytes()) for p in want]
    rk.check_priors()
    with pytest.raises(interop.PqaException, match="maintenance-only"):
        sh.pack_question_blocks([2], ptr)            # the maintenance-mode pack keeps its rule ...
    sh.start_maintenance(True)
    with pytest.raises(interop.PqaException, match="regular-only"):
        sh.pack_given_blocks([2], ptr)               # ... and this one is for regular mode
    text = raw(sh, call, quizzes[:1], [[2]], slots, ptr, slot)
    assert text and "regular-only" in text, text
    sh.finish_maintenance()
    rk.close()
