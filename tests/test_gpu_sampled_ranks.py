"""The sampled selector across separately created shards on a real MI355X (PqaHip_PackSampledParts, PqaHip_SampledPickFromParts,
PqaEngine_TakeSampledPicks).  One process: the shards of one KB sit side by side on the one device as create_hip_engine(def, q_first,
Q, 0) engines with one whole engine beside them; every shard packs its parts into its row of one device tensor -- what an all-gather
would deliver -- and every shard picks from all of them.

Held to: select_py over the concatenation of the shards' own eval_priorities_batch output (exact, for every random number), the
plain-Python model of the part (tests/sampled_ranks_common.py), the whole engine's next_question_sampled_batch and the oracle (the
seeded draws are guarded on the input side: tests/test_sampled_ranks_abi.py checks them without a GPU)."""
import functools

import numpy as np
import pytest
import torch

import cases
import sampled_batch_common as sb
import sampled_ranks_common as sr
from probqa_amd import dist as pdist
from probqa_amd import interop

pytestmark = pytest.mark.gpu

F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)
DEVICE = torch.device("cuda", 0)


class World:
    """A whole engine and the shards that end at `bounds`, all holding `kb`; quizzes are kept in step on all of them."""

    def __init__(self, factory, K, Q, T, kb, bounds, option, qgaps=(), tgaps=(), f32=False):
        self.K, self.Q, self.bounds, self.qgaps = K, Q, list(bounds), list(qgaps)
        self.n_sub = sr.n_sub_of(option)
        self.firsts = [0] + self.bounds[:-1]
        A, D, B = kb
        self.engines = []
        for first, limit in [(0, Q)] + list(zip(self.firsts, self.bounds)):
            eng = factory.create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1, **(F32 if f32 else {})), first, Q, 0)
            eng.set_kb(A[first:limit], D[first:limit], B)
            eng.set_option("workers", cases.WORKERS)
            eng.set_option("eval_subtasks", option)
            if tgaps:
                eng.set_target_gaps(list(tgaps))
            if qgaps:
                eng.set_question_gaps(list(qgaps))
            self.engines.append(eng)
        self.whole, self.shards = self.engines[0], self.engines[1:]
        self.answers = {}            # quiz -> [(question, answer)]
        assert len({e.sampled_part_bytes() for e in self.engines}) == 1
        self.words = self.whole.sampled_part_bytes() // 8
        assert self.words * 8 == sr.layout(Q, self.n_sub)[5]

    def set_form(self, form):
        for e in self.engines:
            e.set_option("batch_form", form)

    def start(self, n):
        ids = [e.start_quiz_batch(n) for e in self.engines]
        assert all(i == ids[0] for i in ids)
        for q in ids[0]:
            self.answers[q] = []
        return ids[0]

    def answer(self, quiz, question, answer):
        """RecordAnswer on the whole engine and the owner, RecordAnswerRemote elsewhere with the owner's posterior copied."""
        owner = pdist.owner_in(self.bounds, question)
        for e in self.engines:
            e.set_active_question(quiz, question)
        self.whole.record_answer(quiz, answer)
        for r, sh in enumerate(self.shards):
            (sh.record_answer if r == owner else sh.record_answer_remote)(quiz, answer)
        self.shards[owner].synchronize()
        src, ld = self.shards[owner].prior_device_ptr(quiz)
        for r, sh in enumerate(self.shards):
            if r != owner:
                dst, _ = sh.prior_device_ptr(quiz)
                pdist.tensor_from_device_ptr(dst, ld, DEVICE).copy_(pdist.tensor_from_device_ptr(src, ld, DEVICE))
        torch.cuda.synchronize()
        self.answers[quiz].append((question, answer))

    def skip(self, quiz):
        out = [False] * self.Q
        for q in self.qgaps + [q for q, _ in self.answers[quiz]]:
            out[q] = True
        return out

    def pack(self, ids, shards=None):
        """Every shard's parts in its row of one tensor [world, n, words]: the all-gather's output."""
        shards = self.shards if shards is None else shards
        parts = torch.zeros(len(shards), len(ids), self.words, dtype=torch.int64, device=DEVICE)
        torch.cuda.synchronize()
        for r, sh in enumerate(shards):
            sh.pack_sampled_parts(ids, parts[r].data_ptr())
        for sh in shards:
            sh.synchronize()
        return parts

    def close(self):
        for e in self.engines:
            e.close()


def case_world(factory, case, bounds, option):
    return World(factory, case.K, case.Q, case.T, case.kb(), bounds, option, qgaps=case.qgaps, tgaps=case.tgaps)


def scripted_quizzes(w, case, n):
    """n quizzes; quiz j has the first j % (len(answers) + 1) answers of the case's script applied."""
    ids = w.start(n)
    steps = len(case.answers) + 1
    for j, quiz in enumerate(ids):
        for q, a in case.answers[:j % steps]:
            w.answer(quiz, q, a)
    return ids


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """The config's guarded draws and, per step, the oracle's question for the edge numbers and the draws -- computed once."""
    _, case, option, _ = next(c for c in sr.gpu_configs() if c[0] == name)
    n_sub = sr.n_sub_of(option)
    _, rnds, _ = sr.guarded_draws(case, n_sub)
    steps = len(case.answers) + 1
    lists = [[r] * steps for r in sb.EDGE_RNDS] + [rnds]
    return rnds, sr.oracle_picks(case, n_sub, lists)


def check_batch(w, ids, rnds, label, want_questions=None):
    """One selection for the batch on the shards and on the whole engine: (a), (b), the parts against the model, the fallback, (f);
    with want_questions (guarded draws and edge numbers) also (c).  Returns the questions."""
    n, world = len(ids), len(w.shards)
    counts = [b - f for f, b in zip(w.firsts, w.bounds)]
    pri = np.concatenate([sh.eval_priorities_batch(ids, m) for sh, m in zip(w.shards, counts)], axis=1)
    parts = w.pack(ids)
    raw = parts.cpu().numpy()
    model = []
    for i, quiz in enumerate(ids):
        skip = w.skip(quiz)
        model.append(sr.parts_of(pri[i].tolist(), skip, w.n_sub, w.bounds))
        for r in range(world):     # the part the kernel wrote is the model's part of the same priorities, bit for bit
            got = sr.parse_part(raw[r, i].tobytes(), w.Q, w.n_sub)
            assert (got["q_first"], got["n"]) == (w.firsts[r], counts[r]) and got["seq"] > 0, (label, r, i)
            assert np.array_equal(np.array(got["total"]).view(np.int64), np.array(model[i][r]["total"]).view(np.int64)), (label, r, i, "totals")
            assert len(got["pieces"]) == len(model[i][r]["pieces"]), (label, r, i)
            for (s, p, k), (ms, mp, mk) in zip(got["pieces"], model[i][r]["pieces"]):
                assert s == ms and k == mk and np.array_equal(np.array(p).view(np.int64), np.array(mp).view(np.int64)), (label, r, i, s)
    per_rank = [sh.sampled_pick_from_parts(ids, rnds, parts.data_ptr(), r, world) for r, sh in enumerate(w.shards)]
    merged = pdist.merge_sampled_picks([[int(x) for x in p[:, 1]] for p in per_rank])
    quot, rem = sr.layout(w.Q, w.n_sub)[:2]
    for i, quiz in enumerate(ids):
        skip = w.skip(quiz)
        want = sb.select_py(pri[i].tolist(), skip, w.n_sub, rnds[i])
        assert merged[i] == want, (label, i, hex(rnds[i]), [int(p[i, 1]) for p in per_rank], want)               # (a)
        tot = sr.pick_from_parts(model[i], w.Q, w.n_sub, rnds[i], 0)[0]
        for r in range(world):                                                                                   # (b)
            assert int(per_rank[r][i, 1]) in (want, -1) and np.float64(per_rank[r][i, 0]).view(np.int64) == np.float64(tot).view(np.int64), (label, i, r)
            assert int(per_rank[r][i, 1]) == sr.pick_from_parts(model[i], w.Q, w.n_sub, rnds[i], r)[1], (label, i, r)
            if any(sr.subtask_range(s, quot, rem)[0] <= want < sr.subtask_range(s, quot, rem)[1] for s, _, _ in model[i][r]["pieces"]):
                assert int(per_rank[r][i, 1]) == want, (label, i, r)
    before = [e.get_total_questions_asked() for e in w.engines]
    taken = [sh.take_sampled_picks(ids, merged) for sh in w.shards]
    expect = [sr.take_py(m, w.Q, {q for q, s in enumerate(w.skip(quiz)) if s}) for m, quiz in zip(merged, ids)]
    assert all(t == expect for t in taken), (label, taken, expect)
    whole = w.whole.next_question_sampled_batch(ids, rnds)
    if want_questions is not None:
        assert expect == whole == want_questions, (label, expect, whole, want_questions)                          # (c)
    for e, b in zip(w.engines, before):                                                                           # (f)
        assert e.get_total_questions_asked() - b == sum(q >= 0 for q in (whole if e is w.whole else expect)), label
    for quiz, q in zip(ids, expect):
        if q >= 0:
            assert [e.get_active_question_id(quiz) for e in (w.engines if want_questions is not None else w.shards)] == [q] * (world + (want_questions is not None)), (label, quiz)
    return expect


CONFIGS = [(name, k) for name, _, _, every in sr.gpu_configs() for k in range(len(every))]


@pytest.mark.parametrize("name,k", CONFIGS, ids=lambda v: str(v))
def test_shards_select_what_the_whole_engine_selects(name, k, factory):
    _, case, option, every = next(c for c in sr.gpu_configs() if c[0] == name)
    bounds = every[k]
    draws, oracle = oracle_of(name)
    steps = len(case.answers) + 1
    w = case_world(factory, case, bounds, option)
    try:
        assert w.whole.get_option("eval_subtasks") == (option or sb.SUBTASKS)
        ids = scripted_quizzes(w, case, 3 if case.Q > 100 else 70)
        if name == "gaps37_sub5":   # across this config's worlds a gap and an asked question lie inside cut pieces
            seen = set()
            for b in every:
                for p in sr.parts_of([1.0] * case.Q, [False] * case.Q, w.n_sub, b):
                    for _, f, m in sr.shape(case.Q, w.n_sub, p["q_first"], p["n"])[2]:
                        seen |= set(range(f, f + m))
            assert set(case.qgaps) & seen and {q for q, _ in case.answers} & seen
        sizes = (1, 3) if case.Q > 100 else (1, 3, 70)
        for form in (1, 2, 3):
            w.set_form(form)
            for n in sizes:
                batch = ids[:n]
                for rnd in sb.EDGE_RNDS:
                    want = [oracle[j % steps][rnd] for j in range(n)]
                    check_batch(w, batch, [rnd] * n, (name, bounds, form, n, hex(rnd)), [x if x >= 0 else -1 for x in want])
                rnds = [draws[j % steps] for j in range(n)]
                want = [oracle[j % steps][rnds[j]] for j in range(n)]
                check_batch(w, batch, rnds, (name, bounds, form, n, "draws"), [x if x >= 0 else -1 for x in want])
                # ... and unguarded draws, exact against the shards' own priorities: (a), (b) and the parts alone
                free = sb.draws(1000 * form + n, n)
                check_batch(w, batch, free, (name, bounds, form, n, "free"))
    finally:
        w.close()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_float_engine(world, factory):
    """Float 120 x 5 x 1000: priorities are doubles either way.  Both sides take the row-sharing sweep, whose priority of a question
    does not depend on how many questions the engine holds -- asserted -- so every draw is compared with the whole engine exactly."""
    K, Q, T = 5, 120, 1000
    kb = cases.Case("float120", K, Q, T, seed=41).kb()
    w = World(factory, K, Q, T, kb, pdist.shard_bounds(Q, world), 7, qgaps=[2, 40, 41], f32=True)
    try:
        assert w.whole.get_option("precision") == 1
        ids = w.start(5)
        for j, quiz in enumerate(ids):
            for q in range(j):
                w.answer(quiz, 39 + 3 * q, (q + j) % K)
        counts = [b - f for f, b in zip(w.firsts, w.bounds)]
        for form in (2, 3):
            w.set_form(form)
            mine = np.concatenate([sh.eval_priorities_batch(ids, m) for sh, m in zip(w.shards, counts)], axis=1)
            assert np.array_equal(mine, w.whole.eval_priorities_batch(ids, Q)), form
            for rnds in ([0] * 5, [2**64 - 1] * 5, sb.draws(77 + form, 5)):
                got = check_batch(w, ids, rnds, ("float", form, hex(rnds[0])))
                assert got == w.whole.next_question_sampled_batch(ids, rnds), (form, rnds)
    finally:
        w.close()


def test_fallback_across_ranks_and_exhausted_quizzes(factory):
    """(d) the last shard's questions all asked or gaps and the random number 2^64 - 1: the pick, the last question, falls back to a
    question on another shard, the oracle's find_nearest; (e) a quiz with nothing left gives -1 in the batch and QuestionsExhausted
    in the single call; a whole engine is a world of one."""
    case = sb.scenarios()[1]
    bounds = pdist.shard_bounds(case.Q, 3)
    w = case_world(factory, case, bounds, 5)
    try:
        late, done, fresh = w.start(3)
        last = [q for q in range(bounds[1], case.Q) if q not in case.qgaps]
        for j, q in enumerate(last):
            w.answer(late, q, j % case.K)
        for j, q in enumerate(q for q in range(case.Q) if q not in case.qgaps):
            w.answer(done, q, j % case.K)
        orc = case.make_oracle()
        orc.start_quiz(cases.WORKERS)
        for q, a in w.answers[late]:
            orc.record_answer(q, a, cases.WORKERS - 1)
        want = orc.find_nearest(case.Q - 1)
        assert 0 <= want < bounds[1]
        # the same state RESUMED from a row package: a shard keeps the answered questions of other ranks too, so its fallback sees them
        aqs = [interop.AnsweredQuestion(q, a) for q, a in w.answers[late]]
        pkg = torch.zeros(len(aqs), 2 * w.shards[0].get_option("ldT"), dtype=torch.float64, device=DEVICE)
        torch.cuda.synchronize()
        for sh in w.shards:
            sh.pack_answer_rows(aqs, pkg.data_ptr())
        for sh in w.shards:
            sh.synchronize()
        resumed = w.whole.resume_quiz(aqs)
        assert [sh.resume_quiz_from_rows(aqs, pkg.data_ptr()) for sh in w.shards] == [resumed] * 3
        w.answers[resumed] = list(w.answers[late])
        got = check_batch(w, [late, done, fresh, resumed], [2**64 - 1] * 4, "fallback")
        assert got[0] == want and got[1] == -1 and got[2] == case.Q - 1 and got[3] == want, got
        assert [e.get_active_question_id(late) for e in w.engines] == [want] * 4
        # the single call, and the whole engine as a world of one through dist
        assert pdist.next_question_sampled(w.whole, late, 2**64 - 1, 0, 1, device=DEVICE) == want
        assert pdist.next_question_sampled_batch(w.whole, [fresh, done, late], [5, 6, 2**64 - 1], 0, 1, device=DEVICE) == \
            w.whole.next_question_sampled_batch([fresh, done, late], [5, 6, 2**64 - 1])
        with pytest.raises(interop.PqaException, match="run out of questions"):
            pdist.next_question_sampled(w.whole, done, 9, 0, 1, device=DEVICE)
    finally:
        w.close()


def test_refusals_change_nothing(factory):
    case = sb.scenarios()[1]
    bounds = pdist.shard_bounds(case.Q, 3)
    w = case_world(factory, case, bounds, 5)
    try:
        ids = scripted_quizzes(w, case, 3)
        rnds = [1 << 62, 1 << 63, 3 << 62]
        first = check_batch(w, ids, rnds, "before")
        state = lambda: [(e.get_total_questions_asked(), [e.get_active_question_id(q) for q in ids]) for e in w.shards]   # noqa: E731
        before = state()
        old = w.pack(ids)
        new = w.pack(ids)
        # a stale pack sequence: the parts of the pack before the engine's latest
        with pytest.raises(interop.PqaException, match="wrong mode.*stale"):
            w.shards[1].sampled_pick_from_parts(ids, rnds, old.data_ptr(), 1, 3)
        # ranges that do not tile: rank 1's part replaced by rank 0's, and a world that leaves a rank out
        broken = new.clone()
        broken[1] = new[0]
        torch.cuda.synchronize()
        with pytest.raises(interop.PqaException, match="wrong mode.*tile"):
            w.shards[0].sampled_pick_from_parts(ids, rnds, broken.data_ptr(), 0, 3)
        with pytest.raises(interop.PqaException, match="wrong mode.*tile"):
            w.shards[0].sampled_pick_from_parts(ids, rnds, new.data_ptr(), 0, 2)
        # another batch than the one packed, a repeated quiz, a bad rank
        with pytest.raises(interop.PqaException, match="wrong mode"):
            w.shards[0].sampled_pick_from_parts(ids[:2], rnds[:2], new.data_ptr(), 0, 3)
        for call in (lambda: w.shards[0].pack_sampled_parts([ids[0], ids[1], ids[0]], new.data_ptr()),
                     lambda: w.shards[0].sampled_pick_from_parts([ids[0], ids[1], ids[0]], rnds, new.data_ptr(), 0, 3),
                     lambda: w.shards[0].take_sampled_picks([ids[0], ids[1], ids[0]], [1, 2, 3])):
            with pytest.raises(interop.PqaException, match=r"quizId=%d\b.*twice|twice.*quizId=%d\b" % (ids[0], ids[0])):
                call()
        with pytest.raises(interop.PqaException, match="rank"):
            w.shards[0].sampled_pick_from_parts(ids, rnds, new.data_ptr(), 3, 3)
        with pytest.raises(interop.PqaException, match="Batch entry 1"):
            w.shards[0].take_sampled_picks(ids, [1, case.Q, 3])
        assert state() == before
        # ... and the latest pack still serves: the same picks as before
        per_rank = [sh.sampled_pick_from_parts(ids, rnds, new.data_ptr(), r, 3) for r, sh in enumerate(w.shards)]
        merged = pdist.merge_sampled_picks([[int(x) for x in p[:, 1]] for p in per_rank])
        assert [sr.take_py(m, case.Q, {q for q, s in enumerate(w.skip(quiz)) if s}) for m, quiz in zip(merged, ids)] == first
        # an answer recorded since the pack: the parts are of an earlier posterior
        w.answer(ids[0], first[0], 1)
        with pytest.raises(interop.PqaException, match="wrong mode"):
            w.shards[0].sampled_pick_from_parts(ids, rnds, new.data_ptr(), 0, 3)
    finally:
        w.close()
