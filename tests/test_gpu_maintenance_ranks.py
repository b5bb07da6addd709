"""Maintenance on process-per-GPU shards, on a real MI355X: AddQsTs / RemoveQuestions / RemoveTargets as collective, replicated calls
and Compact through block packages (PqaHip_CompactPlan, PqaHip_PackQuestionBlocks, PqaEngine_CompactFromBlocks), held to the numpy model
of tests/kb_model.py.  One process: the shards of one KB sit side by side on the one device as create_hip_engine(def, first, Q, 0)
engines (as tests/test_gpu_resume_ranks.py has them); every step goes to every shard and to a KBModel, and after every step the ids, the
ranges, the allocation and the arrays are the model's.  The ranks' vote of a compaction is taken here, in the test, the way
probqa_amd/dist.py's compact takes it over a process group (tests/test_gpu_maintenance_ranks_procs.py runs that one).

The range rule (`Ranks.bounds`): the start is dist.shard_range; appended questions go to the last shard; a compaction clips every bound
to the new question count, and one that would leave a shard without a question is refused on every shard.

Pitches are in elements: a granule is 16 fp64 or 32 fp32 elements."""
import numpy as np
import pytest
import torch

import cases
import maintenance_cases as mc
import test_gpu_parity as tp
from kb_model import random_step
from probqa_amd import dist as pdist
from probqa_amd import interop
from test_gpu_maintenance import PRECISIONS, run_step, same_bits

pytestmark = pytest.mark.gpu


def definition(K, Q, T, f32):
    kw = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24) if f32 else {}
    return interop.EngineDefinition(K, Q, T, init_amount=mc.INIT, **kw)


def whole_engine(factory, model):
    eng = factory.create_hip_engine(definition(model.K, model.Q, model.T, model.f32), 0, model.Q, 0)
    eng.set_option("workers", cases.WORKERS)
    eng.set_kb(model.A, model.D, model.B)
    return eng


class Ranks:
    """The shards of one synthetic KB, the model, and the range model."""

    def __init__(self, factory, dims, seed, f32, world):
        K, Q, T = dims
        self.model = mc.synthetic_model(K, Q, T, seed, f32)
        self.world, self.f32 = world, f32
        self.bounds = pdist.shard_bounds(Q, world)
        self.shards = []
        for r in range(world):
            first, limit = pdist.shard_range(Q, world, r)
            eng = factory.create_hip_engine(definition(K, limit - first, T, f32), first, Q, 0)
            eng.set_option("workers", cases.WORKERS)
            eng.set_kb(self.model.A[first:limit], self.model.D[first:limit], self.model.B)
            self.shards.append(eng)
        self.cap = self.local()

    def firsts(self):
        return [0] + self.bounds[:-1]

    def local(self):
        return [b - f for f, b in zip(self.firsts(), self.bounds)]

    def each(self, call):
        return [call(s) for s in self.shards]

    def close(self):
        self.each(lambda s: s.close())

    # ---- the collective calls, every rank alike ----------------------------------------------------------------------------------
    def would_empty(self):
        n_q = self.model.Q - len(self.model.q_gaps)
        return [r for r, (f, b) in enumerate(zip(self.firsts(), self.bounds)) if min(b, n_q) <= f]

    def compact(self):
        """dist.compact's sequence with the ranks side by side: plan, vote, pack, sum, compact.  -> what every shard returned, or None
        where the vote refused it (InsufficientEngineDimensions asserted on every shard)."""
        plans = self.each(lambda s: s.compact_plan())
        assert all(p[:3] == plans[0][:3] for p in plans), plans
        emptied = [r for r, p in enumerate(plans) if p[3]]
        assert emptied == self.would_empty(), (emptied, self.bounds)
        if emptied:
            texts = []
            for s in self.shards:
                with pytest.raises(interop.PqaException, match="Insufficient engine dimensions") as e:
                    s.compact_from_blocks(0, 0, emptied[0])
                texts.append(str(e.value))
            assert len(set(texts)) == 1 and "rank=%d" % emptied[0] in texts[0], texts
            return None
        moves = plans[0][2]
        slots = self.each(lambda s: s.question_block_slot_bytes())
        elem = 4 if self.f32 else 8
        from kb_model import round_ldt
        assert set(slots) == {(self.model.K + 1) * round_ldt(self.model.T, self.f32) * elem}, slots      # the same on every rank, whatever its ldT
        pkgs = [torch.zeros(max(len(moves), 1), slots[0] // elem, dtype=torch.float32 if self.f32 else torch.float64, device="cuda") for _ in self.shards]
        torch.cuda.synchronize()
        for s, pkg in zip(self.shards, pkgs):
            s.pack_question_blocks([src for _, src in moves], pkg.data_ptr())
        self.each(lambda s: s.synchronize())
        owners = [int(np.searchsorted(self.bounds, src, side="right")) for _, src in moves]
        for r, pkg in enumerate(pkgs):          # a rank fills the slots of the sources it holds and leaves every other one alone
            for i, o in enumerate(owners):
                assert bool(pkg[i].count_nonzero().item()) == (o == r), (r, i, o)
        combined = pkgs[0].clone()
        for pkg in pkgs[1:]:
            combined += pkg                     # (what the all_reduce does)
        torch.cuda.synchronize()
        return self.each(lambda s: s.compact_from_blocks(combined.data_ptr(), slots[0], -1))

    def step(self, step):
        """One step on every shard and on the model.  False where a compaction was refused (nothing has changed then)."""
        op, m = step[0], self.model
        if op == "remove_q":
            self.each(lambda s: s.remove_questions(step[1]))
            m.apply(step)
        elif op == "remove_t":
            self.each(lambda s: s.remove_targets(step[1]))
            m.apply(step)
        elif op == "add":
            got = []
            for s in self.shards:
                aq = [interop.AddQuestionParam(a) for a in step[1]]
                at = [interop.AddTargetParam(a) for a in step[2]]
                s.add_qs_ts(aq, at)
                got.append(([p.i_question for p in aq], [p.i_target for p in at]))
            want = m.apply(step)
            assert all(g == want for g in got), (step, got, want)
            self.bounds[-1] = m.Q                       # appended questions go to the last shard
        else:
            got = self.compact()
            if got is None:
                return False
            want = m.apply(step)
            assert all(g == want for g in got), (step, got, want)
            self.bounds = [min(b, m.Q) for b in self.bounds]       # a compaction clips
        self.cap = [max(c, n) for c, n in zip(self.cap, self.local())]
        return True

    def check(self, where=""):
        m = self.model
        A, D = [], []
        for r, s in enumerate(self.shards):
            d = s.copy_dims()
            assert (d.n_answers, d.n_questions, d.n_targets) == (m.K, m.Q, m.T), (where, r)
            got = tuple(s.get_option(o) for o in ("q_first", "q_total", "local_questions", "ldT", "capQ"))
            assert got == (self.firsts()[r], m.Q, self.local()[r], m.ld_t, self.cap[r]), (where, r, got)
            a, dd, b = s.get_kb(self.local()[r])
            A.append(a)
            D.append(dd)
            assert same_bits(b[m.live_t()], m.B[m.live_t()]), "%s: B on live targets, shard %d" % (where, r)
        A, D = np.concatenate(A), np.concatenate(D)
        lq, lt = m.live_q(), m.live_t()
        assert same_bits(A[lq][:, :, lt], m.A[lq][:, :, lt]), "%s: A on live questions x live targets" % where
        assert same_bits(D[lq][:, lt], m.D[lq][:, lt]), "%s: D on live questions x live targets" % where
        # the replicated bookkeeping: the same permanent ids on every rank, a gap has none
        perms = self.each(lambda s: s.question_perm_from_comp(list(range(m.Q))))
        assert all(p == perms[0] for p in perms) and [q for q in range(m.Q) if perms[0][q] < 0] == sorted(m.q_gaps), (where, perms)


def run_script(factory, dims, seed, steps, f32, world):
    """-> (the ranks after the script, the number of steps that ran: a refused compaction ends the script)"""
    ranks = Ranks(factory, dims, seed, f32, world)
    ranks.check("as loaded")
    ranks.each(lambda s: s.start_maintenance(False))
    done = 0
    for i, step in enumerate(steps):
        if not ranks.step(step):
            ranks.check("refused step %d" % i)           # arrays, gaps, dimensions and q_total as before the call
            break
        ranks.check("step %d %s" % (i, step[0]))
        done += 1
    return ranks, done


WORLD3 = {False: ((3, 12, 40), 27), True: ((3, 12, 70), 27)}


def world3_steps(T):
    return [("remove_q", [8, 1, 10]), ("remove_t", [t for t in range(T) if t % 3 == 1]), ("compact",), ("add", [0.5, 1.5], [0.3, 0.7, 1.0, 0.5])]


# ---- the scripts ----------------------------------------------------------------------------------------------------------------------
@PRECISIONS
@pytest.mark.parametrize("name", list(mc.array_scripts(False)))
def test_array_scripts_on_two_ranks(name, f32, factory):
    dims, seed, steps = mc.array_scripts(f32)[name]
    ranks, done = run_script(factory, dims, seed, steps, f32, 2)
    assert done == len(steps)
    if name == "compact_across_granule":
        assert ranks.bounds == [5, 11] and (ranks.model.Q, ranks.model.T) == (11, 78)      # [5, 9] -> [5, 6] -> [5, 8] -> [5, 11]
    ranks.each(lambda s: s.finish_maintenance())
    ranks.close()


@PRECISIONS
def test_compact_across_granule_is_refused_on_three_ranks(f32, factory):
    dims, seed, steps = mc.array_scripts(f32)["compact_across_granule"]
    ranks, done = run_script(factory, dims, seed, steps, f32, 3)
    assert done == 2 and ranks.bounds == [3, 6, 9]         # the last shard [6, 9) would be emptied: refused, nothing has changed
    assert ranks.each(lambda s: s.compact_plan()[:2]) == [(6, 14)] * 3
    ranks.close()


@PRECISIONS
def test_a_compaction_over_three_ranks_moves_one_question_across_and_one_inside(f32, factory):
    dims, seed = WORLD3[f32]
    ranks = Ranks(factory, dims, seed, f32, 3)
    ranks.each(lambda s: s.start_maintenance(False))
    steps = world3_steps(dims[2])
    for step in steps[:2]:
        assert ranks.step(step)
    assert ranks.shards[0].compact_plan()[2] == [(1, 11), (8, 9)] and ranks.bounds == [4, 8, 12]
    ld_before = ranks.model.ld_t
    for i, step in enumerate(steps[2:]):
        assert ranks.step(step)
        ranks.check("step %d" % (2 + i))
        if step[0] == "compact":
            assert ranks.bounds == [4, 8, 9]
    assert ranks.bounds == [4, 8, 11] and ranks.model.ld_t == ld_before          # the target columns moved down across a row granule; the pitch stays
    ranks.close()


@PRECISIONS
@pytest.mark.parametrize("world", [2, 3])
def test_random_scripts(world, f32, factory):
    complete = []
    for seed in range(mc.N_RANDOM_SCRIPTS):
        rng, dims, kb_seed = mc.random_script_start(seed)
        ranks = Ranks(factory, dims, kb_seed, f32, world)
        ranks.each(lambda s: s.start_maintenance(False))
        for i in range(mc.RANDOM_STEPS):
            step = random_step(ranks.model, rng)
            refusal_due = step[0] == "compact" and bool(ranks.would_empty())
            ran = ranks.step(step)
            assert ran != refusal_due, (seed, i, step)
            ranks.check("script %d step %d %s" % (seed, i, step[0]))
            if not ran:
                break
        else:
            complete.append(seed)
        ranks.close()
    assert len(complete) >= 9, complete        # a condition of the scripts, not a measurement: only seed 6 (Q = 3) is refused (tests/test_maintenance_ranks_abi.py)


# ---- file round-trip ------------------------------------------------------------------------------------------------------------------
@PRECISIONS
@pytest.mark.parametrize("world", [2, 3])
def test_the_shards_save_the_file_a_whole_engine_saves(world, f32, factory, tmp_path):
    if world == 2:
        dims, seed, steps = mc.array_scripts(f32)["compact_across_granule"]
    else:
        (dims, seed), steps = WORLD3[f32], world3_steps(WORLD3[f32][0][2])
    ranks, done = run_script(factory, dims, seed, steps, f32, world)
    assert done == len(steps)
    model = mc.synthetic_model(*dims, seed, f32)
    whole = whole_engine(factory, model)
    whole.start_maintenance(False)
    for step in steps:
        run_step(whole, model, step)
    by_shards, by_whole = str(tmp_path / "shards.kb"), str(tmp_path / "whole.kb")
    open(by_shards, "wb").close()
    for s in reversed(ranks.shards):                      # (any order)
        s.save_kb_shard(by_shards)
    whole.save_kb(by_whole, False)
    assert open(by_shards, "rb").read() == open(by_whole, "rb").read()
    perms = whole.question_perm_from_comp(list(range(model.Q)))
    assert ranks.each(lambda s: s.question_perm_from_comp(list(range(model.Q)))) == [perms] * world
    whole.close()
    ranks.close()
    # ... and loads at the canonical split
    m = ranks.model
    lq, lt = m.live_q(), m.live_t()
    A, D = [], []
    for r in range(world):
        first, limit = pdist.shard_range(m.Q, world, r)
        sh = pdist.load_shard(factory, by_shards, r, world, device=0)
        assert (sh.get_option("q_first"), sh.get_option("local_questions"), sh.get_option("q_total")) == (first, limit - first, m.Q)
        a, d, b = sh.get_kb(limit - first)
        A.append(a)
        D.append(d)
        assert same_bits(b[lt], m.B[lt])
        assert sh.question_perm_from_comp(list(range(m.Q))) == perms
        sh.close()
    A, D = np.concatenate(A), np.concatenate(D)
    assert same_bits(A[lq][:, :, lt], m.A[lq][:, :, lt]) and same_bits(D[lq][:, lt], m.D[lq][:, lt])


# ---- serving --------------------------------------------------------------------------------------------------------------------------
def index_bits(records):
    """[world, 2] (priority, index as a float) -> the records dist.pick_global takes: the index as the bits of an int64"""
    out = np.zeros((len(records), 2))
    out[:, 0] = [r[0] for r in records]
    out[:, 1:2].view(np.int64)[:, 0] = [int(r[1]) for r in records]
    return out


@PRECISIONS
@pytest.mark.parametrize("case", [c for c in mc.SERVING_CASES if c.name in ("grow_1000_1030", "compact_1100_980")], ids=lambda c: c.name)
def test_serving_after_maintenance_like_the_whole_engine(case, f32, factory):
    dims = (case.K, case.Q, case.T0)
    ranks, done = run_script(factory, dims, mc.KB_SEED, case.steps, f32, 2)
    assert done == len(case.steps)
    model = mc.synthetic_model(*dims, mc.KB_SEED, f32)
    whole = whole_engine(factory, model)
    whole.start_maintenance(False)
    for step in case.steps:
        run_step(whole, model, step)
    engines = ranks.shards + [whole]
    for e in engines:
        e.finish_maintenance()
    records = mc.post_training(model)
    assert len(records) >= 24
    for q, a, t, amount in records:                        # every rank sees every Train
        for e in engines:
            e.train([interop.AnsweredQuestion(q, a)], t, amount)
    mc.train_model(ranks.model, records)
    ranks.check("%s after Train" % case.name)
    # -- priorities and the pick
    zs = ranks.each(lambda s: s.start_quiz())
    zw = whole.start_quiz()
    want = whole.eval_priorities(zw)
    got = np.concatenate([s.eval_priorities(z, n) for s, z, n in zip(ranks.shards, zs, ranks.local())])
    has = want != 0
    assert ((got != 0) == has).all() and has.sum() == len(ranks.model.live_q())
    rel = cases.rel_err(got[has], want[has])
    print("%s %s: shards (%s) against the whole engine (%s): %.3g of the bar" % (case.name, "float" if f32 else "double", ranks.shards[0].eval_kernel_name(),
                                                                               whole.eval_kernel_name(), rel.max() / tp.PRIORITY_RTOL))
    assert (rel < tp.PRIORITY_RTOL).all(), rel
    winners = [s.select_argmax_batch([z])[0] for s, z in zip(ranks.shards, zs)]
    assert pdist.pick_global(index_bits(winners))[1] == whole.next_question_argmax(zw)
    # -- a quiz resumed from row packages, its two answered questions on different ranks under the NEW ranges
    live = ranks.model.live_q()
    pair = [next(q for q in live if q < ranks.bounds[0]), next(q for q in reversed(live) if q >= ranks.bounds[0])]
    assert [pdist.owner_in(ranks.bounds, q) for q in pair] == [0, 1]
    aqs = [interop.AnsweredQuestion(pair[0], 1), interop.AnsweredQuestion(pair[1], 0)]
    pkg = pdist._package(ranks.shards[0], len(aqs), torch.device("cuda"))
    torch.cuda.synchronize()
    for s in ranks.shards:
        s.pack_answer_rows(aqs, pkg.data_ptr())
    ranks.each(lambda s: s.synchronize())
    want_priors = whole.get_priors(whole.resume_quiz(aqs))
    for s in ranks.shards:
        assert same_bits(s.get_priors(s.resume_quiz_from_rows(aqs, pkg.data_ptr())), want_priors)
    whole.close()
    ranks.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
@PRECISIONS
def test_refused_calls_change_nothing(f32, factory):
    dims, seed, steps = mc.array_scripts(f32)["compact_across_granule"]
    ranks, done = run_script(factory, dims, seed, steps[:2], f32, 2)       # 26 target gaps, question gaps 0, 4, 8
    assert done == 2
    for bad in ([4], [1, 8], [2, 5, 2], [9], [-1]):                        # a gap (here and elsewhere), a repeated id, ids outside the KB
        for s in ranks.shards:
            with pytest.raises(interop.PqaException, match="The ID is absent from KB"):
                s.remove_questions(bad)
        ranks.check("after the refused removal of %s" % bad)
    for s in ranks.shards:
        with pytest.raises(interop.PqaException, match="Not implemented.*use PqaEngine_CompactFromBlocks"):
            s.compact()
    plan = ranks.shards[0].compact_plan()
    assert plan[:3] == (6, 14, [(0, 7), (4, 6)])
    slot = ranks.shards[0].question_block_slot_bytes()
    pkg = torch.zeros(2, slot // 8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for s in ranks.shards:
        for wrong in (slot - 128, slot + 128, 2 * ranks.model.ld_t * (4 if f32 else 8)):
            with pytest.raises(interop.PqaException, match="slot size is not this engine's"):
                s.compact_from_blocks(pkg.data_ptr(), wrong, -1)
        with pytest.raises(interop.PqaException, match="Index is out of range"):
            s.pack_question_blocks([7, 9], pkg.data_ptr())
    with pytest.raises(interop.PqaException, match="Nullptr"):
        ranks.shards[0].compact_from_blocks(0, 0, -1)                      # rank 0 takes both moved questions from rank 1: no package, no compaction
    ranks.check("after the refused compactions")
    assert ranks.each(lambda s: s.compact_plan()) == [plan, plan[:3] + (False,)]
    ranks.each(lambda s: s.synchronize())
    assert not pkg.count_nonzero().item()
    ranks.close()


def test_a_whole_engine_compacts_from_no_package(factory):
    dims, seed, steps = mc.array_scripts(False)["compact_across_granule"]
    model = mc.synthetic_model(*dims, seed, False)
    whole = whole_engine(factory, model)
    whole.start_maintenance(False)
    for step in steps[:2]:
        run_step(whole, model, step)
    assert whole.compact_plan() == (6, 14, [(0, 7), (4, 6)], False)
    assert whole.compact_from_blocks() == model.apply(("compact",))
    A, D, B = whole.get_kb()
    assert same_bits(A, model.A) and same_bits(D, model.D) and same_bits(B, model.B)
    whole.close()
