"""AddQsTs / RemoveQuestions / RemoveTargets / Compact held to a numpy model (tests/kb_model.py) across the edges of the allocation --
the row pitch ldT and the question capacity, which only ever grow -- and across the row lengths at which the launch wrappers change
their form, some by T and some by ldT.  In layers, so that a failure names its place:

  A  arrays only: after every step of a script the returned ids, the dimensions, the pitch, the capacity and the knowledge base itself
     (live questions x live targets, bit for bit) are the model's.  A failure here is in kb_kernels.hip or HipEngine::ReallocKB.
  B  serving after maintenance: a fixed list of calls on the engine, on a fresh twin engine that was CREATED at the final dimensions and
     loaded with the engine's own arrays and gaps, and on the CPU oracle loaded the same way.  The twin's pitch is RoundLdT(T) and its
     padding columns hold A = 0, D = 1; the engine's pitch may be larger and, after a compaction, its columns [T, old T) hold stale
     non-zero values.  Engine against twin alone: a path that trusts T where it means ldT, or the padding's values.  Both against the
     oracle: not maintenance at all.

(C, the rebuilt shards of a sharded engine, is tests/test_gpu_sharded.py.)  The quiz states of layer B are chosen on the CPU
(tests/maintenance_cases.py; tests/test_kb_model.py asserts them without a device) so that the oracle's best question and its sampled
picks are unambiguous: no selection check is conditional.

On a Float engine the priorities' bars are not the issue's PRIORITY_RTOL / PRIORITY_RTOL_TIGHT, which no fp32 sweep meets, but the
project's own for fp32 sweeps (tests/test_gpu_batch.py): f32_tolerance per question against the oracle, twice that between two sweeps.
Posteriors, listings, resumed quizzes and training are fp64 arithmetic on the rounded cube and bit-identical on both engine types.

Pitches are in elements: a granule is 16 fp64 or 32 fp32 elements, so 40 targets have a pitch of 48 on a Double engine and 64 on a Float one."""
import time

import numpy as np
import pytest

import cases
import maintenance_cases as mc
import test_gpu_kb as tk
import test_gpu_parity as tp
import test_gpu_top_questions as ttq
from kb_model import random_step, round_ldt
from probqa_amd import interop

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def run_step(eng, model, step):
    """One maintenance step on the engine and on the model; what the engine returns is what the model returns."""
    op = step[0]
    if op == "remove_q":
        eng.remove_questions(step[1])
        model.apply(step)
    elif op == "remove_t":
        eng.remove_targets(step[1])
        model.apply(step)
    elif op == "add":
        aq = [interop.AddQuestionParam(a) for a in step[1]]
        at = [interop.AddTargetParam(a) for a in step[2]]
        eng.add_qs_ts(aq, at)
        assert ([p.i_question for p in aq], [p.i_target for p in at]) == model.apply(step), step
    else:
        assert eng.compact() == model.apply(step), step


def check_arrays(eng, model, where=""):
    d = eng.copy_dims()
    assert (d.n_answers, d.n_questions, d.n_targets) == (model.K, model.Q, model.T), where
    assert (eng.get_option("ldT"), eng.get_option("capQ")) == (model.ld_t, model.cap_q), where      # max(previous, RoundLdT(T)), max(previous, Q)
    A, D, B = eng.get_kb()
    lq, lt = model.live_q(), model.live_t()
    assert same_bits(A[lq][:, :, lt], model.A[lq][:, :, lt]), "%s: A on live questions x live targets" % where
    assert same_bits(D[lq][:, lt], model.D[lq][:, lt]), "%s: D on live questions x live targets" % where
    assert same_bits(B[lt], model.B[lt]), "%s: B on live targets" % where


def engine_and_model(factory, K, Q, T, seed, f32):
    eng, *_ = tk.make(factory, K, Q, T, seed=seed, f32=f32)
    model = mc.synthetic_model(K, Q, T, seed, f32)
    check_arrays(eng, model, "as loaded")
    return eng, model


# ---- Layer A ------------------------------------------------------------------------------------------------------------------------
@PRECISIONS
@pytest.mark.parametrize("name", list(mc.array_scripts(False)))
def test_arrays_follow_the_model_across_the_allocation(name, f32, factory):
    (K, Q, T), seed, steps = mc.array_scripts(f32)[name]
    eng, model = engine_and_model(factory, K, Q, T, seed, f32)
    eng.start_maintenance(False)
    trail = [(model.ld_t, model.cap_q)]
    for i, step in enumerate(steps):
        run_step(eng, model, step)
        check_arrays(eng, model, "%s step %d %s" % (name, i, step[0]))
        trail.append((eng.get_option("ldT"), eng.get_option("capQ")))
    if name == "grow_t_inside_granule":
        assert trail[-1] == trail[0]                          # no reallocation
    if name in ("grow_t", "grow_t_and_q"):
        assert trail[-1][0] == 2 * trail[0][0]                # across a granule
    if name == "compact_across_granule":
        d = eng.copy_dims()
        assert trail[3] == trail[0] == trail[4] and trail[5][0] > trail[4][0] and trail[5][1] > trail[4][1]   # the pitch of 40 targets serves 14, then 18; then both grow
        assert (d.n_questions, d.n_targets) == (11, 78)
    eng.finish_maintenance()
    eng.close()


@PRECISIONS
@pytest.mark.parametrize("seed", range(mc.N_RANDOM_SCRIPTS))
def test_arrays_follow_the_model_over_random_scripts(seed, f32, factory):
    rng, (K, Q, T), kb_seed = mc.random_script_start(seed)
    eng, model = engine_and_model(factory, K, Q, T, kb_seed, f32)
    eng.start_maintenance(False)
    done = []
    for i in range(mc.RANDOM_STEPS):
        step = random_step(model, rng)
        run_step(eng, model, step)
        done.append(step[0])
        check_arrays(eng, model, "script %d step %d of %s" % (seed, i, done))
    eng.finish_maintenance()
    eng.close()


# ---- Layer B ------------------------------------------------------------------------------------------------------------------------
def listed(eng, quiz, n):
    return [(t.i_target, t.prob) for t in eng.list_top_targets(quiz, n)]


def check_state(engines, quizzes, orc, model, asked, where):
    """Priorities and single-quiz selections of each engine's quiz in the oracle's current state."""
    s = mc.state_of(orc, model, asked)
    assert s.margin > 10 * tp.PRIORITY_RTOL, "%s: the oracle's top-2 margin %g must exceed ten times the priorities' bar" % (where, s.margin)
    assert s.argmax_clearance > 0 and s.sampled_clearance > 0, (where, s.argmax_clearance, s.sampled_clearance)
    has = s.opri != 0
    pris = [e.eval_priorities(z) for e, z in zip(engines, quizzes)]
    names = [e.eval_kernel_name() for e in engines]
    for who, name, pri in zip(("engine", "twin"), names, pris):
        assert ((pri != 0) == has).all(), "%s, %s: gap and asked questions have priority 0, and only they" % (where, who)
        rel = cases.rel_err(pri[has], s.opri[has])
        print("%s: %s %s against the oracle: %.3g of its bar" % (where, who, name, (rel / s.tol[has]).max()))
        assert (rel < s.tol[has]).all(), "%s: %s against the oracle: %s" % (where, who, rel)      # PRIORITY_RTOL; Float: tests/test_gpu_batch.py f32_tolerance
    if model.f32:      # two fp32 sweeps of one cube: tests/test_gpu_batch.py's bar between two forms
        bar = 2 * s.tol[has]
    else:
        bar = tp.PRIORITY_RTOL_TIGHT if names[0] == names[1] else tp.PRIORITY_RTOL
    rel = cases.rel_err(pris[0][has], pris[1][has])
    print("%s: engine (%s) against twin (%s): %.3g of the bar" % (where, names[0], names[1], (rel / bar).max()))
    assert (rel < bar).all(), "%s: engine (%s) against twin (%s): %s" % (where, names[0], names[1], rel)
    for who, e, z in zip(("engine", "twin"), engines, quizzes):
        assert e.next_question_argmax(z) == s.want, "%s, %s: argmax, launched" % (where, who)
        e.set_option("server", 1)
        assert e.next_question_argmax(z) == s.want, "%s, %s: argmax, resident sweep" % (where, who)
        e.set_option("server", 0)
        for host_sampled in (1, 0):
            e.set_option("host_sampled", host_sampled)
            got = [e.next_question_sampled(z, r) for r in mc.RNDS]
            assert got == s.sampled, "%s, %s: sampled selector, host_sampled=%d" % (where, who, host_sampled)
        e.set_option("host_sampled", 1)
    return s


def assert_serves_like_fresh(eng, model, factory, answers=(0, 0)):
    """Everything a client does with a quiz, on `eng` (which maintenance has brought to the model's state), on a twin created at the
    model's dimensions and on the oracle, both loaded with eng's own arrays and gaps.  answers: what the two questions asked get."""
    K, Q, T, W = model.K, model.Q, model.T, cases.WORKERS
    A, D, B = eng.get_kb()
    twin, *_ = tk.make(factory, K, Q, T, f32=model.f32)
    twin.set_kb(A, D, B)
    twin.set_target_gaps(model.t_gaps)
    twin.set_question_gaps(model.q_gaps)
    orc = mc.oracle_of(model, A, D, B)
    engines = (eng, twin)
    try:
        # -- after StartQuiz
        z0 = [e.start_quiz() for e in engines]
        orc.start_quiz(W)
        for e, z in zip(engines, z0):
            assert same_bits(e.get_priors(z), orc.priors()), "priors after StartQuiz"
            assert listed(e, z, 5) == orc.list_top_targets(5, W), "top targets, no RecordAnswer before them"
        s0 = check_state(engines, z0, orc, model, [], "fresh quiz")
        # -- two answers the way a client gives them: NextQuestion, RecordAnswer, with the speculative sweep and the update fused into it
        for e in engines:
            e.set_option("select", 1)
        qa = [e.start_quiz() for e in engines]
        asked, s = [], s0
        for step, a in enumerate(answers):
            for who, e, z in zip(("engine", "twin"), engines, qa):
                assert e.next_question(z) == s.want, "%s: NextQuestion %d" % (who, step)
                e.record_answer(z, a)
            orc.record_answer(s.want, a, W - 1)
            asked.append((s.want, a))
            for who, e, z in zip(("engine", "twin"), engines, qa):
                assert same_bits(e.get_priors(z), orc.priors()), "%s: posterior after answer %d" % (who, step)
                assert listed(e, z, 5) == orc.list_top_targets(5, W), "%s: top targets right behind RecordAnswer %d" % (who, step)
            if step + 1 < len(answers):
                s = mc.state_of(orc, model, [q for q, _ in asked])
                assert s.margin > 10 * tp.PRIORITY_RTOL and s.argmax_clearance > 0, (step, s.margin, s.argmax_clearance)
        asked_q = [q for q, _ in asked]
        s2 = check_state(engines, qa, orc, model, asked_q, "after two answers")
        for who, e, z, z_fresh in zip(("engine", "twin"), engines, qa, z0):
            assert listed(e, z, 16) == orc.list_top_targets(16, W), "%s: more top targets than RecordAnswer lists ahead" % who
            # (form 3 is taken where EvalMidBatchSupported holds -- Double engines, rows that fit the LDS -- and is the default's choice elsewhere)
            for form in (1, 2, 3):
                e.set_option("batch_form", form)
                assert e.next_question_argmax_batch([z, z_fresh]) == [s2.want, s0.want], "%s: batched argmax, batch_form %d" % (who, form)
            e.set_option("batch_form", 0)
            pri = e.eval_priorities(z)
            assert ttq.same(e.list_top_questions(z, 5), ttq.reference(pri, 5)), "%s: top questions" % who
        # -- the same two answers through ResumeQuiz
        aqs = [interop.AnsweredQuestion(q, a) for q, a in asked]
        for bug in (0, 1):
            assert orc.resume_quiz(asked, W, bool(bug)) == 0
            for who, e in zip(("engine", "twin"), engines):
                e.set_option("bug_compat", bug)
                for r in [e.resume_quiz(aqs)] + e.resume_quiz_batch([aqs] * 3):
                    assert same_bits(e.get_priors(r), orc.priors()), "%s: resumed quiz, bug_compat %d" % (who, bug)
        # -- training on the maintained cube leaves what it leaves on the fresh one
        t = model.live_t()[len(model.live_t()) // 2]
        for e in engines:
            e.train(aqs[:1], t, 1.5)
        for x, y in zip(eng.get_kb(), twin.get_kb()):
            assert same_bits(x, y), "the knowledge base after Train"
        return [s0.margin, s.margin, s2.margin]
    finally:
        twin.close()
        orc.close()


@PRECISIONS
@pytest.mark.parametrize("case", mc.SERVING_CASES, ids=lambda c: c.name)
def test_serving_after_maintenance_like_a_fresh_engine(case, f32, factory):
    t_start = time.perf_counter()
    eng, model = engine_and_model(factory, case.K, case.Q, case.T0, mc.KB_SEED, f32)
    before = eng.eval_kernel_name()
    eng.start_maintenance(False)
    for i, step in enumerate(case.steps):
        run_step(eng, model, step)
        check_arrays(eng, model, "%s step %d %s" % (case.name, i, step[0]))
    eng.finish_maintenance()
    # the added questions say nothing until something is trained on them, and their priority is rounding residue (maintenance_cases.py:
    # untrained_questions): a dozen Train calls each, on the rows the maintenance has just made -- bit for bit what the oracle trains
    records = mc.post_training(model)
    for q, a, t, amount in records:
        eng.train([interop.AnsweredQuestion(q, a)], t, amount)
    mc.train_model(model, records)
    check_arrays(eng, model, "%s after Train" % case.name)
    assert len(records) >= 24 and not mc.untrained_questions(model)
    assert (model.T, len(model.t_gaps), len(model.q_gaps), model.cap_q) == (case.T1, 2, 1, case.Q + 2)
    assert (model.ld_t > round_ldt(model.T, f32)) == ("compact" in case.name)         # T <= ... < ldT where the case is for it
    if case.name == "grow_1000_1030":
        assert eng.eval_kernel_name() != before, before                                  # the sweep's shape follows the pitch
    margins = assert_serves_like_fresh(eng, model, factory, mc.ANSWERS)
    print("%s %s: %s, top-2 margins %s, %.2f s" % (case.name, "float" if f32 else "double", eng.eval_kernel_name(), ["%.3g" % m for m in margins],
                                                 time.perf_counter() - t_start))
    eng.close()
