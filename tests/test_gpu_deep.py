"""Quizzes a hundred and more answers deep on every kernel form, held to the oracle.

The cases (tests/deep_cases.py; qualified on the oracle alone by tests/test_deep_cases.py) are dichotomy quizzes of 250 answers -- 130
on rows of 17000 targets -- whose posterior walks through the whole subnormal range: from about the 90th .. 160th answer on most of
the row is subnormal, then exactly 0, while the hidden target stays above 0.99.  That is where the products and the division by the
total in record_answer_body (prior_device.h), resume_quiz_body's correction and flush (prior_kernels.hip), Log2Hot's exponent field of
-1023, pass 1 and pass 2 of every sweep, the pole watch and its redo, and the listings' ordering meet zero and subnormal operands.

Bars: posteriors np.array_equal with the oracle's at every step, on Double and Float engines; a Double engine's priorities within 1e-9
relative and zero exactly where the oracle's are (no allowance for the subnormal range: Log2Hot reads a
subnormal's exponent field as -1023 on both sides, so a last-place difference of a subnormal likelihood moves its lack term by at most
2^-52 relative, and its entropy and velocity terms are below 1e-300 absolute); the argmax the oracle's where its top-2 margin exceeds
1e-8; the reference's sampled selector the oracle's for the six random numbers of test_gpu_parity.run_script; a Float engine's
priorities held to structure only.  Priorities are compared at deep_cases.compared_steps, posteriors at every step.

Legs: A the single-quiz sweeps stepwise (speculate = 0; the first case also as the engine comes), B the client loop under default
options against a twin with speculate = 0, C the posterior forms, D ResumeQuiz, E the batched sweeps, F the Among call and the listings.

Worst relative deviation of a priority from the oracle's per leg, as measured on an MI355X (fraction of the 1e-9 bar):
  A  single-quiz sweeps   1.5e-12  (0.0015)    2 x 260 x 900 at step 166; the other twelve legs 9.6e-14 .. 7.8e-13
  B  client loop          picks only: 250 of 250 updates ran inside the sweep's launch, 165 picks held to the oracle, per selector
  C  sharded engine       1.0e-13  (0.0001)    (the other forms of leg C compare posteriors only)
  D  resumed quizzes      9.9e-14  (0.0001)    17000 targets, 130 answers; 6.0e-16 at 1000 targets; 2.8e-14 .. 8.2e-14 where the flush is reached
  E  batched sweeps       1.5e-13  (0.00015)   batch_form 1 at 5000 targets; form 2 1.4e-13, form 3 7.5e-14
  F  among                6.0e-14  (0.00006)
Every test prints its own figure and the step where it occurred.

What the file notices, tried on scratch builds of the library.  (1) Subnormal quotients of record_answer_body's division by the total
flushed to 0: 24 of these tests fail, and none of the 1092 GPU tests the suite had before.  (2) x[e] / total replaced by
x[e] * (1.0 / total) there, in the loop for rows beyond 4096 targets: the 5000- and 17000-target legs fail at the first answer; the
suite noticed that before (test_gpu_batch, 4000 targets).  (3) resume_quiz_body's flush `1 > normExp` turned into `0 > normExp` changes
no posterior and cannot: the row is scaled so that its largest element has the exponent field highBound = 2046 - ceil(log2 T) - 2 before
it is divided by the total, which is at least that element, so an element with normExp = 0 is below 2^-1022 then and below 2^-2030
after the division -- 0 either way.  The subnormals a resumed posterior holds come from that division, not from the flush.  (4) The same
flush turned into `-60 > normExp`, so that elements just under the threshold keep a wrapped exponent field: the three tests whose scripts
reach the flush fail (2000, 5000 and 17000 targets at 250 answers); the 1000-target script stops 180 binades short of it, and the
suite's earlier 1092 tests pass.
"""
import numpy as np
import pytest

import cases
import deep_cases as dc
import test_gpu_batch as tb
from probqa_amd import interop

pytestmark = pytest.mark.gpu

BAR = 1e-9
DECIDED = 1e-8
W = cases.WORKERS


def held(pri, ref, worst, what):
    """A Double engine's priorities against the oracle's Ref at the bar; returns the running (worst deviation, where)."""
    rel = tb.rel_vec(pri, ref.opri)                             # (asserts: zero exactly where the oracle's are)
    top = float(rel.max())
    assert top < BAR, (what, top, int(rel.argmax()))
    return (top, what) if top >= worst[0] else worst


def structure(pri, ref, what):
    """What a Float engine's priorities are held to: finite, non-negative, zero exactly where the oracle's are."""
    assert np.isfinite(pri).all() and (pri >= 0).all(), what
    tb.rel_vec(pri, ref.opri)


def report(leg, worst):
    print("%s: worst relative deviation %.3g (%.3g of the bar) at %s" % (leg, worst[0], worst[0] / BAR, worst[1]))


def aq_list(pairs):
    return [interop.AnsweredQuestion(int(q), int(a)) for q, a in pairs]


def at_prefixes(eng, answers, lens):
    """One quiz per entry of lens, in the state after answers[:len]: started in one launch, answered in one launch per step."""
    ids = eng.start_quiz_batch(len(lens))
    for step in range(max(lens)):
        live = [z for z, n in zip(ids, lens) if n > step]
        for z in live:
            eng.set_active_question(z, answers[step][0])
        eng.record_answer_batch(live, [answers[step][1]] * len(live))
    return ids


def answer(eng, quiz, qa):
    eng.set_active_question(quiz, qa[0])
    eng.record_answer(quiz, qa[1])


def stepwise(case, eng, f32=False, selections=True):
    """StartQuiz, then the script answer by answer: the posterior at every step, priorities and selections at compared_steps."""
    tr = dc.trace(case, f32)
    refs = dc.reference(case, dc.compared_steps(case, f32), f32)
    quiz = eng.start_quiz()
    worst, decided = (0.0, None), 0
    for s in range(len(case.answers) + 1):
        assert np.array_equal(eng.get_priors(quiz), tr.posts[s]), (case.name, s, "posterior")
        if s in refs:
            ref = refs[s]
            pri = eng.eval_priorities(quiz, case.Q)
            if f32:
                structure(pri, ref, (case.name, s))
            else:
                worst = held(pri, ref, worst, (case.name, s))
            if selections and not f32:
                if ref.margin > DECIDED:
                    decided += 1
                    assert eng.next_question_argmax(quiz) == ref.want, (case.name, s, "argmax", ref.margin)
                for rnd, want in zip(dc.RNDS, ref.sampled):
                    assert eng.next_question_sampled(quiz, rnd) == want, (case.name, s, "sampled", hex(rnd))
        if s < len(case.answers):
            answer(eng, quiz, case.answers[s])
    return worst, decided, len(refs)


# ---- A: single-quiz sweeps, stepwise ---------------------------------------------------------------------------------------------
SWEEPS = [
    ("d1000", ()), ("d260", ()), ("d900k2", ()), ("d2000k3", ()), ("d700k7", ()), ("d5000", ()),
    ("d1000", (("eval_max_grid", 1),)), ("d1000", (("eval_variant", 99),)), ("d1000", (("server", 1),)), ("d1000wrong9", ()),
    ("d17000", (("cluster_form", 1),)), ("d17000", (("cluster_form", 2),)), ("d1000tgaps", ()),
]


def sweep_id(p):
    return p[0] + "".join("_%s%d" % nv for nv in p[1])


@pytest.mark.parametrize("name,options", SWEEPS, ids=[sweep_id(p) for p in SWEEPS])
def test_single_quiz_sweeps_stepwise(name, options, factory):
    case = dc.get(name)
    eng = case.make_engine(factory)
    eng.set_option("speculate", 0)
    for n, v in options:
        eng.set_option(n, v)
    kernel = eng.eval_kernel_name()
    worst, decided, compared = stepwise(case, eng)
    eng.close()
    report("A %s %s (%d steps compared, %d argmaxes decided)" % (sweep_id((name, options)), kernel, compared, decided), worst)
    assert 2 * decided >= len(dc.landmarks(case))


def test_single_quiz_sweeps_stepwise_as_the_engine_comes(factory):
    """The first case once more with no option touched: every selection of the stepwise loop with the speculative sweep in play."""
    case = dc.get("d1000")
    eng = case.make_engine(factory)
    assert eng.get_option("speculate") == 1
    worst, _, _ = stepwise(case, eng)
    eng.close()
    report("A d1000 default options", worst)


# ---- B: the client loop under default options ------------------------------------------------------------------------------------
@pytest.mark.parametrize("selector", ["argmax", "sampled"])
def test_client_loop_under_default_options(selector, factory):
    """NextQuestion -> RecordAnswer -> ListTopTargets(1), 250 times, as a client does it, with speculate, fuse_update and pole_lazy as
    they come: RecordAnswer's update runs inside the next sweep's launch (eval_questions_f64_upd; the counter fused_updates says that it
    did) and so forms the deep posteriors.  The speculative sweep is launched for the selector the engine's option `select` names, and
    only a NextQuestion of that selector takes it over: "argmax" sets select = 1 and asks through next_question_argmax, "sampled"
    touches no option and asks through next_question_sampled with run_script's random numbers in turn.  Picks equal those of a twin
    engine with speculate = 0 and the oracle's (the argmax where decided); posteriors bit for bit."""
    case = dc.get("d1000")
    tr = dc.trace(case)
    refs = dc.reference(case, dc.compared_steps(case))
    eng, twin = case.make_engine(factory), case.make_engine(factory)
    twin.set_option("speculate", 0)
    if selector == "argmax":
        eng.set_option("select", 1)
        twin.set_option("select", 1)
    assert (eng.get_option("speculate"), eng.get_option("fuse_update"), eng.get_option("pole_lazy")) == (1, 1, 1)
    quiz, tquiz = eng.start_quiz(), twin.start_quiz()
    held_to_oracle = 0
    for s, qa in enumerate(case.answers):
        if selector == "argmax":
            pick, tpick = eng.next_question_argmax(quiz), twin.next_question_argmax(tquiz)
            want = refs[s].want if s in refs and refs[s].margin > DECIDED else None
        else:
            rnd = dc.RNDS[s % len(dc.RNDS)]
            pick, tpick = eng.next_question_sampled(quiz, rnd), twin.next_question_sampled(tquiz, rnd)
            want = refs[s].sampled[s % len(dc.RNDS)] if s in refs else None
        assert pick == tpick, (s, pick, tpick, "twin")
        if want is not None:
            held_to_oracle += 1
            assert pick == want, (s, pick, want)
        answer(eng, quiz, qa)
        answer(twin, tquiz, qa)
        top = eng.list_top_targets(quiz, 1)
        post = tr.posts[s + 1]
        assert [(t.i_target, t.prob) for t in top] == [(int(post.argmax()), float(post.max()))], (s, top)
        assert np.array_equal(eng.get_priors(quiz), post), (s, "posterior")
        assert np.array_equal(twin.get_priors(tquiz), post), (s, "twin's posterior")
    fused, hits = eng.get_option("fused_updates"), eng.get_option("spec_hits")
    eng.close()
    twin.close()
    print("B %s: %d answers, %d updates inside the sweep's launch, %d speculative sweeps taken over, %d picks held to the oracle" % (
        selector, len(case.answers), fused, hits, held_to_oracle))
    assert fused >= len(case.answers) - 1 and 2 * held_to_oracle >= sum(s < len(case.answers) for s in refs)


# ---- C: posterior forms ----------------------------------------------------------------------------------------------------------
def test_record_answer_batch_of_256_quizzes(factory):
    """Quiz j has been given the first j answers (one record_answer_batch launch per step on the way there); then all 256 advance one
    answer -- each its own -- in one launch, eight times: shallow, subnormal and mostly-zero rows side by side in a launch."""
    case = dc.get("d1000")
    tr = dc.trace(case)
    span = len(case.answers) - 8 + 1
    lens = [j % span for j in range(256)]
    eng = case.make_engine(factory)
    ids = at_prefixes(eng, case.answers, lens)
    for launch in range(9):
        for j, z in enumerate(ids):
            assert np.array_equal(eng.get_priors(z), tr.posts[lens[j]]), (launch, j, lens[j])
        if launch < 8:
            for j, z in enumerate(ids):
                eng.set_active_question(z, case.answers[lens[j]][0])
            eng.record_answer_batch(ids, [case.answers[n][1] for n in lens])
            lens = [n + 1 for n in lens]
    assert max(lens) == len(case.answers)
    eng.close()


def test_long_row_posterior_forms(factory):
    """Rows of 17000 targets: the multi-workgroup StartQuiz / RecordAnswer (long_row_form = 1) and the one-workgroup kernels (0)."""
    case = dc.get("d17000")
    tr = dc.trace(case)
    eng = case.make_engine(factory)
    quizzes = []
    for form in (1, 0):
        eng.set_option("long_row_form", form)
        quizzes.append(eng.start_quiz())
    for s in range(len(case.answers) + 1):
        for form, z in zip((1, 0), quizzes):
            assert np.array_equal(eng.get_priors(z), tr.posts[s]), (s, form)
            if s < len(case.answers):
                eng.set_option("long_row_form", form)
                answer(eng, z, case.answers[s])
    eng.close()


def test_sharded_engine_posteriors_and_priorities(factory, monkeypatch):
    """Two shards of one process: RecordAnswer's row crosses from the shard that holds the question to the other one."""
    case = dc.get("d1000")
    monkeypatch.setenv("PQA_DEVICES", "0,0")
    eng = case.make_engine(factory)
    monkeypatch.delenv("PQA_DEVICES")
    assert eng.get_option("shards") == 2
    worst, _, _ = stepwise(case, eng)
    eng.close()
    report("C sharded d1000", worst)


def test_float_engine_posteriors_and_structure(factory):
    case = dc.get("d1000")
    eng, orc = tb.float_engine(case, factory)
    orc.close()
    stepwise(case, eng, f32=True)
    eng.close()


# ---- D: ResumeQuiz ---------------------------------------------------------------------------------------------------------------
def resumed(case, eng, f32, forms=(None,)):
    """Prefixes of the script of lengths 0, 1, 40, every landmark and all, through ResumeQuiz and one ResumeQuizBatch, both settings of
    bug_compat, 1 / 16 / 64 workers: bit-identical to the oracle's resume_quiz; then the deepest resumed quiz's priorities."""
    lens = sorted(set(dc.landmarks(case, f32)) | {0, 1, min(40, len(case.answers)), len(case.answers)})
    orc = dc.make_oracle(case, f32)
    worst = (0.0, None)
    for form in forms:
        if form is not None:
            eng.set_option("long_row_form", form)
        for workers in (1, 16, 64):
            eng.set_option("workers", workers)
            for bug in (0, 1):
                eng.set_option("bug_compat", bug)
                want = []
                for n in lens:
                    if n == 0:
                        orc.start_quiz(workers)
                    else:
                        assert orc.resume_quiz(case.answers[:n], workers, bool(bug)) == 0, (n, workers, bug)
                    want.append(orc.priors())
                batch = eng.resume_quiz_batch([aq_list(case.answers[:n]) for n in lens])
                for n, zb, post in zip(lens, batch, want):
                    zs = eng.resume_quiz(aq_list(case.answers[:n]))
                    assert np.array_equal(eng.get_priors(zs), post), (case.name, form, workers, bug, n, "ResumeQuiz")
                    assert np.array_equal(eng.get_priors(zb), post), (case.name, form, workers, bug, n, "ResumeQuizBatch")
                    eng.release_quiz(zs)
                nsub, nzero = dc.counts(want[-1], case)
                assert 3 * nzero >= case.T and (nsub >= 1 or case.name in dc.FLUSHED), (nsub, nzero)
                if workers == W:            # (the oracle holds the deepest state)
                    ref = dc.Ref(orc)
                    pri = eng.eval_priorities(batch[-1], case.Q)
                    if f32:
                        structure(pri, ref, (case.name, form, bug))
                    else:
                        worst = held(pri, ref, worst, (case.name, "form %s" % form, "bug_compat %d" % bug))
                for z in batch:
                    eng.release_quiz(z)
    orc.close()
    return worst


def test_resume_double(factory):
    case = dc.get("d1000")
    eng = case.make_engine(factory)
    report("D d1000", resumed(case, eng, False))
    eng.close()


def test_resume_float(factory):
    case = dc.get("d1000")
    eng, orc = tb.float_engine(case, factory)
    orc.close()
    resumed(case, eng, True)
    eng.close()


def test_resume_long_rows(factory):
    case = dc.get("d17000")
    eng = case.make_engine(factory)
    report("D d17000", resumed(case, eng, False, forms=(1, 0)))
    eng.close()


@pytest.mark.parametrize("name", ["d2000k3", "d5000"])
def test_resume_reaches_the_flush(name, factory):
    """250 answers on rows of 2000 and 5000 targets take most of the row below NormalizePriors' threshold, 2030 binades under the
    maximum (deep_cases.flush_counts), which the 1000-target script does not reach: resume_quiz_body's flush decides those elements."""
    case = dc.get(name)
    eng = case.make_engine(factory)
    report("D %s" % name, resumed(case, eng, False))
    eng.close()


def test_resume_long_rows_reach_the_flush(factory):
    """The same on rows of 17000 targets, where 130 answers stop 500 binades short of it: the three-launch resume's flush."""
    case = dc.get("d17000r")
    eng = case.make_engine(factory)
    report("D d17000r", resumed(case, eng, False, forms=(1, 0)))
    eng.close()


# ---- E: batched sweeps -----------------------------------------------------------------------------------------------------------
BATCHED = [("d1000", 1, 3), ("d1000", 2, 54), ("d1000", 3, 14), ("d5000", 1, 3), ("d5000", 2, 54)]


@pytest.mark.parametrize("name,form,n_extra", BATCHED, ids=["%s_form%d" % (n, f) for n, f, _ in BATCHED])
def test_batched_sweeps_at_the_landmarks(name, form, n_extra, factory):
    """One quiz per landmark prefix plus copies through the quiz-per-grid.y launches (1), the row-sharing sweep (2) and the
    (quiz, chunk) sweep (3): priorities, the argmax batch and the sampled batch against the oracle."""
    case = dc.get(name)
    tr = dc.trace(case)
    marks = dc.landmarks(case)
    refs = dc.reference(case, marks)
    eng = case.make_engine(factory)
    eng.set_option("batch_form", form)
    eng.set_option("batch_min", 1)
    lens = [marks[j % len(marks)] for j in range(len(marks) + n_extra)]
    ids = at_prefixes(eng, case.answers, lens)
    pri = eng.eval_priorities_batch(ids, case.Q)
    picks = eng.next_question_argmax_batch(ids)
    rnds = [dc.RNDS[j % len(dc.RNDS)] for j in range(len(ids))]
    sampled = eng.next_question_sampled_batch(ids, rnds)
    worst, decided = (0.0, None), 0
    for j, n in enumerate(lens):
        ref = refs[n]
        assert np.array_equal(eng.get_priors(ids[j]), tr.posts[n]), (name, j, n)
        worst = held(pri[j], ref, worst, (name, "quiz %d" % j, n))
        if ref.margin > DECIDED:
            decided += 1
            assert picks[j] == ref.want, (name, j, n, picks[j], ref.want, ref.margin)
        assert sampled[j] == ref.sampled[j % len(dc.RNDS)], (name, j, n, hex(rnds[j]))
    eng.close()
    report("E %s batch_form %d, %d quizzes" % (name, form, len(ids)), worst)
    assert 2 * decided >= len(ids)


# ---- F: the Among call and the listings ------------------------------------------------------------------------------------------
def test_among_and_listings_at_the_landmarks(factory):
    case = dc.get("d1000")
    tr = dc.trace(case)
    marks = dc.landmarks(case)
    refs = dc.reference(case, marks)
    eng, orc = case.make_engine(factory), case.make_oracle()
    ids = at_prefixes(eng, case.answers, marks)
    orc.start_quiz(W)
    worst, played = (0.0, None), 0
    for z, n in zip(ids, marks):
        while played < n:
            orc.record_answer(*case.answers[played], W - 1)
            played += 1
        post = tr.posts[n]
        assert np.array_equal(orc.priors(), post) and np.array_equal(eng.get_priors(z), post), n
        unasked = [q for q in range(case.Q) if q not in {x for x, _ in case.answers[:n]}]
        among = eng.eval_priorities_among(z, unasked)
        rel = cases.rel_err(among, refs[n].opri[unasked])
        assert (among > 0).all() and rel.max() < BAR, (n, float(rel.max()))
        worst = max(worst, (float(rel.max()), ("among", n)), key=lambda w: w[0])
        positive = int((post > 0).sum())
        for count in (1, 10, 32, case.T):
            got = [(t.i_target, t.prob) for t in eng.list_top_targets(z, count)]
            assert got == orc.list_top_targets(count, W), (n, count)
            assert len(got) == min(count, positive) and all(p > 0 for _, p in got), (n, count)
            assert [(t.i_target, t.prob) for t in eng.list_top_targets_batch([z], count)[0]] == got, (n, count, "batch")
        own = eng.eval_priorities(z)                # (descending priority, ascending question among equals; values bit for bit)
        order = [int(q) for q in np.lexsort((np.arange(case.Q), -own)) if own[q] > 0][:10]
        assert eng.list_top_questions(z, 10) == [(q, float(own[q])) for q in order], n
    both = eng.list_top_targets_batch(ids, 32)
    for z, n, lst in zip(ids, marks, both):
        assert [(t.i_target, t.prob) for t in lst] == [(t.i_target, t.prob) for t in eng.list_top_targets(z, 32)], n
    eng.close()
    orc.close()
    report("F among", worst)
