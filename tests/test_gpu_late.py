"""Late quiz states on every kernel form: a posterior element at 1 - 1e-4 ... 1 - 1e-16 (and exactly 1), where the reference's
lack term -sum invD^2 / log2(p) (PqaCore/CEEvalQsSubtaskConsider.cpp:117) has its pole and the ORDER in which W_k was summed
(SRPlatform/Interface/SRAccumVectDbl256.h:40-46, :62-92) decides the ninth digit of the priority -- or, a few answers later, its
first.  That is where real quizzes end (a handful of consistent answers), and the random cases of tests/test_gpu_fuzz.py hardly
ever get there: their answers are random, their rows short.

The cases here are dichotomy quizzes as the reference's own DichotomyTest plays them (PqaCoreTests/DichotomyTest.cpp:50-64): a
window of the synthetic cube with one question per target around a hidden target (probqa_amd/synth.py with q_total = T), answered
consistently 4 - 8 questions deep -- "it is the target" / "just below" / "just above" -- so that the posterior collapses onto the
hidden target by a factor of a few hundred per answer.  Legs: every register shape for rows beyond 4096 targets (the defaults by
row length and the forced ones), the short-row shapes with one or two workgroups streaming more questions than the in-kernel fix
lists, the streaming fallback, both cluster forms (rows of 20000 / 50000 targets), the (quiz, chunk) and row-sharing batched
sweeps, the quiz-per-grid.y launches, and the resident sweep (picks).  Every step of every case is held to 1e-9 against the oracle;
the posterior stays bit-identical; the argmax and the reference's sampled selector pick the oracle's questions.

`pytest -m gpu tests/test_gpu_late.py --late N [--late-first SEED]` runs N more cases than the suite's own."""
import numpy as np
import pytest

import cases
import test_gpu_batch as tb
from deep_cases import LateCase
from probqa_amd import synth
from test_gpu_parity import run_script

pytestmark = pytest.mark.gpu


# (leg, row lengths, engine options)
REG_DEFAULT = [4608, 5120, 6144, 7168, 8192, 9216, 10000, 10240, 16384, 12000]
REG_FORCED = [(8000, 5), (10000, 6), (5000, 9), (10000, 11), (10000, 12), (5000, 21), (3000, 22), (4000, 23), (4500, 24), (5000, 20),
              (900, 1), (1000, 8), (2000, 3), (4096, 4), (16384, 7), (12000, 7)]   # (7: the 16-wave shape, selectable; rows beyond 10240 targets take the cluster sweep by default)
LEGS = ["reg", "reg", "forced", "stream", "cluster", "overflow", "short", "mid", "rowshare", "gridy", "server", "reg"]


def late_case(i):
    rng = np.random.default_rng(770000 + i)
    leg = LEGS[i % len(LEGS)]
    options, K = [], 5
    if leg == "reg":
        T = int(rng.choice(REG_DEFAULT)) if rng.random() < 0.7 else int(rng.integers(4097, 16385))
        Q = int(rng.integers(12, 40))
        if rng.random() < 0.3:
            options.append(("eval_max_grid", int(rng.integers(1, 4))))
    elif leg == "forced":
        T, v = REG_FORCED[int(rng.integers(len(REG_FORCED)))]
        T -= int(rng.integers(0, 40))
        Q = int(rng.integers(12, 40))
        options.append(("eval_variant", v))
        if rng.random() < 0.3:
            options.append(("eval_max_grid", 2))
    elif leg == "stream":
        T, Q = int(rng.integers(300, 9000)), int(rng.integers(8, 30))
        options.append(("eval_variant", 99))
    elif leg == "cluster":
        T, Q = int(rng.choice([20000, 50000, 17000, 33000])), int(rng.integers(8, 20))
        options.append(("cluster_form", int(rng.choice([1, 2]))))
    elif leg == "overflow":   # hundreds of suspects per workgroup (round 4's in-kernel fix listed 62 and let the rest be)
        T, Q = int(rng.integers(64, 1500)), int(rng.integers(70, 200))
        options.append(("eval_max_grid", 1))
    elif leg == "short":
        T, Q = int(rng.integers(40, 4097)), int(rng.integers(10, 60))
    elif leg == "mid":
        T, Q = int(rng.integers(100, 2400)), int(rng.integers(10, 40))
    elif leg == "rowshare":
        T, Q = int(rng.choice([4608, 6000, 10000, 2000, 700])), int(rng.integers(8, 24))
    elif leg == "gridy":
        T, Q = int(rng.choice([1000, 3000, 5000, 10000])), int(rng.integers(8, 24))
    else:   # server
        T, Q = int(rng.integers(100, 1025)), int(rng.integers(10, 60))
        options.append(("server", 1))
    if leg in ("reg", "forced", "stream", "short", "overflow", "rowshare") and rng.random() < 0.35:
        K = int(rng.integers(3, 9))
    Q = min(Q, T)
    hidden = int(rng.integers(Q, T - Q)) if T > 3 * Q else T // 2
    q_offset = min(max(hidden - Q // 2, 0), T - Q)
    depth = int(rng.integers(4, 9))
    # the dichotomy's answers around the hidden target: the question about it, then alternately the ones just above / just below
    order = [0] + [s * d for d in range(1, Q) for s in (1, -1)]
    answers = []
    for off in order:
        x = hidden + off
        q = x - q_offset
        if 0 <= q < Q and len(answers) < depth:
            answers.append((q, min(synth.dichotomy_answer(x, hidden, max(1, (32 * T) // 1000)), K - 1)))
    if rng.random() < 0.5:
        rng.shuffle(answers)
    answers = [(int(q), int(a)) for q, a in answers]
    n_tg = int(rng.integers(0, 6)) if rng.random() < 0.3 else 0
    tgaps = sorted(int(t) for t in rng.choice([t for t in range(T) if t != hidden], n_tg, replace=False)) if n_tg else []
    name = "late%04d_%s_%dx%dx%d" % (i, leg, Q, K, T)
    case = LateCase(name, K, Q, T, seed=3000 + i, hidden=hidden, q_offset=q_offset, init=float(rng.choice([0.1, 0.5])),
                    n_train=float(rng.choice([4.0, 8.0])), noise=float(rng.choice([0.1, 0.5])), tgaps=tgaps, answers=answers)
    return leg, case, options


def batched_states(case, factory, form, n_extra):
    """One quiz per prefix of the answer script (plus copies) through a batched sweep; returns the worst step."""
    eng, orc = case.make_engine(factory), case.make_oracle()
    eng.set_option("batch_form", form)
    eng.set_option("batch_min", 1)
    quizzes, hists = [], []
    n = len(case.answers) + 1 + n_extra
    for j in range(n):
        quiz = eng.start_quiz()
        hist = case.answers[: j % (len(case.answers) + 1)]
        for q, a in hist:
            eng.set_active_question(quiz, q)
            eng.record_answer(quiz, a)
        quizzes.append(quiz)
        hists.append(hist)
    pri = eng.eval_priorities_batch(quizzes, case.Q)
    picks = eng.next_question_argmax_batch(quizzes)
    worst, seen = 0.0, {}
    for j in range(n):
        key = len(hists[j])
        if key not in seen:
            opri, opriors = tb.oracle_priorities(orc, hists[j])
            seen[key] = (opri, opriors, orc.select_argmax(opri))
        opri, opriors, want = seen[key]
        assert np.array_equal(eng.get_priors(quizzes[j]), opriors), (case.name, j)
        if pri is not None:
            rel = tb.rel_vec(pri[j], opri)
            worst = max(worst, float(rel.max()))
            assert (rel < 1e-9).all(), (case.name, j, key, float(rel.max()), int(rel.argmax()))
        top = np.sort(opri)[::-1]
        margin = (top[0] - top[1]) / top[0] if len(top) > 1 and top[0] > 0 else 1.0
        if want < 0:
            assert picks[j] == -1
        elif margin > 1e-8:
            assert picks[j] == want, (case.name, j, key, picks[j], want, margin)
    eng.close()
    return worst


def run_late_case(i, factory):
    leg, case, options = late_case(i)
    if leg == "mid":
        return leg, case, batched_states(case, factory, 3, int(i % 23))
    if leg == "rowshare":
        return leg, case, batched_states(case, factory, 2, int(i % 70))
    if leg == "gridy":
        return leg, case, batched_states(case, factory, 1, int(i % 5))
    return leg, case, max(run_script(case, factory, options))


@pytest.mark.parametrize("i", range(60))
def test_late_state(i, factory):
    leg, case, worst = run_late_case(i, factory)
    assert worst < 1e-9, (case.name, worst)


@pytest.mark.parametrize("i", [0, 2, 6, 10, 12, 26, 30])
def test_lazy_and_eager_fix_agree(i, factory):
    """Synchronous single-quiz selections launch the fix of pole_kernels.hip only when the sweep has listed something (engine option
    pole_lazy, default on: FusedSelect::lazyFix); with pole_lazy = 0 it is launched behind every sweep.  Same picks by the argmax
    and by the reference's selector (host hand-over form) on every step of late-state cases."""
    leg, case, options = late_case(i)
    if leg in ("mid", "rowshare", "gridy", "cluster"):
        pytest.skip("single-quiz register shapes only")
    picks = []
    for lazy in (1, 0):
        eng = case.make_engine(factory)
        for n, v in options:
            eng.set_option(n, v)
        eng.set_option("speculate", 0)
        eng.set_option("pole_lazy", lazy)
        assert eng.get_option("pole_lazy") == lazy
        quiz = eng.start_quiz()
        got = []
        for step in range(len(case.answers) + 1):
            got.append((eng.next_question_argmax(quiz), eng.next_question_sampled(quiz, 0x9E3779B97F4A7C15 * (step + 1) % 2**64)))
            if step < len(case.answers):
                q, a = case.answers[step]
                eng.set_active_question(quiz, q)
                eng.record_answer(quiz, a)
        eng.close()
        picks.append(got)
    assert picks[0] == picks[1], (case.name, picks)


@pytest.mark.parametrize("late_eager", [1, 0, 1000000])
@pytest.mark.parametrize("select", [1, 0])
def test_late_eager_after_a_lazy_fix(select, late_eager, factory):
    """Engine option late_eager = 1 (Quiz::lateStreak): the first selection of a quiz whose sweep lists a row takes the lazy fix -- the
    sweep answers "redo", the fix is launched behind that answer --, every later one has the fix launched right behind its sweep
    again; 0: always behind the sweep; a large value: always lazily.  Two selections per step of the smallest single-quiz late case
    of this file, through NextQuestion with the argmax (select = 1) and with the reference's selector at a fixed seed (select = 0):
    the picks are those of an identical second engine with pole_lazy = 0, whose fix follows every sweep.  That the case's sweep
    does list a row is shown by its priorities, which change when the fix is switched off.  (No counter of the engine tells a
    lazily launched fix from an eager one, so beyond that the picks are all that is compared.)"""
    leg, case, options = late_case(2)
    picks, final = [], []
    for lazy, fix in ((1, 1), (0, 1), (0, 0)):
        eng = case.make_engine(factory)
        for n, v in options:
            eng.set_option(n, v)
        eng.set_option("speculate", 0)
        eng.set_option("pole_fix", fix)
        eng.set_option("pole_lazy", lazy)
        eng.set_option("late_eager", late_eager)
        eng.set_option("select", select)
        eng.set_option("seed", 20260)
        quiz = eng.start_quiz()
        got = []
        for step in range(len(case.answers) + 1):
            got.append((eng.next_question(quiz), eng.next_question(quiz)))
            if step < len(case.answers):
                q, a = case.answers[step]
                eng.set_active_question(quiz, q)
                eng.record_answer(quiz, a)
        final.append(eng.eval_priorities(quiz).copy())
        eng.close()
        picks.append(got)
    assert not np.array_equal(final[1], final[2]), (case.name, "the sweep lists no row: nothing for the fix to do")
    assert np.array_equal(final[0], final[1])
    assert all(q >= 0 for pair in picks[0] for q in pair), (case.name, picks[0])
    assert picks[0] == picks[1], (case.name, picks)


@pytest.mark.parametrize("i", [5, 6, 12, 17])
def test_measurement_hook_without_the_fix_is_harmless(i, factory):
    """Option pole_follow = 0 (bench.py times the watching sweep by itself with it): in a late state the sweep then lists nothing and
    defers nothing -- a fused selection answers at once with the sweep's own sums instead of waiting for a fix that never comes --,
    however often it runs; back at 1 the next selection is the reference-order one again."""
    import time

    leg, case, options = late_case(i)
    assert leg in ("short", "overflow", "reg", "forced"), leg
    eng, orc = case.make_engine(factory), case.make_oracle()
    for n, v in options:
        eng.set_option(n, v)
    quiz = eng.start_quiz()
    orc.start_quiz(cases.WORKERS)
    for q, a in case.answers:
        eng.set_active_question(quiz, q)
        eng.record_answer(quiz, a)
        orc.record_answer(q, a, cases.WORKERS - 1)
    _, opri = orc.eval(8 * cases.WORKERS)
    for lazy in (1, 0):
        eng.set_option("pole_lazy", lazy)
        eng.set_option("pole_follow", 0)
        t0 = time.perf_counter()
        for _ in range(300):                     # (more sweeps than the list has entries: nothing accumulates)
            eng.enqueue_eval(quiz)
        picks = {eng.next_question_argmax(quiz) for _ in range(20)}
        eng.synchronize()
        assert time.perf_counter() - t0 < 10.0 and len(picks) == 1
        eng.set_option("pole_follow", 1)
        pri = eng.eval_priorities(quiz)
        live = opri != 0
        assert cases.rel_err(pri[live], opri[live]).max() < 1e-9
        top = np.sort(opri)[::-1]
        if top[0] > 0 and (top[0] - top[1]) / top[0] > 1e-8:
            assert eng.next_question_argmax(quiz) == orc.select_argmax(opri)
    eng.close()


@pytest.mark.parametrize("i", [0, 1, 2, 5, 6, 11, 12, 13, 14, 17, 18, 23, 26, 29, 30, 35, 38, 42, 47, 50, 54, 59])
def test_gated_fix_picks_what_the_full_fix_picks(i, factory):
    """Engine option pole_gate (default on): NextQuestion with the argmax selector has only the listed questions redone that can still
    be the maximum (pole_kernels.hip: pole_bounds_kernel).  Every step of late-state cases, register shapes: the same question as with
    every listed question redone, and the oracle's where its two best are told apart."""
    leg, case, options = late_case(i)
    if leg in ("mid", "rowshare", "gridy", "cluster", "server"):
        pytest.skip("single-quiz launched register shapes")
    eng, orc = case.make_engine(factory), case.make_oracle()
    for n, v in options:
        eng.set_option(n, v)
    eng.set_option("speculate", 0)
    quiz = eng.start_quiz()
    orc.start_quiz(cases.WORKERS)
    for step in range(len(case.answers) + 1):
        picks = []
        for gate, lazy in ((1, 1), (0, 1), (1, 0), (0, 0)):
            eng.set_option("pole_gate", gate)
            eng.set_option("pole_lazy", lazy)
            picks.append(eng.next_question_argmax(quiz))
        assert len(set(picks)) == 1, (case.name, step, picks)
        _, opri = orc.eval(8 * cases.WORKERS)
        top = np.sort(opri)[::-1]
        if top[0] > 0 and (top[0] - top[1]) / top[0] > 1e-8:
            assert picks[0] == orc.select_argmax(opri), (case.name, step)
        eng.set_option("pole_gate", 1)
        pri = eng.eval_priorities(quiz)                      # (every listed question redone, whatever the gate)
        live = opri != 0
        assert cases.rel_err(pri[live], opri[live]).max() < 1e-9, (case.name, step)
        if step < len(case.answers):
            q, a = case.answers[step]
            eng.set_active_question(quiz, q)
            eng.record_answer(quiz, a)
            orc.record_answer(q, a, cases.WORKERS - 1)
    eng.close()


@pytest.mark.parametrize("i", [11, 24])
def test_rerouted_rows_again_and_again(i, factory):
    """Rows of 10241..16384 targets take the cluster sweep since round 6 -- clusters of 11..16 members, shorter slices than the rows
    that sweep was built for.  The same late case thirty times over (three answers / five answers per question): a race between the
    members shows as a rare wrong priority, not as a wrong one every time (round 6: the five-answer kernel's schedule instantiated for
    two to four answers failed 10 of 150 such runs by up to 10^4 x and was taken out again; these two forms: 0 of 400)."""
    leg, case, options = late_case(i)
    assert case.T > 10240 and leg == "reg"
    for rep in range(30):
        worst = max(run_script(case, factory, options))
        assert worst < 1e-9, (case.name, rep, worst)


def test_late_soak(factory, late):
    """--late N further cases; prints the worst step per leg."""
    n, first = late
    if n <= 0:
        pytest.skip("no --late N given")
    worst, bad = {}, []
    for i in range(first, first + n):
        try:
            leg, case, w = run_late_case(i, factory)
            if w >= worst.get(leg, (-1.0, ""))[0]:
                worst[leg] = (w, case.name)
        except BaseException as ex:  # noqa: BLE001
            if isinstance(ex, KeyboardInterrupt):
                raise
            leg, case, _ = late_case(i)
            bad.append((i, case.name, repr(ex)[:240]))
            print("FAIL", bad[-1])
    print("late-state soak: %d cases from seed %d, worst relative deviation per leg: %s" % (
        n, first, {k: "%.2e %s" % v for k, v in sorted(worst.items())}))
    assert not bad, (len(bad), bad[:8])
