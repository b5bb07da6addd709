"""Float engines' selections where the fp32 sweep cannot decide them, against the fp64 oracle on the rounded cube.

A Float engine's batched argmax lets the fp32 sweep NOMINATE each quiz's 8 best questions (eval_kernels.hip: batch_topk_kernel),
evaluates those in fp64 (batch_rerank_kernel) and returns their fp64 argmax (batch_repick_kernel).  On the fixtures the fp32 sweep
alone names the oracle's question almost everywhere, so none of the three kernels decides anything there.  Here they do:

* CROWDED states (tests/float_cases.py): n + 1 questions within a few 1e-7 of each other at the top, everything else ten fp32
  tolerances below.  The fp32 sweep collapses the crowd onto a few values; the fp64 order inside it is in the eighth and ninth
  digit.  With 3 and 7 copies the crowd fits the width of 8 and the pick must be the oracle's argmax; with 24 it does not, and
  the pick must be the fp64 argmax of the 8 the sweep nominated -- a member of the crowd.
* LATE states (tests/test_gpu_late.py: late_case): a posterior concentrated on one target, where an fp32 sweep is off by
  1e-6 .. 1e-2 and the re-rank has no pole fix.  Batched: the oracle's argmax where its margin exceeds 1e-5 (ten times the largest
  deviation the project has recorded for fp64 sums in another order in these cases).  Single quiz: no fp64
  promise, the structure of the answer.

Measured on an MI355X (each test prints its figures; DESIGN.md section 5, "fp32, the argmax"): the re-ranked priority within 7.9e-14
of the oracle's; with 24 copies the oracle's argmax picked in 14 of 23 decided states, every pick inside the crowd; in late states
the oracle's argmax reaches rank 6 of the fp32 order, against the width of 8; built with a width of 4 the 7- and 24-copy cases fail."""
import re

import numpy as np
import pytest

import cases
import float_cases
import orclib
import test_gpu_batch as tb
import test_gpu_late as tl
from probqa_amd import dist as pdist
from probqa_amd import interop, synth

pytestmark = pytest.mark.gpu

WIDTH = 8                   # eval_kernels.hip: kRerank
UNDECIDED = 1e-9            # a top-2 margin up to this is fp64's own noise (tb.PRIORITY_RTOL)
LATE_BAR = 1e-5
ANSWERS = [(3, 1), (17, 4)]
SEEDS = range(40, 52)
BATCHES = [8, 96, 200]      # batch_kernels.hip: one, two and four questions per block of the fp32 sweep
LATE_BATCHED = [54, 5, 8, 2, 19, 18, 14, 6, 30, 39, 49, 0, 50, 35]      # rows of 271 .. 8192 targets, 4 / 5 / 8 answers
# single quiz: 256 threads x 1 / 2 / 3 / 4 quads, 320 and 512 x 4, the DMA form (8584 targets), the cluster sweep (17000 targets)
LATE_SINGLE = [54, 19, 6, 39, 49, 35, 108, 16]


def margin_of(values):
    top = np.sort(values)[::-1]
    return float((top[0] - top[1]) / top[0]) if len(top) > 1 and top[0] > 0 else 1.0


def fp32_order(row, excluded):
    """The questions in the order batch_topk_kernel takes them: priority descending, index ascending among equal values, NaN last,
    asked and gap questions left out."""
    p = np.where(np.isnan(row), -np.inf, row)
    return [int(q) for q in np.lexsort((np.arange(len(p)), -p)) if int(q) not in excluded]


def oracle_pick(opri, ids):
    """The fp64 argmax over ids (lowest index among equal values) and the top-2 margin within ids."""
    best = max(opri[q] for q in ids)
    return min(q for q in ids if opri[q] == best), margin_of(opri[list(ids)])


def quizzes_at_prefixes(eng, hist, lens):
    """One quiz per entry of lens, in the state after hist[:len]: started in one launch, answered in one launch per step."""
    ids = eng.start_quiz_batch(len(lens))
    for step, (q, a) in enumerate(hist):
        live = [z for z, n in zip(ids, lens) if n > step]
        for z in live:
            eng.set_active_question(z, q)
        if live:
            eng.record_answer_batch(live, [a] * len(live))
    return ids


def check_nominated_picks(eng, ids, lens, hist, opri_at, gaps, bar, what):
    """Assertion 3 of the file: two sweeps give the same matrix; from it, every quiz's nominated set; the pick is the oracle's
    argmax over that set wherever the set's own top-2 margin exceeds `bar`; quizzes in the same state pick alike.  Returns
    (matrix, picks, nominated sets)."""
    n_q = len(opri_at[0])
    matrix = eng.eval_priorities_batch(ids, n_q)
    assert np.array_equal(matrix, eng.eval_priorities_batch(ids, n_q)), (what, "two sweeps of one batch differ")
    picks = eng.next_question_argmax_batch(ids)
    sets, by_state = [], {}
    for j, n in enumerate(lens):
        nom = fp32_order(matrix[j], set(gaps) | {q for q, _ in hist[:n]})[:WIDTH]
        sets.append(nom)
        want, margin = oracle_pick(opri_at[n], nom)
        if margin > bar:
            assert picks[j] == want, (what, j, n, "picked", picks[j], "fp64 argmax of the nominated", want, nom, margin)
        assert by_state.setdefault(n, picks[j]) == picks[j], (what, j, n, "quizzes in one state pick differently")
    return matrix, picks, sets


# ---- crowded states -----------------------------------------------------------------------------------------------------------
class CrowdState:
    """One crowded cube and the oracle's view of the state after its answers, and of every shorter prefix of them."""

    def __init__(self, seed, n_copies, depth):
        self.case, orc = float_cases.crowded(5, 64, 400, seed, n_copies, 0.3, ANSWERS[:depth])
        self.hist = list(self.case.answers)
        self.opri_at, self.priors_at = [], []
        for n in range(depth + 1):
            opri, priors = tb.oracle_priorities(orc, self.hist[:n])
            self.opri_at.append(opri)
            self.priors_at.append(priors)
        self.opri = self.opri_at[-1]
        self.tol = float(tb.f32_tolerance(orc, self.case).max())
        self.want = int(orc.select_argmax(self.opri))
        order = np.argsort(-self.opri, kind="stable")
        top = self.opri[order]
        self.best = sorted(int(q) for q in order[: n_copies + 1])
        self.margin = float((top[0] - top[1]) / top[0])
        self.spread = float((top[0] - top[n_copies]) / top[0])
        self.gap = float((top[n_copies] - top[n_copies + 1]) / top[0])
        self.decided = self.margin > UNDECIDED
        orc.close()

    def lens(self, n_quizzes):
        """Two quizzes of three in the crowded state, the third in one of the states before it."""
        d = len(self.hist)
        return [d if j % 3 else (j // 3) % d for j in range(n_quizzes)]

    def engine(self, factory):
        eng, orc = tb.float_engine(self.case, factory)
        orc.close()
        eng.set_option("batch_min", 1)
        return eng


_crowds = {}


def crowd_states(n_copies):
    """The 24 states of a crowd size (12 cubes x the states after one and after two answers), computed once."""
    if n_copies not in _crowds:
        _crowds[n_copies] = [CrowdState(seed, n_copies, depth) for seed in SEEDS for depth in (1, 2)]
    return _crowds[n_copies]


def check_preconditions(states, n_copies):
    """From the oracle alone: fp32 cannot order the crowd by the project's own stated tolerance, and nothing else can enter it."""
    for s in states:
        assert s.best == s.case.crowd, (s.case.name, s.best, s.case.crowd)
        assert s.spread < 0.1 * tb.F32_RTOL, (s.case.name, s.spread)
        assert s.gap > 10 * s.tol, (s.case.name, s.gap, s.tol)
    undecided = sum(not s.decided for s in states)
    assert 4 * undecided <= len(states), (n_copies, undecided)
    return undecided


@pytest.mark.parametrize("n_copies", [3, 7, 24])
def test_reranked_priority_is_the_oracles(n_copies, factory):
    """The fp64 value the re-rank computes is observable -- PqaHip_SelectArgmaxBatch publishes the winner's priority -- and is the
    oracle's to 1e-9, the bar the Double engine's sweeps meet in these states with another summation order of their own."""
    states = crowd_states(n_copies)
    undecided = check_preconditions(states, n_copies)
    worst = 0.0
    for s in states:
        eng = s.engine(factory)
        lens = s.lens(8)
        ids = quizzes_at_prefixes(eng, s.hist, lens)
        sel = eng.select_argmax_batch(ids)
        for j, n in enumerate(lens):
            winner = int(sel[j, 1])
            assert winner >= 0 and s.opri_at[n][winner] > 0, (s.case.name, j, winner)
            dev = abs(sel[j, 0] - s.opri_at[n][winner]) / s.opri_at[n][winner]
            worst = max(worst, float(dev))
            assert dev < tb.PRIORITY_RTOL, (s.case.name, j, n, winner, dev)
        eng.close()
    print("%d copies, %d states (%d undecided): worst deviation of the re-ranked priority from the oracle's %.3g" % (
        n_copies, len(states), undecided, worst))


@pytest.mark.parametrize("n_quizzes", BATCHES)
@pytest.mark.parametrize("n_copies", [3, 7, 24])
def test_pick_is_the_fp64_argmax_of_the_nominated(n_copies, n_quizzes, factory):
    """Nomination, re-rank and pick pinned together, at every crowd size -- the one that overflows the width included -- and every
    shape of the fp32 sweep: the pick is the oracle's argmax over the 8 questions the sweep's own matrix puts first."""
    states = crowd_states(n_copies)
    check_preconditions(states, n_copies)
    inside = 0
    for s in states:
        eng = s.engine(factory)
        lens = s.lens(n_quizzes)
        ids = quizzes_at_prefixes(eng, s.hist, lens)
        _, _, sets = check_nominated_picks(eng, ids, lens, s.hist, s.opri_at, (), UNDECIDED, (s.case.name, n_quizzes))
        nom, crowd = set(sets[1]), set(s.case.crowd)            # (quiz 1 is in the crowded state)
        # the next question is ten fp32 tolerances below the crowd: the sweep puts the crowd first, as far as the width goes
        assert crowd <= nom if n_copies < WIDTH else nom <= crowd, (s.case.name, n_quizzes, sorted(nom), s.case.crowd)
        inside += int(s.want in nom)
        eng.close()
    print("%d copies, %d quizzes: the oracle's argmax among the 8 nominated in %d of %d states" % (n_copies, n_quizzes, inside, len(states)))


@pytest.mark.parametrize("n_copies", [3, 7])
def test_crowd_within_the_width_gets_the_oracles_argmax(n_copies, factory):
    """Up to 7 copies the crowd fits the 8 nominations (7 fill them exactly): the pick is the oracle's GLOBAL argmax in every decided
    state.  Guard: without the re-rank (option rerank = 0) some decided state picks otherwise -- else the crowd says nothing."""
    states = crowd_states(n_copies)
    undecided = check_preconditions(states, n_copies)
    differ32 = 0
    for s in states:
        eng = s.engine(factory)
        lens = s.lens(8)
        ids = quizzes_at_prefixes(eng, s.hist, lens)
        picks = eng.next_question_argmax_batch(ids)
        eng.set_option("rerank", 0)
        picks32 = eng.next_question_argmax_batch(ids)
        eng.set_option("rerank", 1)
        crowded = [j for j, n in enumerate(lens) if n == len(s.hist)]
        assert all(picks[j] in s.case.crowd for j in crowded), (s.case.name, picks)
        if s.decided:
            assert all(picks[j] == s.want for j in crowded), (s.case.name, picks, s.want, s.margin)
            differ32 += int(picks32[crowded[0]] != s.want)
        eng.close()
    print("%d copies: %d of %d states decided beyond 1e-9; fp32 alone picks another question than the oracle in %d of them" % (
        n_copies, len(states) - undecided, len(states), differ32))
    assert differ32 >= 1


def test_crowd_beyond_the_width_stays_in_the_crowd(factory):
    """24 copies: the 8 nominations cannot hold the crowd, so the oracle's argmax may be left out -- but whatever is picked is a member
    of the crowd, which by the preconditions puts its fp64 priority within 0.1 x F32_RTOL of the maximum."""
    states = crowd_states(24)
    undecided = check_preconditions(states, 24)
    same = 0
    for s in states:
        eng = s.engine(factory)
        lens = s.lens(8)
        ids = quizzes_at_prefixes(eng, s.hist, lens)
        picks = eng.next_question_argmax_batch(ids)
        crowded = [j for j, n in enumerate(lens) if n == len(s.hist)]
        for j in crowded:
            assert picks[j] in s.case.crowd, (s.case.name, j, picks[j], s.case.crowd)
            assert s.opri[picks[j]] >= s.opri[s.want] * (1 - 0.1 * tb.F32_RTOL)
        same += int(s.decided and picks[crowded[0]] == s.want)
        eng.close()
    print("24 copies: the oracle's argmax picked in %d of the %d states decided beyond 1e-9 (%d states)" % (
        same, len(states) - undecided, len(states)))


def test_float_shards_merge_with_a_crowd(factory):
    """Two Float shards of the question axis, the 7-copy crowd on both sides of the bound: the shards' winners merge (dist.pick_batch)
    to the oracle's argmax in the decided states, and each shard's published priority is the oracle's to 1e-9."""
    from test_gpu_record_ranks import pack_and_consume

    states = crowd_states(7)
    check_preconditions(states, 7)
    K, Q, T = 5, 64, 400
    bounds = pdist.shard_bounds(Q, 2)
    firsts = [0] + bounds[:-1]
    worst, merged = 0.0, 0
    for s in states:
        assert min(s.case.crowd) < bounds[0] <= max(s.case.crowd), (s.case.name, s.case.crowd)
        A, D, B = s.case.kb()
        shards = []
        for first, limit in zip(firsts, bounds):
            sh = factory.create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=s.case.init,
                                                                    prec_type=interop.PrecisionType.FLOAT, prec_exponent=8,
                                                                    prec_mantissa=24), first, Q, 0)
            sh.set_kb(A[first:limit], D[first:limit], B)
            sh.set_option("workers", cases.WORKERS)
            sh.set_option("batch_min", 1)
            shards.append(sh)
        lens = s.lens(8)
        ids = shards[0].start_quiz_batch(len(lens))
        assert shards[1].start_quiz_batch(len(lens)) == ids
        for step, (q, a) in enumerate(s.hist):
            live = [z for z, n in zip(ids, lens) if n > step]
            for sh in shards:
                for z in live:
                    sh.set_active_question(z, q)
            pack_and_consume(shards, live, [a] * len(live))
        local = np.stack([sh.select_argmax_batch(ids) for sh in shards])
        picks = pdist.pick_batch(local)
        for j, n in enumerate(lens):
            for r, sh in enumerate(shards):
                assert np.array_equal(sh.get_priors(ids[j]), s.priors_at[n]), (s.case.name, j, r)
                winner = int(local[r, j, 1])
                assert firsts[r] <= winner < bounds[r], (s.case.name, j, r, winner)
                dev = abs(local[r, j, 0] - s.opri_at[n][winner]) / s.opri_at[n][winner]
                worst = max(worst, float(dev))
                assert dev < tb.PRIORITY_RTOL, (s.case.name, j, r, winner, dev)
            if n == len(s.hist) and s.decided:
                assert picks[j] == s.want, (s.case.name, j, picks[j], s.want, s.margin)
                merged += 1
        for sh in shards:
            sh.close()
    print("two shards, 7 copies: %d picks merged to the oracle's argmax; worst deviation of a shard's priority %.3g" % (merged, worst))
    assert merged > 0


# ---- late states --------------------------------------------------------------------------------------------------------------
_late = {}


def late_reference(i):
    """(case, per prefix of its answers: (oracle priorities, posterior, argmax, top-2 margin)) on the cube rounded to fp32, once."""
    if i not in _late:
        _, case, _ = tl.late_case(i)
        orc = orclib.Oracle(case.K, case.Q, case.T, case.init)
        orc.set_kb(*(x.astype(np.float32).astype(np.float64) for x in case.kb()))
        orc.set_target_gaps(case.tgaps)
        orc.set_question_gaps(case.qgaps)
        steps = []
        for n in range(len(case.answers) + 1):
            opri, priors = tb.oracle_priorities(orc, case.answers[:n])
            steps.append((opri, priors, int(orc.select_argmax(opri)), margin_of(opri)))
        orc.close()
        _late[i] = (case, steps)
    return _late[i]


@pytest.mark.parametrize("n_quizzes", [8, 200])
def test_float_late_states_batched(n_quizzes, factory):
    """One quiz per prefix of a late case's answer script (the deepest first, then copies): posteriors bit for bit, the pick the
    oracle's argmax where its margin exceeds 1e-5, and the fp64 argmax of the nominated wherever that is decided by 1e-5.  Guard:
    somewhere the oracle's argmax is NOT the first of the fp32 order, so the re-rank decides."""
    states = under = moved = 0
    deepest = (0, "")
    for i in LATE_BATCHED:
        case, steps = late_reference(i)
        assert case.T <= 9000
        eng, orc = tb.float_engine(case, factory)
        orc.close()
        eng.set_option("batch_min", 1)
        n_prefixes = len(steps)
        lens = [(n_prefixes - 1 - j) % n_prefixes for j in range(n_quizzes)]
        ids = quizzes_at_prefixes(eng, case.answers, lens)
        matrix, picks, _ = check_nominated_picks(eng, ids, lens, case.answers, [st[0] for st in steps], case.qgaps, LATE_BAR,
                                                 (case.name, n_quizzes))
        seen = set()
        for j, n in enumerate(lens):
            opri, priors, want, margin = steps[n]
            assert np.array_equal(eng.get_priors(ids[j]), priors), (case.name, j, n)
            assert want >= 0
            if margin > LATE_BAR:
                assert picks[j] == want, (case.name, j, n, picks[j], want, margin)
            if n not in seen:
                seen.add(n)
                states += 1
                under += int(margin <= LATE_BAR)
                rank = fp32_order(matrix[j], set(case.qgaps) | {q for q, _ in case.answers[:n]}).index(want)
                moved += int(rank > 0)
                deepest = max(deepest, (rank, "%s after %d answers" % (case.name, n)))
        eng.close()
    print("%d quizzes per batch, %d late states: %d under the 1e-5 bar; the oracle's argmax is not the fp32 sweep's first in %d, "
          "its largest fp32 rank is %d (%s)" % (n_quizzes, states, under, moved, deepest[0], deepest[1]))
    assert 10 * under <= states
    assert moved >= 1


def deep_dichotomy():
    """200 x 5 x 200, one question per target, 30 consistent answers around a hidden target: posterior elements far below fp32's range."""
    K, n, hidden, width = 5, 200, 83, max(1, (32 * 200) // 1000)
    offsets = [0] + [s * d for d in range(1, n) for s in (1, -1)]
    asked = [hidden + off for off in offsets if 0 <= hidden + off < n][:30]
    answers = [(x, synth.dichotomy_answer(x, hidden, width)) for x in asked]
    return cases.Case("deep_200x5x200", K, n, n, seed=8301, n_train=8.0, noise=0.5, answers=answers)


SINGLE = [("late%d" % i, i) for i in LATE_SINGLE] + [("deep_dichotomy", None)]


@pytest.mark.parametrize("name,i", SINGLE, ids=[n for n, _ in SINGLE])
def test_float_late_states_single(name, i, factory):
    """A Float engine's single-quiz argmax selects by fp32 values and makes no fp64 promise; what must hold at every step of a late
    quiz, on every form of the fp32 sweep, is structure: the posterior bit for bit, priorities finite, non-negative and zero exactly
    where the oracle's are, the pick the first maximum of the engine's own vector and never an asked or gap question -- and the
    oracle's argmax where the oracle's margin exceeds ten times the fp32 tolerance, which the first steps of every case do."""
    case = deep_dichotomy() if i is None else tl.late_case(i)[1]
    eng, orc = tb.float_engine(case, factory)
    kernel = eng.eval_kernel_name()
    print(case.name, kernel)
    assert re.match({"late54": r"f32_wg256_nq1$", "late19": r"f32_wg256_nq2$", "late6": r"f32_wg256_nq3$",
                     "late39": r"f32_wg256_nq4$", "late49": r"f32_wg320_nq4$", "late35": r"f32_wg512_nq4$", "late108": r"f32_wg\d+_nq5$",
                     "late16": r"f32_cluster", "deep_dichotomy": r"f32_wg256_nq1$"}[name], kernel), kernel
    quiz = eng.start_quiz()
    orc.start_quiz(cases.WORKERS)
    asked, qualified = set(case.qgaps), 0
    for step in range(len(case.answers) + 1):
        priors = orc.priors()
        assert np.array_equal(eng.get_priors(quiz), priors), (case.name, step)
        _, opri = orc.eval(1)
        pri = eng.eval_priorities(quiz)
        assert np.isfinite(pri).all() and (pri >= 0).all(), (case.name, step, pri)
        tb.rel_vec(pri, opri)                                   # (zero exactly where the oracle's is)
        pick = eng.next_question_argmax(quiz)
        assert pick == int(np.argmax(pri)), (case.name, step, pick, int(np.argmax(pri)))
        assert pick not in asked, (case.name, step, pick)
        if margin_of(opri) > 10 * tb.f32_tolerance(orc, case).max():
            qualified += 1
            assert pick == orc.select_argmax(opri), (case.name, step, pick)
        if step < len(case.answers):
            q, a = case.answers[step]
            eng.set_active_question(quiz, q)
            eng.record_answer(quiz, a)
            orc.record_answer(q, a, cases.WORKERS - 1)
            asked.add(q)
    if i is None:       # (the tail of the posterior is below fp32's smallest subnormal)
        live = priors[priors > 0]
        assert live.min() < 2.0 ** -149 and live.max() > 0.5, (live.min(), live.max())
    print(case.name, ": %d of %d steps decided beyond ten fp32 tolerances" % (qualified, len(case.answers) + 1))
    assert qualified >= 1
    eng.close()
