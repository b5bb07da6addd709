"""The maintenance scripts and serving cases that tests/test_kb_model.py (CPU: the model alone) and tests/test_gpu_maintenance.py
(the engine against the model) share, and the CPU-side view of a serving case: the oracle's priorities, top-2 margins and the
sampled selector's distance from its boundaries in every quiz state the GPU test serves from.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import os
import random
import sys
from types import SimpleNamespace

import numpy as np

import cases
import orclib
from kb_model import AMOUNTS, KBModel, random_step
from probqa_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden  # noqa: E402  (RNDS: the random numbers the golden fixtures sample with)

from test_gpu_parity import PRIORITY_RTOL  # noqa: E402  (the project's bar on priorities; the module imports without a device)

INIT = 0.1
SUBTASKS = 8 * cases.WORKERS
RNDS = make_golden.RNDS


def synthetic_model(K, Q, T, seed, f32):
    A, D, B = synth.synthetic_kb(K, Q, T, INIT, 8.0, 0.5, seed)
    if f32:   # a Float engine holds the values rounded to fp32
        A, D, B = (x.astype(np.float32).astype(np.float64) for x in (A, D, B))
    return KBModel(A, D, B, f32=f32)


def amounts(n, first=0):
    return [AMOUNTS[(first + i) % len(AMOUNTS)] for i in range(n)]


# ---- Layer A: the arrays ------------------------------------------------------------------------------------------------------------
def array_scripts(f32):
    """name -> ((K, Q, T), kb seed, steps).  T grows across a row granule (16 fp64 / 32 fp32 elements) from 13 to 19 resp. 30 to 35."""
    t0, grow = (30, 5) if f32 else (13, 6)
    return {
        "grow_t": ((3, 5, t0), 21, [("add", [], amounts(grow))]),
        "grow_t_and_q": ((3, 5, t0), 22, [("add", amounts(2, 3), amounts(grow, 1))]),
        "grow_q": ((3, 5, t0), 23, [("add", amounts(3, 1), [])]),
        "grow_t_inside_granule": ((3, 5, 17), 24, [("add", [], amounts(3, 2))]),
        # 3 question gaps and 5 questions, 2 target gaps and 4 targets, every amount its own: the skip bitmap and the order of the three fills
        "more_additions_than_gaps": ((4, 8, 21), 25, [("remove_q", [1, 6, 3]), ("remove_t", [20, 4]),
                                                      ("add", [0.5, 0.25, 2.0, 1.5, 0.7], [0.3, 1.0, 0.1, 2.5])]),
        # 40 -> 14 targets (the multiples of 3 survive, nine of them move down), 9 -> 6 questions; then additions onto the stale columns
        # and the stale question blocks without a reallocation, then one that reallocates both ways
        "compact_across_granule": ((3, 9, 40), 26, [("remove_t", [t for t in range(40) if t % 3]), ("remove_q", [0, 4, 8]), ("compact",),
                                                    ("add", [1.5, 0.25], [0.3, 0.7, 1.0, 0.5]), ("add", amounts(3, 2), amounts(60, 1))]),
    }


N_RANDOM_SCRIPTS, RANDOM_STEPS = 10, 8


def random_script_start(seed):
    """-> (rng, (K, Q, T), kb seed) of random script `seed`; its steps come from kb_model.random_step(model, rng), one at a time."""
    rng = random.Random(7000 + seed)
    return rng, (rng.choice((2, 3, 5)), rng.randrange(3, 21), rng.randrange(4, 51)), 500 + seed


# ---- Layer B: serving ---------------------------------------------------------------------------------------------------------------
def grow_steps(t0, t1):
    """T t0 -> t1 and two questions past the capacity -- one gap re-used and the rest appended on either axis --, then two target gaps and
    one question gap that stay open."""
    return [("remove_t", [t0 - 1]), ("remove_q", [3]), ("add", [0.5, 1.5, 0.25], amounts(t1 - t0 + 1, 2)),
            ("remove_t", [3, t0 // 2]), ("remove_q", [1])]


def compact_steps(t0, t1):
    """Two questions past the capacity first (the pitch stays), then T t0 -> t1 by a compaction that leaves columns [t1, t0) stale, then
    two target gaps and one question gap that stay open."""
    stride = t0 // (t0 - t1)
    return [("add", [0.5, 1.5], []), ("remove_t", [1 + i * stride for i in range(t0 - t1)]), ("remove_q", [2]), ("compact",),
            ("remove_t", [5, t1 - 2]), ("remove_q", [0])]


def untrained_questions(model):
    """Live questions whose every cell still holds A = D / K -- added by AddQsTs and never trained.  Such a question says nothing: its
    posteriors equal the prior, the velocity sum of its priority is pure rounding residue (1e-18 or exactly 0, by the summation order),
    and the priority formula takes the LOGARITHM of it -- two correct evaluations differ by tens of percent (measured: 21 % between the
    long-row sweep and the oracle at 16390 targets).  No bar on priorities can hold for it, so a serving case trains them first."""
    lt = model.live_t()
    return [q for q in model.live_q() if (model.A[q][:, lt] * model.K == model.D[q][lt][None, :]).all()]


def post_training(model):
    """[(question, answer, target, amount)]: a dozen Train records for every untrained question, each on a target of its own (so a cell
    of a Float cube, and B[t], is rounded once and the oracle's fp64 result rounded once is the engine's)."""
    lt, out = model.live_t(), []
    for q in untrained_questions(model):
        for j in range(12):
            out.append((q, (q + j) % model.K, lt[(5 + 37 * len(out)) % len(lt)], 1.0 + 0.25 * (j % 5)))
    assert len({t for _, _, t, _ in out}) == len(out)
    return out


def train_model(model, records):
    """The records, one Train call each, on the model's arrays: the oracle's arithmetic (bit-identical to the engine's:
    tests/test_gpu_kb.py), rounded once for a Float engine."""
    orc = oracle_of(model)
    for q, a, t, amount in records:
        orc.train([(q, a)], t, amount, cases.WORKERS)
    A, D, B = orc.A[:, :, :model.T].copy(), orc.D[:, :model.T].copy(), orc.B[:model.T].copy()
    orc.close()
    if model.f32:
        A, D, B = (x.astype(np.float32).astype(np.float64) for x in (A, D, B))
    model.A, model.D, model.B = A, D, B


KB_SEED, ANSWERS = 1, (0, 0)     # every serving case: the seed of its synthetic start, and what the two questions asked are answered


class ServingCase(SimpleNamespace):
    """name; K, Q, T0: the synthetic start; T1: the targets it serves; steps.  tests/test_kb_model.py asserts without a device that the
    oracle's top-2 margin clears the bar in each of the three quiz states."""

    def model(self, f32):
        return synthetic_model(self.K, self.Q, self.T0, KB_SEED, f32)


SERVING_CASES = [
    # T 1000 -> 1030, fp64 pitch 1008 -> 1040: across T <= 1024 and ldT <= 1024
    ServingCase(name="grow_1000_1030", K=3, Q=5, T0=1000, T1=1030, steps=grow_steps(1000, 1030)),
    # T 1100 -> 980, the pitch stays 1104: T <= 1024 < ldT
    ServingCase(name="compact_1100_980", K=3, Q=7, T0=1100, T1=980, steps=compact_steps(1100, 980)),
    # T 10235 -> 10245, fp64 pitch 10240 -> 10256: across the default cluster_from
    ServingCase(name="grow_10235_10245", K=2, Q=5, T0=10235, T1=10245, steps=grow_steps(10235, 10245)),
    # T 16380 -> 16390, fp64 pitch 16384 -> 16400: across every switch at 16384
    ServingCase(name="grow_16380_16390", K=3, Q=7, T0=16380, T1=16390, steps=grow_steps(16380, 16390)),
    # T 16400 -> 16300, the pitch stays: T <= 16384 < ldT
    ServingCase(name="compact_16400_16300", K=2, Q=5, T0=16400, T1=16300, steps=compact_steps(16400, 16300)),
]


def oracle_of(model, A=None, D=None, B=None):
    """An oracle at the model's dimensions and gaps over the given arrays (default: the model's own)."""
    orc = orclib.Oracle(model.K, model.Q, model.T, INIT)
    orc.set_kb(model.A if A is None else A, model.D if D is None else D, model.B if B is None else B)
    orc.set_target_gaps(model.t_gaps)
    orc.set_question_gaps(model.q_gaps)
    return orc


def f32_tolerance(orc, model, asked=()):
    """tests/test_gpu_batch.py's per-question bar of an fp32 sweep against the fp64 oracle in the oracle's current quiz state, over the
    questions that have a priority (gap and asked questions: 0 on both sides)."""
    import test_gpu_batch as tb

    with np.errstate(all="ignore"):
        tol = tb.f32_tolerance(orc, SimpleNamespace(T=model.T, tgaps=model.t_gaps))
    dead = list(model.q_gaps) + list(asked)
    tol[dead] = 0.0
    assert np.isfinite(tol).all()
    return tol


def state_of(orc, model, asked):
    """What the tests need of the oracle's current quiz state.
    tol[q]: the bar the engine's priority of question q is held to, relative: PRIORITY_RTOL on a Double engine, tests/test_gpu_batch.py's
    f32_tolerance on a Float one (0 for gap and asked questions, whose priority is 0 on both sides).
    margin: the oracle's top-2 margin, relative to the best.
    argmax_clearance: with every priority anywhere within TEN times its bar, the best question's lowest value minus any other question's
    highest, relative to the best: positive means the engine's argmax is the oracle's.  (On a Double engine that is the margin less
    2e-8.  On a Float one the bars differ by question, which this form accounts for and one bar for all questions cannot.)
    sampled_clearance: the selector draws rnd / 2^64 of the total run length; boundary i between two questions sits at cum[i] and moves
    by at most shift[i] = (sum_{j <= i} tol[j] w[j] + cum[i] sum_j tol[j] w[j]) / W when every weight w[j] moves within its bar.  The
    least |draw - cum[i]| - 2 shift[i] over the draws of RNDS and the boundaries: positive means the engine's pick is the oracle's.  (The
    draws 0 and 2^64 - 1 are left out: they select the first question with a weight and the last question whatever the weights are.)"""
    run, opri = orc.eval(SUBTASKS)
    assert model.Q <= SUBTASKS      # (a subtask per question: run[q] is question q's own weight)
    dead = list(model.q_gaps) + list(asked)
    tol = f32_tolerance(orc, model, asked) if model.f32 else np.full(model.Q, PRIORITY_RTOL)
    tol[dead] = 0.0
    srt = np.sort(opri)[::-1]
    s = SimpleNamespace(run=run, opri=opri, tol=tol, want=orc.select_argmax(opri), margin=(srt[0] - srt[1]) / srt[0])
    hi = opri * (1 + 10 * tol)
    hi[s.want] = 0.0
    s.argmax_clearance = (opri[s.want] * (1 - 10 * tol[s.want]) - hi.max()) / opri[s.want]
    total = run.sum()
    cum = np.cumsum(run) / total
    shift = (np.cumsum(tol * run) + cum * (tol * run).sum()) / total
    inner = [i for i in range(model.Q) if 0 < cum[i] < 1]
    s.sampled_clearance = min([abs(r / float(2 ** 64 - 1) - cum[i]) - 2 * shift[i] for r in RNDS if 0 < r < 2 ** 64 - 1 for i in inner], default=1.0)
    s.sampled = [orc.select_sampled(run, SUBTASKS, r) for r in RNDS]
    return s


def serving_states(model, answers):
    """The three quiz states of a serving case on the CPU: after StartQuiz, after the oracle's best question answered answers[0], after the
    next best answered answers[1].  -> (states, [(question, answer), ...])."""
    orc = oracle_of(model)
    orc.start_quiz(cases.WORKERS)
    states, asked = [state_of(orc, model, [])], []
    for a in answers:
        q = states[-1].want
        orc.record_answer(q, a, cases.WORKERS - 1)
        asked.append((q, a))
        states.append(state_of(orc, model, [x for x, _ in asked]))
    orc.close()
    return states, asked
