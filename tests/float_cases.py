"""Quiz states for Float engines in which the fp32 sweep cannot decide the argmax: a CROWD of questions whose priorities differ in
the seventh to ninth digit, far above every other question (tests/test_gpu_float_select.py).

crowded(): on a trained cube, the best question q* of the state after some answers (by the fp64 oracle on the cube rounded to
fp32, before anything is copied) is copied over n_copies other questions; in every copy a fraction of the fp32 elements is moved one
last place up or down.  In that state the copies' priorities then lie within a few 1e-7 of q*'s, in an order that only fp64 tells;
the other questions and the posterior (the answered questions are never overwritten) stay what they were, so the crowd leads
every other question by the margin q* had.  A question that is best after the answers is not best in a fresh quiz or after other
answers: one cube serves one state, and the shorter prefixes of its answers are ordinary states of the same cube."""
from __future__ import annotations

import numpy as np

import cases
import orclib


class CrowdCase(cases.Case):
    """A Case whose knowledge base is given (fp32-exact values as fp64) instead of generated."""

    def __init__(self, name, K, Q, T, seed, arrays, q_star, copies, **kw):
        super().__init__(name, K, Q, T, seed, **kw)
        self.arrays, self.q_star, self.copies = arrays, q_star, copies
        self.crowd = sorted([q_star] + list(copies))

    def kb(self):
        return self.arrays

    def make_oracle(self):
        o = orclib.Oracle(self.K, self.Q, self.T, self.init)
        o.set_kb(*self.arrays)
        return o


def crowded(K, Q, T, seed, n_copies, frac=0.3, answers=((3, 1), (17, 4))):
    """Returns (case, oracle): case.kb() gives the engine's inputs A, D, B -- every value exactly representable in fp32 --, the oracle
    holds the same values; case.q_star is the fp64 argmax of the state after `answers` on the cube as generated, case.copies the
    ids that now hold nudged copies of its rows (randomly chosen among the questions that are neither q* nor in `answers`, so q* is
    not systematically the crowd's lowest index), case.crowd both, ascending; case.answers is `answers`."""
    base = cases.Case("crowd_base", K, Q, T, seed=seed, n_train=8.0, noise=0.1)
    A, D, B = (x.astype(np.float32) for x in base.kb())
    orc = orclib.Oracle(K, Q, T, base.init)
    orc.set_kb(*(x.astype(np.float64) for x in (A, D, B)))
    orc.start_quiz(cases.WORKERS)
    for q, a in answers:
        orc.record_answer(q, a, cases.WORKERS - 1)
    _, pri = orc.eval(1)
    q_star = int(orc.select_argmax(pri))
    rng = np.random.default_rng(1000 * seed + n_copies)
    asked = {q for q, _ in answers}
    free = [q for q in range(Q) if q != q_star and q not in asked]
    copies = sorted(int(q) for q in rng.choice(free, size=n_copies, replace=False))
    for q in copies:
        rows = A[q_star].copy()
        nudge = rng.random(rows.shape) < frac
        up = rng.random(rows.shape) < 0.5
        moved = np.where(up, np.nextafter(rows, np.float32(np.inf)), np.nextafter(rows, np.float32(0)))
        A[q] = np.where(nudge, moved, rows)
        d = np.zeros(T, dtype=np.float64)
        for k in range(K):                                   # (D in k order, as the generator sums it, then rounded once)
            d = d + A[q, k].astype(np.float64)
        D[q] = d.astype(np.float32)
    arrays = tuple(x.astype(np.float64) for x in (A, D, B))
    case = CrowdCase("crowd%d_seed%d" % (n_copies, seed), K, Q, T, seed, arrays, q_star, copies, n_train=8.0, noise=0.1,
                     answers=list(answers))
    orc.set_kb(*arrays)
    return case, orc
