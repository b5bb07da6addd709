"""Shared by tests/test_gpu_sampled_batch.py and tests/test_sampled_batch_abi.py: a plain-Python restatement of the reference's
sampled selector (PqaCore/CpuEngine.cpp:362-400), the guard that keeps a test's random draws away from run-length boundaries, and
the scenarios (golden cases, quizzes at different steps, seeds) that both the GPU tests and the no-GPU guard check use."""
from __future__ import annotations

from bisect import bisect_right

import numpy as np

import cases

SUBTASKS = 8 * cases.WORKERS          # the engine's default: eval_subtasks = 8 x workers
EDGE_RNDS = [0, 2**64 - 1]            # selRunLen is 0 or the grand total itself: exact by construction, compared unguarded
GUARD = 1e-9                          # the project's priority bar (PRIORITY_RTOL)
DRAW_SEEDS = [101, 202, 303]          # seeded random draws per scenario; every draw must clear GUARD (checked without a GPU)
TWO64M1 = 18446744073709551615.0


def bound(i, quot, rem):              # SRPoolRunner::CalcSplit: end of subtask i
    return (i + 1) * quot + min(i + 1, rem)


def split(n, n_workers):
    quot, rem = divmod(n, n_workers)
    return quot, rem, (rem if quot == 0 else n_workers)


def kahan_add(state, v):
    s, c = state
    y = v - c
    t = s + y
    return t, (t - s) - y


def select_py(pri, skip, n_workers, rnd):
    """The selector over one priority vector: per-subtask Kahan run lengths (gap / asked questions only copy the running sum),
    Kahan grand totals in subtask order, the uniform number, two upper_bounds, the two clamps.  Returns the pick before the
    gap / asked fallback."""
    n = len(pri)
    quot, rem, ns = split(n, n_workers)
    run = [0.0] * n
    grand = []
    for s in range(ns):
        first, limit = (0 if s == 0 else bound(s - 1, quot, rem)), bound(s, quot, rem)
        st = (0.0, 0.0)
        for i in range(first, limit):
            if not skip[i]:
                st = kahan_add(st, float(pri[i]))
            run[i] = st[0] - st[1]
        grand.append(st[0] - st[1])
    st = (0.0, 0.0)
    for s in range(ns):
        st = kahan_add(st, grand[s])
        grand[s] = st[0] - st[1]
    tot = grand[-1]
    sel_run = tot * float(rnd) / TWO64M1
    w = bisect_right(grand, sel_run)
    if w >= ns:
        return n - 1
    in_w = sel_run - (0.0 if w == 0 else grand[w - 1])
    first, limit = (0 if w == 0 else bound(w - 1, quot, rem)), bound(w, quot, rem)
    sel = first + bisect_right(run[first:limit], in_w)
    return min(sel, limit - 1)


def boundary_distance(run, n_workers, rnd):
    """From the oracle's per-subtask run lengths alone: how far selRunLen = totG * rnd / (2^64 - 1) lies from the nearest subtask
    total and the nearest run length, relative to totG."""
    run = np.asarray(run, dtype=np.float64)
    n = len(run)
    quot, rem, ns = split(n, n_workers)
    ends = [bound(s, quot, rem) for s in range(ns)]
    totals = np.cumsum([run[e - 1] for e in ends])
    tot = float(totals[-1])
    if not tot > 0:
        return 0.0
    base = np.zeros(n)
    for s in range(1, ns):
        base[ends[s - 1]:ends[s]] = totals[s - 1]
    edges = np.concatenate([base + run, totals, [0.0]])
    sel_run = tot * float(rnd) / TWO64M1
    return float(np.min(np.abs(edges - sel_run))) / tot


def draws(seed, n):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(0, 2**64, size=n, dtype=np.uint64)]


def synthetic_case():
    return cases.Case("synth_1000x5x1000", 5, 1000, 1000, seed=21, answers=cases.consistent_answers(1000, 1000) + [(100, 2), (900, 4)])


def scenarios():
    """Golden cases and the synthetic cube; quiz i of a scenario has the first i answers of the case's script applied."""
    return cases.small_cases() + [synthetic_case()]


def batches(case):
    """The batches of a scenario: each a list of one random number per quiz (quiz i = the case after i answers) and whether the
    batch is guarded (seeded draws) or exact by construction (the edge numbers)."""
    n = len(case.answers) + 1
    return [([r] * n, False) for r in EDGE_RNDS] + [(draws(seed, n), True) for seed in DRAW_SEEDS]


def oracle_steps(case, n_subtasks=SUBTASKS):
    """Per step i (the quiz after i answers): (run, {rnd: the oracle's pick}) for every random number the scenario's batches give
    that quiz."""
    orc = case.make_oracle()
    orc.start_quiz(cases.WORKERS)
    bs = batches(case)
    out = []
    for i in range(len(case.answers) + 1):
        run, _ = orc.eval(n_subtasks)
        out.append((run, {b[i]: orc.select_sampled(run.copy(), n_subtasks, b[i]) for b, _ in bs}))
        if i < len(case.answers):
            q, a = case.answers[i]
            orc.record_answer(q, a, cases.WORKERS - 1)
    return out
