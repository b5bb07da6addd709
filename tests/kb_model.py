"""A numpy model of the maintenance-mode operations (AddQsTs / RemoveQuestions / RemoveTargets / Compact) as a caller of the
engine observes them: the ids they return, the dimensions, the row pitch and question capacity of the allocation, and the values of
the knowledge base's arrays.  Needs no device.  TEST INFRASTRUCTURE ONLY.

Id planning is add_model / compact_model below (the reference's GapTracker and CompactSpec, PqaCore/CpuEngine.cpp:468-658), which
tests/test_host_logic.py holds to the engine's own planner (kb_plan.h) through the host-logic probe.  Value semantics follow
CpuEngine.cpp:468-575 as probqa_amd/csrc/hip_engine_kb.cpp implements them:
  * a question added in a call gets a^2 in A and a^2 K in D over EVERY column, columns added in the same call included;
  * a target added in a call gets its own amount over every question that was not added in that call, and B[t] = amount;
  * a Float engine rounds each stored value once through fp32 (B is held in fp64 words that carry fp32 values)."""
from __future__ import annotations

import numpy as np


def add_model(Q, T, q_gaps, t_gaps, q_amounts, t_amounts):
    """GapTracker.Acquire pops the back of the gap list; when it is empty the axis grows by one."""
    def axis(gaps, size, amounts):
        gaps, ids = list(gaps), []
        for _ in amounts:
            if gaps:
                ids.append(gaps.pop())
            else:
                ids.append(size)
                size += 1
        return ids, size
    q_ids, new_q = axis(q_gaps, Q, q_amounts)
    t_ids, new_t = axis(t_gaps, T, t_amounts)
    return dict(n_q_reuse=min(len(q_gaps), len(q_amounts)), n_t_reuse=min(len(t_gaps), len(t_amounts)), new_q=new_q, new_t=new_t,
                q_ids=q_ids, t_ids=t_ids, q_init=list(q_amounts), t_init=list(t_amounts))


def compact_model(Q, T, q_gaps, t_gaps):
    """CompactSpec as a caller sees it: the survivors fill 0 .. n-1; a question gap below n takes the LAST question not yet
    taken, a target gap below n (ascending) takes the survivors from n on (ascending)."""
    n_q, n_t = Q - len(q_gaps), T - len(t_gaps)
    tail_q = [q for q in range(Q - 1, n_q - 1, -1) if q not in q_gaps]
    old_q, moves = [], []
    for q in range(n_q):
        if q in q_gaps:
            old_q.append(tail_q.pop(0))
            moves.append((q, old_q[-1]))
        else:
            old_q.append(q)
    tail_t = [t for t in range(n_t, T) if t not in t_gaps]
    old_t = [tail_t.pop(0) if t in t_gaps else t for t in range(n_t)]
    assert not tail_q and not tail_t
    return old_q, old_t, moves


def round_ldt(T, f32=False):
    """The row pitch of a cube created with T targets: rows start on 128-byte lines (16 fp64 or 32 fp32 elements)."""
    granule = 32 if f32 else 16
    return (T + granule - 1) // granule * granule


class KBModel:
    """A[Q, K, T], D[Q, T], B[T] and the two gap lists in the engine's order (the last removed id is re-used first).  Cells of gap
    questions and gap targets hold whatever the operations leave there; only live questions x live targets are the engine's contract.
    ld_t / cap_q: the allocation -- both only ever grow: max(previous, what the new dimensions need)."""

    def __init__(self, A, D, B, f32=False, q_gaps=(), t_gaps=()):
        self.A, self.D, self.B = (np.array(x, dtype=np.float64) for x in (A, D, B))
        self.f32 = bool(f32)
        self.q_gaps, self.t_gaps = list(q_gaps), list(t_gaps)
        self.ld_t, self.cap_q = round_ldt(self.T, f32), self.Q

    Q = property(lambda self: self.A.shape[0])
    K = property(lambda self: self.A.shape[1])
    T = property(lambda self: self.A.shape[2])

    def live_q(self):
        return [q for q in range(self.Q) if q not in self.q_gaps]

    def live_t(self):
        return [t for t in range(self.T) if t not in self.t_gaps]

    def r(self, x):
        """one stored value in the engine's number type"""
        return float(np.float32(x)) if self.f32 else float(x)

    def remove_questions(self, ids):
        assert len(set(ids)) == len(ids) and all(0 <= q < self.Q and q not in self.q_gaps for q in ids)
        self.q_gaps.extend(ids)

    def remove_targets(self, ids):
        assert len(set(ids)) == len(ids) and all(0 <= t < self.T and t not in self.t_gaps for t in ids)
        self.t_gaps.extend(ids)

    def add(self, q_amounts, t_amounts):
        """-> (question ids, target ids) in the order of the amounts"""
        plan = add_model(self.Q, self.T, self.q_gaps, self.t_gaps, q_amounts, t_amounts)
        Q, K, T = self.Q, self.K, self.T
        A = np.full((plan["new_q"], K, plan["new_t"]), np.nan)    # (every new cell is written below: the CPU tests look for a NaN left over)
        D = np.full((plan["new_q"], plan["new_t"]), np.nan)
        B = np.full(plan["new_t"], np.nan)
        A[:Q, :, :T], D[:Q, :T], B[:T] = self.A, self.D, self.B
        for t, a in zip(plan["t_ids"], plan["t_init"]):           # target columns over every question ...
            A[:, :, t], D[:, t], B[t] = self.r(a * a), self.r(a * a * K), self.r(a)
        for q, a in zip(plan["q_ids"], plan["q_init"]):           # ... then the call's questions over every column
            A[q], D[q] = self.r(a * a), self.r(a * a * K)
        self.A, self.D, self.B = A, D, B
        self.q_gaps = self.q_gaps[:len(self.q_gaps) - plan["n_q_reuse"]]
        self.t_gaps = self.t_gaps[:len(self.t_gaps) - plan["n_t_reuse"]]
        self.ld_t = max(self.ld_t, round_ldt(self.T, self.f32))
        self.cap_q = max(self.cap_q, self.Q)
        return plan["q_ids"], plan["t_ids"]

    def compact(self):
        """-> (old_q, old_t): new id i holds what old id old_x[i] held.  The allocation stays."""
        old_q, old_t, _ = compact_model(self.Q, self.T, self.q_gaps, self.t_gaps)
        self.A, self.D, self.B = self.A[old_q][:, :, old_t], self.D[old_q][:, old_t], self.B[old_t]
        self.q_gaps, self.t_gaps = [], []
        return old_q, old_t

    def apply(self, step):
        """One step of a script: ("remove_q", ids) | ("remove_t", ids) | ("add", q_amounts, t_amounts) | ("compact",) -> what the engine returns."""
        op = step[0]
        if op == "remove_q":
            return self.remove_questions(step[1])
        if op == "remove_t":
            return self.remove_targets(step[1])
        if op == "add":
            return self.add(step[1], step[2])
        assert op == "compact", op
        return self.compact()


AMOUNTS = (0.1, 0.25, 0.3, 0.5, 0.7, 1.0, 1.5, 2.5)


def random_step(model, rng, max_q=40, max_t=80):
    """The next step of a random script for the model's current state (rng: random.Random).  Removals leave at least 1 live question and
    2 live targets, additions stay within max_q x max_t, and no compaction leaves fewer than that either."""
    live_q, live_t = model.live_q(), model.live_t()
    for _ in range(100):
        op = rng.choice(("remove_q", "remove_t", "add", "add", "compact"))
        if op == "remove_q" and len(live_q) > 1:
            return ("remove_q", rng.sample(live_q, rng.randrange(1, min(len(live_q) - 1, 6) + 1)))
        if op == "remove_t" and len(live_t) > 2:
            return ("remove_t", rng.sample(live_t, rng.randrange(1, min(len(live_t) - 2, 30) + 1)))
        if op == "add":
            room_q = max_q - model.Q + len(model.q_gaps)
            room_t = max_t - model.T + len(model.t_gaps)
            nq, nt = rng.randrange(0, min(room_q, 7) + 1), rng.randrange(0, min(room_t, 25) + 1)
            if nq + nt > 0:
                return ("add", [rng.choice(AMOUNTS) for _ in range(nq)], [rng.choice(AMOUNTS) for _ in range(nt)])
        if op == "compact" and (model.q_gaps or model.t_gaps):
            return ("compact",)
    raise AssertionError("no step fits the state")
