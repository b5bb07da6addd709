"""Host bookkeeping of the engine that needs no device (runs in the CPU suite): the compact <-> permanent id map, the
eviction rule of ClearOldQuizzes, what the one-device and the sharded engine decide through the same code (kb_plan.h) -- the
ids AddQsTs hands out, what Compact moves where, which removals are refused, which shard's winner is the selection -- and the
table of the engine's options (engine_options.h), driven through PqaHip_HostLogicProbe and held to a Python model of the reference's observable behaviour
(PqaCore/PermanentIdManager.cpp, PqaCore/BaseEngine.cpp:722-765,814-873, PqaCore/CpuEngine.cpp:468-658)."""
import ctypes
import math
import random
import struct

import numpy as np
import pytest

from kb_model import add_model, compact_model   # (the id planning the maintenance model of tests/kb_model.py is built on)
from probqa_amd import interop


def probe(what, words, n_out):
    lib = interop.load_library()
    arr = np.ascontiguousarray(words, dtype=np.int64)
    out = np.zeros(max(1, n_out), dtype=np.int64)
    n = lib.PqaHip_HostLogicProbe(what.encode(), arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(arr),
                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n_out)
    return n, out[:max(0, n)].tolist()


class LedgerModel:
    """What a caller of the reference's id manager can observe."""

    def __init__(self):
        self.next = 0
        self.perm = []        # slot -> permanent id or -1
        self.slot = {}        # permanent id -> slot

    def run(self, op, a, b, extra):
        if op == 0:
            return self.perm[a] if 0 <= a < len(self.perm) else -1
        if op == 1:
            return self.slot.get(a, -1)
        if op == 2:
            if self.next <= a:
                self.next = a + 1
                return 1
            return 0
        if op == 3:
            if not (0 <= a < len(self.perm)) or self.perm[a] == -1:
                return 0
            del self.slot[self.perm[a]]
            self.perm[a] = -1
            return 1
        if op == 4:
            if not (0 <= a < len(self.perm)) or self.perm[a] != -1:
                return 0
            self.perm[a] = self.next
            self.slot[self.next] = a
            self.next += 1
            return 1
        if op == 5:
            if a < len(self.perm):
                return 0
            while len(self.perm) < a:
                self.slot[self.next] = len(self.perm)
                self.perm.append(self.next)
                self.next += 1
            return 1
        if op == 6:
            if b < 0 or b >= self.next or b in self.slot or a not in self.slot:
                return 0
            s = self.slot.pop(a)
            self.slot[b] = s
            self.perm[s] = b
            return 1
        if op == 7:
            live = [s for s, p in enumerate(self.perm) if p != -1]
            if a != len(live) or sorted(extra) != live:
                return 0
            self.perm = [self.perm[s] for s in extra]
            self.slot = {p: i for i, p in enumerate(self.perm)}
            return 1
        if op == 8:
            return 1
        raise AssertionError(op)


def test_id_ledger_follows_the_reference_sequence():
    """The sequence tests/test_gpu_kb.py drives through an engine, here without one: fresh ids, LIFO slot reuse under new
    permanent ids, the raised floor, a rename into the past, compaction."""
    script = [5, 5, 0,     # five slots: permanent 0..4
              3, 1, 0,     # vacate slot 1
              4, 1, 0,     # reissue: permanent 5
              0, 1, 0, 1, 1, 0, 1, 5, 0,
              2, 100, 0, 2, 50, 0,
              5, 6, 0,     # slot 5: permanent 101
              0, 5, 0,
              6, 101, 77, 1, 77, 0, 1, 101, 0,
              6, 77, 500,  # not into the future
              6, 0, 2,     # not onto a live id
              3, 0, 0, 3, 2, 0,
              7, 4, 4, 5, 1, 3, 4,   # slots 5, 1, 3, 4 survive, in that order
              0, 0, 0, 0, 1, 0, 0, 3, 0, 0, 4, 0, 1, 77, 0, 1, 2, 0,
              8, 0, 0, 1, 5, 0, 5, 5, 0, 0, 4, 0]
    n, out = probe("id_ledger", script, 64)
    assert n == 28
    assert out == [1, 1, 1, 5, -1, 1, 1, 0, 1, 101, 1, 5, -1, 0, 0, 1, 1, 1, 77, 5, 4, -1, 0, -1, 1, 1, 1, 102]
    # (the last one: the issue floor survives the file -- the slot added after the round trip continues the sequence)


@pytest.mark.parametrize("seed", range(12))
def test_id_ledger_against_model(seed):
    rng = random.Random(seed)
    model = LedgerModel()
    script, expect = [], []

    def emit(op, a=0, b=0, extra=()):
        script.extend([op, a, b, *extra])
        expect.append(model.run(op, a, b, list(extra)))

    emit(5, rng.randrange(0, 40))
    for _ in range(3000):
        n = len(model.perm)
        r = rng.random()
        if r < 0.25:
            emit(3, rng.randrange(-1, n + 2))
        elif r < 0.45:
            emit(4, rng.randrange(-1, n + 2))
        elif r < 0.55:
            emit(5, n + rng.randrange(-1, 4))
        elif r < 0.63:
            emit(2, model.next + rng.randrange(-3, 3))
        elif r < 0.75:
            src = rng.choice(list(model.slot)) if model.slot and rng.random() < 0.8 else rng.randrange(-1, model.next + 2)
            emit(6, src, rng.randrange(-1, model.next + 2))
        elif r < 0.78:
            live = [s for s, p in enumerate(model.perm) if p != -1]
            rng.shuffle(live)
            if rng.random() < 0.2 and live:
                live[0] = rng.randrange(-1, n + 1)     # a bad list now and then: nothing may change
            emit(7, len(live), len(live), live)
        elif r < 0.80:
            emit(8)
        elif r < 0.82:
            script.extend([9, 0, 0])
            expect.append(len(model.slot))
        elif r < 0.90:
            emit(0, rng.randrange(-2, n + 2))
        else:
            emit(1, rng.randrange(-2, model.next + 2))
    # the whole map at the end, both directions
    for s in range(len(model.perm)):
        emit(0, s)
    for p in range(model.next):
        emit(1, p)
    n, out = probe("id_ledger", script, len(expect))
    assert n == len(expect)
    bad = [i for i in range(n) if out[i] != expect[i]]
    assert not bad, (bad[:5], [script[:0]])


def test_malformed_scripts_are_refused():
    assert probe("id_ledger", [5, 3], 4)[0] == -1
    assert probe("id_ledger", [10, 0, 0], 4)[0] == -1
    assert probe("id_ledger", [7, 3, 3, 0, 1], 4)[0] == -1      # the inline list is cut short
    assert probe("id_ledger", [5, 3, 0, 5, 4, 0], 1)[0] == -1    # output too small
    assert probe("nothing", [], 1)[0] == -1
    assert probe("let_go", [0, 1, 1, 2, 7, 0], 8)[0] == -1


def let_go(now, max_count, max_age, quizzes):
    words = [now, max_count, max_age, len(quizzes)]
    for q, t in quizzes:
        words += [q, t]
    n, out = probe("let_go", words, len(quizzes) + 1)
    assert n == out[0] + 1
    return out[1:]


def test_clear_old_quizzes_rule():
    now = 1_000_000
    quizzes = [(0, now - 50), (1, now - 5), (3, now - 400), (4, now - 5), (7, now - 20), (9, now)]
    assert let_go(now, 10, 1e9, quizzes) == []
    assert let_go(now, 10, 100, quizzes) == [3]                       # older than 100 s
    assert let_go(now, 3, 100, quizzes) == [3, 0, 7]                  # then the longest-unused until three remain
    assert let_go(now, 2, 1e9, quizzes) == [3, 0, 7, 1]               # equal ages: registry order
    assert let_go(now, 0, 1e9, quizzes) == [3, 0, 7, 1, 4, 9]
    assert let_go(now, 5, 0, quizzes) == [0, 1, 3, 4, 7]              # everything used before `now`, in registry order
    assert let_go(now, 0, 10, []) == []


@pytest.mark.parametrize("seed", range(6))
def test_clear_old_quizzes_rule_random(seed):
    rng = random.Random(100 + seed)
    now = 2_000_000
    ids = sorted(rng.sample(range(500), rng.randrange(1, 200)))
    quizzes = [(q, now - rng.randrange(0, 30)) for q in ids]
    max_count, max_age = rng.randrange(0, 220), rng.randrange(0, 30)
    gone = let_go(now, max_count, max_age, quizzes)
    aged = [q for q, t in quizzes if now - t > max_age]
    assert gone[:len(aged)] == aged
    rest = [(q, t) for q, t in quizzes if now - t <= max_age]
    extra = gone[len(aged):]
    assert len(extra) == max(0, len(rest) - max_count) and len(set(gone)) == len(gone)
    kept = [(q, t) for q, t in rest if q not in extra]
    age = dict(quizzes)
    if extra and kept:
        assert max(age[q] for q in extra) <= min(t for _, t in kept)      # nobody kept is older than somebody released
    assert [age[q] for q in extra] == sorted(age[q] for q in extra)       # longest-unused first


# ---- the plans both engines share (kb_plan.h) -------------------------------------------------------------------------------------
def words_of(values):
    return [len(values), *values]


def bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def from_bits(w):
    return struct.unpack("<d", struct.pack("<q", w))[0]


def take_list(out, at):
    n = out[at]
    return out[at + 1:at + 1 + n], at + 1 + n


def add_plan(Q, T, q_gaps, t_gaps, q_amounts, t_amounts):
    words = [Q, T, *words_of(q_gaps), *words_of(t_gaps), *words_of([bits(a) for a in q_amounts]), *words_of([bits(a) for a in t_amounts])]
    n_out = 8 + 2 * (len(q_amounts) + len(t_amounts))
    n, out = probe("add_plan", words, n_out)
    assert n == n_out
    q_ids, at = take_list(out, 4)
    t_ids, at = take_list(out, at)
    q_init, at = take_list(out, at)
    t_init, at = take_list(out, at)
    assert at == n
    return dict(n_q_reuse=out[0], n_t_reuse=out[1], new_q=out[2], new_t=out[3], q_ids=q_ids, t_ids=t_ids,
                q_init=[from_bits(w) for w in q_init], t_init=[from_bits(w) for w in t_init])


def compact_plan(Q, T, q_gaps, t_gaps):
    n_out = 3 + 3 * Q + T
    n, out = probe("compact_plan", [Q, T, *words_of(q_gaps), *words_of(t_gaps)], n_out)
    assert n > 0
    old_q, at = take_list(out, 0)
    old_t, at = take_list(out, at)
    moves, at = take_list(out, at)
    assert at == n
    return old_q, old_t, list(zip(moves[0::2], moves[1::2]))


def test_add_plan_fixed_case():
    """the sequence of tests/test_gpu_kb.py::test_add_remove_compact_against_numpy_model"""
    got = add_plan(12, 19, [2, 9], [0, 5, 18], [0.5, 0.25, 2.0], [0.3, 0.7])
    assert got["q_ids"] == [9, 2, 12] and got["t_ids"] == [18, 5]
    assert (got["n_q_reuse"], got["n_t_reuse"], got["new_q"], got["new_t"]) == (2, 2, 13, 19)
    assert got["q_init"] == [0.5, 0.25, 2.0] and got["t_init"] == [0.3, 0.7]
    assert got == add_model(12, 19, [2, 9], [0, 5, 18], [0.5, 0.25, 2.0], [0.3, 0.7])


def test_add_plan_named_cases():
    # no gaps: everything is appended
    assert add_plan(5, 4, [], [], [1.0, 2.0], [3.0]) == add_model(5, 4, [], [], [1.0, 2.0], [3.0])
    assert add_plan(5, 4, [], [], [1.0, 2.0], [3.0])["q_ids"] == [5, 6]
    # more additions than gaps: the gaps from the back of the list, then new ids
    assert add_plan(6, 6, [4, 1], [3], [1.0] * 4, [1.0] * 3)["q_ids"] == [1, 4, 6, 7]
    assert add_plan(6, 6, [4, 1], [3], [1.0] * 4, [1.0] * 3)["t_ids"] == [3, 6, 7]
    # fewer additions than gaps: the dimensions stay
    got = add_plan(6, 6, [4, 1, 0], [3, 2], [0.5], [0.25])
    assert got["q_ids"] == [0] and got["t_ids"] == [2] and (got["new_q"], got["new_t"]) == (6, 6)
    # every question a gap
    got = add_plan(3, 2, [0, 1, 2], [], [1.0, 1.0, 1.0, 1.0], [])
    assert got["q_ids"] == [2, 1, 0, 3] and got["new_q"] == 4 and got["t_ids"] == []
    # nothing added
    assert add_plan(3, 2, [1], [0], [], []) == add_model(3, 2, [1], [0], [], [])


@pytest.mark.parametrize("seed", range(20))
def test_add_plan_against_model(seed):
    rng = random.Random(300 + seed)
    Q, T = rng.randrange(1, 60), rng.randrange(1, 60)
    q_gaps = rng.sample(range(Q), rng.randrange(0, Q + 1))
    t_gaps = rng.sample(range(T), rng.randrange(0, T + 1))
    q_amounts = [rng.choice([0.1, 0.5, 1.0, 2.5]) for _ in range(rng.randrange(0, 2 * len(q_gaps) + 3))]
    t_amounts = [rng.choice([0.1, 0.5, 1.0, 2.5]) for _ in range(rng.randrange(0, 2 * len(t_gaps) + 3))]
    assert add_plan(Q, T, q_gaps, t_gaps, q_amounts, t_amounts) == add_model(Q, T, q_gaps, t_gaps, q_amounts, t_amounts)


def test_compact_plan_fixed_case():
    """tests/test_gpu_kb.py::test_add_remove_compact_against_numpy_model after its additions: 13 questions, 19 targets"""
    old_q, old_t, moves = compact_plan(13, 19, [3, 11], [0])
    assert len(old_q) == 11 and old_q[3] == 12 and old_q[:3] == [0, 1, 2] and sorted(old_q) == [q for q in range(13) if q not in (3, 11)]
    assert len(old_t) == 18 and old_t[0] == 18 and old_t[1:] == list(range(1, 18))
    assert moves == [(3, 12)]
    assert (old_q, old_t, moves) == compact_model(13, 19, [3, 11], [0])


def test_compact_plan_named_cases():
    # no gaps: nothing moves
    assert compact_plan(4, 3, [], []) == ([0, 1, 2, 3], [0, 1, 2], [])
    # every question a gap (and every target)
    assert compact_plan(3, 2, [2, 0, 1], [1, 0]) == ([], [], [])
    # gaps only in the dropped tail: the prefix stays where it is
    assert compact_plan(6, 5, [5, 4], [3, 4]) == ([0, 1, 2, 3], [0, 1, 2], [])
    # gaps in the prefix AND in the tail: the last survivors come down, the tail's gaps are passed over
    assert compact_plan(7, 7, [1, 5, 0], [6, 0, 4, 1]) == ([6, 4, 2, 3], [3, 5, 2], [(0, 6), (1, 4)])
    assert compact_model(7, 7, [1, 5, 0], [6, 0, 4, 1]) == ([6, 4, 2, 3], [3, 5, 2], [(0, 6), (1, 4)])
    # one survivor, at the very end
    assert compact_plan(4, 1, [0, 1, 2], []) == ([3], [0], [(0, 3)])


@pytest.mark.parametrize("seed", range(20))
def test_compact_plan_against_model(seed):
    rng = random.Random(400 + seed)
    Q, T = rng.randrange(1, 80), rng.randrange(1, 80)
    q_gaps = rng.sample(range(Q), rng.randrange(0, Q + 1))
    t_gaps = rng.sample(range(T), rng.randrange(0, T + 1))
    old_q, old_t, moves = compact_plan(Q, T, q_gaps, t_gaps)
    assert (old_q, old_t, moves) == compact_model(Q, T, q_gaps, t_gaps)
    # what the moves are for: made in their order on an array that holds its own indices, they leave old_q in the kept prefix
    rows = list(range(Q))
    for dst, src in moves:
        rows[dst] = rows[src]
    assert rows[:len(old_q)] == old_q
    assert sorted(old_q) == [q for q in range(Q) if q not in q_gaps] and sorted(old_t) == [t for t in range(T) if t not in t_gaps]


def check_removal(limit, gaps, ids):
    n, out = probe("check_removal", [limit, *words_of(gaps), *words_of(ids)], 2)
    assert n == 2
    return out


ABSENT_ID = 13      # PqaErrors.h: the id is absent from the KB


def removal_model(limit, gaps, ids):
    for i, x in enumerate(ids):
        if x < 0 or x >= limit or x in gaps or x in ids[:i]:
            return [i, ABSENT_ID]
    return [-1, 0]


def test_check_removal_named_cases():
    assert check_removal(10, [], [3, 1, 9, 0]) == [-1, 0]
    assert check_removal(10, [], []) == [-1, 0]
    assert check_removal(10, [4], [3, 1, 3]) == [2, ABSENT_ID]        # a repeated id
    assert check_removal(10, [4, 7], [3, 7, 1]) == [1, ABSENT_ID]     # a gap id
    assert check_removal(10, [], [10]) == [0, ABSENT_ID]
    assert check_removal(10, [], [0, -1]) == [1, ABSENT_ID]
    assert check_removal(0, [], [0]) == [0, ABSENT_ID]


@pytest.mark.parametrize("seed", range(10))
def test_check_removal_against_model(seed):
    rng = random.Random(500 + seed)
    limit = rng.randrange(1, 50)
    gaps = rng.sample(range(limit), rng.randrange(0, limit))
    for _ in range(40):
        ids = [rng.randrange(-1, limit + 1) if rng.random() < 0.1 else rng.randrange(limit) for _ in range(rng.randrange(0, 6))]
        assert check_removal(limit, gaps, ids) == removal_model(limit, gaps, ids), (limit, gaps, ids)


def better_pick(records):
    words = []
    for p, i in records:
        words += [bits(p), i]
    n, out = probe("better_pick", words, 2)
    assert n == 2
    return from_bits(out[0]), out[1]


def pick_model(records):
    """maximum priority, lowest index on ties, a NaN counts as -infinity, a negative index is no candidate"""
    best = None
    for p, i in records:
        if i < 0:
            continue
        p = -math.inf if math.isnan(p) else p
        if best is None or p > best[0] or (p == best[0] and i < best[1]):
            best = (p, i)
    return best or (0.0, -1)


def test_better_pick_named_cases():
    assert better_pick([]) == (0.0, -1)
    assert better_pick([(5.0, -1), (7.0, -3), (1.0, -1)]) == (0.0, -1)             # all indices negative
    assert better_pick([(math.nan, 4), (-1e300, 9)]) == (-1e300, 9)                # a NaN against a number, either order
    assert better_pick([(-1e300, 9), (math.nan, 4)]) == (-1e300, 9)
    assert better_pick([(math.nan, 4), (-math.inf, 9)]) == (-math.inf, 4)          # ... and against -infinity: the lower index
    assert better_pick([(5.0, -1), (math.nan, 6)]) == (-math.inf, 6)               # a NaN alone still is the selection
    assert better_pick([(math.nan, 6), (math.nan, 2)]) == (-math.inf, 2)
    assert better_pick([(2.0, 8), (2.0, 3), (2.0, 5)]) == (2.0, 3)                 # equal priorities: the lowest index
    assert better_pick([(1.0, 0), (3.0, 7), (2.0, 1), (9.0, -1)]) == (3.0, 7)
    assert better_pick([(-0.0, 5), (0.0, 2)]) == (0.0, 2)


@pytest.mark.parametrize("seed", range(10))
def test_better_pick_against_model(seed):
    rng = random.Random(600 + seed)
    for _ in range(200):
        records = [(rng.choice([math.nan, -math.inf, math.inf, 0.0, 1.5, 1.5, -2.0, rng.random()]), rng.randrange(-2, 12))
                   for _ in range(rng.randrange(0, 9))]
        assert better_pick(records) == pick_model(records), records


def test_malformed_plan_scripts_are_refused():
    assert probe("add_plan", [5, 5, 1, 9, 0, 0, 0], 32)[0] == -1            # a gap beyond the dimension
    assert probe("add_plan", [5, 5, 2, 1, 1, 0, 0, 0], 32)[0] == -1         # a gap listed twice
    assert probe("add_plan", [5, 5, 0, 0, 1, bits(1.0), 0], 4)[0] == -1     # output too small
    assert probe("compact_plan", [5, 5, 0, 0, 0], 32)[0] == -1              # words left over
    assert probe("compact_plan", [5, 5, 3, 1], 32)[0] == -1                 # the list is cut short
    assert probe("check_removal", [5, 0, 1, 2], 1)[0] == -1
    assert probe("better_pick", [bits(1.0)], 2)[0] == -1


# ---- the host's prefix of a rated vector (kb_plan.h: RatedPrefix), the one listing of more than 256 records ------------------------
def rated_prefix(values, eligible, id_base, want):
    words = [want, id_base, len(values)]
    for v, e in zip(values, eligible):
        words += [bits(v), int(e)]
    n, out = probe("rated_prefix", words, 1 + len(values))
    assert n == 1 + out[0], (n, out)
    return out[1:]


def prefix_model(values, eligible, id_base, want):
    """the eligible entries with a value > 0 (a NaN is not), value descending, id ascending, the first `want`"""
    v = np.asarray(values, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        at = np.flatnonzero(np.asarray(eligible, dtype=bool) & (v > 0)) if len(v) else np.zeros(0, dtype=np.int64)
    ids = at + id_base
    return [int(i) for i in ids[np.lexsort((ids, -v[at]))][:want]]


def test_rated_prefix_named_cases():
    def check(values, eligible=None, id_base=0, want=3):
        eligible = [1] * len(values) if eligible is None else eligible
        got = rated_prefix(values, eligible, id_base, want)
        assert got == prefix_model(values, eligible, id_base, want), (values, eligible, id_base, want, got)
        return got

    assert check([2.5] * 7, want=4) == [0, 1, 2, 3]                                      # all values equal: by id
    assert check([1.0, 3.0, 3.0, 2.0, 3.0, 2.0, 2.0, 1.0], want=4) == [1, 2, 4, 3]       # runs of ties across the boundary of `want`
    assert check([1.0, 3.0, 3.0, 2.0, 3.0, 2.0, 2.0, 1.0], want=2) == [1, 2]
    assert check([3.0, 2.0, 3.0, 2.0], eligible=[0, 1, 1, 1], id_base=100, want=2) == [102, 101]
    assert check([0.0, 1.0, 0.0, 2.0], want=4) == [3, 1]                                 # zeros
    assert check([-0.0, 1.0, -0.0], want=3) == [1]                                       # negative zero
    assert check([-1.0, -math.inf, 5e-324], want=3) == [2]
    assert check([1.0, math.nan, 2.0, math.nan], want=4) == [2, 0]                       # a NaN is not > 0: never listed
    assert check([math.inf, 1.0, math.inf], want=3) == [0, 2, 1]
    assert check([3.0, 1.0, 2.0], want=0) == []                                          # `want` of 0
    assert check([1.0, 3.0, 2.0], want=1) == [1]                                         # ... of 1
    assert check([1.0, 0.0, 3.0, 2.0], eligible=[1, 1, 1, 0], want=2) == [2, 0]          # ... exactly the eligible count
    assert check([1.0, 0.0, 3.0, 2.0], eligible=[1, 1, 1, 0], want=9) == [2, 0]          # ... beyond it
    assert check([], want=5) == []                                                       # an empty vector
    assert check([4.0, 4.0], eligible=[0, 0], want=2) == []


def test_rated_prefix_against_lexsort():
    rng = np.random.default_rng(77)
    for _ in range(50):   # values from 4 distinct numbers: ties are the rule
        n = int(rng.integers(1, 301))
        values = rng.choice([0.0, 0.25, 1.0, 7.5], size=n)
        eligible = rng.random(n) < 0.8
        id_base, want = int(rng.integers(0, 1000)), int(rng.integers(0, n + 5))
        assert rated_prefix(values, eligible, id_base, want) == prefix_model(values, eligible, id_base, want), (n, id_base, want)


def test_malformed_rated_prefix_scripts_are_refused():
    assert probe("rated_prefix", [1, 0], 4)[0] == -1                                  # no count
    assert probe("rated_prefix", [1, 0, 2, bits(1.0), 1], 4)[0] == -1                 # the vector is cut short
    assert probe("rated_prefix", [1, 0, 1, bits(1.0), 1, 7], 4)[0] == -1              # words left over
    assert probe("rated_prefix", [-1, 0, 1, bits(1.0), 1], 4)[0] == -1                # a negative `want`
    assert probe("rated_prefix", [1, 0, -1], 4)[0] == -1                              # a negative count
    assert probe("rated_prefix", [1, 0, 1, bits(1.0), 2], 4)[0] == -1                 # eligibility is a bit
    assert probe("rated_prefix", [2, 0, 2, bits(1.0), 1, bits(2.0), 1], 2)[0] == -1   # output too small


# ---- the options (engine_options.h) -----------------------------------------------------------------------------------------------
# Every option PqaHip_SetOption accepts, as SetOption, GetOption and ApplyEnvironment treated it before there was a table (this
# list was written from those three functions, not from the table): the accepted values lo..hi, the default, whether it is a flag
# (any integer accepted, stored as 0 or 1), the side effects of setting it, and whether a PQA_* variable presets it as an integer.
# ("select" has PQA_SELECT, but that takes words -- sample, argmax -- and is read by itself: no integer variable.)
STOP_SERVER, SETTLE_POLE_LIST, BUMP_KB_VERSION = 1, 2, 4
POLE = STOP_SERVER | SETTLE_POLE_LIST
I64_MAX = 2**63 - 1
MAX_WORKERS = 1000
OPTIONS = [
    # name, lo, hi, default, flag, effects, has_env
    ("combine", 0, 1, 1, 1, 0, 1),
    ("combine_spin", 0, 1, 1, 1, 0, 0),
    ("top_exact", 0, 1, 1, 1, 0, 0),
    ("time_sweeps", 0, 1, 0, 1, 0, 0),
    ("long_row_form", 0, 1, 1, 1, 0, 0),
    ("rows_stage", 0, 1, 1, 1, 0, 0),
    ("fuse_update", 0, 1, 1, 1, 0, 0),
    ("post_always", 0, 1, 0, 1, 0, 0),
    ("bug_compat", 0, 1, 1, 1, 0, 1),
    ("use_graph", 0, 1, 0, 1, 0, 0),
    ("fused_sampled", 0, 1, 0, 1, 0, 0),
    ("host_sampled", 0, 1, 1, 1, 0, 0),
    ("sampled_batch_host", 0, 1, 0, 1, 0, 0),
    ("rerank", 0, 1, 1, 1, 0, 0),
    ("batch_tail", 0, 1, 1, 1, 0, 0),
    ("server", 0, 1, 0, 1, STOP_SERVER, 1),
    ("speculate", 0, 1, 1, 1, 0, 1),
    ("server_vram_mailbox", 0, 1, 1, 1, 0, 0),
    ("pole_fix", 0, 1, 1, 1, POLE | BUMP_KB_VERSION, 1),
    ("pole_gate", 0, 1, 1, 1, POLE, 0),
    ("pole_lazy", 0, 1, 1, 1, POLE, 0),
    ("pole_follow", 0, 1, 1, 1, POLE, 0),
    ("select", 0, 1, 0, 0, 0, 0),
    ("late_eager", 0, 1000000, 3, 0, 0, 0),
    ("combine_linger_us", 0, 10000, 20, 0, 0, 0),
    ("train_chunk_steps", 1, 2**28, 2**22, 0, 0, 0),
    ("workers", 1, MAX_WORKERS, 16, 0, 0, 1),
    ("eval_subtasks", 0, 8192, 0, 0, 0, 0),
    ("eval_variant", 0, I64_MAX, 0, 0, 0, 0),
    ("top_cache", 0, 256, 10, 0, 0, 0),
    ("eval_max_grid", 0, 65535, 0, 0, STOP_SERVER | BUMP_KB_VERSION, 0),
    ("batch_min", 0, 257, 0, 0, 0, 0),
    ("batch_form", 0, 3, 0, 0, 0, 0),
    ("batch_qb", 0, 4, 0, 0, 0, 0),
    ("batch_tile", 0, 8192, 0, 0, 0, 0),
    ("batch_groups", 0, 8, 0, 0, 0, 0),
    ("cluster_shape", 0, 2, 0, 0, 0, 0),
    ("cluster_form", 0, 2, 0, 0, 0, 0),
    ("cluster_from", 1024, 16384, 10240, 0, STOP_SERVER, 0),
    ("server_idle_us", 10, 1000000, 500, 0, STOP_SERVER, 0),
]


def test_option_table_is_the_contract():
    assert len(OPTIONS) == 40 and len({o[0] for o in OPTIONS}) == 40
    for name, *spec in OPTIONS:
        assert probe("option_spec:" + name, [], 6) == (6, spec), name
    # what is no settable option: the write-only seed, a counter, a name nobody knows, no name
    for name in ("seed", "posted_ops", "shards", "no_such_option", "", "#", "#x", "#-1", "Combine", "combine "):
        assert probe("option_spec:" + name, [], 6)[0] == -1, name
    assert probe("option_spec:combine", [], 5)[0] == -1          # output too small
    # the table holds nothing beyond the list: as many rows as the list, each of them one of the list's
    rows = []
    while probe("option_spec:#%d" % len(rows), [], 6)[0] == 6:
        rows.append(probe("option_spec:#%d" % len(rows), [], 6)[1])
        assert len(rows) <= len(OPTIONS)
    assert len(rows) == len(OPTIONS)
    assert sorted(rows) == sorted(list(o[1:]) for o in OPTIONS)
