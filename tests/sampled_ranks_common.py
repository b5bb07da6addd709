"""Shared by tests/test_sampled_ranks_abi.py and the GPU tests of the sampled selector across process-per-GPU shards: a plain-Python
model of the selection part (probqa_amd/csrc/sampled_part.h), of the pick from the gathered parts of all ranks and of the fallback
over the whole question axis (BaseEngine::FindNearestQuestion), plus the cases the GPU tests run and the seeds of their draws."""
from __future__ import annotations

import struct
from bisect import bisect_right

import numpy as np

import cases
import sampled_batch_common as sb
from probqa_amd import dist as pdist

HEADER_BYTES = 32


def layout(Q, n_sub):
    """(quot, rem, nS, L, W, bytes of a part)."""
    quot, rem, ns = sb.split(Q, n_sub)
    L = quot + (1 if rem > 0 else 0)
    W = (L + 63) // 64
    return quot, rem, ns, L, W, (HEADER_BYTES + 8 * ns + 2 * 8 * (L + W) + 15) // 16 * 16


def subtask_range(s, quot, rem):
    return (0 if s == 0 else sb.bound(s - 1, quot, rem)), sb.bound(s, quot, rem)


def shape(Q, n_sub, q_first, n):
    """What the shard [q_first, q_first + n) contributes: (first whole subtask, how many, [(subtask, first question, length)] of its
    at most two pieces): every subtask that meets the range lies whole inside it or is cut by one of its bounds."""
    quot, rem, ns, _, _, _ = layout(Q, n_sub)
    lo, hi = q_first, q_first + n
    whole, pieces = [], []
    for s in range(ns):
        first, limit = subtask_range(s, quot, rem)
        if limit <= lo or first >= hi:
            continue
        if lo <= first and limit <= hi:
            whole.append(s)
        else:
            pieces.append((s, max(first, lo), min(limit, hi) - max(first, lo)))
    assert len(pieces) <= 2 and (not whole or whole == list(range(whole[0], whole[0] + len(whole)))), (whole, pieces)
    return (whole[0] if whole else (pieces[0][0] + 1 if pieces else 0)), len(whole), pieces


def make_part(pri, skip, Q, n_sub, q_first, seq=1):
    """The part of a shard whose LOCAL priorities and skip flags are pri / skip; 'run' is what the shard keeps for itself: the
    running sums of its whole subtasks."""
    n = len(pri)
    quot, rem, ns, _, _, _ = layout(Q, n_sub)
    first_whole, n_whole, pieces = shape(Q, n_sub, q_first, n)
    total, run = [0.0] * ns, {}
    for s in range(first_whole, first_whole + n_whole):
        first, limit = subtask_range(s, quot, rem)
        st, sums = (0.0, 0.0), []
        for i in range(first - q_first, limit - q_first):
            if not skip[i]:
                st = sb.kahan_add(st, float(pri[i]))
            sums.append(st[0] - st[1])
        total[s], run[s] = st[0] - st[1], sums
    cut = [(s, [float(pri[i]) for i in range(f - q_first, f - q_first + m)], [bool(skip[i]) for i in range(f - q_first, f - q_first + m)]) for s, f, m in pieces]
    return {"q_first": q_first, "n": n, "nS": ns, "seq": seq, "total": total, "pieces": cut, "run": run}


def pick_from_parts(parts, Q, n_sub, rnd, rank):
    """(grand total, GLOBAL pick or -1) as `rank` computes it from the parts of all ranks: whole subtasks' totals from their holders,
    cut subtasks' by ONE Kahan chain continued through the ranks' pieces in rank order, then select_py's finish."""
    quot, rem, ns, _, _, _ = layout(Q, n_sub)
    at = 0
    for p in parts:
        assert p["q_first"] == at and p["n"] >= 1 and p["nS"] == ns
        at += p["n"]
    assert at == Q
    bounds = [p["q_first"] + p["n"] for p in parts]
    grand, chains = [], {}
    for s in range(ns):
        first, limit = subtask_range(s, quot, rem)
        r = bisect_right(bounds, first)
        if limit <= bounds[r]:
            grand.append(parts[r]["total"][s])
            continue
        st, sums = (0.0, 0.0), []
        while r < len(parts) and parts[r]["q_first"] < limit:
            (pri, skip), = [(pp, sk) for ss, pp, sk in parts[r]["pieces"] if ss == s]
            for v, k in zip(pri, skip):
                if not k:
                    st = sb.kahan_add(st, v)
                sums.append(st[0] - st[1])
            r += 1
        assert len(sums) == limit - first
        grand.append(st[0] - st[1])
        chains[s] = sums
    st = (0.0, 0.0)
    for s in range(ns):
        st = sb.kahan_add(st, grand[s])
        grand[s] = st[0] - st[1]
    tot = grand[-1]
    sel_run = tot * float(rnd) / sb.TWO64M1
    w = bisect_right(grand, sel_run)
    if w >= ns:
        return tot, Q - 1
    in_w = sel_run - (0.0 if w == 0 else grand[w - 1])
    first, limit = subtask_range(w, quot, rem)
    if w in chains:
        return tot, min(first + bisect_right(chains[w], in_w), limit - 1)
    if w in parts[rank]["run"]:
        return tot, min(first + bisect_right(parts[rank]["run"][w], in_w), limit - 1)
    return tot, -1


def merged_pick(parts, Q, n_sub, rnd):
    """The one pick of all ranks that is not -1 (they must agree), and every rank's own."""
    per_rank = [pick_from_parts(parts, Q, n_sub, rnd, r)[1] for r in range(len(parts))]
    seen = {p for p in per_rank if p >= 0}
    assert len(seen) == 1, per_rank
    return seen.pop(), per_rank


def parts_of(pri, skip, n_sub, bounds):
    """The parts of the shards that end at `bounds`, from the WHOLE vector."""
    Q, out, first = len(pri), [], 0
    for r, b in enumerate(bounds):
        out.append(make_part(pri[first:b], skip[first:b], Q, n_sub, first, seq=r + 1))
        first = b
    return out


def parse_part(raw: bytes, Q, n_sub):
    """A part as PqaHip_PackSampledParts writes it -> the model's fields (the pieces by the header's range; 'run' stays with the engine)."""
    _, _, ns, L, W, size = layout(Q, n_sub)
    assert len(raw) == size
    q_first, n, hns, seq = struct.unpack_from("<qqqQ", raw, 0)
    assert hns == ns and 0 <= q_first and n >= 1 and q_first + n <= Q, (q_first, n, hns)
    total = list(struct.unpack_from("<%dd" % ns, raw, HEADER_BYTES))
    pieces = []
    for k, (s, _, m) in enumerate(shape(Q, n_sub, q_first, n)[2]):
        off = HEADER_BYTES + 8 * ns + k * 8 * (L + W)
        pri = list(struct.unpack_from("<%dd" % m, raw, off))
        words = struct.unpack_from("<%dQ" % W, raw, off + 8 * L)
        pieces.append((s, pri, [bool((words[j >> 6] >> (j & 63)) & 1) for j in range(m)]))
    return {"q_first": q_first, "n": n, "nS": ns, "seq": seq, "total": total, "pieces": pieces, "run": {}}


def find_nearest_py(middle, Q, unavailable):
    """BaseEngine::FindNearestQuestion (PqaCore/BaseEngine.cpp:60-124) over Q questions: exact within `middle`'s 64-question pack,
    then pack by pack outwards, comparing only the two packs at the same distance.  -1: no question is left."""
    inf = 200
    avail = lambda p: sum(1 << i for i in range(64) if 64 * p + i < Q and (64 * p + i) not in unavailable)   # noqa: E731
    low = lambda x: (x & -x).bit_length() - 1   # noqa: E731
    pack, within = middle >> 6, middle & 63
    a = avail(pack)
    if a:
        base = (1 << within) - 1
        higher, lower = a & ~base, a & base
        d_hi = low(higher) - within if higher else inf
        d_lo = within - (lower.bit_length() - 1) if lower else inf
        return middle + d_hi if d_hi < d_lo else middle - d_lo
    lim, i = (Q + 63) >> 6, 1
    while pack >= i and pack + i < lim:
        left, right = avail(pack - i), avail(pack + i)
        if not (left | right):
            i += 1
            continue
        d_hi = low(right) + 64 - within if right else inf
        d_lo = within + 64 - (left.bit_length() - 1) if left else inf
        if d_hi < d_lo:
            return middle + d_hi + ((i - 1) << 6)
        return middle - d_lo - ((i - 1) << 6)
    while pack >= i:
        left = avail(pack - i)
        if left:
            return middle - (within + 64 - (left.bit_length() - 1)) - ((i - 1) << 6)
        i += 1
    while pack + i < lim:
        right = avail(pack + i)
        if right:
            return middle + (low(right) + 64 - within) + ((i - 1) << 6)
        i += 1
    return -1


def take_py(pick, Q, unavailable):
    return find_nearest_py(pick, Q, unavailable) if pick in unavailable else pick


# ---- what the GPU tests run (tests/test_gpu_sampled_ranks.py) and what the no-GPU test checks of it ----------------------------------
def hand_bounds(Q):
    return [3, 5, 6, Q]


def gpu_configs():
    """(name, case, eval_subtasks option (0: the default, 8 x workers), [bounds per world])."""
    small = sb.scenarios()[1]
    assert small.name == "gaps_37x5x101"
    synth = sb.synthetic_case()
    return [
        ("gaps37_sub5", small, 5, [pdist.shard_bounds(small.Q, w) for w in (2, 3, 8)]),        # every bound cuts a subtask
        ("gaps37_sub16_hand", small, 16, [hand_bounds(small.Q)]),                              # shards inside one subtask, three bounds in it
        ("gaps37_default", small, 0, [pdist.shard_bounds(small.Q, 3)]),                        # subtasks are single questions: no pieces
        ("synth1000_default", synth, 0, [pdist.shard_bounds(synth.Q, w) for w in (2, 3, 8)]),
    ]


def n_sub_of(option):
    return option if option else sb.SUBTASKS


DRAW_SEEDS = range(500, 564)


def guarded_draws(case, n_sub):
    """One random number per quiz (quiz i = the case after i answers) for the configs above: the first seed of a fixed sequence whose
    draws ALL lie more than GUARD from every run-length boundary of the oracle at n_sub.  -> (seed, draws, the oracle's steps)."""
    steps = sb.oracle_steps(case, n_sub)
    n = len(case.answers) + 1
    for seed in DRAW_SEEDS:
        rnds = sb.draws(seed, n)
        if all(sb.boundary_distance(steps[i][0], n_sub, rnds[i]) > sb.GUARD for i in range(n)):
            return seed, rnds, steps
    raise AssertionError("no seed found")


def oracle_picks(case, n_sub, rnd_lists):
    """Per step i (the quiz after i answers): {rnd: the oracle's question} for every list's number i -- its selector's pick, and where
    that is a gap or was asked its FindNearestQuestion, as CpuEngine::NextQuestion goes on (-1: no question left)."""
    orc = case.make_oracle()
    orc.start_quiz(cases.WORKERS)
    out = []
    for i in range(len(case.answers) + 1):
        run, _ = orc.eval(n_sub)
        out.append({rnds[i]: orc.select_sampled(run.copy(), n_sub, rnds[i]) for rnds in rnd_lists})
        if i < len(case.answers):
            q, a = case.answers[i]
            orc.record_answer(q, a, cases.WORKERS - 1)
    return out
