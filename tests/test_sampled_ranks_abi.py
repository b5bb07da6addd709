"""No-GPU checks of the sampled selector across process-per-GPU shards: the four exports are declared in include/PqaHipExt.h, bound in
probqa_amd/interop.py and exported by the built libPqaCore.so; the plain-Python model of the selection part picks what select_py
picks over the whole vector; the library's layout of a part (PqaHip_HostLogicProbe "sampled_part") is the model's; the fallback of the
model is the oracle's; the two-rank collective runs over gloo against a fake engine that records its calls; and every guarded draw of
the GPU tests keeps its distance from the oracle's run-length boundaries at the subtask count the test uses."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

import abi_common as abi
import ranks_common as rc
import sampled_batch_common as sb
import sampled_ranks_common as sr
from probqa_amd import dist as pdist
from probqa_amd import interop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (argument count, Python method)
EXPORTS = {
    "PqaHip_SampledPartBytes": (1, "sampled_part_bytes"),
    "PqaHip_PackSampledParts": (6, "pack_sampled_parts"),
    "PqaHip_SampledPickFromParts": (8, "sampled_pick_from_parts"),
    "PqaEngine_TakeSampledPicks": (5, "take_sampled_picks"),
}


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_header_declares(name):
    params = abi.header_params(name)
    assert len([a for a in params.split(",") if a.strip()]) == EXPORTS[name][0], params


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_binding_carries(name):
    _, argtypes = abi.bound_as(name)
    assert len(argtypes) == EXPORTS[name][0]
    assert callable(getattr(interop.PqaEngine, EXPORTS[name][1], None))


def test_library_exports(factory):
    assert set(EXPORTS) <= abi.exported_symbols(), set(EXPORTS) - abi.exported_symbols()
    for name in EXPORTS:
        assert getattr(interop.load_library(), name) is not None


def test_dist_offers_the_collective():
    for name in ("next_question_sampled_batch", "next_question_sampled", "broadcast_rnds", "merge_sampled_picks"):
        assert callable(getattr(pdist, name, None)), name


# ---- the model: the pick from parts is select_py's over the whole vector ----------------------------------------------------------------
def random_bounds(rng, Q, world):
    world = min(world, Q)
    return sorted(rng.choice(np.arange(1, Q), size=world - 1, replace=False).tolist()) + [Q] if world > 1 else [Q]


def vectors(rng, Q):
    pri = (10.0 ** rng.uniform(-12, 3, size=Q)).tolist()          # fifteen decades
    skip = (rng.random(Q) < 0.3).tolist()
    return pri, skip


@pytest.mark.parametrize("Q", [1, 2, 7, 37, 64, 129, 500, 1000])
def test_model_pick_from_parts_equals_select_py(Q):
    rng = np.random.default_rng(7000 + Q)
    checked = pieces_seen = 0
    for n_sub in (1, 5, 16, 128, Q + 3):
        for world in (1, 2, 3, 8):
            every = [pdist.shard_bounds(Q, world)] if world <= Q else []
            every.append(random_bounds(rng, Q, world))
            if Q >= 8:   # one-question shards, and several bounds inside one subtask
                every.append([1, 2, 3, Q])
                every.append(sr.hand_bounds(Q))
            for bounds in every:
                pri, skip = vectors(rng, Q)
                parts = sr.parts_of(pri, skip, n_sub, bounds)
                assert all(len(p["pieces"]) <= 2 for p in parts)
                pieces_seen += sum(len(p["pieces"]) for p in parts)
                for rnd in sb.EDGE_RNDS + sb.draws(Q + n_sub + world, 3):
                    want = sb.select_py(pri, skip, n_sub, rnd)
                    got, per_rank = sr.merged_pick(parts, Q, n_sub, rnd)
                    assert got == want, (Q, n_sub, bounds, rnd, per_rank)
                    # every rank that holds a piece of a chosen cut subtask reports the pick itself
                    quot, rem, _, _, _, _ = sr.layout(Q, n_sub)
                    for r, p in enumerate(parts):
                        if any(sr.subtask_range(s, quot, rem)[0] <= want < sr.subtask_range(s, quot, rem)[1] for s, _, _ in p["pieces"]):
                            assert per_rank[r] == want, (Q, n_sub, bounds, rnd, per_rank)
                    checked += 1
    assert checked > 100 and (Q < 8 or pieces_seen > 0)


def test_all_skipped_and_single_rank():
    pri, skip = [1.0, 2.0, 3.0, 4.0, 5.0], [True] * 5
    for bounds in ([5], [2, 5], [1, 2, 3, 4, 5]):
        for rnd in sb.EDGE_RNDS:
            assert sr.merged_pick(sr.parts_of(pri, skip, 2, bounds), 5, 2, rnd)[0] == sb.select_py(pri, skip, 2, rnd) == 4


# ---- the library's layout is the model's -----------------------------------------------------------------------------------------------
def probe(Q, n_sub, q_first, n):
    inp = (ctypes.c_int64 * 4)(Q, n_sub, q_first, n)
    out = (ctypes.c_int64 * 7)()
    got = interop.load_library().PqaHip_HostLogicProbe(b"sampled_part", inp, 4, out, 7)
    return got, list(out)


@pytest.mark.parametrize("Q", [1, 2, 37, 64, 1000, 1001])
def test_part_layout_of_the_library_is_the_models(Q, factory):
    rng = np.random.default_rng(Q)
    for n_sub in (1, 5, 16, 128, Q, Q + 7):
        _, _, _, _, _, size = sr.layout(Q, n_sub)
        assert size % 16 == 0
        ranges = [(0, Q)]
        for world in (2, 3, 8):
            for bounds in ([pdist.shard_bounds(Q, world)] if world <= Q else []) + [random_bounds(rng, Q, world)] + ([sr.hand_bounds(Q)] if Q >= 8 else []):
                ranges += list(zip([0] + bounds[:-1], bounds))
        for first, limit in ranges:
            got, out = probe(Q, n_sub, first, limit - first)
            first_whole, n_whole, pieces = sr.shape(Q, n_sub, first, limit - first)
            flat = [(s, m) for s, _, m in pieces] + [(-1, 0)] * (2 - len(pieces))
            assert got == 7 and out[0] == size and out[2] == n_whole and [tuple(out[3:5]), tuple(out[5:7])] == flat, (Q, n_sub, first, limit, out)
            if n_whole:
                assert out[1] == first_whole
    for bad in ((0, 1, 0, 1), (5, 0, 0, 1), (5, 2, -1, 1), (5, 2, 0, 0), (5, 2, 3, 3)):
        assert probe(*bad)[0] == -1, bad


def test_probe_needs_room():
    inp = (ctypes.c_int64 * 4)(10, 3, 0, 10)
    out = (ctypes.c_int64 * 6)()
    assert interop.load_library().PqaHip_HostLogicProbe(b"sampled_part", inp, 4, out, 6) == -1


# ---- the fallback of the model is the oracle's -----------------------------------------------------------------------------------------
def test_find_nearest_py_is_the_oracles(oracle_lib):
    import orclib

    rng = np.random.default_rng(3)
    for Q in (5, 37, 64, 65, 200, 333):
        for density in (0.5, 0.9, 0.99, 1.0):
            gaps = set(np.flatnonzero(rng.random(Q) < density / 2).tolist())
            asked = [int(q) for q in np.flatnonzero(rng.random(Q) < density) if int(q) not in gaps]
            orc = orclib.Oracle(2, Q, 4, 0.1)
            orc.set_question_gaps(sorted(gaps))
            orc.resume_quiz([(q, 0) for q in asked], 4)
            for middle in sorted(set([0, Q - 1, Q // 2] + rng.integers(0, Q, size=8).tolist())):
                assert sr.find_nearest_py(int(middle), Q, gaps | set(asked)) == orc.find_nearest(int(middle)), (Q, density, middle)


# ---- the guarded draws of the GPU tests -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", sr.gpu_configs(), ids=lambda c: c[0])
def test_guarded_draws_clear_the_boundaries(config, oracle_lib):
    _, case, option, _ = config
    n_sub = sr.n_sub_of(option)
    seed, rnds, steps = sr.guarded_draws(case, n_sub)
    assert len(rnds) == len(case.answers) + 1          # no draw left out: one per quiz of the batch
    for i, r in enumerate(rnds):
        assert sb.boundary_distance(steps[i][0], n_sub, r) > sb.GUARD, (case.name, n_sub, seed, i, r)
    assert sr.guarded_draws(case, n_sub)[:2] == (seed, rnds)   # a fixed sequence: the GPU tests draw the same numbers


# ---- the collective over gloo, against a fake engine -----------------------------------------------------------------------------------
Q_FAKE, WORDS = 10, 4


class FakeEngine:
    """Holds questions [first, limit); its part of quiz i is {rank, quiz, first, limit}; it picks question 7 for every quiz and
    reports it on the rank that holds it (-1 elsewhere) -- or, with `lie`, a pick of its own on every rank; records every call."""

    def __init__(self, rank, first, limit, lie=False, fail_pack=False):
        self.rank, self.first, self.limit, self.lie, self.fail_pack = rank, first, limit, lie, fail_pack
        self.calls, self.seen, self.active = [], None, {}

    def sampled_part_bytes(self):
        return 8 * WORDS

    def synchronize(self):
        self.calls.append("sync")

    def pack_sampled_parts(self, quizzes, dst, flag=0, flag_value=0):
        self.calls.append(("pack", list(quizzes)))
        if self.fail_pack:
            raise interop.PqaException("[IndexOutOfRange] fake refusal")
        buf = (ctypes.c_int64 * (WORDS * len(quizzes))).from_address(dst)
        for i, q in enumerate(quizzes):
            buf[WORDS * i:WORDS * i + WORDS] = [self.rank, q, self.first, self.limit]

    def sampled_pick_from_parts(self, quizzes, rnds, parts, rank, world):
        self.calls.append(("pick", list(quizzes), list(rnds), rank, world))
        n = len(quizzes)
        buf = (ctypes.c_int64 * (WORDS * n * world)).from_address(parts)
        self.seen = [list(buf[WORDS * k:WORDS * k + WORDS]) for k in range(n * world)]
        pick = 7 - self.rank if self.lie else (7 if self.first <= 7 < self.limit else -1)
        return np.array([(1.0, pick)] * n, dtype=np.float64).reshape(n, 2)

    def take_sampled_picks(self, quizzes, picks):
        self.calls.append(("take", list(quizzes), list(picks)))
        for q, p in zip(quizzes, picks):
            self.active[q] = p
        return [p if q != 99 else -1 for q, p in zip(quizzes, picks)]


def _fake_worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    rc.init_group("gloo", rank, world, port)
    cpu = torch.device("cpu")
    first, limit = pdist.shard_range(Q_FAKE, world, rank)
    out = {}
    mine = [2**64 - 1, 5, 2**63] if rank == 0 else [1, 2, 3]
    out["rnds"] = pdist.broadcast_rnds(mine)
    eng = FakeEngine(rank, first, limit)
    out["questions"] = pdist.next_question_sampled_batch(eng, [4, 2, 9], out["rnds"], rank, world, device=cpu)
    out["calls"] = [c if isinstance(c, str) else c[0] for c in eng.calls]
    out["pick_args"] = eng.calls[2][1:]
    out["take_args"] = eng.calls[3][1:]
    out["seen"] = eng.seen
    out["single"] = pdist.next_question_sampled(eng, 5, 11, rank, world, device=cpu)
    try:
        pdist.next_question_sampled(eng, 99, 11, rank, world, device=cpu)
        out["exhausted"] = None
    except interop.PqaException as e:
        out["exhausted"] = str(e)
    for name, bad in (("disagree", FakeEngine(rank, first, limit, lie=True)), ("refused", FakeEngine(rank, first, limit, fail_pack=(rank == 1)))):
        try:
            pdist.next_question_sampled_batch(bad, [4, 2], [1, 2], rank, world, device=cpu)
            out[name] = None
        except interop.PqaException as e:
            out[name] = str(e)
        out[name + "_calls"] = [c if isinstance(c, str) else c[0] for c in bad.calls]
        out[name + "_active"] = dict(bad.active)
    ret[rank] = out
    dist.destroy_process_group()


def test_two_rank_collective_over_gloo():
    world = 2
    ret = rc.run_gloo(_fake_worker, world)
    a, b = ret[0], ret[1]
    for rank, r in enumerate((a, b)):
        assert r["rnds"] == [2**64 - 1, 5, 2**63], r["rnds"]                      # rank 0's numbers win, all 64 bits of them
        assert r["calls"] == ["pack", "sync", "pick", "take"], r["calls"]
        assert r["pick_args"] == ([4, 2, 9], [2**64 - 1, 5, 2**63], rank, world)
        assert r["take_args"] == ([4, 2, 9], [7, 7, 7]) and r["questions"] == [7, 7, 7]
        # the gathered parts, rank-major: rank 0's three, then rank 1's
        assert r["seen"] == [[0, q, 0, 5] for q in (4, 2, 9)] + [[1, q, 5, 10] for q in (4, 2, 9)], r["seen"]
        assert r["single"] == 7
        assert r["exhausted"] is not None and "run out of questions" in r["exhausted"]
        assert r["disagree"] is not None and "different picks [6, 7]" in r["disagree"], r["disagree"]
        assert r["disagree_calls"] == ["pack", "sync", "pick"] and r["disagree_active"] == {}      # nothing was taken
        assert r["refused"] is not None and "rank 1" in r["refused"] and "fake refusal" in r["refused"], r["refused"]
        assert r["refused_active"] == {}
    assert a["disagree"] == b["disagree"] and a["refused"] == b["refused"]
    assert a["refused_calls"] == ["pack", "sync", "pick"] and b["refused_calls"] == ["pack", "sync"]


def test_merge_sampled_picks():
    assert pdist.merge_sampled_picks([[-1, 4, 9], [3, -1, 9], [-1, -1, -1]]) == [3, 4, 9]
    with pytest.raises(ValueError, match="entry 1.*different picks"):
        pdist.merge_sampled_picks([[1, 4], [-1, 5]])
    with pytest.raises(ValueError, match="entry 0.*no pick"):
        pdist.merge_sampled_picks([[-1], [-1]])
