"""No-GPU checks of maintenance on process-per-GPU shards: the four exports are declared in include/PqaHipExt.h, bound in
probqa_amd/interop.py and exported by the built libPqaCore.so; and the host logic of a compaction over shards -- which shard would be
left without a question, the ranges afterwards, which rank a moved question leaves and which it reaches (kb_plan.h: PlanShardCompact,
through the "shard_compact" script of PqaHip_HostLogicProbe) -- is held to tests/kb_model.py's compact_model plus the clip rule: a
shard keeps the part of its range below the new question count."""
import bisect
import ctypes
import os
import random

import pytest

import abi_common as abi
import maintenance_cases as mc
import ranks_common as rc
from kb_model import KBModel, compact_model, random_step
from probqa_amd import dist as pdist
from probqa_amd import interop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (argument count, Python method)
EXPORTS = {
    "PqaHip_CompactPlan": (6, "compact_plan"),
    "PqaHip_QuestionBlockSlotBytes": (1, "question_block_slot_bytes"),
    "PqaHip_PackQuestionBlocks": (6, "pack_question_blocks"),
    "PqaEngine_CompactFromBlocks": (8, "compact_from_blocks"),
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
    lib = interop.load_library()
    for name in EXPORTS:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == tuple(abi.bound_as(name))


def test_dist_has_the_collectives():
    for name in ("gather_bounds", "owner_in", "remove_questions", "remove_targets", "add_qs_ts", "compact"):
        assert callable(getattr(pdist, name, None)), name
    bounds = [5, 8, 11]
    assert [pdist.owner_in(bounds, q) for q in (0, 4, 5, 7, 8, 10)] == [0, 0, 1, 1, 2, 2]
    for bad in (-1, 11):
        with pytest.raises(IndexError):
            pdist.owner_in(bounds, bad)


# ---- the host logic of a compaction over shards --------------------------------------------------------------------------------------
def probe(bounds, Q, T, q_gaps, t_gaps):
    """-> (refused, new bounds, [(dst, src, dst's shard, src's shard)]) from the library, or None for a refused script."""
    lib = interop.load_library()
    words = [len(bounds)] + list(bounds) + [Q, T, len(q_gaps)] + list(q_gaps) + [len(t_gaps)] + list(t_gaps)
    src = (ctypes.c_int64 * len(words))(*words)
    out = (ctypes.c_int64 * (4 + len(bounds) + 4 * Q))()
    n = lib.PqaHip_HostLogicProbe(b"shard_compact", src, len(words), out, len(out))
    if n < 0:
        return None
    res = list(out[:n])
    nb = res[1]
    new_bounds = res[2:2 + nb]
    nm = res[2 + nb]
    flat = res[3 + nb:3 + nb + nm]
    assert len(flat) == nm and nm % 4 == 0 and 3 + nb + nm == n
    return bool(res[0]), new_bounds, [tuple(flat[i:i + 4]) for i in range(0, nm, 4)]


def model(bounds, Q, T, q_gaps, t_gaps):
    """compact_model plus the clip rule."""
    old_q, _, moves = compact_model(Q, T, q_gaps, t_gaps)
    n_q = len(old_q)
    firsts = [0] + list(bounds[:-1])
    refused = any(min(b, n_q) <= f for f, b in zip(firsts, bounds))
    owner = lambda q: bisect.bisect_right(bounds, q)      # noqa: E731
    return refused, [min(b, n_q) for b in bounds], [(d, s, owner(d), owner(s)) for d, s in moves]


def compaction_states(K, Q, T, steps, f32=False):
    """(Q, T, question gaps, target gaps) in front of every compaction of a script, from the model alone."""
    import numpy as np

    m = KBModel(np.zeros((Q, K, T)), np.zeros((Q, T)), np.zeros(T), f32=f32)
    for step in steps:
        if step[0] == "compact":
            yield m.Q, m.T, list(m.q_gaps), list(m.t_gaps)
        m.apply(step)


WORLD3_STEPS = [("remove_q", [8, 1, 10]), ("remove_t", [t for t in range(40) if t % 3 == 1]), ("compact",), ("add", [0.5, 1.5], [0.3, 0.7, 1.0, 0.5])]


def test_compact_across_granule_crosses_the_ranks_at_world_2_and_is_refused_at_world_3():
    (K, Q, T), _, steps = mc.array_scripts(False)["compact_across_granule"]
    (state,) = list(compaction_states(K, Q, T, steps))
    got = probe(pdist.shard_bounds(Q, 2), *state)
    assert got == model(pdist.shard_bounds(Q, 2), *state)
    assert got == (False, [5, 6], [(0, 7, 0, 1), (4, 6, 0, 1)])
    got = probe(pdist.shard_bounds(Q, 3), *state)
    assert got == model(pdist.shard_bounds(Q, 3), *state)
    assert got[0] and got[1] == [3, 6, 6]                   # the last shard [6, 9) would be emptied


def test_the_world_3_script_moves_one_question_across_and_one_inside():
    (state,) = list(compaction_states(3, 12, 40, WORLD3_STEPS))
    got = probe([4, 8, 12], *state)
    assert got == model([4, 8, 12], *state)
    assert got == (False, [4, 8, 9], [(1, 11, 0, 2), (8, 9, 2, 2)])


@pytest.mark.parametrize("world", [2, 3])
def test_random_scripts_refuse_only_seed_6(world):
    """The ten random scripts of the GPU test under its range model: appended questions go to the last shard, a compaction clips."""
    import numpy as np

    refused_seeds, cross = [], {}
    for seed in range(mc.N_RANDOM_SCRIPTS):
        rng, (K, Q, T), _ = mc.random_script_start(seed)
        m = KBModel(np.zeros((Q, K, T)), np.zeros((Q, T)), np.zeros(T))
        bounds = pdist.shard_bounds(Q, world)
        for _ in range(mc.RANDOM_STEPS):
            step = random_step(m, rng)
            if step[0] == "compact":
                state = (m.Q, m.T, list(m.q_gaps), list(m.t_gaps))
                got = probe(bounds, *state)
                assert got == model(bounds, *state), (seed, step)
                cross[seed] = cross.get(seed, 0) + sum(1 for _, _, d, s in got[2] if d != s)
                if got[0]:
                    refused_seeds.append(seed)
                    break
                bounds = got[1]
            m.apply(step)
            if step[0] == "add":
                bounds = bounds[:-1] + [m.Q]
            assert bounds[-1] == m.Q
    assert refused_seeds == [6], refused_seeds
    if world == 2:
        assert cross.get(3, 0) == 2, cross


def test_200_random_states_follow_the_model():
    rng = random.Random(20260)
    seen_refused = seen_cross = 0
    for _ in range(200):
        Q, T = rng.randrange(1, 40), rng.randrange(2, 30)
        world = rng.randrange(1, min(Q, 8) + 1)
        cuts = sorted(rng.sample(range(1, Q), world - 1))
        bounds = cuts + [Q]
        q_gaps = rng.sample(range(Q), rng.randrange(0, Q))          # at least one question survives
        t_gaps = rng.sample(range(T), rng.randrange(0, T - 1))
        got = probe(bounds, Q, T, q_gaps, t_gaps)
        want = model(bounds, Q, T, q_gaps, t_gaps)
        assert got == want, (bounds, Q, T, q_gaps, t_gaps)
        seen_refused += got[0]
        seen_cross += any(d != s for _, _, d, s in got[2])
    assert 20 < seen_refused < 180 and seen_cross > 20, (seen_refused, seen_cross)


def test_malformed_scripts_are_refused():
    assert probe([3, 3, 9], 9, 4, [], []) is None           # a shard without a question
    assert probe([3, 6], 9, 4, [], []) is None              # bounds that do not end at Q
    assert probe([9], 9, 4, [9], []) is None                # a gap outside the axis
    assert probe([9], 9, 4, [], []) == (False, [9], [])


# ---- the collectives over gloo, against a fake engine ---------------------------------------------------------------------------------
W = 6      # elements of a fake question block


class FakeShard:
    """Questions [first, first + n) of a fake KB whose block of question q holds 100 q + 1 .. 100 q + W (later: whatever moved there);
    the global gap list as every rank keeps it.  compact_from_blocks follows the engine's rule: the holder of dst takes src from
    its own blocks or from slot i of the package."""

    def __init__(self, first, n, q_total, fail_add=False):
        import torch

        self.first, self.n, self.q_total, self.fail_add = first, n, q_total, fail_add
        self.gaps, self.calls = [], []
        self.blocks = {q: torch.arange(1, W + 1, dtype=torch.float64) + 100 * q for q in range(first, first + n)}

    def get_option(self, name):
        return {"q_first": self.first, "local_questions": self.n, "q_total": self.q_total, "precision": 3}[name]

    def owns(self, q):
        return self.first <= q < self.first + self.n

    def synchronize(self):
        self.calls.append("sync")

    def remove_questions(self, ids):
        if any(q in self.gaps or not 0 <= q < self.q_total for q in ids):
            raise interop.PqaException("[The ID is absent from KB] fake")
        self.gaps.extend(ids)

    def add_qs_ts(self, add_questions, add_targets):
        if self.fail_add:
            raise interop.PqaException("[fake] out of memory")
        for p in add_questions:
            p.i_question = self.gaps.pop() if self.gaps else self.q_total
            if p.i_question == self.q_total:
                self.q_total += 1
                if self.first + self.n == self.q_total - 1:
                    self.n += 1

    def compact_plan(self):
        old_q, _, moves = compact_model(self.q_total, 2, self.gaps, [])
        return len(old_q), 2, moves, min(self.first + self.n, len(old_q)) <= self.first

    def question_block_slot_bytes(self):
        return 8 * W

    def _view(self, address, n):
        import torch

        return torch.frombuffer((ctypes.c_double * (n * W)).from_address(address), dtype=torch.float64).view(n, W)

    def pack_question_blocks(self, questions, dst, flag=0, flag_value=0):
        self.calls.append(("pack", list(questions)))
        view = self._view(dst, len(questions))
        for i, q in enumerate(questions):
            if self.owns(q):
                view[i] = self.blocks[q]

    def compact_from_blocks(self, blocks=0, slot_bytes=0, emptied_rank=-1):
        n_q, _, moves, _ = self.compact_plan()
        if emptied_rank >= 0:
            raise interop.PqaException("[Insufficient engine dimensions] [rank=%d] fake" % emptied_rank)
        self.calls.append(("compact", slot_bytes))
        for i, (dst, src) in enumerate(moves):
            if self.owns(dst):
                self.blocks[dst] = self.blocks[src] if self.owns(src) else self._view(blocks, len(moves))[i].clone()
        self.n = min(self.first + self.n, n_q) - self.first
        self.q_total, self.gaps = n_q, []
        self.blocks = {q: b for q, b in self.blocks.items() if self.owns(q)}
        return [src for _, src in moves], [0, 1]          # (a stand-in for the maps: the same on every rank is what is looked at)


def _fake_worker(rank, world, port, ret):
    import sys

    import torch
    import torch.distributed as dist

    sys.path.insert(0, ROOT)
    rc.init_group("gloo", rank, world, port)
    cpu = torch.device("cpu")
    out = {}
    first, limit = pdist.shard_range(9, world, rank)
    eng = FakeShard(first, limit - first, 9)
    out["bounds"] = [pdist.gather_bounds(eng)]
    pdist.remove_questions(eng, [0, 4, 8], rank, world, device=cpu)
    try:
        pdist.remove_questions(eng, [4], rank, world, device=cpu)
        out["bad_removal"] = None
    except interop.PqaException as e:
        out["bad_removal"] = str(e)
    try:
        out["compact"] = pdist.compact(eng, rank, world, device=cpu)
        out["refused"] = None
    except interop.PqaException as e:
        out["refused"] = str(e)
    out["bounds"].append(pdist.gather_bounds(eng))
    out["blocks"] = {q: b.tolist() for q, b in eng.blocks.items()}
    out["gaps"] = list(eng.gaps)
    if out["refused"] is None:
        aq = [interop.AddQuestionParam(1.0), interop.AddQuestionParam(2.0)]
        pdist.add_qs_ts(eng, aq, [], rank, world, device=cpu)
        out["added"] = [p.i_question for p in aq]
        out["bounds"].append(pdist.gather_bounds(eng))
        eng.fail_add = rank == 1                      # one rank fails: every rank raises its text
        try:
            pdist.add_qs_ts(eng, [interop.AddQuestionParam(1.0)], [], rank, world, device=cpu)
            out["failed_add"] = None
        except interop.PqaException as e:
            out["failed_add"] = str(e)
    out["calls"] = [c if isinstance(c, str) else c[0] for c in eng.calls]
    ret[rank] = out
    dist.destroy_process_group()


def _run_fake(world):
    ret = rc.run_gloo(_fake_worker, world)
    return [ret[r] for r in range(world)]


def test_two_rank_collectives_over_gloo():
    a, b = _run_fake(2)
    block = lambda q: [100.0 * q + i for i in range(1, W + 1)]      # noqa: E731
    for r in (a, b):
        assert r["bounds"] == [[5, 9], [5, 6], [5, 8]], r["bounds"]
        assert r["bad_removal"] is not None and "rank 0" in r["bad_removal"] and "absent" in r["bad_removal"]
        assert r["refused"] is None and r["compact"] == ([7, 6], [0, 1]) and r["gaps"] == []
        assert r["added"] == [6, 7]
        assert r["failed_add"] is not None and "rank 1" in r["failed_add"] and "out of memory" in r["failed_add"]
        assert r["calls"] == ["pack", "sync", "compact"], r["calls"]
    assert a["bad_removal"] == b["bad_removal"] and a["failed_add"] == b["failed_add"]
    # both moves 0 <- 7 and 4 <- 6 crossed from rank 1 to rank 0 through the summed package
    assert a["blocks"] == {0: block(7), 1: block(1), 2: block(2), 3: block(3), 4: block(6)}
    assert b["blocks"] == {5: block(5)}


def test_three_ranks_refuse_the_compaction_alike_over_gloo():
    got = _run_fake(3)
    texts = {r["refused"] for r in got}
    assert len(texts) == 1 and "Insufficient engine dimensions" in got[0]["refused"] and "rank=2" in got[0]["refused"], texts
    for r in got:
        assert r["bounds"] == [[3, 6, 9], [3, 6, 9]] and r["gaps"] == [0, 4, 8] and r["calls"] == []
