"""No-GPU checks of question pages across process-per-GPU shards: the three exports are declared in include/PqaHipExt.h, bound in
probqa_amd/interop.py and exported by the built libPqaCore.so; dist.merge_page_step on hand-made records; and the bookkeeping of
dist.list_question_page_batch / dist.eval_conditional_gains_batch (what is packed when, which quizzes a step carries, a refusal on one
rank) over gloo on the CPU, at 2 and 3 ranks, against a fake engine that records what it is asked to do."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

import abi_common as abi
import ranks_common as rc
from probqa_amd import dist as pdist
from probqa_amd import interop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (argument count, Python method)
EXPORTS = {
    "PqaHip_PackGivenBlocks": (6, "pack_given_blocks"),
    "PqaEngine_EvalConditionalGainsBatchFromBlocks": (11, "eval_conditional_gains_batch_from_blocks"),
    "PqaHip_SelectPageStepFromBlocks": (10, "select_page_step_from_blocks"),
}


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_header_declares(name):
    params = abi.header_params(name)
    assert len([a for a in params.split(",") if a.strip()]) == EXPORTS[name][0], params


def test_header_argument_lists():
    squeeze = lambda s: " ".join(s.split())
    assert squeeze(abi.header_params("PqaHip_PackGivenBlocks")) == \
        "void *pvEngine, int64_t nQuestions, const int64_t *pQuestions, void *pDst, void *pFlag, uint64_t flagValue"
    given = "void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven, "
    package = "int64_t nBlocks, const int64_t *pBlockQuestions, const void *pBlocks, int64_t slotBytes, "
    assert squeeze(abi.header_params("PqaEngine_EvalConditionalGainsBatchFromBlocks")) == given + package + "double *pOut, int64_t n"
    assert squeeze(abi.header_params("PqaHip_SelectPageStepFromBlocks")) == given + package + "CiHipSelection *pOut"
    assert "left to a later change" not in abi.header_text()


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_binding_carries(name):
    _, argtypes = abi.bound_as(name)
    assert len(argtypes) == EXPORTS[name][0]
    assert callable(getattr(interop.PqaEngine, EXPORTS[name][1], None))


def test_library_exports(factory):
    assert set(EXPORTS) <= abi.exported_symbols(), set(EXPORTS) - abi.exported_symbols()
    for name in EXPORTS:
        assert getattr(interop.load_library(), name) is not None


def test_dist_has_the_collectives():
    for name in ("eval_conditional_gains_batch", "list_question_page_batch", "list_question_page", "merge_page_step"):
        assert callable(getattr(pdist, name, None)), name


# ---- the pure merge ----------------------------------------------------------------------------------------------------------
def test_merge_page_step():
    ranks = [[(0.5, 3), (0.0, -1), (0.25, 1), (0.0, 2), (float("nan"), 0)],
             [(0.5, 12), (0.0, -1), (0.75, 20), (0.0, 11), (0.125, 15)],
             [(0.5, 2), (0.0, -1), (0.75, 30), (-1.0, 25), (0.0, -1)]]
    want = [(2, 0.5),        # equal bits: the lowest GLOBAL id, whichever rank reports it
            (-1, 0.0),       # nobody has a candidate
            (20, 0.75),      # the largest bits; among equals the lowest id
            (-1, 0.0),       # bits of 0 (or below) are no candidate, even with an id
            (15, 0.125)]     # a NaN is none
    assert pdist.merge_page_step(ranks) == want
    assert pdist.merge_page_step(np.array(ranks, dtype=np.float64)) == want
    assert pdist.merge_page_step(torch.tensor(ranks, dtype=torch.float64)) == want
    assert pdist.merge_page_step([[(0.5, 7)]]) == [(7, 0.5)]
    assert pdist.merge_page_step([[], []]) == []


# ---- the collectives over gloo, against a fake engine ----------------------------------------------------------------------
Q_TOTAL, K, SLOT = 10, 2, 16            # (K = 2: sets up to 8 deep pass the branch limit)
# quiz -> question -> bits: the quizzes 0 and 1 share their first pick (question 7), quiz 2 has two candidates only, quiz 3 none
SCORES = {0: {7: 0.9, 1: 0.8, 4: 0.7, 9: 0.6, 5: 0.5}, 1: {7: 0.95, 8: 0.5, 0: 0.5, 3: 0.25}, 2: {2: 0.5, 6: 0.25}, 3: {}}


def block_value(q):
    return 100.0 + q


def greedy_page(quiz, page_size, given):
    cand = sorted(((-bits, q) for q, bits in SCORES[quiz].items() if q not in given))
    return [(q, -neg) for neg, q in cand[:page_size]]


class FakeEngine:
    """Holds questions [first, limit); question q's block is SLOT doubles of block_value(q); a question's bits for a quiz are SCORES',
    whatever the set.  Records every call and every collective (`log`); fail_* make that step raise."""

    def __init__(self, first, limit, log, fail_pack=False, fail_select=False, fail_eval=False):
        self.first, self.limit, self.log = first, limit, log
        self.fail_pack, self.fail_select, self.fail_eval = fail_pack, fail_select, fail_eval

    def question_block_slot_bytes(self):
        return SLOT * 8

    def get_option(self, name):
        return {"precision": 3, "local_questions": self.limit - self.first, "q_first": self.first}[name]

    def copy_dims(self):
        return interop.EngineDimensions(K, Q_TOTAL, 13)

    def synchronize(self):
        self.log.append(("sync",))

    @staticmethod
    def _view(address, n):
        buf = (ctypes.c_double * (n * SLOT)).from_address(address)
        return torch.frombuffer(buf, dtype=torch.float64).view(n, SLOT)

    def pack_given_blocks(self, questions, dst, flag=0, flag_value=0):
        self.log.append(("pack", list(questions)))
        if self.fail_pack:
            raise interop.PqaException("[IndexOutOfRange] questionId=99 fake pack refusal")
        view = self._view(dst, max(len(questions), 1))
        assert not view.any()                       # the new slots arrive zero-filled
        for i, q in enumerate(questions):
            if self.first <= q < self.limit:
                view[i] = block_value(q)

    def _check_package(self, given, block_questions, blocks_ptr):
        named = list(block_questions)
        assert len(set(named)) == len(named)        # every distinct question once
        view = self._view(blocks_ptr, max(len(named), 1))
        for s in given:
            for q in s:
                assert q in named, (q, named)
                assert bool((view[named.index(q)] == block_value(q)).all()), (q, view[named.index(q)])
        return view, named

    def select_page_step_from_blocks(self, quizzes, given, block_questions=(), blocks_ptr=0):
        self.log.append(("select", list(quizzes), [list(s) for s in given], list(block_questions)))
        if self.fail_select:
            raise interop.PqaException("[IndexOutOfRange] entry=0 fake select refusal")
        self._check_package(given, block_questions, blocks_ptr)
        out = np.zeros((len(quizzes), 2))
        for i, (quiz, s) in enumerate(zip(quizzes, given)):
            mine = sorted((-bits, q) for q, bits in SCORES[quiz].items() if self.first <= q < self.limit and q not in s)
            out[i] = (-mine[0][0], mine[0][1]) if mine else (0.0, -1)
        return out

    def eval_conditional_gains_batch_from_blocks(self, quizzes, given, block_questions=(), blocks_ptr=0):
        self.log.append(("eval", list(quizzes), [list(s) for s in given], list(block_questions)))
        if self.fail_eval:
            raise interop.PqaException("[WrongMode] fake eval refusal")
        view, named = self._check_package(given, block_questions, blocks_ptr)
        out = np.zeros((len(quizzes), self.limit - self.first))
        for i, (quiz, s) in enumerate(zip(quizzes, given)):
            for j in range(self.limit - self.first):
                out[i, j] = 1000 * quiz + self.first + j + sum(float(view[named.index(q)][0]) for q in s)
        return out


QUIZZES = [0, 1, 2, 3]
GIVEN = [[4, 9], [], [9], [0, 4, 0]]        # questions of several ranks, one shared by two sets, a duplicate member


def _fake_worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    rc.init_group("gloo", rank, world, port)
    cpu = torch.device("cpu")
    first, limit = pdist.shard_range(Q_TOTAL, world, rank)
    log = []
    real_all_reduce, real_all_gather = dist.all_reduce, dist.all_gather

    def logged_all_reduce(t, op=dist.ReduceOp.SUM, **kw):
        log.append(("sum", t.numel() // SLOT) if op == dist.ReduceOp.SUM else ("min",))
        return real_all_reduce(t, op=op, **kw)

    def logged_all_gather(parts, t, **kw):
        log.append(("gather", t.numel() * t.element_size()))
        return real_all_gather(parts, t, **kw)

    dist.all_reduce, dist.all_gather = logged_all_reduce, logged_all_gather
    out = {}
    eng = FakeEngine(first, limit, log)
    for page_size in (0, 1, 3, 6):
        del log[:]
        out["pages%d" % page_size] = pdist.list_question_page_batch(eng, QUIZZES, page_size, GIVEN, rank, world, device=cpu)
        out["log%d" % page_size] = list(log)
    out["single"] = pdist.list_question_page(eng, 1, 2, [7], rank, world, device=cpu)
    out["fresh"] = pdist.list_question_page_batch(eng, [0, 1], 2, None, rank, world, device=cpu)
    try:
        pdist.list_question_page_batch(eng, QUIZZES, 7, GIVEN, rank, world, device=cpu)     # 2^(3 + 6) rows for quiz 3
        out["limit"] = None
    except interop.PqaException as e:
        out["limit"] = str(e)
    del log[:]
    got = pdist.eval_conditional_gains_batch(eng, QUIZZES, GIVEN, rank, world, device=cpu)
    out["eval"], out["eval_log"] = got.tolist(), list(log)
    # a refusal on rank 1 only: the same text everywhere, and the ranks stay in step
    for name, kw, call in (("no_pack", {"fail_pack": rank == 1}, "page"), ("no_select", {"fail_select": rank == 1}, "page"),
                           ("no_eval_pack", {"fail_pack": rank == 1}, "eval"), ("no_eval", {"fail_eval": rank == 1}, "eval")):
        del log[:]
        bad = FakeEngine(first, limit, log, **kw)
        try:
            if call == "page":
                pdist.list_question_page_batch(bad, QUIZZES, 3, GIVEN, rank, world, device=cpu)
            else:
                pdist.eval_conditional_gains_batch(bad, QUIZZES, GIVEN, rank, world, device=cpu)
            out[name + "_raised"] = None
        except interop.PqaException as e:
            out[name + "_raised"] = str(e)
        out[name + "_log"] = [x[0] for x in log]
        out[name + "_again"] = pdist.list_question_page_batch(eng, QUIZZES, 3, GIVEN, rank, world, device=cpu)
    ret[rank] = out
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_collective_bookkeeping_over_gloo(world):
    ret = rc.run_gloo(_fake_worker, world)
    given0 = [4, 9, 0]                                # the distinct given questions in order of first appearance
    for r in range(world):
        got = ret[r]
        for page_size in (0, 1, 3, 6):
            want = [greedy_page(z, page_size, s) for z, s in zip(QUIZZES, GIVEN)]
            assert got["pages%d" % page_size] == want, (r, page_size, got["pages%d" % page_size])
        assert got["log0"] == []                      # a page of 0 runs no step
        assert got["single"] == greedy_page(1, 2, [7]) and got["fresh"] == [greedy_page(0, 2, []), greedy_page(1, 2, [])]
        assert got["limit"] is not None and "entry=3" in got["limit"] and "branches=" in got["limit"] and got["limit"] == ret[0]["limit"]
        # ---- a page of 3: what crosses per step, and who is still in it
        log = got["log3"]
        assert [x[0] for x in log] == ["pack", "sync", "sum", "min", "select", "min", "gather"] * 3, (r, log)
        packs = [x[1] for x in log if x[0] == "pack"]
        # step 1 picks 7, 7, 2 -- question 7 crosses ONCE --; step 2 picks 1, 0 (8 and 0 are equal: the lowest id), 6 -- 0 is in the package already
        assert packs == [given0, [7, 2], [1, 6]], (r, packs)
        assert [x[1] for x in log if x[0] == "sum"] == [len(p) for p in packs]                       # ONE all-reduce over the new slots only
        selects = [x for x in log if x[0] == "select"]
        assert [s[1] for s in selects] == [[0, 1, 2, 3], [0, 1, 2], [0, 1, 2]]                      # quiz 3 has no pick: it leaves
        assert selects[1][2] == [[4, 9, 7], [7], [9, 2]] and selects[2][2] == [[4, 9, 7, 1], [7, 0], [9, 2, 6]]
        assert selects[2][3] == given0 + [7, 2, 1, 6] and len(set(selects[2][3])) == len(selects[2][3])
        assert [x[1] for x in log if x[0] == "gather"] == [16 * 4, 16 * 3, 16 * 3]                   # 16 bytes a quiz of the step
        # ---- a page of 6: quiz 2 finishes after its two candidates, quiz 0 after three; the sixth step has nobody left and does not run
        selects = [x for x in got["log6"] if x[0] == "select"]
        assert [s[1] for s in selects] == [[0, 1, 2, 3], [0, 1, 2], [0, 1, 2], [0, 1], [1]], (r, [s[1] for s in selects])
        assert [x[1] for x in got["log6"] if x[0] == "pack"] == [given0, [7, 2], [1, 6], [5, 8], [3]]
        # ---- Eval: one package of the distinct given questions, this rank's columns
        first, limit = pdist.shard_range(Q_TOTAL, world, r)
        want = [[1000 * z + q + sum(block_value(g) for g in s) for q in range(first, limit)] for z, s in zip(QUIZZES, GIVEN)]
        assert got["eval"] == want, r
        assert [x[0] for x in got["eval_log"]] == ["pack", "sync", "sum", "min", "eval", "min"]
        assert got["eval_log"][0][1] == given0 and got["eval_log"][4][3] == given0
        # ---- refusals
        for name, steps in (("no_pack", ["pack", "sync", "sum", "min"]), ("no_select", ["pack", "sync", "sum", "min", "select", "min"]),
                            ("no_eval_pack", ["pack", "sync", "sum", "min"]), ("no_eval", ["pack", "sync", "sum", "min", "eval", "min"])):
            text = got[name + "_raised"]
            assert text is not None and text.startswith("rank 1: ") and "fake" in text, (r, name, text)
            assert text == ret[0][name + "_raised"]
            assert got[name + "_log"] == steps, (r, name, got[name + "_log"])      # nobody goes on behind the status word
            assert got[name + "_again"] == [greedy_page(z, 3, s) for z, s in zip(QUIZZES, GIVEN)], (r, name)
