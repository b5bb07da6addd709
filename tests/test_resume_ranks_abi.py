"""No-GPU checks of ResumeQuiz across process-per-GPU shards: the four exports are declared in include/PqaHipExt.h, bound in
probqa_amd/interop.py and exported by the built libPqaCore.so; dist.row_owners agrees with owner_of; and the two-rank
collective's bookkeeping (pack, combine, resume, one status word, release on a failure elsewhere) runs over gloo on the CPU
against a fake engine that records what it is asked to do."""
import os
import sys

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
    "PqaHip_PackAnswerRows": (6, "pack_answer_rows"),
    "PqaHip_AnswerRowSlotBytes": (1, "answer_row_slot_bytes"),
    "PqaEngine_ResumeQuizFromRows": (5, "resume_quiz_from_rows"),
    "PqaEngine_ResumeQuizBatchFromRows": (6, "resume_quiz_batch_from_rows"),
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


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n_questions", [8, 37, 64, 1000, 1001])
def test_row_owners_agree_with_owner_of(world, n_questions):
    qs = sorted(set(list(range(0, n_questions, max(1, n_questions // 53))) + [0, n_questions - 1] + pdist.shard_bounds(n_questions, world)[:-1]))
    want = [pdist.owner_of(q, n_questions, world) for q in qs]
    assert pdist.row_owners([(q, 1) for q in qs], n_questions, world) == want
    assert pdist.row_owners([interop.AnsweredQuestion(q, 0) for q in qs], n_questions, world) == want
    assert set(want) == set(range(world))          # every rank owns something, and its range starts where the bounds say
    for r in range(world):
        first, limit = pdist.shard_range(n_questions, world, r)
        assert pdist.row_owners([(first, 0), (limit - 1, 0)], n_questions, world) == [r, r]
    for bad in (-1, n_questions):
        with pytest.raises(IndexError):
            pdist.row_owners([(bad, 0)], n_questions, world)


# ---- the collective over gloo, against a fake engine ------------------------------------------------------------------------
LD, Q_TOTAL = 16, 10


class FakeEngine:
    """Holds questions [first, limit) of a 'cube' whose row of (question q, answer k) is 1000 q + 10 k + 1 .. and whose D row
    is 1000 q + 500 ..; records every call; `fail` makes its resume raise."""

    def __init__(self, first, limit, fail=False):
        self.first, self.limit, self.fail = first, limit, fail
        self.calls, self.live, self.next_id, self.seen = [], set(), 0, None

    @staticmethod
    def rows(q, k):
        return torch.arange(LD, dtype=torch.float64) + 1000 * q + 10 * k + 1, torch.arange(LD, dtype=torch.float64) + 1000 * q + 500

    def answer_row_slot_bytes(self):
        return 2 * LD * 8

    def get_option(self, name):
        assert name == "ldT"
        return LD

    def synchronize(self):
        self.calls.append("sync")

    def _view(self, address, n):
        import ctypes

        buf = (ctypes.c_double * (n * 2 * LD)).from_address(address)
        return torch.frombuffer(buf, dtype=torch.float64).view(n, 2 * LD)

    def pack_answer_rows(self, answered, dst, flag=0, flag_value=0):
        self.calls.append(("pack", [(a.i_question, a.i_answer) for a in answered]))
        view = self._view(dst, max(len(answered), 1))
        for i, a in enumerate(answered):
            if self.first <= a.i_question < self.limit:
                view[i, :LD], view[i, LD:] = self.rows(a.i_question, a.i_answer)

    def _take(self):
        self.live.add(self.next_id)
        self.next_id += 1
        return self.next_id - 1

    def resume_quiz_from_rows(self, answered, rows):
        self.calls.append(("resume", len(answered)))
        self.seen = self._view(rows, max(len(answered), 1)).clone()
        if self.fail:
            raise interop.PqaException("[I64Underflow] fake failure")
        return self._take()

    def resume_quiz_batch_from_rows(self, lists, rows):
        self.calls.append(("resume_batch", [len(l) for l in lists]))
        self.seen = self._view(rows, max(sum(len(l) for l in lists), 1)).clone()
        if self.fail:
            raise interop.PqaException("[I64Underflow] fake failure")
        return [self._take() for _ in lists]

    def release_quiz(self, quiz):
        self.calls.append(("release", quiz))
        self.live.remove(quiz)


def _fake_worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    rc.init_group("gloo", rank, world, port)
    cpu = torch.device("cpu")
    first, limit = pdist.shard_range(Q_TOTAL, world, rank)
    answered = [interop.AnsweredQuestion(q, k) for q, k in ((7, 1), (0, 2), (4, 0), (9, 3), (5, 4))]
    want = torch.stack([torch.cat(FakeEngine.rows(a.i_question, a.i_answer)) for a in answered])
    out = {}
    # all succeed: every rank resumes from the same combined package, every slot as its owner has it
    eng = FakeEngine(first, limit)
    out["quiz"] = pdist.resume_quiz(eng, answered, rank, world, device=cpu)
    out["package_ok"] = bool(torch.equal(eng.seen, want))
    out["calls_ok"] = [c if isinstance(c, str) else c[0] for c in eng.calls]
    # the batch: slots count through the lists
    lists = [answered[:2], [], answered[2:]]
    out["quizzes"] = pdist.resume_quiz_batch(eng, lists, rank, world, device=cpu)
    out["batch_package_ok"] = bool(torch.equal(eng.seen, want))
    out["live"] = sorted(eng.live)
    # rank 1 fails: both raise the same text, rank 0 lets its quiz go again
    for name, call in (("single", lambda e: pdist.resume_quiz(e, answered, rank, world, device=cpu)),
                       ("batch", lambda e: pdist.resume_quiz_batch(e, lists, rank, world, device=cpu))):
        bad = FakeEngine(first, limit, fail=(rank == 1))
        try:
            call(bad)
            out[name + "_raised"] = None
        except interop.PqaException as e:
            out[name + "_raised"] = str(e)
        out[name + "_live"] = sorted(bad.live)
        out[name + "_released"] = [c[1] for c in bad.calls if not isinstance(c, str) and c[0] == "release"]
    ret[rank] = out
    dist.destroy_process_group()


def test_two_rank_collective_bookkeeping_over_gloo():
    ret = rc.run_gloo(_fake_worker, 2)
    a, b = ret[0], ret[1]
    for r in (a, b):
        assert r["package_ok"] and r["batch_package_ok"], r
        assert r["calls_ok"] == ["pack", "sync", "resume"], r["calls_ok"]
        assert r["quiz"] == 0 and r["quizzes"] == [1, 2, 3] and r["live"] == [0, 1, 2, 3], r
        for name in ("single", "batch"):
            assert r[name + "_raised"] is not None and "rank 1" in r[name + "_raised"] and "fake failure" in r[name + "_raised"], r
            assert r[name + "_live"] == [], r                    # nothing is left behind on either rank
    assert a["single_raised"] == b["single_raised"] and a["batch_raised"] == b["batch_raised"]
    assert a["single_released"] == [0] and a["batch_released"] == [0, 1, 2]    # the rank that had succeeded released
    assert b["single_released"] == [] and b["batch_released"] == []
