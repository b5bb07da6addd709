"""No-GPU checks of RecordAnswer for many quizzes across process-per-GPU shards: the three exports are declared in
include/PqaHipExt.h, bound in probqa_amd/interop.py and exported by the built libPqaCore.so; and dist.record_answer_batch's
bookkeeping (pack, all-reduce, status word, consume, status word; nobody consumes after a refused pack) runs over gloo on the CPU,
at 2 and 3 ranks, against a fake engine that records what it is asked to do."""
import ctypes
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
    "PqaHip_PosteriorSlotBytes": (1, "posterior_slot_bytes"),
    "PqaHip_PackAnswerPosteriors": (7, "pack_answer_posteriors"),
    "PqaEngine_RecordAnswerBatchFromPosteriors": (5, "record_answer_batch_from_posteriors"),
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


def test_dist_has_the_collective():
    assert callable(pdist.record_answer_batch) and callable(pdist.record_answer)


# ---- the collective over gloo, against a fake engine ------------------------------------------------------------------------
T, PITCH, Q_TOTAL = 13, 16, 10
ACTIVE = {0: 7, 1: 0, 2: 4, 3: 9, 4: 5}      # quiz -> its active question: they cross the ranks at 2 and at 3 ranks


def posterior(quiz, answer):
    v = torch.zeros(PITCH, dtype=torch.float64)
    v[:T] = torch.arange(T, dtype=torch.float64) + 1000 * quiz + 10 * answer + 1
    return v


class FakeEngine:
    """Holds questions [first, limit); the posterior of (quiz, answer) is posterior(quiz, answer); records every call, the
    collectives' all-reduces among them (`log`); fail_pack / fail_consume make that step raise."""

    def __init__(self, first, limit, log, fail_pack=False, fail_consume=False):
        self.first, self.limit, self.calls = first, limit, log
        self.fail_pack, self.fail_consume, self.seen, self.packed = fail_pack, fail_consume, None, None

    def posterior_slot_bytes(self):
        return PITCH * 8

    def synchronize(self):
        self.calls.append("sync")

    @staticmethod
    def _view(address, n):
        buf = (ctypes.c_double * (n * PITCH)).from_address(address)
        return torch.frombuffer(buf, dtype=torch.float64).view(n, PITCH)

    def pack_answer_posteriors(self, quizzes, answers, dst, flag=0, flag_value=0):
        self.calls.append("pack")
        if self.fail_pack:
            raise interop.PqaException("[NoQuizActiveQuestion] Batch entry 1: fake refusal")
        view = self._view(dst, max(len(quizzes), 1))
        assert not view.any()                       # the package arrives zero-filled
        for i, (q, a) in enumerate(zip(quizzes, answers)):
            if self.first <= ACTIVE[q] < self.limit:
                view[i] = posterior(q, a)
        self.packed = (list(quizzes), list(answers))

    def record_answer_batch_from_posteriors(self, quizzes, answers, posteriors):
        self.calls.append("consume")
        assert self.packed == (list(quizzes), list(answers))
        self.seen = self._view(posteriors, max(len(quizzes), 1)).clone()
        if self.fail_consume:
            raise interop.PqaException("[WrongMode] fake consume failure")


def _fake_worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    rc.init_group("gloo", rank, world, port)
    cpu = torch.device("cpu")
    first, limit = pdist.shard_range(Q_TOTAL, world, rank)
    log = []
    real_all_reduce = dist.all_reduce

    def logged_all_reduce(t, op=dist.ReduceOp.SUM, **kw):
        log.append("sum" if op == dist.ReduceOp.SUM else "min")
        return real_all_reduce(t, op=op, **kw)

    dist.all_reduce = logged_all_reduce
    quizzes, answers = sorted(ACTIVE), [2, 0, 1, 3, 4]
    want = torch.stack([posterior(q, a) for q, a in zip(quizzes, answers)])
    out = {}
    # all succeed: the order of the steps, and every slot as its owner has it
    eng = FakeEngine(first, limit, log)
    pdist.record_answer_batch(eng, quizzes, answers, rank, world, device=cpu)
    out["order"] = list(log)
    out["package_ok"] = bool(torch.equal(eng.seen, want))
    out["owners"] = sorted({pdist.owner_of(ACTIVE[q], Q_TOTAL, world) for q in quizzes})
    # the batch of one, and the empty batch
    del log[:]
    pdist.record_answer(eng, 3, 1, rank, world, device=cpu)
    out["single_ok"] = bool(torch.equal(eng.seen, posterior(3, 1).unsqueeze(0)))
    pdist.record_answer_batch(eng, [], [], rank, world, device=cpu)
    out["empty_order"] = log[6:]
    # a refused pack on rank 1: it still enters the all-reduce, nobody consumes, everybody raises its text
    for name, kw in (("pack", {"fail_pack": rank == 1}), ("consume", {"fail_consume": rank == world - 1})):
        del log[:]
        bad = FakeEngine(first, limit, log, **kw)
        try:
            pdist.record_answer_batch(bad, quizzes, answers, rank, world, device=cpu)
            out[name + "_raised"] = None
        except interop.PqaException as e:
            out[name + "_raised"] = str(e)
        out[name + "_order"] = list(log)
    ret[rank] = out
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_collective_bookkeeping_over_gloo(world):
    ret = rc.run_gloo(_fake_worker, world)
    steps = ["pack", "sync", "sum", "min", "consume", "min"]
    for r in range(world):
        got = ret[r]
        assert got["order"] == steps, (r, got["order"])
        assert got["package_ok"] and got["single_ok"], (r, got)
        assert got["owners"] == list(range(world)), got["owners"]       # the batch's questions lie on every rank
        assert got["empty_order"] == steps, (r, got["empty_order"])
        # the refused pack: the step sequence stops behind the first status word on EVERY rank, the failing one included
        assert got["pack_order"] == steps[:4], (r, got["pack_order"])
        assert got["pack_raised"] is not None and "rank 1" in got["pack_raised"] and "fake refusal" in got["pack_raised"], got
        assert got["pack_raised"] == ret[0]["pack_raised"]
        assert got["consume_order"] == steps, (r, got["consume_order"])
        assert got["consume_raised"] is not None and "rank %d" % (world - 1) in got["consume_raised"] and "fake consume failure" in got["consume_raised"], got
        assert got["consume_raised"] == ret[0]["consume_raised"]
