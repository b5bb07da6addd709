"""The N>1 path on CPU: world_size-2 `gloo` processes run probqa_amd.dist (shard bounds, all-gather of the 16-byte
(priority, index) records, global pick, prior broadcast after RecordAnswer).  The local sweep is supplied by the CPU
oracle here (tests may use it as a stand-in selector); on GPUs the same ShardedSelector wraps
PqaHip_EnqueueSelectArgmax and RCCL."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

import ranks_common as rc
from probqa_amd import dist as pdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shard_bounds_follow_calc_split():
    assert pdist.shard_bounds(10, 4) == [3, 6, 8, 10]
    assert pdist.shard_bounds(1000, 8) == [125 * (i + 1) for i in range(8)]
    assert pdist.shard_range(10, 4, 2) == (6, 8)
    assert [pdist.owner_of(q, 10, 4) for q in (0, 2, 3, 7, 9)] == [0, 0, 1, 2, 3]


def test_pick_global_ties_nan_and_empty():
    def rec(rows):
        t = torch.zeros(len(rows), 2, dtype=torch.float64)
        for i, (p, q) in enumerate(rows):
            t[i, 0] = p
            t[i, 1:].view(torch.int64)[0] = q
        return t

    assert pdist.pick_global(rec([(1.0, 5), (3.0, 9), (2.0, 1)])) == (3.0, 9)
    assert pdist.pick_global(rec([(3.0, 9), (3.0, 4)])) == (3.0, 4)           # tie -> lowest index
    assert pdist.pick_global(rec([(float("nan"), 2), (1.0, 7)])) == (1.0, 7)  # NaN never wins
    assert pdist.pick_global(rec([(0.0, -1), (2.0, 3)])) == (2.0, 3)          # shard without eligible questions
    assert pdist.pick_global(rec([(0.0, -1), (0.0, -1)]))[1] == -1


def _worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cases
    import orclib

    rc.init_group("gloo", rank, world, port)
    case = cases.Case("dist", 5, 61, 90, seed=77, qgaps=[4], answers=[])
    A, D, B = case.kb()
    q0, q1 = pdist.shard_range(case.Q, world, rank)
    # this rank's shard of the KB, plus a full oracle as the single-process truth
    shard = orclib.Oracle(case.K, q1 - q0, case.T, case.init)
    shard.set_kb(A[q0:q1], D[q0:q1], B)
    shard.set_question_gaps([q - q0 for q in case.qgaps if q0 <= q < q1])
    full = case.make_oracle()
    shard.start_quiz(16)
    full.start_quiz(16)

    def local_select(out):
        _, pri = shard.eval(8)
        i = shard.select_argmax(pri)
        out[0] = pri[i] if i >= 0 else 0.0
        out[1:].view(torch.int64)[0] = (i + q0) if i >= 0 else -1

    sel = pdist.ShardedSelector(local_select, torch.device("cpu"))
    picks = []
    for _ in range(4):
        pri_g, q = sel.select()
        _, fpri = full.eval(8)
        want = full.select_argmax(fpri)
        assert q == want and pri_g == fpri[want], (rank, q, want)
        picks.append(q)
        # RecordAnswer: the owner updates the prior, everybody receives it (8*ldT-byte broadcast)
        owner = pdist.owner_of(q, case.Q, world)
        ans = q % case.K
        prior = torch.from_numpy(shard.mants)  # shares memory with the shard's quiz
        if rank == owner:
            shard.record_answer(q - q0, ans, 15)
        pdist.broadcast_prior(prior, owner)
        full.record_answer(q, ans, 15)
        assert np.array_equal(shard.priors(), full.priors())
    ret[rank] = picks
    dist.destroy_process_group()


def test_two_rank_sharded_selection_matches_single_process():
    ret = rc.run_gloo(_worker, 2)
    assert ret[0] == ret[1] and len(ret[0]) == 4 and len(set(ret[0])) == 4


def test_pick_when_all_host_half_of_the_shm_exchange():
    """PqaHip_PickWhenAll: the host side of ShmSelector (no GPU involved): waits for every slot's step number, then the
    exact pick.  Writers are threads that publish late and out of order."""
    import ctypes
    import struct
    import threading
    import time

    from probqa_amd import interop

    world, slot = 5, 64
    buf = (ctypes.c_char * (world * slot))()
    base = ctypes.addressof(buf)
    records = [(2.0, 40), (7.5, 12), (float("nan"), 3), (7.5, 9), (0.0, -1)]   # tie on 7.5 -> index 9; NaN and -1 lose

    def publish(r, delay):
        time.sleep(delay)
        struct.pack_into("<dq", buf, r * slot, *records[r])
        struct.pack_into("<Q", buf, r * slot + 16, 17)

    threads = [threading.Thread(target=publish, args=(r, 0.02 * (world - r))) for r in range(world)]
    for t in threads:
        t.start()
    pri, idx = interop.pick_when_all(base, world, slot, 17, 5.0)
    for t in threads:
        t.join()
    assert (pri, idx) == (7.5, 9)
    with pytest.raises(interop.PqaException, match="Timed out"):
        interop.pick_when_all(base, world, slot, 18, 0.05)          # nobody publishes step 18
    struct.pack_into("<dq", buf, 3 * slot, 0.0, -1)
    struct.pack_into("<dq", buf, 1 * slot, 0.0, -1)
    struct.pack_into("<dq", buf, 0 * slot, 0.0, -1)
    assert interop.pick_when_all(base, world, slot, 17, 1.0)[1] == 3   # only the NaN shard is left: it still has a question


def test_pick_batch_ties_nan_and_empty():
    allw = np.zeros((3, 4, 2))
    allw[:, :, 1] = -1
    allw[0, 0], allw[1, 0], allw[2, 0] = (1.0, 5), (3.0, 9), (2.0, 1)            # plain maximum
    allw[0, 1], allw[1, 1] = (3.0, 9), (3.0, 4)                                   # tie -> lowest index
    allw[0, 2], allw[2, 2] = (float("nan"), 2), (1.0, 7)                          # NaN never wins
    assert pdist.pick_batch(allw) == [9, 4, 7, -1]                                # last quiz: no shard has a question


def _batch_worker(rank, world, port, ret):
    """BASELINE configs[4]'s N > 1 path (bench.py run_batched): every rank sweeps ITS shard for all B quizzes, the per-quiz
    winners meet in one all-gather, every rank makes the same picks -- the single-process oracle's argmaxes."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cases
    import orclib

    rc.init_group("gloo", rank, world, port)
    case = cases.Case("distb", 5, 47, 70, seed=78, qgaps=[11], answers=[])
    A, D, B = case.kb()
    q0, q1 = pdist.shard_range(case.Q, world, rank)
    n_quizzes = 6
    histories = [[((7 * i + 3 * j) % case.Q, (i + j) % case.K) for j in range(i % 3)] for i in range(n_quizzes)]
    histories = [[(q, a) for q, a in h if q != 11] for h in histories]
    mine, want = np.zeros((n_quizzes, 2)), []
    for b, hist in enumerate(histories):
        full = case.make_oracle()
        full.start_quiz(16)
        for q, a in hist:
            full.record_answer(q, a, 15)
        _, fpri = full.eval(8)
        want.append(full.select_argmax(fpri))
        shard = orclib.Oracle(case.K, q1 - q0, case.T, case.init)      # the rank's shard with the SAME posterior and asked bits
        shard.set_kb(A[q0:q1], D[q0:q1], B)
        shard.set_question_gaps([q - q0 for q in case.qgaps if q0 <= q < q1])
        shard.start_quiz(16)
        shard.mants[: case.T] = full.priors()
        asked = np.ctypeslib.as_array(shard.quiz.contents.asked, shape=((q1 - q0 + 7) // 8,))
        for q, _ in hist:
            if q0 <= q < q1:
                asked[(q - q0) >> 3] |= 1 << ((q - q0) & 7)
        _, pri = shard.eval(8)
        i = shard.select_argmax(pri)
        mine[b] = (pri[i], i + q0) if i >= 0 else (0.0, -1)
    picks = pdist.select_batch(torch.from_numpy(mine))
    assert picks == want, (rank, picks, want)
    ret[rank] = picks
    dist.destroy_process_group()


def test_two_rank_batched_selection_matches_single_process():
    ret = rc.run_gloo(_batch_worker, 2)
    assert ret[0] == ret[1] and len(ret[0]) == 6


# ---- ShmBatchExchange between two processes (host only: numpy over /dev/shm) -------------------------------------------------------
NAN = float("nan")
# [step][rank] -> the rank's B = 3 records (priority, GLOBAL question or -1); step 3 reuses the half of step 1 with other winners
EXCHANGE_RECORDS = [
    [[(1.0, 5), (NAN, 2), (0.0, -1)], [(3.0, 9), (1.0, 7), (0.0, -1)]],
    [[(2.0, 4), (2.0, 3), (NAN, 1)], [(2.0, 8), (0.0, -1), (0.0, -1)]],
    [[(0.5, 0), (0.0, -1), (7.0, 2)], [(0.25, 6), (4.0, 10), (7.0, 11)]],
]
EXCHANGE_PICKS = [[9, 7, -1], [4, 3, 1], [0, 10, 2]]       # maximum; NaN and -1 lose; a tie goes to the lower question; a lone NaN still wins


def _exchange_worker(rank, name):
    ex = pdist.ShmBatchExchange(3, rank, 2, name, create=False)
    res = {"picks": [ex.exchange(np.array(step[rank]), timeout_s=60.0) for step in EXCHANGE_RECORDS], "timeout": None}
    if rank == 0:                               # a fourth step that rank 1 never takes
        try:
            ex.exchange(np.array(EXCHANGE_RECORDS[0][0]), timeout_s=0.2)
        except TimeoutError as e:
            res["timeout"] = str(e)
    res["step"] = ex.step
    ex.close()
    return res


def test_two_processes_exchange_batches_through_shared_memory():
    assert [pdist.pick_batch(np.array(step)) for step in EXCHANGE_RECORDS] == EXCHANGE_PICKS
    owner = pdist.ShmBatchExchange(3, 0, 2, "test_%d" % os.getpid(), create=True)     # the segment exists, zeroed, before a rank opens it
    try:
        assert owner.path == "/dev/shm/pqa_batch_test_%d" % os.getpid() and os.path.getsize(owner.path) == 2 * 2 * (16 * 3 + 64)
        got = rc.run_ranks(_exchange_worker, 2, (owner.path[len("/dev/shm/pqa_batch_"):],), timeout_s=120)
    finally:
        owner.close()
    assert not os.path.exists(owner.path)       # closing the owner removes the file; the ranks' closes did not
    for r in range(2):
        assert got[r]["picks"] == EXCHANGE_PICKS, (r, got[r])
    assert got[0]["timeout"] == "rank 1 never published step 4" and (got[0]["step"], got[1]["step"]) == (4, 3), got


# ---- list_top_questions_batch over gloo, against a fake engine ----------------------------------------------------------------------
# [rank][quiz]: lists of unequal length, one empty list, and in quiz 2 the same priority on both ranks
TOP_LISTS = [[[(4, 0.9), (1, 0.5), (2, 0.125)], [], [(3, 0.625)]],
             [[(7, 0.75)], [(8, 0.25), (6, 0.125)], [(9, 0.625), (5, 0.5)]]]
TOP_MERGED = [[(4, 0.9), (7, 0.75), (1, 0.5)], [(8, 0.25), (6, 0.125)], [(3, 0.625), (9, 0.625), (5, 0.5)]]


class FakeTopEngine:
    def __init__(self, rank):
        self.lists, self.calls = TOP_LISTS[rank], []

    def list_top_questions_batch(self, quizzes, max_count):
        self.calls.append((list(quizzes), max_count))
        return [self.lists[q][:max_count] for q in quizzes]

    def list_top_questions(self, quiz, max_count):
        return self.list_top_questions_batch([quiz], max_count)[0]


def _top_worker(rank, world, port, ret):
    rc.init_group("gloo", rank, world, port)
    eng = FakeTopEngine(rank)
    out = {"three": pdist.list_top_questions_batch(eng, [0, 1, 2], 3), "two": pdist.list_top_questions_batch(eng, (2, 0), 2),
           "none": pdist.list_top_questions_batch(eng, [0, 1, 2], 0), "single": pdist.list_top_questions(eng, 2, 3), "calls": eng.calls}
    ret[rank] = out
    dist.destroy_process_group()


def test_two_rank_top_questions_over_gloo():
    assert [pdist.merge_top_questions([TOP_LISTS[0][q], TOP_LISTS[1][q]], 3) for q in range(3)] == TOP_MERGED
    ret = rc.run_gloo(_top_worker, 2)
    for r in range(2):
        assert ret[r]["three"] == TOP_MERGED, (r, ret[r])
        assert ret[r]["two"] == [TOP_MERGED[2][:2], TOP_MERGED[0][:2]] and ret[r]["single"] == TOP_MERGED[2], (r, ret[r])
        assert ret[r]["none"] == [[], [], []], (r, ret[r])
        assert ret[r]["calls"] == [([0, 1, 2], 3), ([2, 0], 2), ([0, 1, 2], 0), ([2], 3)], ret[r]["calls"]
