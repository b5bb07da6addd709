"""Question redundancy across separately created shards (PqaHip_PackQuestionWeights, PqaEngine_EvalQuestionRedundancyFromWeights,
PqaEngine_ListRedundantQuestionsFromWeights).  One process: the shards of one synthetic KB sit side by side on the one device as
create_hip_engine(def, q_first, Q, 0) engines, one whole engine holds the same KB.  Every shard packs the sources it holds into a
zero-filled package of its own; the packages are summed in numpy -- what the all-reduce delivers: one writer per slot -- and every shard
evaluates and lists its own questions from the sum.  The summation over the targets does not depend on the split of the question axis:
the concatenated rows are the whole engine's Eval bit for bit, the merged listings its listing record for record."""
import numpy as np
import pytest
import torch

from probqa_amd import dist as pdist
from probqa_amd import interop
from test_gpu_redundant_questions import F32, listing_of_row

pytestmark = pytest.mark.gpu

TGAPS, QGAPS = (3, 17, 100), (0, 5, 36)
CASES = {
    "two_k5_t101": dict(world=2, K=5, T=101),
    "three_k5_t101": dict(world=3, K=5, T=101),
    "three_k7_t1025": dict(world=3, K=7, T=1025),
    "two_k2_t257_float": dict(world=2, K=2, T=257, f32=True),
    "three_k5_t101_float": dict(world=3, K=5, T=101, f32=True),
}
Q = 37


def engine_of(first, limit, K, T, f32):
    eng = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1, **(F32 if f32 else {})), first, Q, 0)
    eng.fill_synthetic(8.0, 0.5, 5)       # (the same seed on every shard: each fills its part of the one cube)
    eng.set_target_gaps(list(TGAPS))
    eng.set_question_gaps(list(QGAPS))    # (global ids: every rank is told of all of them)
    eng.set_option("workers", 16)
    return eng


@pytest.mark.parametrize("case", sorted(CASES))
def test_shards_pack_sum_evaluate_and_list(case):
    c = CASES[case]
    world, K, T, f32 = c["world"], c["K"], c["T"], c.get("f32", False)
    bounds = pdist.shard_bounds(Q, world)
    firsts = [0] + bounds[:-1]
    # both sides of every shard boundary, both ends, a gap source, a repeated id
    sources = [0, Q - 1, 5, 9, 9, 20] + [b - 1 for b in bounds[:-1]] + [b for b in bounds[:-1]]
    whole = engine_of(0, Q, K, T, f32)
    shards = [engine_of(f, b, K, T, f32) for f, b in zip(firsts, bounds)]
    slot = shards[0].question_weight_slot_bytes() // 8
    assert slot == K * ((T + 15) // 16 * 16) and whole.question_weight_slot_bytes() == slot * 8
    total = np.zeros((len(sources), slot))
    for sh, f, b in zip(shards, firsts, bounds):
        pkg = torch.full((len(sources), slot), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        sh.pack_question_weights(sources, pkg.data_ptr())
        sh.synchronize()
        part = pkg.cpu().numpy()
        for i, s in enumerate(sources):
            if f <= s < b:      # the owner writes the slot whole: zeros behind the rows, at gap targets, and for a gap source
                rows = part[i].reshape(K, slot // K)
                assert (rows >= 0).all() and not rows[:, T:].any() and not rows[:, list(TGAPS)].any() and (s in QGAPS) == (not rows.any())
                total[i] += part[i]
            else:               # not this rank's: untouched
                assert (part[i] == -1.0).all(), (case, i)
    # the whole engine's own package is the sum, bit for bit
    pkg = torch.zeros(len(sources), slot, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    whole.pack_question_weights(sources, pkg.data_ptr())
    whole.synchronize()
    assert pkg.cpu().numpy().tobytes() == total.tobytes()
    want = whole.eval_question_redundancy(sources)
    assert want.any()
    summed = torch.from_numpy(total).cuda()
    torch.cuda.synchronize()
    got = np.concatenate([sh.eval_question_redundancy_from_weights(sources, summed.data_ptr(), b - f) for sh, f, b in zip(shards, firsts, bounds)], axis=1)
    assert got.tobytes() == want.tobytes()                 # shards return the whole engine's bits
    assert whole.eval_question_redundancy_from_weights(sources, summed.data_ptr()).tobytes() == want.tobytes()
    for max_count in (0, 1, 10, 300):
        parts = []
        for sh, f, b in zip(shards, firsts, bounds):
            mine = sh.list_redundant_questions_from_weights(sources, summed.data_ptr(), max_count)
            for i, s in enumerate(sources):
                assert mine[i] == listing_of_row(want[i, f:b], s, max_count, f), (case, max_count, i)
            parts.append(mine)
        merged = [pdist.merge_top_questions([p[i] for p in parts], max_count) for i in range(len(sources))]
        assert merged == whole.list_redundant_questions_batch(sources, max_count), (case, max_count)
        assert merged == whole.list_redundant_questions_from_weights(sources, summed.data_ptr(), max_count)
    for sh in shards:
        for call in (lambda: sh.eval_question_redundancy([1]), lambda: sh.list_redundant_questions_batch([1], 3)):
            with pytest.raises(interop.PqaException, match=r"Not implemented.*PqaHip_PackQuestionWeights.*FromWeights"):
                call()
        with pytest.raises(interop.PqaException, match=r"entry=0 questionId=%d" % Q):   # ids are global: [0, q_total)
            sh.pack_question_weights([Q], 16)
    for e in [whole] + shards:
        e.close()


def test_flag_and_staged_host_package():
    """The pack's flag arrives behind the slots -- also from an engine that holds none of the sources --; a summed package in
    registered host memory is staged under rows_stage."""
    import ctypes
    import mmap

    K, T = 5, 101
    sources = [0, 36, 5, 9, 9, 20]
    whole = engine_of(0, Q, K, T, False)
    last = engine_of(30, Q, K, T, False)
    slot = whole.question_weight_slot_bytes() // 8
    n = len(sources)
    seg = mmap.mmap(-1, ((n * slot + 2) * 8 + 4095) // 4096 * 4096)
    address = ctypes.addressof(ctypes.c_char.from_buffer(seg))
    dev = interop.host_register(address, len(seg))
    try:
        host = np.frombuffer(seg, dtype=np.float64, count=n * slot + 2)
        flag = np.frombuffer(seg, dtype=np.uint64, count=n * slot + 2)
        whole.pack_question_weights(sources, dev, dev + n * slot * 8, 77)
        whole.synchronize()
        assert int(flag[n * slot]) == 77
        kept = host[:n * slot].copy()
        last.pack_question_weights([0, 5, 9], dev, dev + n * slot * 8, 78)      # holds none of them: the flag alone, nothing written
        last.synchronize()
        assert int(flag[n * slot]) == 78 and np.array_equal(host[:n * slot], kept)
        whole.pack_question_weights([], 0, dev + n * slot * 8, 79)
        whole.synchronize()
        assert int(flag[n * slot]) == 79
        want = whole.eval_question_redundancy(sources)
        for stage in (1, 0):
            whole.set_option("rows_stage", stage)
            staged0 = whole.get_option("rows_staged")
            assert whole.eval_question_redundancy_from_weights(sources, dev).tobytes() == want.tobytes()
            got = whole.list_redundant_questions_from_weights(sources, dev, 10)
            assert whole.get_option("rows_staged") - staged0 == 2 * stage
            assert got == whole.list_redundant_questions_batch(sources, 10)
        del host, flag
    finally:
        whole.close()
        last.close()
        interop.host_unregister(address)
