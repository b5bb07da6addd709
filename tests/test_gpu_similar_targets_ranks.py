"""Target similarity across separately created shards (PqaHip_PackTargetSimilaritySums, PqaEngine_ListSimilarTargetsFromSums).  One
process: the shards of one synthetic KB sit side by side on the one device as create_hip_engine(def, q_first, Q, 0) engines, one whole
engine holds the same KB.  Every shard packs into a zero-filled package of its own; the packages are summed in numpy -- what the
all-reduce delivers -- and must be within the bar (test_gpu_similar_targets.py) of the whole engine's Eval x nValidQuestions; every
shard then lists from the summed package record for record what numpy lists from (summed package / nValidQuestions)."""
import numpy as np
import pytest
import torch

from probqa_amd import dist as pdist
from probqa_amd import interop
from test_gpu_similar_targets import bar, listing_of_row, model_rows, records, valid_top_k

pytestmark = pytest.mark.gpu

K, Q, T, TGAPS = 5, 37, 101, (3, 17, 100)
SOURCES = [0, 100, 3, 9, 9, 55, 64, 31]
CASES = {"two": (2, (0, 5, 36)), "three": (3, (0, 5, 36)), "eight": (8, (0, 5, 36)), "a_shard_all_gaps": (3, tuple(range(13, 25)))}


def engine_of(first, limit, qgaps):
    eng = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1), first, Q, 0)
    eng.fill_synthetic(8.0, 0.5, 5)       # (the same seed on every shard: each fills its part of the one cube)
    eng.set_target_gaps(list(TGAPS))
    eng.set_question_gaps(list(qgaps))    # (global ids: every rank is told of all of them)
    eng.set_option("workers", 16)
    return eng


@pytest.mark.parametrize("case", sorted(CASES))
def test_shards_pack_sum_and_list(case):
    world, qgaps = CASES[case]
    bounds = pdist.shard_bounds(Q, world)
    firsts = [0] + bounds[:-1]
    if case == "a_shard_all_gaps":
        assert (firsts[1], bounds[1]) == (13, 25)
    whole = engine_of(0, Q, qgaps)
    shards = [engine_of(f, b, qgaps) for f, b in zip(firsts, bounds)]
    n_valid = Q - len(qgaps)
    pitch = shards[0].posterior_slot_bytes() // 8
    assert pitch == 112
    total = np.zeros((len(SOURCES), pitch))
    for sh in shards:
        pkg = torch.full((len(SOURCES), pitch), -1.0, dtype=torch.float64, device="cuda")   # (every slot is written whole)
        torch.cuda.synchronize()
        sh.pack_target_similarity_sums(SOURCES, pkg.data_ptr())
        sh.synchronize()
        part = pkg.cpu().numpy()
        assert (part >= 0).all() and not part[:, T:].any() and not part[:, list(TGAPS)].any() and not part[2].any()
        total += part
    want = whole.eval_target_similarity(SOURCES)
    b = bar(Q, K)
    assert (np.abs(total[:, :T] - want * n_valid) <= b * want * n_valid).all()
    A, D, _ = whole.get_kb()
    ref = model_rows(A, D, SOURCES, TGAPS, qgaps)
    summed = torch.from_numpy(total).cuda()
    torch.cuda.synchronize()
    rows = total[:, :T] / n_valid
    for max_count in (0, 1, 10, 300):
        for sh in shards:
            got = sh.list_similar_targets_from_sums(SOURCES, summed.data_ptr(), max_count)
            for i, s in enumerate(SOURCES):
                assert records(got[i]) == listing_of_row(rows[i], s, max_count), (case, max_count, i)
                valid_top_k((case, max_count, i), records(got[i]), ref[i], s, TGAPS, max_count, Q, K)
    # a whole engine is a world of one: its own package, its own listing
    pkg = torch.zeros(len(SOURCES), pitch, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    whole.pack_target_similarity_sums(SOURCES, pkg.data_ptr())
    whole.synchronize()
    assert [records(x) for x in whole.list_similar_targets_from_sums(SOURCES, pkg.data_ptr(), 10)] == [records(x) for x in whole.list_similar_targets_batch(SOURCES, 10)]
    for sh in shards:
        for call in (lambda: sh.eval_target_similarity([1]), lambda: sh.list_similar_targets_batch([1], 3)):
            with pytest.raises(interop.PqaException, match=r"Not implemented.*PqaHip_PackTargetSimilaritySums"):
                call()
    for e in [whole] + shards:
        e.close()


def test_flag_and_staged_host_package():
    """The pack's flag arrives behind the slots; a summed package in registered host memory is staged under rows_stage."""
    import ctypes
    import mmap

    qgaps = (0, 5, 36)
    whole = engine_of(0, Q, qgaps)
    pitch = whole.posterior_slot_bytes() // 8
    n = len(SOURCES)
    bytes_ = (n * pitch + 2) * 8
    seg = mmap.mmap(-1, (bytes_ + 4095) // 4096 * 4096)
    address = ctypes.addressof(ctypes.c_char.from_buffer(seg))
    dev = interop.host_register(address, len(seg))
    try:
        host = np.frombuffer(seg, dtype=np.float64, count=n * pitch + 2)
        flag = np.frombuffer(seg, dtype=np.uint64, count=n * pitch + 2)
        whole.pack_target_similarity_sums(SOURCES, dev, dev + n * pitch * 8, 77)
        whole.synchronize()
        assert int(flag[n * pitch]) == 77
        want = whole.eval_target_similarity(SOURCES)
        n_valid = Q - len(qgaps)
        assert np.array_equal(host[:n * pitch].reshape(n, pitch)[:, :T] / n_valid, want)
        whole.pack_target_similarity_sums([], 0, dev + n * pitch * 8, 78)      # a flag alone
        whole.synchronize()
        assert int(flag[n * pitch]) == 78
        for stage in (1, 0):
            whole.set_option("rows_stage", stage)
            staged0 = whole.get_option("rows_staged")
            got = whole.list_similar_targets_from_sums(SOURCES, dev, 10)
            assert whole.get_option("rows_staged") - staged0 == stage
            assert [records(x) for x in got] == [records(x) for x in whole.list_similar_targets_batch(SOURCES, 10)]
        del host, flag
    finally:
        whole.close()
        interop.host_unregister(address)
