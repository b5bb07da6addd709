"""Target separation across separately created shards (PqaEngine_EvalTargetSeparation, PqaEngine_ListSeparatingQuestionsBatch called on the
shards directly).  One process: the shards of one synthetic KB sit side by side on the one device as create_hip_engine(def, q_first, Q, 0)
engines, one whole engine holds the same KB.  A value needs the group's columns of one question's block and nothing else, so there is no
package: every shard evaluates and lists its own questions.  The concatenated rows are the whole engine's Eval bit for bit, the merged
listings its listing record for record -- also where a shard holds a single question."""
import ctypes

import numpy as np
import pytest

from probqa_amd import dist as pdist
from probqa_amd import interop
from test_gpu_separating_questions import F32, listing_of_row

pytestmark = pytest.mark.gpu

TGAPS, QGAPS = (3, 17, 100), (0, 5, 36)
Q = 37
CASES = {
    "two_k5_t101": dict(bounds=pdist.shard_bounds(Q, 2), K=5, T=101),
    "three_k5_t101": dict(bounds=pdist.shard_bounds(Q, 3), K=5, T=101),
    "three_k7_t257_one_question": dict(bounds=[18, 19, Q], K=7, T=257),          # the middle shard holds question 18 alone
    "two_k2_t257_float": dict(bounds=pdist.shard_bounds(Q, 2), K=2, T=257, f32=True),
    "three_k5_t101_float_one_question": dict(bounds=[1, 20, Q], K=5, T=101, f32=True),   # the first shard holds question 0 alone, a gap
}


def engine_of(first, limit, K, T, f32):
    eng = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1, **(F32 if f32 else {})), first, Q, 0)
    eng.fill_synthetic(8.0, 0.5, 5)       # (the same seed on every shard: each fills its part of the one cube)
    eng.set_target_gaps(list(TGAPS))
    eng.set_question_gaps(list(QGAPS))    # (global ids: every rank is told of all of them)
    eng.set_option("workers", 16)
    return eng


@pytest.mark.parametrize("case", sorted(CASES))
def test_shards_evaluate_and_list_their_own_questions(case):
    c = CASES[case]
    bounds, K, T, f32 = c["bounds"], c["K"], c["T"], c.get("f32", False)
    firsts = [0] + bounds[:-1]
    rng = np.random.default_rng(13)
    free = [t for t in range(T) if t not in TGAPS]
    groups = [[int(t) for t in rng.choice(free, size=n)] for n in (2, 3, 17, 64, 2, 2, 5)] + [[1, 3, 2], [4, 4, 6]]   # a gap member; a member twice
    whole = engine_of(0, Q, K, T, f32)
    shards = [engine_of(f, b, K, T, f32) for f, b in zip(firsts, bounds)]
    want = whole.eval_target_separation(groups)
    assert want.shape == (len(groups), Q) and want.any() and not want[7].any() and not want[:, list(QGAPS)].any()
    parts = [sh.eval_target_separation(groups) for sh in shards]
    assert [p.shape for p in parts] == [(len(groups), b - f) for f, b in zip(firsts, bounds)]
    assert np.concatenate(parts, axis=1).tobytes() == want.tobytes()            # invariant (b): shards return the whole engine's bits
    for max_count in (0, 1, 10, 300):
        lists = []
        for sh, f, b in zip(shards, firsts, bounds):
            mine = sh.list_separating_questions_batch(groups, max_count)
            for i in range(len(groups)):
                assert mine[i] == listing_of_row(want[i, f:b], max_count, f), (case, max_count, i)      # GLOBAL ids
            lists.append(mine)
        merged = [pdist.merge_top_questions([p[i] for p in lists], max_count) for i in range(len(groups))]
        assert merged == whole.list_separating_questions_batch(groups, max_count), (case, max_count)
    for sh, f, b in zip(shards, firsts, bounds):
        with pytest.raises(interop.PqaException, match=r"subjIndex=%d" % Q):      # the row length is the LOCAL question count
            out = np.zeros((1, Q))
            cnt, tg = np.array([2], dtype=np.int64), np.array([1, 2], dtype=np.int64)
            p64 = ctypes.POINTER(ctypes.c_int64)
            interop._check(interop.load_library().PqaEngine_EvalTargetSeparation(sh.c_engine, 1, cnt.ctypes.data_as(p64), tg.ctypes.data_as(p64),
                                                                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), Q))
        with pytest.raises(interop.PqaException, match=r"entry=0 member=1 targetId=%d" % T):
            sh.eval_target_separation([[1, T]])
    for e in [whole] + shards:
        e.close()
