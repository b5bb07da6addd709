"""Question gains across separately created shards (PqaEngine_EvalQuestionGainsBatch, PqaEngine_ListInformativeQuestionsBatch called on the
shards directly).  One process: the shards of one synthetic KB sit side by side on the one device as create_hip_engine(def, q_first, Q, 0)
engines, one whole engine holds the same KB, and every engine holds the same quizzes (the shards record through posterior packages, as
dist.record_answer_batch does).  A value needs the quiz's posterior, which every shard holds whole, and one question's block: there is no
package, every shard evaluates and lists its own questions.  The concatenated rows are the whole engine's Eval bit for bit, the merged
listings its listing record for record -- also where a shard holds a single question, or only a gap."""
import ctypes

import numpy as np
import pytest
import torch

from probqa_amd import dist as pdist
from probqa_amd import interop
from test_gpu_question_gains import F32, listing_of_row

pytestmark = pytest.mark.gpu

TGAPS, QGAPS = (3, 17, 100), (0, 5, 36)
Q = 37
N_QUIZZES = 4
CASES = {
    "two_k5_t101": dict(bounds=pdist.shard_bounds(Q, 2), K=5, T=101),
    "three_k5_t101": dict(bounds=pdist.shard_bounds(Q, 3), K=5, T=101),
    "three_k7_t257_one_question": dict(bounds=[18, 19, Q], K=7, T=257),          # the middle shard holds question 18 alone
    "two_k2_t257_float": dict(bounds=pdist.shard_bounds(Q, 2), K=2, T=257, f32=True),
    "three_k5_t101_one_gap_question": dict(bounds=[1, 20, Q], K=5, T=101),       # the first shard holds question 0 alone, a gap
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
    whole = engine_of(0, Q, K, T, f32)
    shards = [engine_of(f, b, K, T, f32) for f, b in zip(firsts, bounds)]
    quizzes = whole.start_quiz_batch(N_QUIZZES)
    for sh in shards:
        assert sh.start_quiz_batch(N_QUIZZES) == quizzes
    asked = [set() for _ in quizzes]
    for r in range(3):                    # quiz i takes i of three rounds of answers (quiz 0 stays fresh), the questions crossing the ranks
        part = [i for i in range(N_QUIZZES) if i > r]
        ids = [quizzes[i] for i in part]
        questions = [(8 + 11 * i + 13 * r) % Q for i in part]
        assert not set(questions) & set(QGAPS)
        answers = [(i + r) % K for i in part]
        for i, q in zip(part, questions):
            asked[i].add(q)
        for e in [whole] + shards:
            for quiz, q in zip(ids, questions):
                e.set_active_question(quiz, q)
        whole.record_answer_batch(ids, answers)
        pkg = torch.zeros(len(ids), shards[0].posterior_slot_bytes() // 8, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for sh in shards:
            sh.pack_answer_posteriors(ids, answers, pkg.data_ptr())
        for sh in shards:
            sh.synchronize()
        for sh in shards:
            sh.record_answer_batch_from_posteriors(ids, answers, pkg.data_ptr())
    for sh in shards:
        for quiz in quizzes:
            assert sh.get_priors(quiz).tobytes() == whole.get_priors(quiz).tobytes()
    batch = quizzes + [quizzes[2]]
    asked.append(asked[2])
    want = whole.eval_question_gains_batch(batch)
    assert want.shape == (len(batch), Q) and (want > 1e-6).sum() >= len(batch) * (Q - len(QGAPS)) // 2 and not want[:, list(QGAPS)].any()
    parts = [sh.eval_question_gains_batch(batch) for sh in shards]
    assert [p.shape for p in parts] == [(len(batch), b - f) for f, b in zip(firsts, bounds)]
    assert np.concatenate(parts, axis=1).tobytes() == want.tobytes()            # shards return the whole engine's bits
    for max_count in (0, 1, 10, 300):
        lists = []
        for sh, f, b in zip(shards, firsts, bounds):
            mine = sh.list_informative_questions_batch(batch, max_count)
            for i in range(len(batch)):
                assert mine[i] == listing_of_row(want[i, f:b], max_count, asked[i], f), (case, max_count, i)      # GLOBAL ids, the quiz's asked bits
            lists.append(mine)
        merged = [pdist.merge_top_questions([p[i] for p in lists], max_count) for i in range(len(batch))]
        assert merged == whole.list_informative_questions_batch(batch, max_count), (case, max_count)
        assert merged == [listing_of_row(want[i], max_count, asked[i]) for i in range(len(batch))]
    for sh, f, b in zip(shards, firsts, bounds):
        with pytest.raises(interop.PqaException, match=r"subjIndex=%d" % Q):      # the row length is the LOCAL question count
            out = np.zeros((1, Q))
            qs = np.array([quizzes[0]], dtype=np.int64)
            interop._check(interop.load_library().PqaEngine_EvalQuestionGainsBatch(sh.c_engine, 1, qs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), Q))
        with pytest.raises(interop.PqaException, match=r"entry=1 quizId=12345"):
            sh.eval_question_gains_batch([quizzes[0], 12345])
        for quiz in quizzes:              # nothing changed on the shard
            assert sh.get_priors(quiz).tobytes() == whole.get_priors(quiz).tobytes()
    for e in [whole] + shards:
        e.close()
