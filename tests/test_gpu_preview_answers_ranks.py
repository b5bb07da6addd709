"""PqaEngine_PreviewAnswersBatch across separately created shards, called on the shards directly.  One process: the shards of one
synthetic KB sit side by side on the one device as create_hip_engine(def, q_first, Q, 0) engines, one whole engine holds the same KB, and
every engine holds the same quizzes (the shards record through posterior packages, as dist.record_answer_batch does).  Every shard holds
every posterior whole, so a shard answers for the pairs whose question it holds -- the whole engine's bits -- and leaves zeros for the
others; taking each pair from its owner, as dist.preview_answers_batch does, gives the whole engine's result bit for bit."""
import numpy as np
import pytest
import torch

from probqa_amd import dist as pdist
from probqa_amd import interop

pytestmark = pytest.mark.gpu

F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)
CASES = {
    "k5_q37_t101": dict(K=5, Q=37, T=101, tgaps=(3, 17, 100), qgaps=(4, 36)),
    "k3_q40_t1025_float": dict(K=3, Q=40, T=1025, tgaps=(1024,), qgaps=(0,), f32=True),
}
N_QUIZZES, MAX_COUNT = 3, 10


def engine_of(c, first, limit):
    eng = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(c["K"], limit - first, c["T"], init_amount=0.1, **(F32 if c.get("f32") else {})),
                                                       first, c["Q"], 0)
    eng.fill_synthetic(8.0, 0.5, 5)       # (the same seed on every shard: each fills its part of the one cube)
    eng.set_target_gaps(list(c["tgaps"]))
    eng.set_question_gaps(list(c["qgaps"]))   # (global ids: every rank is told of all of them)
    eng.set_option("workers", 16)
    return eng


def key(preview):
    return (np.float64(preview.likelihood).tobytes(), np.float64(preview.entropy).tobytes(), [(t.i_target, t.prob) for t in preview.targets])


def keys(result):
    return [[key(p) for p in previews] for previews in result]


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("case", sorted(CASES))
def test_shards_answer_for_their_own_questions(case, world):
    c = CASES[case]
    K, Q = c["K"], c["Q"]
    bounds = pdist.shard_bounds(Q, world)
    firsts = [0] + bounds[:-1]
    whole = engine_of(c, 0, Q)
    shards = [engine_of(c, f, b) for f, b in zip(firsts, bounds)]
    quizzes = whole.start_quiz_batch(N_QUIZZES)
    for sh in shards:
        assert sh.start_quiz_batch(N_QUIZZES) == quizzes
    for r in range(2):                    # two rounds of answers, the questions crossing the ranks
        questions = [(7 + 11 * i + 13 * r) % Q for i in range(N_QUIZZES)]
        assert not set(questions) & set(c["qgaps"])
        answers = [(i + r) % K for i in range(N_QUIZZES)]
        for e in [whole] + shards:
            for quiz, q in zip(quizzes, questions):
                e.set_active_question(quiz, q)
        whole.record_answer_batch(quizzes, answers)
        pkg = torch.zeros(N_QUIZZES, shards[0].posterior_slot_bytes() // 8, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for sh in shards:
            sh.pack_answer_posteriors(quizzes, answers, pkg.data_ptr())
        for sh in shards:
            sh.synchronize()
        for sh in shards:
            sh.record_answer_batch_from_posteriors(quizzes, answers, pkg.data_ptr())
    asked = (7 + 11 * 0 + 13 * 0) % Q     # quiz 0 has answered it
    pairs = [(quizzes[i % N_QUIZZES], q) for i, q in enumerate(q for q in range(0, Q, 3) if q not in c["qgaps"])] + [(quizzes[0], asked), (quizzes[1], Q - 2), (quizzes[1], Q - 2)]
    want = keys(whole.preview_answers_batch(pairs, MAX_COUNT))
    assert all(len(k[2]) == MAX_COUNT for previews in want for k in previews)
    zero = key(interop.AnswerPreview(0.0, 0.0, []))
    per_rank = []
    for rank, sh in enumerate(shards):
        pairs0 = sh.get_option("preview_pairs")
        mine = keys(sh.preview_answers_batch(pairs, MAX_COUNT))
        held = [pdist.owner_in(bounds, q) == rank for _, q in pairs]
        assert sh.get_option("preview_pairs") == pairs0 + sum(held)
        for i, previews in enumerate(mine):
            assert previews == (want[i] if held[i] else [zero] * K), (case, world, rank, i)      # the whole engine's bits, or zeros
        per_rank.append(mine)
        for quiz in quizzes:              # nothing changed on the shard
            assert sh.get_priors(quiz).tobytes() == whole.get_priors(quiz).tobytes()
    assert [per_rank[pdist.owner_in(bounds, q)][i] for i, (_, q) in enumerate(pairs)] == want       # each pair from the rank that holds its question
    # a question that is a gap is refused by the shard that holds it alone; one that is out of range by every shard
    gap = c["qgaps"][0]
    for rank, sh in enumerate(shards):
        if pdist.owner_in(bounds, gap) == rank:
            with pytest.raises(interop.PqaException, match=r"entry=1 questionId=%d" % gap):
                sh.preview_answers_batch([(quizzes[0], 1), (quizzes[0], gap)], MAX_COUNT)
        else:
            assert keys(sh.preview_answers_batch([(quizzes[0], gap)], MAX_COUNT)) == [[zero] * K]
        with pytest.raises(interop.PqaException, match=r"entry=0 questionId=%d" % Q):
            sh.preview_answers_batch([(quizzes[0], Q)], MAX_COUNT)
    for e in [whole] + shards:
        e.close()
