"""dist.next_question_sampled_batch / dist.next_question_sampled over shards in separate processes: two spawned ranks with a gloo group
share the one GPU of the test box, each holding half of the questions; both must return the same questions, equal to the whole
engine's in the parent for the guarded draws (tests/test_sampled_ranks_abi.py checks the draws without a GPU).  Every wait is
bounded: the collectives time out, and the parent takes the results with a time limit."""
import pytest

import ranks_common as rc
import sampled_batch_common as sb
import sampled_ranks_common as sr

pytestmark = pytest.mark.gpu

WORLD, CONFIG = 2, "gaps37_sub5"


def config():
    _, case, option, _ = next(c for c in sr.gpu_configs() if c[0] == CONFIG)
    return case, option


def engine_of(case, option, first, limit):
    from probqa_amd import interop

    A, D, B = case.kb()
    eng = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(case.K, limit - first, case.T, init_amount=case.init), first, case.Q, 0)
    eng.set_kb(A[first:limit], D[first:limit], B)
    eng.set_option("workers", 16)
    eng.set_option("eval_subtasks", option)
    eng.set_target_gaps(case.tgaps)
    eng.set_question_gaps(case.qgaps)
    return eng


def _rank_main(rank, port, rnd_lists):
    import torch
    import torch.distributed as dist

    from probqa_amd import dist as pdist

    case, option = config()
    first, limit = pdist.shard_range(case.Q, WORLD, rank)
    eng = engine_of(case, option, first, limit)
    torch.cuda.set_device(0)
    rc.init_group("gloo", rank, WORLD, port)
    quizzes = eng.start_quiz_batch(3)            # (fresh quizzes: an answer would need the posterior's broadcast, which other tests cover)
    res = {"batch": [], "rnds": []}
    for rnds in rnd_lists:
        mine = pdist.broadcast_rnds(rnds if rank == 0 else [0] * len(rnds))       # rank 0's numbers win
        res["rnds"].append(mine)
        res["batch"].append(pdist.next_question_sampled_batch(eng, quizzes, mine, rank, WORLD))
        res["active"] = [eng.get_active_question_id(q) for q in quizzes]
    res["single"] = pdist.next_question_sampled(eng, quizzes[1], rnd_lists[-1][1], rank, WORLD)
    res["asked"] = eng.get_total_questions_asked()
    dist.destroy_process_group()
    eng.close()
    return res


def test_two_processes_select_over_gloo(factory):
    case, option = config()
    n_sub = sr.n_sub_of(option)
    _, draws, _ = sr.guarded_draws(case, n_sub)
    rnd_lists = [[r] * 3 for r in sb.EDGE_RNDS] + [[draws[0]] * 3]     # (every quiz is at step 0: the draw guarded for that step)
    got = rc.run_ranks(_rank_main, WORLD, (rc.free_port(), rnd_lists))   # (both ranks have reported before anything more is started on the device)
    whole = engine_of(case, option, 0, case.Q)
    quizzes = whole.start_quiz_batch(3)
    want = [whole.next_question_sampled_batch(quizzes, rnds) for rnds in rnd_lists]
    single = whole.next_question_sampled(quizzes[1], rnd_lists[-1][1])
    for r in range(WORLD):
        assert got[r]["rnds"] == rnd_lists, r
        assert got[r]["batch"] == want, (r, got[r]["batch"], want)
        assert got[r]["active"] == want[-1] and got[r]["single"] == single, r
        assert got[r]["asked"] == whole.get_total_questions_asked() == 3 * len(rnd_lists) + 1, r
    whole.close()
