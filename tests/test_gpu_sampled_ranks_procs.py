"""dist.next_question_sampled_batch / dist.next_question_sampled over shards in separate processes: two spawned ranks with a gloo group
share the one GPU of the test box, each holding half of the questions; both must return the same questions, equal to the whole
engine's in the parent for the guarded draws (tests/test_sampled_ranks_abi.py checks the draws without a GPU).  Every wait is
bounded: the collectives time out, and the parent takes the results with a time limit."""
import multiprocessing as mp
import os
import queue
import socket

import pytest

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


def _rank_main(rank, port, rnd_lists, out):
    try:
        import datetime

        import torch
        import torch.distributed as dist

        from probqa_amd import dist as pdist

        case, option = config()
        first, limit = pdist.shard_range(case.Q, WORLD, rank)
        eng = engine_of(case, option, first, limit)
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=120))
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
        out.put((rank, res))
    except Exception as e:  # noqa: BLE001 - reported to the parent
        out.put((rank, repr(e)))


def test_two_processes_select_over_gloo(factory):
    case, option = config()
    n_sub = sr.n_sub_of(option)
    _, draws, _ = sr.guarded_draws(case, n_sub)
    rnd_lists = [[r] * 3 for r in sb.EDGE_RNDS] + [[draws[0]] * 3]     # (every quiz is at step 0: the draw guarded for that step)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, port, rnd_lists, out)) for r in range(WORLD)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(300):                                       # (a rank that dies ends the wait at once, not a hang)
            try:
                rank, res = out.get(timeout=1)
                got[rank] = res
            except queue.Empty:
                if any(not p.is_alive() for p in procs) and out.empty():
                    break
            if len(got) == WORLD:
                break
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r in range(WORLD):   # (both ranks reported, before anything more is started on the device)
        assert isinstance(got.get(r), dict), got.get(r)
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
