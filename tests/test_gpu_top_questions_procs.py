"""dist.list_top_questions / dist.list_top_questions_batch over shards in separate processes: two spawned ranks with a gloo group
share the one GPU of the test box, each holding half of the questions; both must return the same lists, equal to the whole engine's
in the parent.  Every wait is bounded: the collectives time out, and the parent takes the results with a time limit."""
import multiprocessing as mp
import os
import queue
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, Q, T, SEED, WORLD = 5, 2300, 40, 31, 2
COUNTS = (1, 10, 256)


def _rank_main(rank, port, out):
    from probqa_amd import dist as pdist
    from probqa_amd import interop

    try:
        import datetime

        import torch
        import torch.distributed as dist

        first, limit = pdist.shard_range(Q, WORLD, rank)
        eng = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1), first, Q, 0)
        eng.fill_synthetic(8.0, 0.5, SEED)
        eng.set_option("workers", 16)
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=120))
        quizzes = eng.start_quiz_batch(3)
        res = {"single": [pdist.list_top_questions(eng, quizzes[0], n) for n in COUNTS],
               "batch": [pdist.list_top_questions_batch(eng, quizzes, n) for n in COUNTS]}
        dist.destroy_process_group()
        eng.close()
        out.put((rank, res))
    except Exception as e:  # noqa: BLE001 - reported to the parent
        out.put((rank, repr(e)))


def test_two_processes_list_over_gloo(factory):
    from probqa_amd import interop

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, port, out)) for r in range(WORLD)]
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
    whole = factory.create_hip_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1), 0, Q, 0)
    whole.fill_synthetic(8.0, 0.5, SEED)
    whole.set_option("workers", 16)
    quizzes = whole.start_quiz_batch(3)
    bits = lambda lst: [(q, np.float64(p).view(np.int64)) for q, p in lst]   # noqa: E731
    for r in range(WORLD):
        for k, n in enumerate(COUNTS):
            assert bits(got[r]["single"][k]) == bits(whole.list_top_questions(quizzes[0], n)), (r, n)
            want = whole.list_top_questions_batch(quizzes, n)
            assert [bits(l) for l in got[r]["batch"][k]] == [bits(l) for l in want], (r, n)
    whole.close()
