"""What the tests over several ranks share: a free port, the process group of a child, the runner of spawned GPU ranks and the
runner of the no-GPU gloo fakes.  Every wait is bounded: the collectives time out, and the parent takes the results with a time
limit."""
import datetime
import multiprocessing
import os
import queue
import socket

MAX_WORLD = 8    # at most 16 processes have the GPU open at a time, the parent included: half of that for the ranks of one test


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def init_group(backend, rank, world, port, **kw):
    """In a child: the process group of `world` ranks on this host, its collectives timing out after 120 s."""
    import torch.distributed as dist

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    kw.setdefault("timeout", datetime.timedelta(seconds=120))
    dist.init_process_group(backend, rank=rank, world_size=world, **kw)


def _rank_child(target, rank, args, out):
    try:
        out.put((rank, target(rank, *args)))
    except Exception as e:  # noqa: BLE001 - reported to the parent
        out.put((rank, repr(e)))


def run_ranks(target, world, args=(), timeout_s=300):
    """target(rank, *args) -> a dict, in `world` spawned processes; -> {rank: dict}.  A rank that dies ends the wait at once, not a
    hang; and every rank has reported a dict before this returns, so that a test starts nothing more on the device after a rank failed."""
    assert 1 <= world <= MAX_WORLD, world
    ctx = multiprocessing.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_rank_child, args=(target, r, tuple(args), out)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(int(timeout_s)):
            try:
                rank, res = out.get(timeout=1)
                got[rank] = res
            except queue.Empty:
                if any(not p.is_alive() and r not in got for r, p in enumerate(procs)) and out.empty():
                    break
            if len(got) == world:
                break
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r in range(world):
        assert isinstance(got.get(r), dict), (r, got.get(r), [p.exitcode for p in procs])
    return got


def run_gloo(worker, world, *args):
    """worker(rank, world, port, *args, ret) in `world` processes that mp.spawn starts and joins (the no-GPU gloo fakes; a worker that
    fails raises here); -> {rank: what the worker put into ret[rank]}."""
    import torch.multiprocessing as tmp

    ret = tmp.Manager().dict()
    tmp.spawn(worker, args=(world, free_port()) + args + (ret,), nprocs=world, join=True)
    return dict(ret)
