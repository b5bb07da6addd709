"""Cost of ResumeQuiz over separately created shards (a tool, not a test).  One process, the shards side by side on one device,
the legs interleaved rep by rep, medians with min and max, in us per call (a call = the work of ALL shards, one after another):
  a  ResumeQuiz on the whole engine
  b  ResumeQuiz on the one-process sharded engine (PQA_DEVICES) with the same shard count: the yardstick
  c  PackAnswerRows on every shard + ResumeQuizFromRows on every shard, package in device memory
  d  the same with the package in registered host memory, read in place (rows_stage = 0) and staged (rows_stage = 1)
and the same four for one batch of `batch` quizzes (ResumeQuizBatch / ResumeQuizBatchFromRows).  The pack kernel's own time,
between events on the engine's stream, comes beside the bytes it moved.  One JSON line per shard count.
usage: resume_ranks_bench.py Q K T [answers=16] [shards=2,4,8] [batch=64] [reps=7]"""
import ctypes
import json
import mmap
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probqa_amd import dist as pdist
from probqa_amd import interop

Q, K, T = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
M = int(sys.argv[4]) if len(sys.argv) > 4 else 16
SHARDS = [int(x) for x in (sys.argv[5] if len(sys.argv) > 5 else "2,4,8").split(",")]
B = int(sys.argv[6]) if len(sys.argv) > 6 else 64
REPS = int(sys.argv[7]) if len(sys.argv) > 7 else 7
SEED = 20261016

factory = interop.PqaEngineFactory()
rng = np.random.default_rng(7)


def aqs(pairs):
    return [interop.AnsweredQuestion(q, a) for q, a in pairs]


def engine(first, limit):
    e = factory.create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1), first, Q, 0)
    e.fill_synthetic(8.0, 0.5, SEED)
    return e


def stats(us):
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


single = aqs([(int(q), int(rng.integers(K))) for q in rng.choice(Q, M, replace=False)])
lists = [aqs([(int(q), int(rng.integers(K))) for q in rng.choice(Q, M, replace=True)]) for _ in range(B)]
flat = [a for l in lists for a in l]
whole = engine(0, Q)
want = whole.get_priors(whole.resume_quiz(single))

for world in SHARDS:
    shards = [engine(*pdist.shard_range(Q, world, r)) for r in range(world)]
    stream = torch.cuda.Stream()
    for sh in shards:
        sh.set_stream(stream.cuda_stream)
    saved = os.environ.get("PQA_DEVICES")
    os.environ["PQA_DEVICES"] = ",".join(["0"] * world)
    try:
        one, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
        assert err is None, err
    finally:
        if saved is None:
            os.environ.pop("PQA_DEVICES", None)
        else:
            os.environ["PQA_DEVICES"] = saved
    one.fill_synthetic(8.0, 0.5, SEED)
    assert one.get_option("shards") == world
    slot = shards[0].answer_row_slot_bytes()
    n_max = max(len(single), len(flat))
    dev_pkg = torch.zeros(n_max * slot // 8, dtype=torch.float64, device="cuda")
    seg = mmap.mmap(-1, n_max * slot)
    host = ctypes.addressof(ctypes.c_char.from_buffer(seg))
    host_dev = interop.host_register(host, n_max * slot)
    torch.cuda.synchronize()

    def release(e, ids):
        for i in ids:
            e.release_quiz(i)

    def leg_plain(e, batch):
        t0 = time.perf_counter()
        ids = e.resume_quiz_batch(lists) if batch else [e.resume_quiz(single)]
        dt = time.perf_counter() - t0
        release(e, ids)
        return dt

    def leg_rows(address, stage, batch):
        for sh in shards:
            sh.set_option("rows_stage", stage)
        t0 = time.perf_counter()
        for sh in shards:
            sh.pack_answer_rows(flat if batch else single, address)
        for sh in shards:
            sh.synchronize()
        ids = [sh.resume_quiz_batch_from_rows(lists, address) if batch else [sh.resume_quiz_from_rows(single, address)] for sh in shards]
        dt = time.perf_counter() - t0
        for sh, i in zip(shards, ids):
            release(sh, i)
        return dt

    legs = {
        "a_whole": lambda b: leg_plain(whole, b),
        "b_sharded_engine": lambda b: leg_plain(one, b),
        "c_rows_device": lambda b: leg_rows(dev_pkg.data_ptr(), 1, b),
        "d_rows_host_in_place": lambda b: leg_rows(host_dev, 0, b),
        "d_rows_host_staged": lambda b: leg_rows(host_dev, 1, b),
    }
    # what the legs compute is what the whole engine computes
    for address, stage in ((dev_pkg.data_ptr(), 1), (host_dev, 0), (host_dev, 1)):
        for sh in shards:
            sh.set_option("rows_stage", stage)
            sh.pack_answer_rows(single, address)
        for sh in shards:
            sh.synchronize()
        for sh in shards:
            q = sh.resume_quiz_from_rows(single, address)
            assert np.array_equal(sh.get_priors(q), want)
            sh.release_quiz(q)
    q = one.resume_quiz(single)
    assert np.array_equal(one.get_priors(q), want)
    one.release_quiz(q)
    out = {"shape": "%dx%dx%d" % (Q, K, T), "shards": world, "answers": M, "batch": B, "reps": REPS, "slot_bytes": slot}
    for batch in (False, True):
        times = {name: [] for name in legs}
        for rep in range(REPS + 1):          # (the first round warms up: tables grown, buffers pooled)
            for name, fn in legs.items():
                dt = fn(batch)
                if rep > 0:
                    times[name].append(dt * 1e6)
        key = "batch_us" if batch else "single_us"
        out[key] = {name: stats(us) for name, us in times.items()}
        out[key]["c_over_b"] = round(out[key]["c_rows_device"]["median"] / out[key]["b_sharded_engine"]["median"], 2)
    # the pack kernels alone, all shards back to back on the one stream, between events
    for name, what in (("pack_single", single), ("pack_batch", flat)):
        us = []
        for rep in range(REPS + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            for sh in shards:
                sh.pack_answer_rows(what, dev_pkg.data_ptr())
            stop.record(stream)
            stop.synchronize()
            if rep > 0:
                us.append(start.elapsed_time(stop) * 1e3)
        moved = len(what) * slot
        out[name] = {"us": stats(us), "bytes": moved, "GBps": round(2 * moved / (statistics.median(us) * 1e-6) / 1e9, 1)}   # (read + written)
    print(json.dumps(out), flush=True)
    interop.host_unregister(host)
    for e in shards + [one]:
        e.close()
    del dev_pkg
whole.close()
