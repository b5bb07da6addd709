"""Per-quiz cost of restoring quizzes (tools, not a test): a loop of single PqaEngine_ResumeQuiz calls, one
PqaEngine_ResumeQuizBatch, and 64 client threads calling PqaEngine_ResumeQuiz with option "combine" on.  On rows beyond 16384
targets also the single call with long_row_form = 0 (the one-workgroup kernel).  Prints one JSON line: per-quiz us, median of
`reps` runs with their min and max.
usage: resume_bench.py Q K T [quizzes=256] [answers=16] [ragged=0] [reps=5]
  ragged = 1: answer counts 0 .. 2 * answers - 1 instead of `answers` each"""
import ctypes
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probqa_amd import interop

Q, K, T = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
N = int(sys.argv[4]) if len(sys.argv) > 4 else 256
M = int(sys.argv[5]) if len(sys.argv) > 5 else 16
ragged = len(sys.argv) > 6 and sys.argv[6] == "1"
reps = int(sys.argv[7]) if len(sys.argv) > 7 else 5
THREADS = 64

f = interop.PqaEngineFactory()
eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
assert err is None, err
eng.fill_synthetic(8.0, 0.5, 20261016)
lib = interop.load_library()
rng = np.random.default_rng(7)
counts = [int(rng.integers(0, 2 * M)) if ragged else M for _ in range(N)]
lists = [[(int(q), int(rng.integers(K))) for q in rng.choice(Q, c, replace=True)] for c in counts]
arrs = []
for l in lists:
    a = (interop.CiAnsweredQuestion * max(len(l), 1))()
    for i, (q, ans) in enumerate(l):
        a[i].iQuestion, a[i].iAnswer = q, ans
    arrs.append(a)
flat = (interop.CiAnsweredQuestion * max(sum(counts), 1))()
j = 0
for l in lists:
    for q, ans in l:
        flat[j].iQuestion, flat[j].iAnswer = q, ans
        j += 1
c_counts = (ctypes.c_int64 * N)(*counts)
c_out = (ctypes.c_int64 * N)()


def release(ids):
    for i in ids:
        eng.release_quiz(i)


def single():
    err = ctypes.c_void_p()
    t0 = time.perf_counter()
    ids = [lib.PqaEngine_ResumeQuiz(eng.c_engine, ctypes.byref(err), len(l), a) for l, a in zip(lists, arrs)]
    dt = time.perf_counter() - t0
    assert err.value is None and min(ids) >= 0
    release(ids)
    return dt


def batch():
    t0 = time.perf_counter()
    interop._check(lib.PqaEngine_ResumeQuizBatch(eng.c_engine, N, c_counts, flat, c_out))
    dt = time.perf_counter() - t0
    release(list(c_out))
    return dt


def combined():
    ids = [None] * N
    barrier = threading.Barrier(THREADS + 1)

    def client(t):
        err = ctypes.c_void_p()
        barrier.wait()
        for i in range(t, N, THREADS):
            ids[i] = lib.PqaEngine_ResumeQuiz(eng.c_engine, ctypes.byref(err), len(lists[i]), arrs[i])
        assert err.value is None

    th = [threading.Thread(target=client, args=(t,)) for t in range(THREADS)]
    for x in th:
        x.start()
    barrier.wait()
    t0 = time.perf_counter()
    for x in th:
        x.join()
    dt = time.perf_counter() - t0
    assert min(ids) >= 0
    release(ids)
    return dt


def measure(fn):
    fn()   # warm-up: tables grown, buffers pooled
    us = [fn() / N * 1e6 for _ in range(reps)]
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


eng.set_option("combine", 1)
out = {"shape": "%dx%dx%d" % (Q, K, T), "quizzes": N, "answers": "ragged 0-%d" % (2 * M - 1) if ragged else M, "reps": reps}
out["single_us"] = measure(single)
out["batch_us"] = measure(batch)
b0, r0 = eng.get_option("resume_batches"), eng.get_option("resumes_batched")
out["combined64_us"] = measure(combined)
out["combined_posted"] = eng.get_option("resumes_batched") - r0
out["combined_batches"] = eng.get_option("resume_batches") - b0
if T > 16384:
    eng.set_option("long_row_form", 0)
    out["single_one_workgroup_us"] = measure(single)
    eng.set_option("long_row_form", 1)
out["batch_speedup"] = round(out["single_us"]["median"] / out["batch_us"]["median"], 2)
if T > 16384:
    out["long_row_speedup"] = round(out["single_one_workgroup_us"]["median"] / out["single_us"]["median"], 2)
print(json.dumps(out))
eng.close()
