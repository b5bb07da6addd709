"""Records per second of training (tools, not a test): consecutive PqaEngine_Train calls from Python (raw ctypes, one call per
record), one PqaEngine_TrainBatch over numpy arrays (train_batch_arrays), and RecordQuizTarget of 256 finished quizzes --
consecutive calls and one PqaEngine_RecordQuizTargetBatch.  Shapes 1000x5x1000 and 10000x5x10000; 1e5 records of 8-24 answers
over random targets, and a skewed set in which 10 % of the records share one target.  For the batch, the engine's own split:
host preparation and launching ("train_bulk_host_ns") and the kernels between events ("train_bulk_device_ns").
Prints one JSON line.
usage: train_batch_bench.py [records=100000] [single=5000]"""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probqa_amd import interop

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
N_SINGLE = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
QUIZZES, QUIZ_ANSWERS = 256, 16

f = interop.PqaEngineFactory()
lib = interop.load_library()


def records(rng, n, Q, K, T, skew):
    counts = rng.integers(8, 25, size=n).astype(np.int64)
    aqs = np.stack([rng.integers(0, Q, size=int(counts.sum())), rng.integers(0, K, size=int(counts.sum()))], axis=1).astype(np.int64)
    targets = rng.integers(0, T, size=n).astype(np.int64)
    if skew:
        targets[rng.random(n) < 0.1] = T // 3
    return counts, np.ascontiguousarray(aqs), targets, rng.uniform(0.3, 2.0, size=n)


def single_rate(eng, counts, aqs, targets, amounts, n):
    base, at = aqs.ctypes.data, 0
    c_l, t_l, a_l = counts[:n].tolist(), targets[:n].tolist(), amounts[:n].tolist()
    t0 = time.perf_counter()
    for c, t, a in zip(c_l, t_l, a_l):
        e = lib.PqaEngine_Train(eng.c_engine, c, ctypes.cast(base + 16 * at, ctypes.POINTER(interop.CiAnsweredQuestion)), t, a)
        if e:
            interop._check(e)
        at += c
    eng.synchronize()   # (the launches' device work too)
    return n / (time.perf_counter() - t0)


def batch_rate(eng, counts, aqs, targets, amounts):
    h0, d0, l0 = (eng.get_option(x) for x in ("train_bulk_host_ns", "train_bulk_device_ns", "train_bulk_launches"))
    t0 = time.perf_counter()
    eng.train_batch_arrays(counts, aqs, targets, amounts)
    wall = time.perf_counter() - t0
    h1, d1, l1 = (eng.get_option(x) for x in ("train_bulk_host_ns", "train_bulk_device_ns", "train_bulk_launches"))
    return {"records_per_s": round(len(counts) / wall), "wall_ms": round(wall * 1e3, 3), "host_ms": round((h1 - h0) / 1e6, 3),
            "device_ms": round((d1 - d0) / 1e6, 3), "launches": l1 - l0, "steps": int(counts.sum())}


def quiz_rates(eng, rng, Q, K, T):
    out = {}
    for form in ("single", "batch"):
        lists = [[interop.AnsweredQuestion(int(q), int(a)) for q, a in zip(rng.integers(0, Q, QUIZ_ANSWERS), rng.integers(0, K, QUIZ_ANSWERS))]
                 for _ in range(QUIZZES)]
        ids = eng.resume_quiz_batch(lists)
        targets = rng.integers(0, T, size=QUIZZES)
        amounts = rng.uniform(0.3, 2.0, size=QUIZZES)
        t0 = time.perf_counter()
        if form == "single":
            for qz, t, a in zip(ids, targets.tolist(), amounts.tolist()):
                eng.record_quiz_target(qz, t, a)
            eng.synchronize()
        else:
            eng.record_quiz_target_batch(ids, targets, amounts)
        out[form] = round(QUIZZES / (time.perf_counter() - t0))
        for qz in ids:
            eng.release_quiz(qz)
    return {"record_quiz_target_per_s": out["single"], "record_quiz_target_batch_per_s": out["batch"]}


result = {"bench": "train_batch", "records": N, "single_records": N_SINGLE}
for Q, K, T in ((1000, 5, 1000), (10000, 5, 10000)):
    eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1))
    assert err is None, err
    eng.fill_synthetic(8.0, 0.5, 20261016)
    rng = np.random.default_rng(1)
    w = records(rng, 2000, Q, K, T, False)        # warm-up: staging and scratch grown, code paths loaded
    eng.train_batch_arrays(*w)
    single_rate(eng, *w, 200)
    shape = {}
    for skew in (False, True):
        counts, aqs, targets, amounts = records(rng, N, Q, K, T, skew)
        r = {"train_single_records_per_s": round(single_rate(eng, counts, aqs, targets, amounts, N_SINGLE))}
        r.update(batch_rate(eng, counts, aqs, targets, amounts))
        r["batch_over_single"] = round(r["records_per_s"] / r["train_single_records_per_s"], 1)
        shape["skewed" if skew else "uniform"] = r
    shape.update(quiz_rates(eng, rng, Q, K, T))
    result[f"{Q}x{K}x{T}"] = shape
    eng.close()
print(json.dumps(result))
