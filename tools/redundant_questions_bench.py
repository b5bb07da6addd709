"""What listing the questions whose answers a given one predicts costs (a tool, not a test).  One process, one engine per shape and
precision; per number of sources two legs:
  (a) PqaEngine_ListRedundantQuestionsBatch, top 10: the sources' weighted rows packed on the device, per tile of sources one streaming
      pass over the cube there, the rows listed there, nSources x 10 records come back;
  (b) today's way to the same listing: PqaHip_GetKB -- the whole cube copied to the host -- and numpy there, the copy and the compute
      timed apart.  Run once: the copy and the part of the compute that does not depend on the sources once per shape and precision,
      the sources' tables and their listing once per source count.  It is slow.
Both legs go through the C ABI / the binding with their buffers built beforehand.  Before the timing the legs are compared as a valid
top-k: leg (a) sorted by (-bits, id), each value within twice the derived bar (8 + K^2) (T + 16) 2^-52 bits of leg (b)'s (either leg is
within the bar of the exact value), and no unlisted question of leg (b) above leg (a)'s last value plus that.  Leg (a): two warm-ups,
then `rounds` timed calls: ms_min / ms_median / ms_max, and the cube's bytes per pass over the median as a fraction of the 8 TB/s peak
(passes = tiles of `tile` sources: a pass per tile is what the kernel asks of the memory system if nothing stays in a cache).
Prints one JSON line per shape, precision and source count.
usage: redundant_questions_bench.py [rounds=9]                   1000x5x1000 and 10000x5x10000, Double and Float, 1 / one tile / 32 sources
       redundant_questions_bench.py Q K T rounds sources...      one shape of your own, both precisions (what the suite runs, tiny)"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probqa_amd import interop

WARMUP = 2
TOP = 10
PEAK_BYTES_PER_MS = 8e12 / 1e3
RECORD = np.dtype([("q", "<i8"), ("p", "<f8")])
F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)
TILE = {2: 8, 3: 4, 4: 4, 5: 2}   # pqa_kernels.h: RedundancyTileWidth


def check(err):
    if err:
        raise RuntimeError(interop.PqaError(err).to_string(True))


def host_rows(p, w, sources):
    """numpy on the host, from p = A * (1 / D) as [Q][K][T]: the sources' tables against every question, then the bits"""
    Q, K, T = p.shape
    flat = p.reshape(Q * K, T)
    rows = np.zeros((len(sources), Q))
    for i, s in enumerate(sources):
        J = ((w * p[s]) @ flat.T).reshape(K, Q, K).transpose(1, 0, 2)   # [Q][k][k']
        Z = J.sum(axis=(1, 2))
        r, c = J.sum(axis=2), J.sum(axis=1)
        with np.errstate(all="ignore"):
            term = (J / Z[:, None, None]) * np.log2(J * Z[:, None, None] / (r[:, :, None] * c[:, None, :]))
        rows[i] = np.where(J > 0, term, 0.0).sum(axis=(1, 2))
    return rows


def run_shape(lib, f, Q, K, T, rounds, counts, prec):
    p64, prec_p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(interop.CiRatedQuestion)
    eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **(F32 if prec == "float" else {})))
    shape = f"{Q}x{K}x{T}"
    if err is not None or eng is None:
        print(json.dumps({"shape": shape, "precision": prec, "skipped": err.to_string(True) if err else "no engine"}), flush=True)
        return
    eng.fill_synthetic(8.0, 0.5, 7)
    elem = 4 if prec == "float" else 8
    ld = (T * elem + 127) // 128 * 128 // elem
    cube_bytes = Q * (K + 1) * ld * elem
    bar = 2 * (8 + K * K) * (T + 16) * 2.0 ** -52
    tile = TILE.get(K, 1)
    # leg (b), once per shape: the copy, and the part of the compute that does not depend on the sources
    t0 = time.perf_counter()
    A, D, B = eng.get_kb()
    t1 = time.perf_counter()
    np.multiply(A, (1.0 / D)[:, None, :], out=A)
    t2 = time.perf_counter()
    del D
    for n in counts:
        sources = np.ascontiguousarray(np.random.default_rng(100 + n).integers(0, Q, size=n), dtype=np.int64)
        got = np.zeros((n, TOP), dtype=RECORD)
        got_counts = np.zeros(n, dtype=np.int64)

        def leg_a():
            check(lib.PqaEngine_ListRedundantQuestionsBatch(eng.c_engine, n, sources.ctypes.data_as(p64), TOP, got.ctypes.data_as(prec_p), got_counts.ctypes.data_as(p64)))

        leg_a()
        t3 = time.perf_counter()
        want = host_rows(A, B, sources)
        t4 = time.perf_counter()
        agree = True
        for i in range(n):
            rec, row = got[i, :got_counts[i]], want[i]
            ok = list(rec["q"]) == [x["q"] for x in sorted(rec, key=lambda x: (-x["p"], x["q"]))] and sources[i] not in rec["q"]
            ok = ok and len(rec) <= TOP and bool((np.abs(rec["p"] - row[rec["q"]]) <= bar).all())
            if ok:
                rest = np.ones(Q, dtype=bool)
                rest[rec["q"]] = False
                rest[sources[i]] = False
                ok = not (row[rest] > (rec["p"][-1] if len(rec) == TOP else 0.0) + bar).any()
            agree = agree and bool(ok)
        for _ in range(WARMUP):
            leg_a()
        ts = []
        for _ in range(rounds):
            t = time.perf_counter()
            leg_a()
            ts.append(time.perf_counter() - t)
        med = statistics.median(ts) * 1e3
        passes = n // tile + n % tile if tile > 1 else n
        out = {"shape": shape, "precision": prec, "sources": n, "tile": tile, "top": TOP, "rounds": rounds, "legs_agree": agree,
               "a_list": {"ms_median": round(med, 4), "ms_min": round(min(ts) * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)},
               "cube_bytes": cube_bytes, "passes": passes, "fraction_of_peak": round(cube_bytes * passes / med / PEAK_BYTES_PER_MS, 4),
               "b_today": {"ms_copy": round((t1 - t0) * 1e3, 3), "ms_compute": round((t2 - t1 + t4 - t3) * 1e3, 3)}}
        print(json.dumps(out), flush=True)
    eng.close()


def main():
    lib = interop.load_library()
    f = interop.PqaEngineFactory()
    if len(sys.argv) > 5:
        Q, K, T, rounds = (int(x) for x in sys.argv[1:5])
        for prec in ("double", "float"):
            run_shape(lib, f, Q, K, T, rounds, [int(x) for x in sys.argv[5:]], prec)
        return
    rounds = max(9, int(sys.argv[1])) if len(sys.argv) > 1 else 9
    for Q, K, T in ((1000, 5, 1000), (10000, 5, 10000)):
        for prec in ("double", "float"):
            run_shape(lib, f, Q, K, T, rounds, [1, TILE[K], 32], prec)


if __name__ == "__main__":
    main()
