"""What listing the targets that answer like a given one costs (a tool, not a test).  One process, one engine per shape and precision;
per number of sources two legs:
  (a) PqaEngine_ListSimilarTargetsBatch, top 10: per tile of 32 sources one streaming pass over the cube on the device, the rows listed
      there, nSources x 10 records come back;
  (b) today's way to the same listing: PqaHip_GetKB -- the whole cube copied to the host -- and numpy there, the copy and the compute
      timed apart.  Run once: the copy and the part of the compute that does not depend on the sources once per shape and precision,
      the sources' rows and their listing once per source count.  It is slow.
Both legs go through the C ABI / the binding with their buffers built beforehand.  Before the timing the legs are compared as a valid
top-k under the derived bar (Q K + 16) 2^-52: leg (a) sorted by (-value, id), each value within the bar of leg (b)'s, and no unlisted
target of leg (b) above leg (a)'s last value plus the bar.  Leg (a): a warm-up, then `rounds` timed calls: ms_min / ms_median / ms_max,
and the cube's bytes per pass over the median as a fraction of the 8 TB/s peak (passes = tiles of 32 sources).
Prints one JSON line per shape, precision and source count.
usage: similar_targets_bench.py [rounds=9]                       1000x5x1000 and 10000x5x10000, Double and Float, 1 / 32 / 256 sources
       similar_targets_bench.py Q K T rounds sources...          one shape of your own, both precisions (what the suite runs, tiny)"""
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
RECORD = np.dtype([("t", "<i8"), ("p", "<f8")])
F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)


def check(err):
    if err:
        raise RuntimeError(interop.PqaError(err).to_string(True))


def host_listing(r, Q, sources):
    """numpy on the host, from r = sqrt(A / D) as [Q K][T]: the sources' rows, then the first TOP by (-value, id) without the source"""
    rows = (r[:, sources].T @ r) / Q
    out = []
    for i, s in enumerate(sources):
        row = rows[i].copy()
        row[s] = 0.0
        ids = np.flatnonzero(row > 0)
        out.append((ids[np.lexsort((ids, -row[ids]))[:TOP]], rows[i]))
    return out


def run_shape(lib, f, Q, K, T, rounds, counts, prec):
    p64, prec_p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(interop.CiRatedTarget)
    eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **(F32 if prec == "float" else {})))
    shape = f"{Q}x{K}x{T}"
    if err is not None or eng is None:
        print(json.dumps({"shape": shape, "precision": prec, "skipped": err.to_string(True) if err else "no engine"}), flush=True)
        return
    eng.fill_synthetic(8.0, 0.5, 7)
    elem = 4 if prec == "float" else 8
    ld = (T * elem + 127) // 128 * 128 // elem
    cube_bytes = Q * (K + 1) * ld * elem
    bar = (Q * K + 16) * 2.0 ** -52
    # leg (b), once per shape: the copy, and the part of the compute that does not depend on the sources
    t0 = time.perf_counter()
    A, D, _ = eng.get_kb()
    t1 = time.perf_counter()
    np.divide(A, D[:, None, :], out=A)
    r = np.sqrt(A, out=A).reshape(Q * K, T)
    t2 = time.perf_counter()
    del D
    for n in counts:
        sources = np.ascontiguousarray(np.random.default_rng(100 + n).integers(0, T, size=n), dtype=np.int64)
        got = np.zeros((n, TOP), dtype=RECORD)
        got_counts = np.zeros(n, dtype=np.int64)

        def leg_a():
            check(lib.PqaEngine_ListSimilarTargetsBatch(eng.c_engine, n, sources.ctypes.data_as(p64), TOP, got.ctypes.data_as(prec_p), got_counts.ctypes.data_as(p64)))

        leg_a()
        t3 = time.perf_counter()
        want = host_listing(r, Q, sources)
        t4 = time.perf_counter()
        agree = True
        for i in range(n):
            rec, (take, row) = got[i, :got_counts[i]], want[i]
            ok = len(rec) == len(take) and list(rec["t"]) == [x["t"] for x in sorted(rec, key=lambda x: (-x["p"], x["t"]))] and sources[i] not in rec["t"]
            ok = ok and bool((np.abs(rec["p"] - row[rec["t"]]) <= bar * row[rec["t"]]).all())
            if ok and len(rec):
                rest = np.ones(T, dtype=bool)
                rest[rec["t"]] = False
                rest[sources[i]] = False
                ok = not (row[rest] > rec["p"][-1] + bar * row[rest]).any()
            agree = agree and bool(ok)
        for _ in range(WARMUP):
            leg_a()
        ts = []
        for _ in range(rounds):
            t = time.perf_counter()
            leg_a()
            ts.append(time.perf_counter() - t)
        med = statistics.median(ts) * 1e3
        passes = (n + 31) // 32
        out = {"shape": shape, "precision": prec, "sources": n, "top": TOP, "rounds": rounds, "legs_agree": agree,
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
            run_shape(lib, f, Q, K, T, rounds, [1, 32, 256], prec)


if __name__ == "__main__":
    main()
