"""What listing the questions that tell listed targets apart costs (a tool, not a test).  One process, one engine per shape and
precision; three loads -- 1 pair, 256 pairs of distinct targets, 32 groups of 16 -- and per load two legs:
  (a) PqaEngine_ListSeparatingQuestionsBatch, top 10: the groups staged on the device, one gathering sweep over the listed columns of
      every question's block, the rows listed there, nGroups x 10 records come back;
  (b) today's only way to the same listing: PqaHip_GetKB -- the whole cube copied to the host -- and numpy there over the listed
      columns, the copy and the compute timed apart (the copy does not depend on the load: one per round serves the three loads).
Both legs go through the C ABI / the binding with their buffers built beforehand.  Before the timing the legs are compared as a valid
top-k: leg (a) sorted by (-bits, id), each value within twice the derived bar (16 + 8 n K) 2^-52 bits of leg (b)'s (either leg is within
the bar of the exact value), and no unlisted question of leg (b) above leg (a)'s last value plus that.  Then two warm-ups of leg (a) per
load, and `rounds` rounds in which the legs are INTERLEAVED: leg (a) of every load, then leg (b).  Per load ms_min / ms_median / ms_max
of either leg, and against leg (a)'s median the bytes the sweep must touch as a fraction of the 8 TB/s peak: per question and row of its
block the distinct 64-byte lines of the call's listed columns (`line_bytes`; not the cube) -- and what the sweep asks for if no line is
shared between its tiles (`tile_line_bytes`: distinct lines per tile of 256 entries).
Prints one JSON line per shape, precision and load.
usage: separating_questions_bench.py [rounds=7]        10000x5x10000, Double and Float
       separating_questions_bench.py Q K T rounds      one shape of your own, both precisions (what the suite runs, tiny)"""
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
LINE = 64
TILE_ENTRIES, TILE_GROUPS = 256, 128   # pqa_kernels.h: kSepTileEntries, kSepTileGroups
RECORD = np.dtype([("q", "<i8"), ("p", "<f8")])
F32 = dict(prec_type=interop.PrecisionType.FLOAT, prec_exponent=8, prec_mantissa=24)


def check(err):
    if err:
        raise RuntimeError(interop.PqaError(err).to_string(True))


def loads_for(T):
    rng = np.random.default_rng(100)
    n_pairs = min(256, T // 2)
    distinct = rng.permutation(T)[:2 * n_pairs].reshape(n_pairs, 2)
    return {"1 pair": [[int(t) for t in distinct[0]]],
            "%d pairs" % n_pairs: [[int(a), int(b)] for a, b in distinct],
            "32 groups of 16": [[int(t) for t in rng.choice(T, size=16, replace=T < 16)] for _ in range(32)]}


def host_rows(A, D, groups):
    """numpy on the host over the listed columns of one get_kb: sep(G, q) for every question"""
    def f(x):
        with np.errstate(all="ignore"):
            return np.where(x > 0, x * np.log2(x), 0.0)

    rows = np.zeros((len(groups), A.shape[0]))
    for i, g in enumerate(groups):
        p = A[:, :, g] * (1.0 / D[:, g])[:, None, :]                      # [Q][K][n]
        rows[i] = np.maximum(0.0, (1.0 / len(g)) * f(p).sum(axis=(1, 2)) - f(p.sum(axis=2) * (1.0 / len(g))).sum(axis=1))
    return rows


def tiles_of(groups):
    """kb_plan.h: PlanGroupTiles -- runs of whole groups, at most TILE_ENTRIES entries and TILE_GROUPS groups"""
    tiles, cur, entries = [], [], 0
    for g in groups:
        if cur and (entries + len(g) > TILE_ENTRIES or len(cur) >= TILE_GROUPS):
            tiles.append(cur)
            cur, entries = [], 0
        cur.append(g)
        entries += len(g)
    return tiles + ([cur] if cur else [])


def lines_of(targets, elem):
    return len({t * elem // LINE for t in targets})


def spread(ts):
    return {"ms_median": round(statistics.median(ts) * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)}


def run_shape(lib, f, Q, K, T, rounds, prec):
    p64, prec_p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(interop.CiRatedQuestion)
    eng, err = f.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **(F32 if prec == "float" else {})))
    shape = f"{Q}x{K}x{T}"
    if err is not None or eng is None:
        print(json.dumps({"shape": shape, "precision": prec, "skipped": err.to_string(True) if err else "no engine"}), flush=True)
        return
    eng.fill_synthetic(8.0, 0.5, 7)
    elem = 4 if prec == "float" else 8
    loads, legs = loads_for(T), {}
    for name, groups in loads.items():
        counts = np.ascontiguousarray([len(g) for g in groups], dtype=np.int64)
        targets = np.ascontiguousarray([t for g in groups for t in g], dtype=np.int64)
        got = np.zeros((len(groups), TOP), dtype=RECORD)
        got_counts = np.zeros(len(groups), dtype=np.int64)

        def leg_a(counts=counts, targets=targets, got=got, got_counts=got_counts):
            check(lib.PqaEngine_ListSeparatingQuestionsBatch(eng.c_engine, len(counts), counts.ctypes.data_as(p64), targets.ctypes.data_as(p64), TOP,
                                                             got.ctypes.data_as(prec_p), got_counts.ctypes.data_as(p64)))

        legs[name] = dict(groups=groups, leg_a=leg_a, got=got, got_counts=got_counts, a=[], b_compute=[])
    # the legs compared, once
    A, D, _ = eng.get_kb()
    for name, leg in legs.items():
        leg["leg_a"]()
        want = host_rows(A, D, leg["groups"])
        agree = True
        for i, g in enumerate(leg["groups"]):
            bar = 2 * (16 + 8 * len(g) * K) * 2.0 ** -52
            rec, row = leg["got"][i, :leg["got_counts"][i]], want[i]
            ok = list(rec["q"]) == [x["q"] for x in sorted(rec, key=lambda x: (-x["p"], x["q"]))] and len(rec) <= TOP
            ok = ok and bool((np.abs(rec["p"] - row[rec["q"]]) <= bar).all())
            if ok:
                rest = np.ones(Q, dtype=bool)
                rest[rec["q"]] = False
                ok = not (row[rest] > (rec["p"][-1] if len(rec) == TOP else 0.0) + bar).any()
            agree = agree and bool(ok)
        leg["agree"] = agree
        for _ in range(WARMUP):
            leg["leg_a"]()
    del A, D
    copies = []
    for _ in range(rounds):
        for leg in legs.values():
            t = time.perf_counter()
            leg["leg_a"]()
            leg["a"].append(time.perf_counter() - t)
        t = time.perf_counter()
        A, D, _ = eng.get_kb()
        copies.append(time.perf_counter() - t)
        for leg in legs.values():
            t = time.perf_counter()
            rows = host_rows(A, D, leg["groups"])
            for r in rows:   # ... and the listing: the best TOP by (-bits, id)
                ids = np.flatnonzero(r > 0)
                ids[np.lexsort((ids, -r[ids]))[:TOP]]
            leg["b_compute"].append(time.perf_counter() - t)
        del A, D
    for name, leg in legs.items():
        groups = leg["groups"]
        line_bytes = Q * (K + 1) * LINE * lines_of([t for g in groups for t in g], elem)
        tile_line_bytes = Q * (K + 1) * LINE * sum(lines_of([t for g in tile for t in g], elem) for tile in tiles_of(groups))
        a = spread(leg["a"])
        out = {"shape": shape, "precision": prec, "load": name, "groups": len(groups), "entries": sum(len(g) for g in groups), "top": TOP, "rounds": rounds,
               "legs_agree": leg["agree"], "a_list": a, "b_today": {"copy": spread(copies), "compute": spread(leg["b_compute"])},
               "line_bytes": line_bytes, "tile_line_bytes": tile_line_bytes, "fraction_of_peak": round(line_bytes / a["ms_median"] / PEAK_BYTES_PER_MS, 7)}
        print(json.dumps(out), flush=True)
    eng.close()


def main():
    lib = interop.load_library()
    f = interop.PqaEngineFactory()
    if len(sys.argv) > 4:
        Q, K, T, rounds = (int(x) for x in sys.argv[1:5])
        shapes = [(Q, K, T)]
    else:
        rounds = max(3, int(sys.argv[1])) if len(sys.argv) > 1 else 7
        shapes = [(10000, 5, 10000)]
    for Q, K, T in shapes:
        for prec in ("double", "float"):
            run_shape(lib, f, Q, K, T, rounds, prec)


if __name__ == "__main__":
    main()
