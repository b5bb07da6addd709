"""GB/s of moving a knowledge base between a .kb file and the device:
  (a) the same-type Load / SaveKB (the file's number type is the engine's: straight copies);
  (b) the converting load and save (a Double file into a Float engine and back out as Double: rows through convert_rows_kernel);
  (c) the GetKB -> SetKB detour they replace (dense fp64 host arrays of the whole cube, rounded on the host);
  (d) eight shard loads of the one file, one after the other, on one device (each seeks to its two blocks).
GB/s = the Double file's bytes / wall time of the call (for (c): of both calls).  The file lives in `folder` (default: the system's temporary
directory) and is read through the page cache after the first round: the figures compare the paths, not the disk.

usage: kb_convert_bench.py Q K T [rounds=5] [folder]     -> one JSON line"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from probqa_amd import dist as pdist  # noqa: E402
from probqa_amd import interop  # noqa: E402

P = interop.PrecisionType


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    Q, K, T = (int(x) for x in sys.argv[1:4])
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    folder = sys.argv[5] if len(sys.argv) > 5 else tempfile.gettempdir()
    src, out = os.path.join(folder, "kb_convert_bench_src.kb"), os.path.join(folder, "kb_convert_bench_out.kb")
    f = interop.PqaEngineFactory()
    eng = f.create_hip_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1), 0, Q, 0)
    eng.fill_synthetic(8.0, 0.5, 3)
    eng.save_kb(src, False)
    eng.close()
    size = os.path.getsize(src)
    legs = {k: [] for k in ("a_load_same", "a_save_same", "b_load_convert", "b_save_convert", "c_getkb_setkb", "d_eight_shard_loads")}
    try:
        for _ in range(rounds):
            t, e64 = timed(lambda: f.load_cpu_engine(src)[0])
            legs["a_load_same"].append(t)
            legs["a_save_same"].append(timed(lambda: e64.save_kb(out, False))[0])
            t, e32 = timed(lambda: f.load_hip_engine(src, P.FLOAT))
            legs["b_load_convert"].append(t)
            legs["b_save_convert"].append(timed(lambda: e32.save_kb_as(out, P.DOUBLE))[0])
            e32.close()
            fresh = f.create_hip_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, prec_type=P.FLOAT, prec_exponent=8, prec_mantissa=24), 0, Q, 0)
            legs["c_getkb_setkb"].append(timed(lambda: fresh.set_kb(*e64.get_kb()))[0])
            fresh.close()
            e64.close()

            def shards():
                for r in range(8):
                    pdist.load_shard(f, src, r, 8, P.FLOAT, device=0).close()
            if Q >= 8:
                legs["d_eight_shard_loads"].append(timed(shards)[0])
    finally:
        for p in (src, out):
            if os.path.exists(p):
                os.remove(p)
    gbps = {k: {"median": size / statistics.median(v) / 1e9, "min": size / max(v) / 1e9, "max": size / min(v) / 1e9} for k, v in legs.items() if v}
    print(json.dumps({"shape": [Q, K, T], "file_bytes": size, "rounds": rounds, "gbps": gbps}))


if __name__ == "__main__":
    main()
