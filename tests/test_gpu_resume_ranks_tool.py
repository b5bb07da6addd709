"""tools/resume_ranks_bench.py on a small cube, one round: it must still run against the library as it is, and its legs must agree
with the whole engine (the tool asserts that itself)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resume_ranks_bench_tool():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resume_ranks_bench.py"), "120", "5", "300", "6", "2,3", "8", "1"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [x["shards"] for x in rows] == [2, 3], r.stdout
    for x in rows:
        for key in ("single_us", "batch_us"):
            for leg in ("a_whole", "b_sharded_engine", "c_rows_device", "d_rows_host_in_place", "d_rows_host_staged"):
                assert x[key][leg]["median"] > 0
        assert x["pack_single"]["bytes"] == 6 * x["slot_bytes"] and x["pack_batch"]["bytes"] == 48 * x["slot_bytes"]
        assert x["pack_single"]["us"]["median"] > 0
