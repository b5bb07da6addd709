"""tools/record_ranks_bench.py on a small cube, two rounds: it must still run against the library as it is, print its three legs,
and its legs must agree with the whole engine (the tool asserts that itself)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_ranks_bench_tool():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "record_ranks_bench.py"), "60", "5", "301", "2,3", "8", "2"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [x["shards"] for x in rows] == [2, 3], r.stdout
    for x in rows:
        assert x["package_bytes"] == 8 * 8 * 304, x
        for leg in ("a_single_quiz_form", "b_posterior_package", "c_whole_engine"):
            assert x["answers_per_s"][leg]["median"] > 0
