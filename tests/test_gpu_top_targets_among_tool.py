"""tools/top_targets_among_bench.py on a tiny shape: it must still run against the library as it is and print its table, and its two
legs -- the new call, and ListTopTargetsBatch(T) plus a host filter -- must agree (the tool compares them before it times them)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_top_targets_among_bench_tool():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "top_targets_among_bench.py"), "40", "5", "1300", "2", "8", "16", "700", "5000"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [x["list"] for x in rows] == [16, 700], r.stdout          # (a list longer than T is left out)
    for x in rows:
        assert x["shape"] == "40x5x1300" and x["quizzes"] == 8 and x["top"] == 10 and x["rounds"] == 2
        assert x["a_equals_b"] and x["mass_agrees"], x
        for leg in ("a_among", "b_today"):
            assert 0 < x[leg]["ms_min"] <= x[leg]["ms_median"] <= x[leg]["ms_max"]
