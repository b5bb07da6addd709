"""tools/separating_questions_bench.py on a tiny shape: it must still run against the library as it is and print its table, its two
legs -- the new listing, and get_kb plus numpy on the host -- must agree (the tool compares them before it times them), and its
timings must be ordered."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_separating_questions_bench_tool():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "separating_questions_bench.py"), "40", "5", "1300", "2"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    loads = [("1 pair", 1, 2), ("256 pairs", 256, 512), ("32 groups of 16", 32, 512)]
    assert [(x["precision"], x["load"], x["groups"], x["entries"]) for x in rows] == [(p,) + l for p in ("double", "float") for l in loads], r.stdout
    for x in rows:
        assert x["shape"] == "40x5x1300" and x["top"] == 10 and x["rounds"] == 2
        assert x["legs_agree"], x
        assert 0 < x["a_list"]["ms_min"] <= x["a_list"]["ms_median"] <= x["a_list"]["ms_max"]
        assert x["b_today"]["copy"]["ms_median"] > 0 and x["b_today"]["compute"]["ms_median"] > 0
        assert 0 < x["line_bytes"] <= x["tile_line_bytes"] and 0 < x["fraction_of_peak"] < 1
