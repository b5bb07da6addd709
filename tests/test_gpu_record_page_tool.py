"""tools/record_page_bench.py --quick on a small shape: the three legs run for every batch and page size, the page call's posteriors are
those of today's route, every line carries ordered timings, and the table is printed."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_tool_runs_and_its_legs_agree(factory):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "record_page_bench.py"), "--quick", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert [(x["quizzes"], x["page_size"]) for x in lines] == [(1, 3), (1, 5), (8, 3), (8, 5)], lines
    for x in lines:
        print(x)
        assert x["legs_agree"] is True, x
        assert x["shape"] == "60x5x1300" and x["rounds"] == 2
        for leg in ("page", "a_todays_route", "b_floor"):
            assert 0 < x[leg]["ms_min"] <= x[leg]["ms_median"] <= x[leg]["ms_max"], x
        assert x["page_over_a"] > 0 and x["page_over_b"] > 0
    table = [x for x in out.stdout.splitlines() if x.startswith("|")]
    assert len(table) == 2 + len(lines) and table[0].startswith("| shape | quizzes | page |") and all(r.startswith("| 60x5x1300 |") for r in table[2:]), table
