"""tools/quiz_status_bench.py --quick on a small shape: the three legs run for every load, the new calls agree with numpy over get_priors,
every line carries ordered timings, and the table is printed."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_tool_runs_and_its_legs_agree(factory):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "quiz_status_bench.py"), "--quick", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert [(x["load"], x["entries"]) for x in lines] == [("status_1_quizzes", 1), ("status_64_quizzes", 64), ("status_256_quizzes", 256),
                                                          ("rank_256_pairs_16_quizzes_x_16_targets", 256)], lines
    for x in lines:
        print(x)
        assert x["legs_agree"] is True, x
        assert x["shape"] == "40x5x1300" and x["rounds"] == 2 and x["levels"] == (0 if x["load"].startswith("rank") else 4)
        for leg in ("a_new_call", "b_get_priors_numpy", "c_top1_floor"):
            assert 0 < x[leg]["ms_min"] <= x[leg]["ms_median"] <= x[leg]["ms_max"], x
        assert x["b_over_a"] > 0 and x["a_over_c"] > 0
    table = [x for x in out.stdout.splitlines() if x.startswith("|")]
    assert len(table) == 2 + len(lines) and table[0].startswith("| shape | load |") and all(r.startswith("| 40x5x1300 |") for r in table[2:]), table
