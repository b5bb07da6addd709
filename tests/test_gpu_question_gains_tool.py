"""tools/question_gains_bench.py --quick on a small shape: the four legs run for every batch, the new call agrees with the status-and-preview
route, every line carries ordered timings, and the table is printed."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_tool_runs_and_its_legs_agree(factory):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "question_gains_bench.py"), "--quick", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    batches = [x for x in lines if "quizzes" in x]
    assert [x["quizzes"] for x in batches] == [1, 8, 64, 256], lines
    for x in batches:
        print(x)
        assert x["legs_agree"] is True, x
        assert x["shape"] == "40x5x1300" and x["rounds"] == 2 and x["a_sampled_questions"] == 40 and x["a_scaled_by"] == 1.0
        for leg in ("eval", "list10", "a_status_preview", "b_priorities_floor"):
            assert 0 < x[leg]["ms_min"] <= x[leg]["ms_median"] <= x[leg]["ms_max"], x
        assert x["a_over_eval"] > 0 and x["eval_over_b"] > 0
    derived = [x for x in lines if "Glog2_per_s" in x]
    assert len(derived) == 1 and derived[0]["cube_GB_per_s"] > 0
    table = [x for x in out.stdout.splitlines() if x.startswith("|")]
    assert len(table) == 2 + len(batches) and table[0].startswith("| shape | quizzes |") and all(r.startswith("| 40x5x1300 |") for r in table[2:]), table
