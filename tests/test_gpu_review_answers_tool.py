"""tools/review_answers_bench.py on a tiny shape: both legs run on both precisions, the legs agree (records and likelihoods equal, entropies
within twice the model's bar), and every line carries its table's columns with ordered timings."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_tool_runs_and_its_legs_agree(factory):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "review_answers_bench.py"), "40", "5", "1300", "2", "3,26"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    loads = [("1_quiz_3_answers", 1, 3), ("1_quiz_26_answers", 1, 26), ("16_quizzes_26_answers", 16, 16 * 26)]
    assert [(x["precision"], x["load"], x["quizzes"], x["rows"]) for x in lines] == [(p,) + l for p in ("double", "float") for l in loads], lines
    for x in lines:
        print(x)
        assert x["legs_agree"] is True, x
        assert x["shape"] == "40x5x1300" and x["top"] == 10 and x["rounds"] == 2
        for leg in ("a_review", "b_today"):
            assert 0 < x[leg]["ms_min"] <= x[leg]["ms_median"] <= x[leg]["ms_max"], x
        assert x["b_over_a"] > 0
