"""tools/preview_answers_bench.py on a tiny shape: both legs run on both precisions, the legs agree (records equal, entropies within twice
the model's bar), and every line carries ordered timings and a sane fraction of the peak rate."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_tool_runs_and_its_legs_agree(factory):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "preview_answers_bench.py"), "40", "5", "1300", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert [(x["precision"], x["pairs"]) for x in lines] == [(p, n) for p in ("double", "float") for n in (1, 64, 256)], lines
    for x in lines:
        print(x)
        assert x["legs_agree"] is True, x
        assert x["shape"] == "40x5x1300" and x["rows"] == 5 * x["pairs"] and x["top"] == 10 and x["rounds"] == 2
        for leg in ("a_preview", "b_today"):
            assert 0 < x[leg]["ms_min"] <= x[leg]["ms_median"] <= x[leg]["ms_max"], x
        assert x["b_over_a"] > 0
        elem = 8 if x["precision"] == "double" else 4
        assert x["rows_kernel_bytes"] == x["pairs"] * 1300 * (6 * elem + 8 + 5 * 8)
        assert 0 < x["fraction_of_8TBps"] < 1, x
