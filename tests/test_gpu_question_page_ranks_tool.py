"""tools/question_page_ranks_bench.py --quick on a small shape: every shard count and page size runs, the shards' pages are the whole
engine's (the tool asserts it), every line carries ordered timings and the share of the device time before the sweep, and the table is
printed."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_tool_runs_and_the_shards_agree(factory):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "question_page_ranks_bench.py"), "--quick", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert [(x["shards"], x["page_size"]) for x in lines] == [(2, 2), (2, 3), (3, 2), (3, 3)], lines
    for x in lines:
        print(x)
        assert x["pages_agree"] is True and x["shape"] == "40x5x1300" and x["rounds"] == 2 and x["quizzes"] == 8
        assert len(x["shard_steps"]) == x["shards"] == len(x["head_share"]) and 0 <= x["slowest_shard"] < x["shards"]
        for leg in [x["whole"], x["slowest"], x["pack"]] + x["shard_steps"]:
            assert 0 < leg["ms_min"] <= leg["ms_median"] <= leg["ms_max"], x
        assert x["slowest"]["ms_median"] == max(s["ms_median"] for s in x["shard_steps"])
        assert all(0 < share < 1 for share in x["head_share"]), x
        assert x["whole_over_slowest"] > 0
    table = [x for x in out.stdout.splitlines() if x.startswith("|")]
    assert len(table) == 2 + len(lines) and table[0].startswith("| shape | shards | quizzes | page |") and all(r.startswith("| 40x5x1300 |") for r in table[2:]), table
