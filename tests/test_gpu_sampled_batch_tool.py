"""tools/sampled_batch_bench.py on a small cube: it must still run against the library as it is, and its host and device legs must
agree with each other (the tool asserts that itself)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sampled_batch_bench_tool():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sampled_batch_bench.py"), "300", "5", "200", "3"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [x["quizzes"] for x in rows] == [8, 32, 64, 256], r.stdout
    for x in rows:
        for leg in ("a_single_calls", "b_batch_host", "c_batch_device", "d_argmax_batch"):
            assert x[leg]["selections_per_s"] > 0
        assert x["selector_kernels_us"]["median"] > 0 and 0 <= x["pick0"] < 300
