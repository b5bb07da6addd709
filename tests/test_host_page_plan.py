"""The branch counts, limits and chunking of the question page calls (probqa_amd/csrc/page_plan.h), no GPU: tests/page_plan_check.cpp, a
program of its own built with g++ under AddressSanitizer and UndefinedBehaviorSanitizer (a CPU build, run as a process, as
tests/test_host_status_plan.py runs its check).  Run bare it checks named edges and seeded calls against the rule; asked a question it
answers on stdout, and the answers are held against a plain-Python restatement: K^|S| branches for Eval, K^(|S| + pageSize - 1) for a
page, at most 256 rows and 64 MiB a quiz, chunks of whole quizzes in call order that close only when the next quiz does not fit."""
import os
import re
import subprocess

import numpy as np
import pytest

ROWS, BYTES = 256, 64 << 20


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    here = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path_factory.mktemp("page_plan") / "page_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", path,
                           os.path.join(here, "page_plan_check.cpp")])
    return path


def ask(exe, *words):
    res = subprocess.run([exe] + [str(w) for w in words], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, (words, res.returncode, res.stderr[-2000:])
    return [int(x) for x in res.stdout.split()]


def fits(rows, row_doubles):
    return 1 <= rows <= ROWS and rows * row_doubles * 8 <= BYTES


def chunks(largest, row_doubles):
    start, rows = [0], 0
    for i, b in enumerate(largest):
        if rows and not fits(rows + b, row_doubles):
            start.append(i)
            rows = 0
        rows += b
    return start + [len(largest)] if largest else start


def test_planner_under_sanitizers(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
    assert re.fullmatch(r"ok \d+\n", res.stdout), res.stdout
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]


@pytest.mark.parametrize("K", [2, 3, 4, 5, 6, 7])
def test_branch_counts(exe, K):
    for given in (0, 1, 2, 3, 8, 9):
        assert ask(exe, "branches", K, given, 0, 0) == [min(K ** given, ROWS + 1)], (K, given)
        for page in (0, 1, 3):
            want = K ** (given + max(page, 1) - 1)
            assert ask(exe, "branches", K, given, page, 1) == [min(want, ROWS + 1)], (K, given, page)


def test_the_limits_at_their_edges(exe):
    assert ask(exe, "branches", 2, 8, 1, 1) == [256] and ask(exe, "branches", 2, 8, 2, 1) == [257]      # 2^8 is the last that passes
    assert ask(exe, "branches", 4, 4, 0, 0) == [256] and ask(exe, "branches", 4, 4, 2, 1) == [257]
    assert ask(exe, "branches", 2, 0, 1 << 62, 1) == [257] and ask(exe, "branches", 2, 1 << 62, 1 << 62, 1) == [257]
    for rows, row_doubles in [(256, 16), (257, 16), (0, 16), (256, 32768), (256, 32769), (255, 32896), (1, 8388608), (1, 8388609), (128, 40000), (256, 40000)]:
        assert ask(exe, "fits", rows, row_doubles) == [int(fits(rows, row_doubles))], (rows, row_doubles)
    assert fits(256, 32768) and not fits(256, 32769) and fits(128, 40000) and not fits(256, 40000)


def test_chunks_never_split_a_quiz(exe):
    assert ask(exe, "chunks", 16) == [0]
    assert ask(exe, "chunks", 16, 125, 125, 125) == [0, 2, 3]                 # 3 quizzes x 125 branches: the third opens a chunk
    assert ask(exe, "chunks", 16, 256, 256) == [0, 1, 2]
    assert ask(exe, "chunks", 16, 128, 128, 1) == [0, 2, 3]
    assert ask(exe, "chunks", 16, *([1] * 600)) == [0, 256, 512, 600]
    assert ask(exe, "chunks", 40000, 128, 64, 64, 100) == [0, 2, 4]           # the scratch limit closes a chunk before the row limit does
    rng = np.random.default_rng(9)
    for _ in range(60):
        row_doubles = int(16 << rng.integers(0, 16))
        cap = max(b for b in (256, 128, 64, 32, 16, 8, 4, 2, 1) if fits(b, row_doubles))
        largest = [int(b) for b in rng.integers(1, cap + 1, size=int(rng.integers(0, 80)))]
        got = ask(exe, "chunks", row_doubles, *largest)
        assert got == chunks(largest, row_doubles), (row_doubles, largest)
        for a, b in zip(got, got[1:]):
            assert a < b and fits(sum(largest[a:b]), row_doubles)             # whole quizzes, within both limits
