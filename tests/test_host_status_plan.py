"""The tile grouping of RankTargetsBatch (probqa_amd/csrc/status_plan.h: PlanRankTiles), no GPU: driven through the "status_plan" script
of PqaHip_HostLogicProbe and held against a plain-Python restatement of the rule -- the pairs of one quiz kept in call order, at most 32
per tile, every pair in exactly one tile, the tiles in the order they were opened, outputs scattered back to call positions.
The same rules again in tests/status_plan_check.cpp, a program of its own built with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer (a CPU build, run as a process, as tests/test_host_separation.py runs its check)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from probqa_amd import interop

CAP = 32   # pqa_kernels.h: kRankTile


def probe(words, n_out):
    lib = interop.load_library()
    arr = np.ascontiguousarray(words, dtype=np.int64)
    out = np.zeros(max(1, n_out), dtype=np.int64)
    n = lib.PqaHip_HostLogicProbe(b"status_plan", arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(arr),
                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n_out)
    return n, out[:max(0, n)].tolist()


def plan(quizzes, cap=CAP):
    """the tiles, each a list of positions in the call"""
    n, out = probe([cap, len(quizzes)] + list(quizzes), 1 + 2 * len(quizzes))
    assert n >= 1, (n, out)
    tiles, at = [], 1
    for _ in range(out[0]):
        tiles.append(out[at + 1:at + 1 + out[at]])
        at += 1 + out[at]
    assert at == n
    return tiles


def restated(quizzes, cap=CAP):
    tiles, open_of = [], {}
    for i, q in enumerate(quizzes):
        if q not in open_of or len(tiles[open_of[q]]) >= cap:
            open_of[q] = len(tiles)
            tiles.append([])
        tiles[open_of[q]].append(i)
    return tiles


def check(quizzes, cap=CAP):
    tiles = plan(quizzes, cap)
    assert tiles == restated(quizzes, cap), (quizzes[:40], cap)
    assert sorted(i for t in tiles for i in t) == list(range(len(quizzes)))          # every pair in exactly one tile
    for t in tiles:
        assert 1 <= len(t) <= cap and len({quizzes[i] for i in t}) == 1 and t == sorted(t)   # one quiz, call order, within the cap
    for q in set(quizzes):                                                            # a quiz's pairs in call order across its tiles, all full but the last
        mine = [t for t in tiles if quizzes[t[0]] == q]
        assert [i for t in mine for i in t] == [i for i, x in enumerate(quizzes) if x == q]
        assert all(len(t) == cap for t in mine[:-1])
    # results per position of the tile order scatter back to the call
    order = [i for t in tiles for i in t]
    out = [None] * len(quizzes)
    for k, i in enumerate(order):
        out[i] = ("result", quizzes[i], i)
    assert out == [("result", q, i) for i, q in enumerate(quizzes)]
    return tiles


def test_named_cases():
    assert check([]) == []
    assert check([5]) == [[0]]
    assert check([5] * 32) == [list(range(32))]                      # one tile exactly
    assert check([5] * 33) == [list(range(32)), [32]]
    assert [len(t) for t in check([5] * 70)] == [32, 32, 6]          # one quiz under 70 targets: three tiles
    assert check([1, 2, 1, 2, 1]) == [[0, 2, 4], [1, 3]]             # interleaved quizzes: grouped, order of first appearance
    assert check([3, 1, 3, 3], cap=2) == [[0, 2], [1], [3]]          # a quiz's second tile opens behind the tiles opened meanwhile
    assert check([7, 7, 7, 7], cap=1) == [[0], [1], [2], [3]]
    assert check([2 ** 40, -3, 2 ** 40]) == [[0, 2], [1]]            # ids are only compared (the engine validates them)
    tiles = check([i % 16 for i in range(256)])                      # 16 quizzes x 16 targets
    assert len(tiles) == 16 and all(len(t) == 16 for t in tiles)


def test_random_calls_against_the_rule():
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(0, 400))
        quizzes = [int(q) for q in rng.integers(0, int(rng.integers(1, 12)), size=n)]
        check(quizzes)
        check(quizzes, int(rng.integers(1, 40)))


def test_malformed_scripts_are_refused():
    assert probe([32], 4)[0] == -1                 # no count
    assert probe([32, 2, 5], 8)[0] == -1           # the quizzes are cut short
    assert probe([32, 1, 5, 5], 8)[0] == -1        # words left over
    assert probe([0, 1, 5], 8)[0] == -1            # a cap below 1
    assert probe([32, -1], 8)[0] == -1             # a negative number of pairs
    assert probe([32, 2, 5, 6], 3)[0] == -1        # output too small
    assert probe([32, 0], 0)[0] == -1


def test_planner_under_sanitizers(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "status_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(here, "status_plan_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
    assert re.fullmatch(r"ok \d+\n", res.stdout), res.stdout
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
