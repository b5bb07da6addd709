"""The tile planner of the separation sweep (probqa_amd/csrc/kb_plan.h: PlanGroupTiles), no GPU: driven through the "group_tiles" script
of PqaHip_HostLogicProbe, as tests/test_host_logic.py drives RatedPrefix.  A tile is a run of whole groups: the planner never splits a
group, keeps to its caps of entries and groups, covers every group once and in order, and fills a tile as far as the caps let it.
The same rules again in tests/group_tiles_check.cpp, a program of its own built with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer (a CPU build, run as a process, as tests/test_abi_shims.py runs its check)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from probqa_amd import interop

ENTRIES, GROUPS = 256, 128   # the sweep's caps (pqa_kernels.h: kSepTileEntries, kSepTileGroups)


def probe(words, n_out):
    lib = interop.load_library()
    arr = np.ascontiguousarray(words, dtype=np.int64)
    out = np.zeros(max(1, n_out), dtype=np.int64)
    n = lib.PqaHip_HostLogicProbe(b"group_tiles", arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(arr),
                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n_out)
    return n, out[:max(0, n)].tolist()


def plan(counts, max_entries=ENTRIES, max_groups=GROUPS):
    """the first group of every tile, and the number of groups behind them"""
    n, out = probe([max_entries, max_groups, len(counts)] + list(counts), len(counts) + 3)
    assert n >= 2 and out[0] == n - 2, (n, out)
    return out[1:]


def check(counts, max_entries=ENTRIES, max_groups=GROUPS):
    tiles = plan(counts, max_entries, max_groups)
    if not counts:
        assert tiles == [0]
        return tiles
    # every group once, in order: the bounds rise strictly from 0 to the number of groups -- a bound is a GROUP index, so no group is split
    assert tiles[0] == 0 and tiles[-1] == len(counts) and all(a < b for a, b in zip(tiles, tiles[1:])), tiles
    for i, (a, b) in enumerate(zip(tiles, tiles[1:])):
        entries = sum(counts[a:b])
        assert b - a <= max_groups, (i, a, b)
        assert entries <= max_entries or b - a == 1, (i, a, b, entries)      # (a group beyond the cap -- the engine admits none -- stands alone)
        if b < len(counts):   # greedy: the next group did not fit
            assert entries + counts[b] > max_entries or b - a == max_groups, (i, a, b)
    return tiles


def test_named_cases():
    assert check([]) == [0]                                       # zero groups: no tile
    assert check([2]) == [0, 1]                                   # a single group
    assert check([64]) == [0, 1]
    assert check([2] * 128) == [0, 128]                           # one tile exactly: both caps met at once
    assert check([2] * 129) == [0, 128, 129]                      # ... and a single group more
    assert check([64] * 4) == [0, 4]                              # the entry cap met exactly by whole groups
    assert check([64] * 5) == [0, 4, 5]
    assert check([64, 2, 2, 64, 64, 2, 64, 2]) == [0, 6, 8]       # a group of 64 beside groups of 2: 64+2+2+64+64+2 = 198, + 64 > 256
    assert check([2, 64] * 4) == [0, 7, 8]                        # 2+64+2+64+2+64+2 = 200; the last 64 does not fit and is not split
    assert check([63] * 9) == [0, 4, 8, 9]                        # 252 entries a tile: the cap is not a multiple of the group
    assert check([3] * 200) == [0, 85, 170, 200]                  # 85 groups of 3 = 255 entries
    assert check([2] * 256) == [0, 128, 256]                      # a host chunk of 256 pairs
    assert check([64] * 256)[-1] == 256 and len(check([64] * 256)) == 65


def test_other_caps():
    assert check([2, 2, 2, 2, 2], 256, 2) == [0, 2, 4, 5]         # the group cap alone
    assert check([5, 5, 5], 9, 128) == [0, 1, 2, 3]
    assert check([5, 5, 5], 10, 128) == [0, 2, 3]
    assert check([300, 2, 2], 256, 128) == [0, 1, 3]              # beyond the cap: alone, never split


def test_random_calls_against_the_rules():
    rng = np.random.default_rng(3)
    for _ in range(300):
        n = int(rng.integers(0, 300))
        kind = int(rng.integers(3))
        counts = [int(c) for c in (rng.integers(2, 65, size=n) if kind == 0 else rng.choice([2, 64], size=n) if kind == 1 else rng.integers(2, 5, size=n))]
        check(counts)
        check(counts, int(rng.integers(64, 300)), int(rng.integers(1, 140)))


def test_malformed_scripts_are_refused():
    assert probe([256, 128], 4)[0] == -1               # no count
    assert probe([256, 128, 2, 2], 4)[0] == -1         # the counts are cut short
    assert probe([256, 128, 1, 2, 2], 4)[0] == -1      # words left over
    assert probe([0, 128, 1, 2], 4)[0] == -1           # a cap below 1
    assert probe([256, 0, 1, 2], 4)[0] == -1
    assert probe([256, 128, -1], 4)[0] == -1           # a negative number of groups
    assert probe([256, 128, 1, -2], 4)[0] == -1        # a negative count
    assert probe([256, 128, 2, 64, 64], 2)[0] == -1    # output too small


def test_planner_under_sanitizers(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "group_tiles_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(here, "group_tiles_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
    assert re.fullmatch(r"ok \d+\n", res.stdout), res.stdout
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
