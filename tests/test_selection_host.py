"""What a selection does on the host after the sweep (probqa_amd/csrc/selection_host.h) -- the nearest free question, the
reference's sampled selector, the wait for a priority vector the sweep hands over, the finish over a snapshot -- driven by
tests/selection_host_check.cpp, no GPU: built with g++ as it is, again under AddressSanitizer + UBSan and, for the hand-over, under
ThreadSanitizer (CPU builds of a stand-alone program), which must report nothing.  The picks the program prints are compared with
the Python models the GPU tests use (sampled_ranks_common.find_nearest_py, sampled_batch_common.select_py)."""
import os
import subprocess

import pytest

from sampled_batch_common import select_py
from sampled_ranks_common import find_nearest_py
from test_gpu_publish import SAMPLED_RNDS

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "selection_host_check.cpp")
BUILDS = {
    "plain": ["-O2"],
    "asan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
    "tsan": ["-O1", "-g", "-fsanitize=thread"],
}
PARTS = {"plain": ["nearest", "selector", "handover", "finish"], "asan": ["nearest", "selector", "handover", "finish"], "tsan": ["handover"]}
QS = [1, 2, 63, 64, 65, 130, 200]


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """{(build, part): stdout lines} of every run; each must end clean."""
    out = tmp_path_factory.mktemp("selection_host")
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = {}
    for name, flags in BUILDS.items():
        exe = str(out / ("selection_host_check_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SOURCE])
        for part in PARTS[name]:
            run = subprocess.run([exe, part], capture_output=True, text=True, timeout=120, env=env)
            assert run.returncode == 0, (name, part, run.returncode, run.stderr[-4000:])
            assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
            lines = run.stdout.splitlines()
            assert lines and lines[-1] == "ok " + part, (name, part, run.stdout[-400:])
            res[(name, part)] = lines[:-1]
    return res


def unavailable_of(mask_hex, Q):
    bits = int(mask_hex, 16)
    return {q for q in range(Q) if (bits >> q) & 1}


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_nearest_free_question(outputs, build):
    """FindNearestInPacks = find_nearest_py for every middle, over at least 200 random masks per Q plus the all-clear and all-set ones."""
    seen = {Q: 0 for Q in QS}
    kinds = {Q: set() for Q in QS}
    for line in outputs[(build, "nearest")]:
        tag, Q, mask_hex, *picks = line.split()
        Q = int(Q)
        assert tag == "N" and len(picks) == Q
        unavailable = unavailable_of(mask_hex, Q)
        kinds[Q].add("clear" if not unavailable else "set" if len(unavailable) == Q else "random")
        seen[Q] += 1
        for middle, pick in enumerate(picks):
            assert int(pick) == find_nearest_py(middle, Q, unavailable), (Q, mask_hex, middle)
    assert all(n >= 202 for n in seen.values()), seen
    assert all(k >= ({"clear", "set"} if Q == 1 else {"clear", "set", "random"}) for Q, k in kinds.items()), kinds


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_sampled_selector(outputs, build):
    """SelectSampledHost = select_py on the same priorities and skip bits, for subtask counts {1, 3, 8, Q, Q + 5} and the eight random
    numbers of the publish test (the program itself checks that its closure, one-word and two-word forms agree)."""
    vectors, seen = {}, set()
    for line in outputs[(build, "selector")]:
        f = line.split()
        if f[0] == "V":
            Q, s = int(f[1]), int(f[2])
            unavailable = unavailable_of(f[3], Q)
            vectors[(Q, s)] = ([float.fromhex(x) for x in f[4:]], [q in unavailable for q in range(Q)])
            assert len(vectors[(Q, s)][0]) == Q
            continue
        assert f[0] == "S"
        Q, s, n_sub, rnd, pick = (int(x) for x in f[1:])
        pri, skip = vectors[(Q, s)]
        assert pick == select_py(pri, skip, n_sub, rnd), (Q, s, n_sub, rnd)
        seen.add((Q, n_sub, rnd))
    assert seen == {(Q, n_sub, rnd) for Q in QS for n_sub in (1, 3, 8, Q, Q + 5) for rnd in SAMPLED_RNDS}


@pytest.mark.parametrize("build,part", [(b, p) for b in sorted(BUILDS) for p in PARTS[b] if p in ("handover", "finish")])
def test_hand_over_and_finish(outputs, build, part):
    """handover: TakePriorities returns exactly what a writer thread stored, in the three layouts (plain, quiz-minor, tagged), 0 for
    skipped questions without waiting for their entries, and false -- not before its timeout -- for a vector whose last entry keeps
    the previous tag.  finish: an available pick stays, a skipped one falls to the nearest free question, nothing left gives -1.
    The program checks these itself; the run ended with "ok" (fixture)."""
    assert (build, part) in outputs
