"""The shared protocols of probqa_amd/csrc/combining.h -- the posting lock and the combiner of concurrent selection calls -- driven
by tests/combining_check.cpp with fake operations and fake sweeps, no GPU: built with g++ as it is and again under ThreadSanitizer
(a CPU build), which must report nothing."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "combining_check.cpp")
BUILDS = {"plain": ["-O2"], "tsan": ["-O1", "-g", "-fsanitize=thread"]}
# (part, threads, calls per thread): the sanitizer's build runs fewer calls
RUNS = {"plain": [("lock", 64, 400), ("combine", 64, 300), ("take", 8, 4000)], "tsan": [("lock", 64, 200), ("combine", 64, 100), ("take", 8, 2000)]}


@pytest.fixture(scope="module")
def checks(tmp_path_factory):
    out = tmp_path_factory.mktemp("combining")
    exes = {}
    for name, flags in BUILDS.items():
        exe = str(out / ("combining_check_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SOURCE])
        exes[name] = exe
    return exes


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_combining_protocols(checks, build):
    """Posting lock: 64 threads post while others take and release the lock and run records through RunOrPost -- every record runs
    exactly once, each drain in post order, no poster stranded.  Combiner: 64 clients, two per quiz -- every request served exactly
    once, a quiz once per batch, batches within the limit and trimmed to the lane groups, the lead to the oldest waiting request,
    and a context reused only once the clients selecting out of it are done (readers back at 0).  TryLockOrPost: 8 threads mix forced
    and unforced calls -- every record runs exactly once and with the lock held, by its poster or by the holder, a forced one never
    on the direct path, nobody stranded."""
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    for part, threads, calls in RUNS[build]:
        res = subprocess.run([checks[build], part, str(threads), str(calls)], capture_output=True, text=True, timeout=60, env=env)
        assert res.returncode == 0, (part, res.returncode, res.stderr[-4000:])
        assert "ThreadSanitizer" not in res.stderr, res.stderr[-4000:]
        assert res.stdout.startswith("ok " + part), res.stdout
