"""The packed selection record of probqa_amd/csrc/select_record.h -- what the sweep's finisher writes for the engine's own
selections and the host thread polls -- checked on the host by tests/select_record_check.cpp, built with g++: no GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "select_record_check.cpp")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("select_record") / "select_record_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, SOURCE])
    return exe


@pytest.mark.parametrize("part", ["roundtrip", "tags"])
def test_select_record(check, part):
    """roundtrip: pack -> unpack for index 0, 1 and 2^31 - 4 and for the three codes (nothing left, incomplete sweep, redo with the
    fix), outBase added to questions only.  tags: tag 0 is never produced, a wrap past 2^32 gives a different low word, and a record
    carrying the previous tag (or a cleared one) is not accepted."""
    res = subprocess.run([check, part], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, (part, res.returncode, res.stdout[-4000:], res.stderr[-4000:])
    assert res.stdout.startswith("ok " + part), res.stdout
