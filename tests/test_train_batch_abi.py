"""No-GPU checks that PqaEngine_TrainBatch and PqaEngine_RecordQuizTargetBatch are part of the boundary: declared in
include/PqaHipExt.h, bound in probqa_amd/interop.py with their Python methods, and exported by the built libPqaCore.so."""
import os
import re
import subprocess

import pytest

from probqa_amd import interop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"PqaEngine_TrainBatch": 6, "PqaEngine_RecordQuizTargetBatch": 5}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_declares_train_batch(name):
    text = open(os.path.join(ROOT, "include", "PqaHipExt.h")).read()
    m = re.search(r"PQACORE_API\s+void\s*\*\s*" + name + r"\s*\(([^)]*)\)", text)
    assert m, "PqaHipExt.h does not declare " + name
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == NAMES[name], args
    if name == "PqaEngine_TrainBatch":
        assert "CiAnsweredQuestion" in args[3] and "double" in args[5], args
    else:
        assert "double" in args[4], args


@pytest.mark.parametrize("name", sorted(NAMES))
def test_binding_carries_train_batch(name):
    assert name in interop.HIP_EXPORTS
    _, argtypes = interop.HIP_EXPORTS[name]
    assert len(argtypes) == NAMES[name]


def test_python_methods_present():
    for m in ("train_batch", "train_batch_arrays", "record_quiz_target_batch"):
        assert callable(getattr(interop.PqaEngine, m, None)), m


def test_library_exports_train_batch(factory):
    out = subprocess.check_output(["nm", "-D", "--defined-only", interop.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert name in exported
        assert getattr(interop.load_library(), name) is not None
