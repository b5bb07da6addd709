"""No-GPU checks that PqaEngine_ResumeQuizBatch is part of the boundary: declared in include/PqaHipExt.h, bound in
probqa_amd/interop.py, and exported by the built libPqaCore.so."""
import os
import re
import subprocess

from probqa_amd import interop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "PqaEngine_ResumeQuizBatch"


def test_header_declares_resume_quiz_batch():
    text = open(os.path.join(ROOT, "include", "PqaHipExt.h")).read()
    m = re.search(r"PQACORE_API\s+void\s*\*\s*" + NAME + r"\s*\(([^)]*)\)", text)
    assert m, "PqaHipExt.h does not declare " + NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 5 and "CiAnsweredQuestion" in args[3], args


def test_binding_carries_resume_quiz_batch():
    assert NAME in interop.HIP_EXPORTS
    restype, argtypes = interop.HIP_EXPORTS[NAME]
    assert len(argtypes) == 5
    assert callable(getattr(interop.PqaEngine, "resume_quiz_batch", None))


def test_library_exports_resume_quiz_batch(factory):
    out = subprocess.check_output(["nm", "-D", "--defined-only", interop.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert NAME in exported
    assert getattr(interop.load_library(), NAME) is not None
