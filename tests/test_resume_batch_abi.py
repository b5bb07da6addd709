"""No-GPU checks that PqaEngine_ResumeQuizBatch is part of the boundary: declared in include/PqaHipExt.h, bound in
probqa_amd/interop.py, and exported by the built libPqaCore.so."""
import abi_common as abi
from probqa_amd import interop

NAME = "PqaEngine_ResumeQuizBatch"


def test_header_declares_resume_quiz_batch():
    args = [a.strip() for a in abi.header_params(NAME, r"void\s*\*").split(",")]
    assert len(args) == 5 and "CiAnsweredQuestion" in args[3], args


def test_binding_carries_resume_quiz_batch():
    restype, argtypes = abi.bound_as(NAME)
    assert len(argtypes) == 5
    assert callable(getattr(interop.PqaEngine, "resume_quiz_batch", None))


def test_library_exports_resume_quiz_batch(factory):
    assert NAME in abi.exported_symbols()
    assert getattr(interop.load_library(), NAME) is not None
