"""No-GPU checks that PqaEngine_PreviewAnswersBatch is part of the boundary: declared in include/PqaHipExt.h, bound in
probqa_amd/interop.py with as many argument types, exported by the built libPqaCore.so, with its Python methods and the collective of
probqa_amd/dist.py."""
import ctypes
import inspect

import abi_common as abi
from probqa_amd import dist as pdist
from probqa_amd import interop

NAME = "PqaEngine_PreviewAnswersBatch"


def test_header_declares_the_call():
    args = [a.strip() for a in " ".join(abi.header_params(NAME, r"void\s*\*").split()).split(",")]
    assert args == ["void *pvEngine", "int64_t nPairs", "const int64_t *pQuizzes", "const int64_t *pQuestions", "int64_t maxCount",
                    "double *pLikelihood", "double *pEntropy", "CiRatedTarget *pDest", "int64_t *pCounts"], args
    assert NAME in abi.declared_functions("PqaHipExt.h")


def test_binding_carries_the_call():
    restype, argtypes = abi.bound_as(NAME)
    p64, pdbl = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    assert restype is ctypes.c_void_p
    assert argtypes == [ctypes.c_void_p, ctypes.c_int64, p64, p64, ctypes.c_int64, pdbl, pdbl, ctypes.POINTER(interop.CiRatedTarget), p64], argtypes


def test_python_entry_points_present():
    assert list(inspect.signature(interop.PqaEngine.preview_answers_batch).parameters) == ["self", "pairs", "max_count"]
    assert list(inspect.signature(interop.PqaEngine.preview_answers).parameters) == ["self", "i_quiz", "i_question", "max_count"]
    assert list(inspect.signature(pdist.preview_answers_batch).parameters) == ["engine", "pairs", "max_count", "rank", "world", "group", "device"]
    p = interop.AnswerPreview(0.25, 1.5, [interop.RatedTarget(3, 0.5)])
    assert (p.likelihood, p.entropy, p.targets[0].i_target) == (0.25, 1.5, 3)


def test_library_exports_the_call(factory):
    assert NAME in abi.exported_symbols()
    assert getattr(interop.load_library(), NAME) is not None
