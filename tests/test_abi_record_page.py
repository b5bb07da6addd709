"""No-GPU checks that the two page-of-answers calls -- PqaEngine_RecordAnswerPageBatch, PqaEngine_RecordAnswerPageBatchFromRows -- are
part of the boundary: declared in include/PqaHipExt.h, bound in probqa_amd/interop.py with the same argument types, exported by the
built libPqaCore.so, with their Python methods here and in probqa_amd/dist.py, and their counters in the engine's table of read-only
options."""
import ctypes
import inspect
import os
import re

import pytest

import abi_common as abi
from probqa_amd import interop

PLAIN = ["void *pvEngine", "int64_t nQuizzes", "const int64_t *pQuizzes", "const int64_t *pCounts", "const CiAnsweredQuestion *pAQs", "double *pLikelihood"]
PARAMS = {
    "PqaEngine_RecordAnswerPageBatch": PLAIN,
    "PqaEngine_RecordAnswerPageBatchFromRows": PLAIN + ["const void *pRows"],
}
P64, PD, PAQ = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(interop.CiAnsweredQuestion)
ARGTYPES = [ctypes.c_void_p, ctypes.c_int64, P64, P64, PAQ, PD]


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_header_declares_the_call(name):
    args = [re.sub(r"\s+", " ", a.strip()) for a in abi.header_params(name, r"void\s*\*").split(",")]
    assert args == PARAMS[name], args


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_binding_carries_the_call(name):
    restype, argtypes = abi.bound_as(name)
    assert restype is ctypes.c_void_p
    assert list(argtypes) == ARGTYPES + ([ctypes.c_void_p] if name.endswith("FromRows") else [])


def test_python_methods_present():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(interop.PqaEngine.record_answer_page_batch) == ["self", "quizzes", "pages", "likelihoods"]
    assert sig(interop.PqaEngine.record_answer_page) == ["self", "i_quiz", "page", "likelihoods"]
    assert sig(interop.PqaEngine.record_answer_page_batch_from_rows) == ["self", "quizzes", "pages", "rows", "likelihoods"]
    for m in ("record_answer_page_batch", "record_answer_page", "record_answer_page_batch_from_rows"):
        assert inspect.signature(getattr(interop.PqaEngine, m)).parameters["likelihoods"].default is False, m


def test_dist_functions_present():
    from probqa_amd import dist as pdist

    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(pdist.record_answer_page_batch) == ["engine", "quizzes", "pages", "rank", "world", "group", "device", "likelihoods"]
    assert sig(pdist.record_answer_page) == ["engine", "quiz", "page", "rank", "world", "group", "device", "likelihoods"]
    for f in (pdist.record_answer_page_batch, pdist.record_answer_page):
        p = inspect.signature(f).parameters
        assert p["group"].default is None and p["device"].default is None and p["likelihoods"].default is False


def test_library_exports_the_calls(factory):
    exported = abi.exported_symbols()
    lib = interop.load_library()
    for name in PARAMS:
        assert name in exported, name
        assert getattr(lib, name) is not None


def test_counters_are_in_the_options_table():
    """The read-only counters' table (HipEngine::GetOption).  "page_calls" and "page_device_ns" were the question pages' already, so
    the calls and the device time of the pages of answers carry the call's name."""
    text = open(os.path.join(abi.ROOT, "probqa_amd", "csrc", "hip_engine.cpp")).read()
    for name in ("record_page_calls", "page_answers", "page_launches", "record_page_device_ns"):
        assert len(re.findall(r'\{"%s", &HipEngine::\w+\}' % name, text)) == 1, name
    header = abi.header_text()
    for name in ("record_page_calls", "page_answers", "page_launches", "record_page_device_ns"):
        assert '"%s"' % name in header, name
