"""No-GPU checks that the two question-page calls -- PqaEngine_EvalConditionalGainsBatch, PqaEngine_ListQuestionPageBatch -- are part of
the boundary: declared in include/PqaHipExt.h, bound in probqa_amd/interop.py with as many argument types, exported by the built
libPqaCore.so, with their Python methods."""
import inspect

import pytest

import abi_common as abi
from probqa_amd import interop

ARGS = {
    "PqaEngine_EvalConditionalGainsBatch": 7,
    "PqaEngine_ListQuestionPageBatch": 8,
}


def params(name, returns=r"void\s*\*"):
    return [a.strip() for a in abi.header_params(name, returns).split(",")]


@pytest.mark.parametrize("name", sorted(ARGS))
def test_header_declares_the_call(name):
    args = params(name)
    assert len(args) == ARGS[name], args
    assert args[:5] == ["void *pvEngine", "int64_t nQuizzes", "const int64_t *pQuizzes", "const int64_t *pGivenCounts", "const int64_t *pGiven"], args


def test_header_argument_kinds():
    ev = params("PqaEngine_EvalConditionalGainsBatch")
    assert ev[5] == "double *pOut" and ev[6] == "int64_t n", ev
    ls = params("PqaEngine_ListQuestionPageBatch")
    assert ls[5] == "int64_t pageSize" and ls[6] == "CiRatedQuestion *pDest" and ls[7] == "int64_t *pCounts", ls


@pytest.mark.parametrize("name", sorted(ARGS))
def test_binding_carries_the_call(name):
    assert name in interop.HIP_EXPORTS, name
    _, argtypes = abi.bound_as(name)
    assert len(argtypes) == ARGS[name]


def test_python_methods_present():
    for m in ("eval_conditional_gains_batch", "list_question_page_batch", "list_question_page"):
        assert callable(getattr(interop.PqaEngine, m, None)), m
    assert list(inspect.signature(interop.PqaEngine.eval_conditional_gains_batch).parameters) == ["self", "quizzes", "given"]
    assert list(inspect.signature(interop.PqaEngine.list_question_page_batch).parameters) == ["self", "quizzes", "page_size", "given"]
    assert list(inspect.signature(interop.PqaEngine.list_question_page).parameters) == ["self", "quiz", "page_size", "given"]
    assert inspect.signature(interop.PqaEngine.eval_conditional_gains_batch).parameters["given"].default is None
    assert inspect.signature(interop.PqaEngine.list_question_page).parameters["given"].default == ()


def test_library_exports_the_calls(factory):
    exported = abi.exported_symbols()
    lib = interop.load_library()
    for name in ARGS:
        assert name in exported, name
        assert getattr(lib, name) is not None
