"""No-GPU checks that the two question-gain calls -- PqaEngine_EvalQuestionGainsBatch, PqaEngine_ListInformativeQuestionsBatch -- are part
of the boundary: declared in include/PqaHipExt.h, bound in probqa_amd/interop.py with as many argument types, exported by the built
libPqaCore.so, with their Python methods and the collective of probqa_amd/dist.py."""
import inspect

import pytest

import abi_common as abi
from probqa_amd import dist as pdist
from probqa_amd import interop

ARGS = {
    "PqaEngine_EvalQuestionGainsBatch": 5,
    "PqaEngine_ListInformativeQuestionsBatch": 6,
}


def params(name, returns=r"void\s*\*"):
    return [a.strip() for a in abi.header_params(name, returns).split(",")]


@pytest.mark.parametrize("name", sorted(ARGS))
def test_header_declares_the_call(name):
    args = params(name)
    assert len(args) == ARGS[name], args
    assert args[:3] == ["void *pvEngine", "int64_t nQuizzes", "const int64_t *pQuizzes"], args


def test_header_argument_kinds():
    ev = params("PqaEngine_EvalQuestionGainsBatch")
    assert ev[3] == "double *pOut" and ev[4] == "int64_t n", ev
    ls = params("PqaEngine_ListInformativeQuestionsBatch")
    assert ls[3] == "int64_t maxCount" and ls[4] == "CiRatedQuestion *pDest" and ls[5] == "int64_t *pCounts", ls


@pytest.mark.parametrize("name", sorted(ARGS))
def test_binding_carries_the_call(name):
    assert name in interop.HIP_EXPORTS, name
    _, argtypes = abi.bound_as(name)
    assert len(argtypes) == ARGS[name]


def test_python_methods_present():
    for m in ("eval_question_gains_batch", "list_informative_questions_batch", "list_informative_questions"):
        assert callable(getattr(interop.PqaEngine, m, None)), m
    assert list(inspect.signature(interop.PqaEngine.eval_question_gains_batch).parameters) == ["self", "quizzes"]
    assert list(inspect.signature(interop.PqaEngine.list_informative_questions_batch).parameters) == ["self", "quizzes", "max_count"]
    assert list(inspect.signature(interop.PqaEngine.list_informative_questions).parameters) == ["self", "quiz", "max_count"]
    assert list(inspect.signature(pdist.list_informative_questions_batch).parameters) == ["engine", "quizzes", "max_count", "rank", "world", "group", "device"]


def test_library_exports_the_calls(factory):
    exported = abi.exported_symbols()
    lib = interop.load_library()
    for name in ARGS:
        assert name in exported, name
        assert getattr(lib, name) is not None
