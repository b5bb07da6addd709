"""No-GPU checks that the six question-redundancy calls -- PqaEngine_EvalQuestionRedundancy, PqaEngine_ListRedundantQuestionsBatch,
PqaHip_QuestionWeightSlotBytes, PqaHip_PackQuestionWeights, PqaEngine_EvalQuestionRedundancyFromWeights,
PqaEngine_ListRedundantQuestionsFromWeights -- are part of the boundary: declared in include/PqaHipExt.h, bound in
probqa_amd/interop.py with as many argument types, exported by the built libPqaCore.so, with their Python methods and the collective
of probqa_amd/dist.py."""
import inspect

import pytest

import abi_common as abi
from probqa_amd import dist as pdist
from probqa_amd import interop

ARGS = {
    "PqaEngine_EvalQuestionRedundancy": 5,
    "PqaEngine_ListRedundantQuestionsBatch": 6,
    "PqaHip_PackQuestionWeights": 6,
    "PqaEngine_EvalQuestionRedundancyFromWeights": 6,
    "PqaEngine_ListRedundantQuestionsFromWeights": 7,
}
SIZE_CALL = "PqaHip_QuestionWeightSlotBytes"


def params(name, returns=r"void\s*\*"):
    return [a.strip() for a in abi.header_params(name, returns).split(",")]


@pytest.mark.parametrize("name", sorted(ARGS))
def test_header_declares_the_call(name):
    args = params(name)
    assert len(args) == ARGS[name], args
    assert "pvEngine" in args[0] and "nSources" in args[1] and "const int64_t *pSources" in args[2], args


def test_header_argument_kinds():
    assert params(SIZE_CALL, r"int64_t") == ["void *pvEngine"]
    ev = params("PqaEngine_EvalQuestionRedundancy")
    assert ev[3] == "double *pOut" and ev[4] == "int64_t n", ev
    ls = params("PqaEngine_ListRedundantQuestionsBatch")
    assert "maxCount" in ls[3] and ls[4] == "CiRatedQuestion *pDest" and ls[5] == "int64_t *pCounts", ls
    pk = params("PqaHip_PackQuestionWeights")
    assert pk[3] == "void *pDst" and pk[4] == "void *pFlag" and pk[5] == "uint64_t flagValue", pk
    ew = params("PqaEngine_EvalQuestionRedundancyFromWeights")
    assert ew[3] == "const void *pWeights" and ew[4] == "double *pOut" and ew[5] == "int64_t n", ew
    lw = params("PqaEngine_ListRedundantQuestionsFromWeights")
    assert lw[3] == "const void *pWeights" and "maxCount" in lw[4] and lw[5] == "CiRatedQuestion *pDest" and lw[6] == "int64_t *pCounts", lw


@pytest.mark.parametrize("name", sorted(ARGS) + [SIZE_CALL])
def test_binding_carries_the_call(name):
    _, argtypes = abi.bound_as(name)
    assert len(argtypes) == ARGS.get(name, 1)


def test_python_methods_present():
    for m in ("eval_question_redundancy", "list_redundant_questions_batch", "list_redundant_questions", "question_weight_slot_bytes",
              "pack_question_weights", "eval_question_redundancy_from_weights", "list_redundant_questions_from_weights"):
        assert callable(getattr(interop.PqaEngine, m, None)), m
    assert list(inspect.signature(interop.PqaEngine.pack_question_weights).parameters) == ["self", "sources", "ptr", "flag_ptr", "flag_value"]
    assert list(inspect.signature(pdist.list_redundant_questions_batch).parameters) == ["engine", "sources", "max_count", "rank", "world", "group", "device"]


def test_library_exports_the_calls(factory):
    exported = abi.exported_symbols()
    lib = interop.load_library()
    for name in list(ARGS) + [SIZE_CALL]:
        assert name in exported, name
        assert getattr(lib, name) is not None
