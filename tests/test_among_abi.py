"""No-GPU checks that the Among calls -- evaluate and select over a listed set of questions per quiz -- are part of the boundary:
declared in include/PqaHipExt.h, bound in probqa_amd/interop.py with as many argument types, exported by the built libPqaCore.so,
with their Python methods and the merge over process-per-GPU shards (probqa_amd/dist.py: select_among_batch)."""
import pytest

import abi_common as abi
from probqa_amd import dist as pdist
from probqa_amd import interop

NAMES = {
    "PqaEngine_EvalPrioritiesAmongBatch": 6,
    "PqaHip_SelectArgmaxAmongBatch": 6,
    "PqaEngine_NextQuestionArgmaxAmongBatch": 6,
    "PqaEngine_NextQuestionSampledAmongBatch": 7,
    "PqaEngine_NextQuestionAmongBatch": 6,
}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_declares_among(name):
    args = [a.strip() for a in abi.header_params(name, r"void\s*\*").split(",")]
    assert len(args) == NAMES[name], args
    assert "pQuizzes" in args[2] and "pCounts" in args[3] and "pQuestions" in args[4], args
    assert all("const int64_t *" in a for a in args[2:5]), args
    assert "const" not in args[-1], args              # the results
    if name == "PqaEngine_NextQuestionSampledAmongBatch":
        assert "const uint64_t" in args[5], args


@pytest.mark.parametrize("name", sorted(NAMES))
def test_binding_carries_among(name):
    _, argtypes = abi.bound_as(name)
    assert len(argtypes) == NAMES[name]


def test_python_methods_present():
    for m in ("eval_priorities_among_batch", "select_argmax_among_batch", "next_question_argmax_among_batch",
              "next_question_sampled_among_batch", "next_question_among_batch", "next_question_argmax_among",
              "next_question_sampled_among", "eval_priorities_among"):
        assert callable(getattr(interop.PqaEngine, m, None)), m
    assert callable(getattr(pdist, "select_among_batch", None))


def test_library_exports_among(factory):
    for name in NAMES:
        assert name in abi.exported_symbols()
        assert getattr(interop.load_library(), name) is not None
