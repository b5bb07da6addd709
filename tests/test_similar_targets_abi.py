"""No-GPU checks that the four target-similarity calls -- PqaEngine_EvalTargetSimilarity, PqaEngine_ListSimilarTargetsBatch,
PqaHip_PackTargetSimilaritySums, PqaEngine_ListSimilarTargetsFromSums -- are part of the boundary: declared in include/PqaHipExt.h,
bound in probqa_amd/interop.py with as many argument types, exported by the built libPqaCore.so, with their Python methods and the
collective of probqa_amd/dist.py."""
import inspect

import pytest

import abi_common as abi
from probqa_amd import dist as pdist
from probqa_amd import interop

ARGS = {
    "PqaEngine_EvalTargetSimilarity": 5,
    "PqaEngine_ListSimilarTargetsBatch": 6,
    "PqaHip_PackTargetSimilaritySums": 6,
    "PqaEngine_ListSimilarTargetsFromSums": 7,
}


def params(name):
    return [a.strip() for a in abi.header_params(name, r"void\s*\*").split(",")]


@pytest.mark.parametrize("name", sorted(ARGS))
def test_header_declares_the_call(name):
    args = params(name)
    assert len(args) == ARGS[name], args
    assert "pvEngine" in args[0] and "nSources" in args[1] and "const int64_t *pSources" in args[2], args


def test_header_argument_kinds():
    ev = params("PqaEngine_EvalTargetSimilarity")
    assert ev[3] == "double *pOut" and ev[4] == "int64_t n", ev
    ls = params("PqaEngine_ListSimilarTargetsBatch")
    assert "maxCount" in ls[3] and ls[4] == "CiRatedTarget *pDest" and ls[5] == "int64_t *pCounts", ls
    pk = params("PqaHip_PackTargetSimilaritySums")
    assert pk[3] == "void *pDst" and pk[4] == "void *pFlag" and pk[5] == "uint64_t flagValue", pk
    fs = params("PqaEngine_ListSimilarTargetsFromSums")
    assert fs[3] == "const void *pSums" and "maxCount" in fs[4] and fs[5] == "CiRatedTarget *pDest" and fs[6] == "int64_t *pCounts", fs


@pytest.mark.parametrize("name", sorted(ARGS))
def test_binding_carries_the_call(name):
    _, argtypes = abi.bound_as(name)
    assert len(argtypes) == ARGS[name]


def test_python_methods_present():
    for m in ("eval_target_similarity", "list_similar_targets_batch", "list_similar_targets", "pack_target_similarity_sums",
              "list_similar_targets_from_sums"):
        assert callable(getattr(interop.PqaEngine, m, None)), m
    assert list(inspect.signature(interop.PqaEngine.pack_target_similarity_sums).parameters) == ["self", "sources", "ptr", "flag_ptr", "flag_value"]
    assert list(inspect.signature(pdist.list_similar_targets_batch).parameters) == ["engine", "sources", "max_count", "rank", "world", "group", "device"]


def test_library_exports_the_calls(factory):
    exported = abi.exported_symbols()
    lib = interop.load_library()
    for name in ARGS:
        assert name in exported, name
        assert getattr(lib, name) is not None
