"""No-GPU checks that PqaEngine_ListTopTargetsAmongBatch -- a quiz's best targets within a listed set -- is part of the boundary:
declared in include/PqaHipExt.h, bound in probqa_amd/interop.py with as many argument types, exported by the built libPqaCore.so,
with its two Python methods."""
import abi_common as abi
from probqa_amd import interop

NAME = "PqaEngine_ListTopTargetsAmongBatch"


def test_header_declares_the_call():
    args = [a.strip() for a in abi.header_params(NAME, r"void\s*\*").split(",")]
    assert len(args) == 11, args
    assert "pQuizzes" in args[2] and "pListOf" in args[3] and "nLists" in args[4] and "pListCounts" in args[5] and "pTargets" in args[6], args
    assert all("const int64_t *" in args[i] for i in (2, 3, 5, 6)), args      # the quizzes and the lists
    assert "maxCount" in args[7], args
    assert "CiRatedTarget *" in args[8] and "int64_t *" in args[9] and "double *" in args[10], args
    assert all("const" not in a for a in args[8:]), args                      # the three outputs


def test_binding_carries_the_call():
    _, argtypes = abi.bound_as(NAME)
    assert len(argtypes) == 11


def test_python_methods_present():
    for m in ("list_top_targets_among_batch", "list_top_targets_among"):
        assert callable(getattr(interop.PqaEngine, m, None)), m


def test_library_exports_the_call(factory):
    assert NAME in abi.exported_symbols()
    assert getattr(interop.load_library(), NAME) is not None
