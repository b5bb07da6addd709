"""No-GPU checks that PqaEngine_QuizStatusBatch and PqaEngine_RankTargetsBatch are part of the boundary: declared in include/PqaHipExt.h,
bound in probqa_amd/interop.py with as many argument types, exported by the built libPqaCore.so, with their Python methods and the
QuizStatus record."""
import ctypes
import inspect

import abi_common as abi
from probqa_amd import interop

STATUS, RANK = "PqaEngine_QuizStatusBatch", "PqaEngine_RankTargetsBatch"


def params(name):
    return [a.strip() for a in " ".join(abi.header_params(name, r"void\s*\*").split()).split(",")]


def test_header_declares_the_calls():
    assert params(STATUS) == ["void *pvEngine", "int64_t nQuizzes", "const int64_t *pQuizzes", "int64_t nLevels", "const double *pLevels",
                              "CiHipQuizStatus *pStatus", "int64_t *pLevelCounts", "double *pLevelMass"], params(STATUS)
    assert params(RANK) == ["void *pvEngine", "int64_t nPairs", "const int64_t *pQuizzes", "const int64_t *pTargets", "double *pProb", "int64_t *pRank"], params(RANK)
    assert STATUS in abi.declared_functions("PqaHipExt.h") and RANK in abi.declared_functions("PqaHipExt.h")


def test_binding_carries_the_calls():
    p64, pdbl = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    restype, argtypes = abi.bound_as(STATUS)
    assert restype is ctypes.c_void_p
    assert argtypes == [ctypes.c_void_p, ctypes.c_int64, p64, ctypes.c_int64, pdbl, ctypes.POINTER(interop.CiHipQuizStatus), p64, pdbl], argtypes
    restype, argtypes = abi.bound_as(RANK)
    assert restype is ctypes.c_void_p
    assert argtypes == [ctypes.c_void_p, ctypes.c_int64, p64, p64, pdbl, p64], argtypes
    assert ctypes.sizeof(interop.CiHipQuizStatus) == 40
    assert [(n, t) for n, t in interop.CiHipQuizStatus._fields_] == [("entropy", ctypes.c_double), ("mass", ctypes.c_double), ("topProb", ctypes.c_double),
                                                                     ("iTopTarget", ctypes.c_int64), ("nCandidates", ctypes.c_int64)]


def test_python_entry_points_present():
    assert list(inspect.signature(interop.PqaEngine.quiz_status_batch).parameters) == ["self", "quizzes", "levels"]
    assert list(inspect.signature(interop.PqaEngine.quiz_status).parameters) == ["self", "i_quiz", "levels"]
    assert inspect.signature(interop.PqaEngine.quiz_status_batch).parameters["levels"].default == ()
    assert list(inspect.signature(interop.PqaEngine.rank_targets_batch).parameters) == ["self", "pairs"]
    assert list(inspect.signature(interop.PqaEngine.rank_target).parameters) == ["self", "i_quiz", "i_target"]
    s = interop.QuizStatus(1.5, 1.0, 0.25, 3, 7, [7, 2], [1.0, 0.5])
    assert (s.entropy, s.mass, s.top_prob, s.i_top_target, s.n_candidates, s.level_counts, s.level_mass) == (1.5, 1.0, 0.25, 3, 7, [7, 2], [1.0, 0.5])


def test_library_exports_the_calls(factory):
    for name in (STATUS, RANK):
        assert name in abi.exported_symbols()
        assert getattr(interop.load_library(), name) is not None
