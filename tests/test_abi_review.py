"""No-GPU checks that PqaHip_GetQuizAnswers, PqaEngine_ReviewAnswersBatch and PqaEngine_ReviewAnswersBatchFromRows are part of the
boundary: declared in include/PqaHipExt.h, bound in probqa_amd/interop.py with as many argument types, exported by the built
libPqaCore.so, with their Python methods and the collective of probqa_amd/dist.py; and the chunk planner of the review
(probqa_amd/csrc/review_plan.h) through the "review_plan" script of PqaHip_HostLogicProbe."""
import ctypes
import inspect

import numpy as np
import pytest

import abi_common as abi
from probqa_amd import dist as pdist
from probqa_amd import interop

REVIEW = ["void *pvEngine", "int64_t nPairs", "const int64_t *pQuizzes", "const int64_t *pPositions", "int64_t maxCount",
          "double *pLikelihood", "double *pEntropy", "CiRatedTarget *pDest", "int64_t *pCounts"]
DECLARED = {
    "PqaHip_GetQuizAnswers": (r"int64_t", ["void *pvEngine", "void **ppError", "int64_t iQuiz", "CiAnsweredQuestion *pDest", "int64_t capacity"]),
    "PqaEngine_ReviewAnswersBatch": (r"void\s*\*", REVIEW),
    "PqaEngine_ReviewAnswersBatchFromRows": (r"void\s*\*", REVIEW + ["const void *pRows", "const int64_t *pRowFirst"]),
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_header_declares_the_call(name):
    restype, want = DECLARED[name]
    args = [a.strip() for a in " ".join(abi.header_params(name, restype).split()).split(",")]
    assert args == want, args
    assert name in abi.declared_functions("PqaHipExt.h")


def test_bindings_carry_the_calls():
    p64, pdbl, vp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    review = [vp, ctypes.c_int64, p64, p64, ctypes.c_int64, pdbl, pdbl, ctypes.POINTER(interop.CiRatedTarget), p64]
    assert abi.bound_as("PqaEngine_ReviewAnswersBatch") == (vp, review)
    assert abi.bound_as("PqaEngine_ReviewAnswersBatchFromRows") == (vp, review + [vp, p64])
    restype, argtypes = abi.bound_as("PqaHip_GetQuizAnswers")
    assert restype is ctypes.c_int64
    assert argtypes == [vp, ctypes.POINTER(vp), ctypes.c_int64, ctypes.POINTER(interop.CiAnsweredQuestion), ctypes.c_int64], argtypes


def test_python_entry_points_present():
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(interop.PqaEngine.get_quiz_answers) == ["self", "i_quiz"]
    assert names(interop.PqaEngine.review_answers_batch) == ["self", "pairs", "max_count"]
    assert names(interop.PqaEngine.review_answers) == ["self", "i_quiz", "max_count"]
    assert names(interop.PqaEngine.review_answers_batch_from_rows) == ["self", "pairs", "max_count", "rows", "row_first"]
    assert names(pdist.review_answers_batch) == ["engine", "pairs", "max_count", "rank", "world", "group", "device"]


def test_library_exports_the_calls(factory):
    for name in DECLARED:
        assert name in abi.exported_symbols()
        assert getattr(interop.load_library(), name) is not None


# ---- the chunk planner ------------------------------------------------------------------------------------------------------------
def plan(ld, row_cap, budget, lds_answers, pairs):
    """pairs: [(quiz, its answer count)] -> the chunks, lists of pair indices."""
    words = np.array([ld, row_cap, budget, lds_answers, len(pairs)] + [w for p in pairs for w in p], dtype=np.int64)
    out = np.zeros(2 * len(pairs) + 2, dtype=np.int64)
    p64 = ctypes.POINTER(ctypes.c_int64)
    n = interop.load_library().PqaHip_HostLogicProbe(b"review_plan", words.ctypes.data_as(p64), len(words), out.ctypes.data_as(p64), len(out))
    assert n >= 1, n
    chunks, at = [], 1
    for _ in range(int(out[0])):
        chunks.append([int(x) for x in out[at + 1:at + 1 + out[at]]])
        at += 1 + int(out[at])
    assert at == n
    return chunks


def chunk_bytes(chunk, pairs, ld, lds_answers):
    spilled = {pairs[i][0]: pairs[i][1] for i in chunk if pairs[i][1] > lds_answers}
    return 16 * ld * len(chunk) + sum(8 * n * ld for n in spilled.values())


def check_plan(ld, row_cap, budget, lds_answers, pairs):
    chunks = plan(ld, row_cap, budget, lds_answers, pairs)
    # every pair exactly once; within a quiz in call order; the quizzes in the order they first appear
    placed = [i for c in chunks for i in c]
    assert sorted(placed) == list(range(len(pairs)))
    first_seen = list(dict.fromkeys(q for q, _ in pairs))
    assert placed == [i for q in first_seen for i in range(len(pairs)) if pairs[i][0] == q]
    for c in chunks:
        assert 1 <= len(c) <= row_cap
        assert chunk_bytes(c, pairs, ld, lds_answers) <= budget or len(c) == 1, (c, budget)
        # a quiz's rows are a run of the chunk
        quizzes = [pairs[i][0] for i in c]
        assert all(quizzes[j] == quizzes[j - 1] or quizzes[j] not in quizzes[:j] for j in range(1, len(c)))
    # a quiz is split only where an empty chunk could not hold it whole: all its chunks but the last hold nothing else
    for q in first_seen:
        mine = [c for c in chunks if any(pairs[i][0] == q for i in c)]
        for c in mine[:-1]:
            assert all(pairs[i][0] == q for i in c), (q, c)
        if len(mine) > 1:
            assert all(pairs[i][0] == q for i in mine[-1][:1])
    return chunks


def test_review_plan_keeps_a_quiz_together_and_within_the_caps():
    lds = 24
    # three quizzes interleaved, everything fits one chunk: grouped by quiz, call order within
    pairs = [(7, 3), (9, 5), (7, 3), (4, 2), (9, 5), (7, 3)]
    assert check_plan(64, 256, 1 << 26, lds, pairs) == [[0, 2, 5, 1, 4, 3]]
    # the row cap: 200 + 100 rows do not share a chunk, the second quiz moves whole
    pairs = [(1, 200)] * 200 + [(2, 100)] * 100
    chunks = check_plan(64, 256, 1 << 30, 1000, pairs)
    assert [len(c) for c in chunks] == [200, 100]
    # a quiz with more rows than a chunk holds is split, and the next quiz does not join its tail's chunk unless it fits whole
    pairs = [(1, 300)] * 300 + [(2, 10)] * 10 + [(3, 250)] * 250
    chunks = check_plan(64, 256, 1 << 30, 1000, pairs)
    assert [len(c) for c in chunks] == [256, 54, 250]
    assert chunks[1] == list(range(256, 310))
    # the byte budget: rows of 1000 elements are 16000 bytes; 10 rows fit 160000 bytes
    pairs = [(q, 4) for q in range(5) for _ in range(4)]
    chunks = check_plan(1000, 256, 160000, lds, pairs)
    assert [len(c) for c in chunks] == [8, 8, 4]
    # spilled ratios count against the budget once per quiz and chunk: 30 answers x 1000 x 8 = 240000 bytes
    pairs = [(1, 30)] * 30 + [(2, 3)] * 3
    chunks = check_plan(1000, 256, 240000 + 20 * 16000, lds, pairs)
    assert [len(c) for c in chunks] == [20, 13]
    # a single row over the budget still gets a chunk of its own
    assert check_plan(100000, 256, 1000, lds, [(1, 2), (1, 2), (5, 1)]) == [[0], [1], [2]]
    # repeated pairs and an empty call
    assert check_plan(64, 4, 1 << 20, lds, [(3, 2)] * 9) == [[0, 1, 2, 3], [4, 5, 6, 7], [8]]
    assert plan(64, 4, 1 << 20, lds, []) == []
