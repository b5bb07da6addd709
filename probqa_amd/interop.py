"""ctypes binding of libPqaCore.so (the MI355X engine) with the reference wrapper's Python API.

The class and method names, argument meaning and error behaviour mirror the reference's
``Interop/Python/ProbQAInterop/ProbQA.py`` (structs :72-116, prototypes :119-296, ``PqaEngine`` :423-741,
``PqaEngineFactory`` :743-783) so that code written against it runs unchanged; the reference module itself cannot be
imported on Linux (it subclasses ``ctypes.WinDLL`` and loads ``DLLs/PqaCore.dll``).  Everything below the C ABI is
HIP; there is no CPU fallback: loading fails loudly when the library is missing, and engine creation returns an
error when no GPU is present.

Additive, MI355X-specific methods (``eval_priorities``, ``next_question_argmax`` ...) bind ``include/PqaHipExt.h``.
"""
from __future__ import annotations

import ctypes
import os
from enum import Enum
from typing import List, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PQACORE_LIB", os.path.join(_HERE, "libPqaCore.so"))


class CiEngineDefinition(ctypes.Structure):  # reference PqaCInterop.h:10-19
    _pack_ = 8
    _fields_ = [("nAnswers", ctypes.c_int64), ("nQuestions", ctypes.c_int64), ("nTargets", ctypes.c_int64),
                ("precType", ctypes.c_uint8), ("precExponent", ctypes.c_uint16), ("precMantissa", ctypes.c_uint32),
                ("initAmount", ctypes.c_double), ("memPoolMaxBytes", ctypes.c_uint64)]


class CiAnsweredQuestion(ctypes.Structure):
    _pack_ = 8
    _fields_ = [("iQuestion", ctypes.c_int64), ("iAnswer", ctypes.c_int64)]


class CiEngineDimensions(ctypes.Structure):
    _pack_ = 8
    _fields_ = [("nAnswers", ctypes.c_int64), ("nQuestions", ctypes.c_int64), ("nTargets", ctypes.c_int64)]


class CiRatedTarget(ctypes.Structure):
    _pack_ = 8
    _fields_ = [("iTarget", ctypes.c_int64), ("prob", ctypes.c_double)]


class CiRatedQuestion(ctypes.Structure):  # include/PqaHipExt.h
    _pack_ = 8
    _fields_ = [("iQuestion", ctypes.c_int64), ("priority", ctypes.c_double)]


class CiAddQorTParam(ctypes.Structure):
    _pack_ = 8
    _fields_ = [("index", ctypes.c_int64), ("initAmount", ctypes.c_double)]


class CiHipShard(ctypes.Structure):  # include/PqaHipExt.h
    _pack_ = 8
    _fields_ = [("qFirst", ctypes.c_int64), ("qTotal", ctypes.c_int64), ("device", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class CiHipSelection(ctypes.Structure):
    _pack_ = 8
    _fields_ = [("priority", ctypes.c_double), ("iQuestion", ctypes.c_int64)]


class CiHipQuizStatus(ctypes.Structure):  # include/PqaHipExt.h, 40 bytes
    _pack_ = 8
    _fields_ = [("entropy", ctypes.c_double), ("mass", ctypes.c_double), ("topProb", ctypes.c_double), ("iTopTarget", ctypes.c_int64),
                ("nCandidates", ctypes.c_int64)]


_vp, _i64, _u64, _u8, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint8, ctypes.c_double
_pvp = ctypes.POINTER(ctypes.c_void_p)
_pi64 = ctypes.POINTER(ctypes.c_int64)
_pu64 = ctypes.POINTER(ctypes.c_uint64)
_pdbl = ctypes.POINTER(ctypes.c_double)
_pAQ = ctypes.POINTER(CiAnsweredQuestion)

# name -> (restype, argtypes): the 40 reference exports (PqaCInterop.h:48-108) ...
REFERENCE_EXPORTS = {
    "CiDebugBreak": (None, []),
    "Logger_Init": (_u8, [_pvp, ctypes.c_char_p]),
    "CiReleaseString": (None, [_vp]),
    "CiGetPqaEngineFactory": (_vp, []),
    "PqaEngineFactory_CreateCpuEngine": (_vp, [_vp, _pvp, ctypes.POINTER(CiEngineDefinition)]),
    "PqaEngineFactory_LoadCpuEngine": (_vp, [_vp, _pvp, ctypes.c_char_p, _u64]),
    "CiReleasePqaError": (None, [_vp]),
    "PqaError_ToString": (_vp, [_vp, _u8]),
    "CiReleasePqaEngine": (None, [_vp]),
    "PqaEngine_Train": (_vp, [_vp, _i64, _pAQ, _i64, _dbl]),
    "PqaEngine_QuestionPermFromComp": (_u8, [_vp, _i64, _pi64]),
    "PqaEngine_QuestionCompFromPerm": (_u8, [_vp, _i64, _pi64]),
    "PqaEngine_TargetPermFromComp": (_u8, [_vp, _i64, _pi64]),
    "PqaEngine_TargetCompFromPerm": (_u8, [_vp, _i64, _pi64]),
    "PqaEngine_QuizPermFromComp": (_u8, [_vp, _i64, _pi64]),
    "PqaEngine_QuizCompFromPerm": (_u8, [_vp, _i64, _pi64]),
    "PqaEngine_EnsurePermQuizGreater": (_u8, [_vp, _i64]),
    "PqaEngine_RemapQuizPermId": (_u8, [_vp, _i64, _i64]),
    "PqaEngine_GetTotalQuestionsAsked": (_u64, [_vp, _pvp]),
    "PqaEngine_CopyDims": (_u8, [_vp, ctypes.POINTER(CiEngineDimensions)]),
    "PqaEngine_StartQuiz": (_i64, [_vp, _pvp]),
    "PqaEngine_ResumeQuiz": (_i64, [_vp, _pvp, _i64, _pAQ]),
    "PqaEngine_NextQuestion": (_i64, [_vp, _pvp, _i64]),
    "PqaEngine_RecordAnswer": (_vp, [_vp, _i64, _i64]),
    "PqaEngine_ClearOldQuizzes": (_vp, [_vp, _i64, _dbl]),
    "PqaEngine_GetActiveQuestionId": (_i64, [_vp, _pvp, _i64]),
    "PqaEngine_SetActiveQuestion": (_vp, [_vp, _i64, _i64]),
    "PqaEngine_ListTopTargets": (_i64, [_vp, _pvp, _i64, _i64, ctypes.POINTER(CiRatedTarget)]),
    "PqaEngine_RecordQuizTarget": (_vp, [_vp, _i64, _i64, _dbl]),
    "PqaEngine_ReleaseQuiz": (_vp, [_vp, _i64]),
    "PqaEngine_SaveKB": (_vp, [_vp, ctypes.c_char_p, _u8]),
    "PqaEngine_StartMaintenance": (_vp, [_vp, ctypes.c_bool]),
    "PqaEngine_FinishMaintenance": (_vp, [_vp]),
    "PqaEngine_AddQsTs": (_vp, [_vp, _i64, ctypes.POINTER(CiAddQorTParam), _i64, ctypes.POINTER(CiAddQorTParam)]),
    "PqaEngine_RemoveQuestions": (_vp, [_vp, _i64, _pi64]),
    "PqaEngine_RemoveTargets": (_vp, [_vp, _i64, _pi64]),
    "PqaEngine_Compact": (_vp, [_vp, _pi64, ctypes.POINTER(_pi64), _pi64, ctypes.POINTER(_pi64)]),
    "CiReleaseCompaction": (None, [_pi64]),
    "PqaEngine_Shutdown": (_vp, [_vp, ctypes.c_char_p]),
    "PqaEngine_SetLogger": (_vp, [_vp, _vp]),
}
# ... and the additive ones (include/PqaHipExt.h)
HIP_EXPORTS = {
    "PqaEngineFactory_CreateHipEngine": (_vp, [_vp, _pvp, ctypes.POINTER(CiEngineDefinition)]),
    "PqaEngineFactory_CreateHipEngineSharded": (_vp, [_vp, _pvp, ctypes.POINTER(CiEngineDefinition),
                                                      ctypes.POINTER(CiHipShard)]),
    "PqaEngineFactory_LoadHipEngine": (_vp, [_vp, _pvp, ctypes.c_char_p, _u64]),
    "PqaHip_SetOption": (_vp, [_vp, ctypes.c_char_p, _i64]),
    "PqaHip_GetOption": (_i64, [_vp, ctypes.c_char_p]),
    "PqaHip_EvalKernelName": (ctypes.c_char_p, [_vp]),
    "PqaHip_SetKB": (_vp, [_vp, _pdbl, _pdbl, _pdbl]),
    "PqaHip_GetKB": (_vp, [_vp, _pdbl, _pdbl, _pdbl]),
    "PqaHip_FillSynthetic": (_vp, [_vp, _dbl, _dbl, _u64]),
    "PqaHip_SetTargetGaps": (_vp, [_vp, _i64, _pi64]),
    "PqaHip_SetQuestionGaps": (_vp, [_vp, _i64, _pi64]),
    "PqaEngine_EvalPriorities": (_vp, [_vp, _i64, _pdbl, _i64]),
    "PqaEngine_NextQuestionArgmax": (_i64, [_vp, _pvp, _i64]),
    "PqaHip_Log2Hot": (_vp, [_vp, _pdbl, _pdbl, _i64]),
    "PqaEngine_EvalPrioritiesBatch": (_vp, [_vp, _i64, _pi64, _pdbl]),
    "PqaHip_SelectArgmaxBatch": (_vp, [_vp, _i64, _pi64, ctypes.POINTER(CiHipSelection)]),
    "PqaEngine_NextQuestionArgmaxBatch": (_vp, [_vp, _i64, _pi64, _pi64]),
    "PqaEngine_NextQuestionSampledBatch": (_vp, [_vp, _i64, _pi64, _pu64, _pi64]),
    "PqaEngine_EvalPrioritiesAmongBatch": (_vp, [_vp, _i64, _pi64, _pi64, _pi64, _pdbl]),
    "PqaHip_SelectArgmaxAmongBatch": (_vp, [_vp, _i64, _pi64, _pi64, _pi64, ctypes.POINTER(CiHipSelection)]),
    "PqaEngine_NextQuestionArgmaxAmongBatch": (_vp, [_vp, _i64, _pi64, _pi64, _pi64, _pi64]),
    "PqaEngine_NextQuestionSampledAmongBatch": (_vp, [_vp, _i64, _pi64, _pi64, _pi64, _pu64, _pi64]),
    "PqaEngine_NextQuestionAmongBatch": (_vp, [_vp, _i64, _pi64, _pi64, _pi64, _pi64]),
    "PqaEngine_NextQuestionBatch": (_vp, [_vp, _i64, _pi64, _pi64]),
    "PqaEngine_NextQuestionSampled": (_i64, [_vp, _pvp, _i64, _u64]),
    "PqaHip_GetPriors": (_vp, [_vp, _i64, _pdbl, _i64]),
    "PqaHip_GetStream": (_vp, [_vp]),
    "PqaHip_SetStream": (_vp, [_vp, _vp]),
    "PqaHip_Synchronize": (_vp, [_vp]),
    "PqaHip_Quiesce": (_vp, [_vp]),
    "PqaHip_EnqueueSelectArgmax": (_vp, [_vp, _i64, _vp]),
    "PqaHip_EnqueueSelectArgmaxFlag": (_vp, [_vp, _i64, _vp, _vp, ctypes.c_uint64]),
    "PqaHip_HostRegister": (_vp, [_vp, _i64, _pvp]),
    "PqaHip_HostUnregister": (_vp, [_vp]),
    "PqaHip_PickWhenAll": (_vp, [_vp, _i64, _i64, ctypes.c_uint64, ctypes.c_double, _pdbl, _pi64]),
    "PqaHip_SelectThroughSlots": (_vp, [_vp, _i64, _vp, _vp, _i64, _i64, _i64, ctypes.c_uint64, ctypes.c_double, _pdbl, _pi64]),
    "PqaHip_SelectArgmaxRccl": (_vp, [_vp, _i64, _vp, _i64, _pdbl, _pi64]),
    "PqaHip_EnqueueEval": (_vp, [_vp, _i64]),
    "PqaHip_GetPriorDevicePtr": (_vp, [_vp, _i64, _pvp, _pi64]),
    "PqaHip_RecordAnswerRemote": (_vp, [_vp, _i64, _i64]),
    "PqaHip_AnswerRowSlotBytes": (_i64, [_vp]),
    "PqaHip_PackAnswerRows": (_vp, [_vp, _i64, _pAQ, _vp, _vp, ctypes.c_uint64]),
    "PqaHip_SampledPartBytes": (_i64, [_vp]),
    "PqaHip_PackSampledParts": (_vp, [_vp, _i64, _pi64, _vp, _vp, ctypes.c_uint64]),
    "PqaHip_SampledPickFromParts": (_vp, [_vp, _i64, _pi64, _pu64, _vp, _i64, _i64, ctypes.POINTER(CiHipSelection)]),
    "PqaEngine_TakeSampledPicks": (_vp, [_vp, _i64, _pi64, _pi64, _pi64]),
    "PqaHip_PosteriorSlotBytes": (_i64, [_vp]),
    "PqaHip_PackAnswerPosteriors": (_vp, [_vp, _i64, _pi64, _pi64, _vp, _vp, ctypes.c_uint64]),
    "PqaEngine_RecordAnswerBatchFromPosteriors": (_vp, [_vp, _i64, _pi64, _pi64, _vp]),
    "PqaEngine_ResumeQuizFromRows": (_i64, [_vp, _pvp, _i64, _pAQ, _vp]),
    "PqaEngine_ResumeQuizBatchFromRows": (_vp, [_vp, _i64, _pi64, _pAQ, _vp, _pi64]),
    "PqaEngine_RecordAnswerPageBatch": (_vp, [_vp, _i64, _pi64, _pi64, _pAQ, _pdbl]),
    "PqaEngine_RecordAnswerPageBatchFromRows": (_vp, [_vp, _i64, _pi64, _pi64, _pAQ, _pdbl, _vp]),
    "PqaEngine_RecordAnswerBatch": (_vp, [_vp, _i64, _pi64, _pi64]),
    "PqaEngine_StartQuizBatch": (_vp, [_vp, _i64, _pi64]),
    "PqaEngine_ResumeQuizBatch": (_vp, [_vp, _i64, _pi64, _pAQ, _pi64]),
    "PqaEngine_TrainBatch": (_vp, [_vp, _i64, _pi64, _pAQ, _pi64, _pdbl]),
    "PqaEngine_RecordQuizTargetBatch": (_vp, [_vp, _i64, _pi64, _pi64, _pdbl]),
    "PqaEngine_ListTopTargetsBatch": (_vp, [_vp, _i64, _pi64, _i64, ctypes.POINTER(CiRatedTarget), _pi64]),
    "PqaEngine_ListTopTargetsAmongBatch": (_vp, [_vp, _i64, _pi64, _pi64, _i64, _pi64, _pi64, _i64, ctypes.POINTER(CiRatedTarget), _pi64, _pdbl]),
    "PqaEngine_PreviewAnswersBatch": (_vp, [_vp, _i64, _pi64, _pi64, _i64, _pdbl, _pdbl, ctypes.POINTER(CiRatedTarget), _pi64]),
    "PqaEngine_QuizStatusBatch": (_vp, [_vp, _i64, _pi64, _i64, _pdbl, ctypes.POINTER(CiHipQuizStatus), _pi64, _pdbl]),
    "PqaEngine_RankTargetsBatch": (_vp, [_vp, _i64, _pi64, _pi64, _pdbl, _pi64]),
    "PqaHip_GetQuizAnswers": (_i64, [_vp, ctypes.POINTER(_vp), _i64, _pAQ, _i64]),
    "PqaEngine_ReviewAnswersBatch": (_vp, [_vp, _i64, _pi64, _pi64, _i64, _pdbl, _pdbl, ctypes.POINTER(CiRatedTarget), _pi64]),
    "PqaEngine_ReviewAnswersBatchFromRows": (_vp, [_vp, _i64, _pi64, _pi64, _i64, _pdbl, _pdbl, ctypes.POINTER(CiRatedTarget), _pi64, _vp, _pi64]),
    "PqaEngine_EvalTargetSimilarity": (_vp, [_vp, _i64, _pi64, _pdbl, _i64]),
    "PqaEngine_ListSimilarTargetsBatch": (_vp, [_vp, _i64, _pi64, _i64, ctypes.POINTER(CiRatedTarget), _pi64]),
    "PqaHip_PackTargetSimilaritySums": (_vp, [_vp, _i64, _pi64, _vp, _vp, ctypes.c_uint64]),
    "PqaEngine_ListSimilarTargetsFromSums": (_vp, [_vp, _i64, _pi64, _vp, _i64, ctypes.POINTER(CiRatedTarget), _pi64]),
    "PqaEngine_EvalQuestionRedundancy": (_vp, [_vp, _i64, _pi64, _pdbl, _i64]),
    "PqaEngine_ListRedundantQuestionsBatch": (_vp, [_vp, _i64, _pi64, _i64, ctypes.POINTER(CiRatedQuestion), _pi64]),
    "PqaHip_QuestionWeightSlotBytes": (_i64, [_vp]),
    "PqaHip_PackQuestionWeights": (_vp, [_vp, _i64, _pi64, _vp, _vp, ctypes.c_uint64]),
    "PqaEngine_EvalQuestionRedundancyFromWeights": (_vp, [_vp, _i64, _pi64, _vp, _pdbl, _i64]),
    "PqaEngine_ListRedundantQuestionsFromWeights": (_vp, [_vp, _i64, _pi64, _vp, _i64, ctypes.POINTER(CiRatedQuestion), _pi64]),
    "PqaEngine_EvalTargetSeparation": (_vp, [_vp, _i64, _pi64, _pi64, _pdbl, _i64]),
    "PqaEngine_ListSeparatingQuestionsBatch": (_vp, [_vp, _i64, _pi64, _pi64, _i64, ctypes.POINTER(CiRatedQuestion), _pi64]),
    "PqaEngine_EvalQuestionGainsBatch": (_vp, [_vp, _i64, _pi64, _pdbl, _i64]),
    "PqaEngine_ListInformativeQuestionsBatch": (_vp, [_vp, _i64, _pi64, _i64, ctypes.POINTER(CiRatedQuestion), _pi64]),
    "PqaEngine_EvalConditionalGainsBatch": (_vp, [_vp, _i64, _pi64, _pi64, _pi64, _pdbl, _i64]),
    "PqaEngine_ListQuestionPageBatch": (_vp, [_vp, _i64, _pi64, _pi64, _pi64, _i64, ctypes.POINTER(CiRatedQuestion), _pi64]),
    "PqaHip_PackGivenBlocks": (_vp, [_vp, _i64, _pi64, _vp, _vp, ctypes.c_uint64]),
    "PqaEngine_EvalConditionalGainsBatchFromBlocks": (_vp, [_vp, _i64, _pi64, _pi64, _pi64, _i64, _pi64, _vp, _i64, _pdbl, _i64]),
    "PqaHip_SelectPageStepFromBlocks": (_vp, [_vp, _i64, _pi64, _pi64, _pi64, _i64, _pi64, _vp, _i64, ctypes.POINTER(CiHipSelection)]),
    "PqaEngine_ListTopQuestions": (_i64, [_vp, _pvp, _i64, _i64, ctypes.POINTER(CiRatedQuestion)]),
    "PqaEngine_ListTopQuestionsBatch": (_vp, [_vp, _i64, _pi64, _i64, ctypes.POINTER(CiRatedQuestion), _pi64]),
    "PqaHip_HostLogicProbe": (_i64, [ctypes.c_char_p, _pi64, _i64, _pi64, _i64]),
    "PqaEngineFactory_LoadHipEngineAs": (_vp, [_vp, _pvp, ctypes.c_char_p, _u8, ctypes.POINTER(CiHipShard), _i64]),
    "PqaHip_SaveKBAs": (_vp, [_vp, ctypes.c_char_p, _u8]),
    "PqaHip_SaveKBShard": (_vp, [_vp, ctypes.c_char_p, _u8]),
    "PqaHip_CompactPlan": (_vp, [_vp, _pi64, _pi64, _pi64, ctypes.POINTER(_pi64), ctypes.POINTER(_u8)]),
    "PqaHip_QuestionBlockSlotBytes": (_i64, [_vp]),
    "PqaHip_PackQuestionBlocks": (_vp, [_vp, _i64, _pi64, _vp, _vp, ctypes.c_uint64]),
    "PqaEngine_CompactFromBlocks": (_vp, [_vp, _vp, _i64, _i64, _pi64, ctypes.POINTER(_pi64), _pi64, ctypes.POINTER(_pi64)]),
}

_lib = None


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """Load libPqaCore.so and declare every prototype.  Raises OSError if the HIP library is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise OSError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(there is no CPU fallback)")
    lib = ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)
    for table in (REFERENCE_EXPORTS, HIP_EXPORTS):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


class PqaClientStats(ctypes.Structure):  # probqa_amd/client/pqa_client.cpp
    _fields_ = [("nQuizzes", ctypes.c_int64), ("nQuestions", ctypes.c_int64), ("nGuessedOnTop", ctypes.c_int64),
                ("nErrors", ctypes.c_int64), ("seconds", ctypes.c_double), ("transcriptHash", ctypes.c_uint64)]


CLIENT_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libPqaClient.so")
_client = None


def run_learners(engine: "PqaEngine", n_threads: int, n_quizzes: int, max_questions: int = 30, seed: int = 1, train: bool = True,
                 list_targets: bool = True) -> dict:
    """The reference's learner client (PqaClient/PqaClient.cpp:150-245) as native threads on ONE engine, through the C ABI only:
    `n_threads` threads share `n_quizzes` quizzes (StartQuiz, NextQuestion / RecordAnswer / ListTopTargets(1) until the guess is
    on top or `max_questions` were asked, RecordQuizTarget if `train`, ReleaseQuiz).  `list_targets=False`: clients that go from
    RecordAnswer straight to the next NextQuestion."""
    global _client
    load_library()
    if _client is None:
        if not os.path.exists(CLIENT_LIB_PATH):
            raise OSError(f"{CLIENT_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        _client = ctypes.CDLL(CLIENT_LIB_PATH)
        _client.PqaClient_RunLearners.restype = ctypes.c_int64
        _client.PqaClient_RunLearners.argtypes = [_vp, _i64, _i64, _i64, ctypes.c_uint64, _i64, ctypes.POINTER(PqaClientStats)]
    st = PqaClientStats()
    rc = _client.PqaClient_RunLearners(engine.c_engine, n_threads, n_quizzes, max_questions, seed, (1 if train else 0) | (0 if list_targets else 2), ctypes.byref(st))
    if rc != 0:
        raise PqaException("PqaClient_RunLearners refused its arguments")
    return {"quizzes": st.nQuizzes, "questions": st.nQuestions, "guessed_on_top": st.nGuessedOnTop, "errors": st.nErrors,
            "seconds": st.seconds, "transcript_hash": st.transcriptHash, "threads": n_threads}


def time_selections_native(engine: "PqaEngine", i_quiz: int, n_warm: int, n: int):
    """(seconds, last selected question) of n synchronous PqaEngine_NextQuestion calls made by native code (libPqaClient.so): the
    step of bench.py without the Python wrapper around every call."""
    global _client
    load_library()
    if _client is None:
        _client = ctypes.CDLL(CLIENT_LIB_PATH)
        _client.PqaClient_RunLearners.restype = ctypes.c_int64
        _client.PqaClient_RunLearners.argtypes = [_vp, _i64, _i64, _i64, ctypes.c_uint64, _i64, ctypes.POINTER(PqaClientStats)]
    _client.PqaClient_TimeSelections.restype = ctypes.c_double
    _client.PqaClient_TimeSelections.argtypes = [_vp, _i64, _i64, _i64, ctypes.POINTER(_i64)]
    last = _i64(-1)
    dt = _client.PqaClient_TimeSelections(engine.c_engine, i_quiz, n_warm, n, ctypes.byref(last))
    if dt < 0:
        raise PqaException("PqaClient_TimeSelections: a call of the ABI failed")
    return dt, int(last.value)


class PqaException(Exception):  # reference ProbQA.py:300-302
    pass


class PrecisionType(Enum):  # reference PqaCommon.h:17-24
    NONE = 0
    FLOAT = 1
    FLOAT_PAIR = 2
    DOUBLE = 3
    DOUBLE_PAIR = 4
    ARBITRARY = 5


class AnsweredQuestion:
    def __init__(self, i_question: int, i_answer: int):
        self.i_question = i_question
        self.i_answer = i_answer

    def __repr__(self):
        return f"[q={self.i_question}, a={self.i_answer}]"


class RatedTarget:
    def __init__(self, i_target: int, prob: float):
        self.i_target = i_target
        self.prob = prob

    def __repr__(self):
        return f"[t={self.i_target}, p={self.prob}]"


class AnswerPreview:
    """What one answer would do to a quiz (PqaEngine.preview_answers_batch): the answer's predictive probability, the entropy in
    bits of the posterior it would leave (NaN for a dead answer) and that posterior's best targets."""

    def __init__(self, likelihood: float, entropy: float, targets: List[RatedTarget]):
        self.likelihood = likelihood
        self.entropy = entropy
        self.targets = targets

    def __repr__(self):
        return f"[l={self.likelihood}, H={self.entropy}, {self.targets}]"


class QuizStatus:
    """Where a quiz stands (PqaEngine.quiz_status_batch): the entropy of its posterior in bits, the posterior's mass, the best target
    and its probability (-1 and 0.0 without a candidate), the number of candidates, and per level of the call the number and the
    mass of the candidates at or above it."""

    def __init__(self, entropy: float, mass: float, top_prob: float, i_top_target: int, n_candidates: int, level_counts: List[int],
                 level_mass: List[float]):
        self.entropy = entropy
        self.mass = mass
        self.top_prob = top_prob
        self.i_top_target = i_top_target
        self.n_candidates = n_candidates
        self.level_counts = level_counts
        self.level_mass = level_mass

    def __repr__(self):
        return f"[H={self.entropy}, mass={self.mass}, top={self.i_top_target}:{self.top_prob}, n={self.n_candidates}, {self.level_counts}, {self.level_mass}]"


class EngineDefinition:
    DEFAULT_MEM_POOL_MAX_BYTES = 512 * 1024 * 1024

    def __init__(self, n_answers: int, n_questions: int, n_targets: int, init_amount=1.0,
                 prec_type=PrecisionType.DOUBLE, prec_exponent=11, prec_mantissa=53,
                 mem_pool_max_bytes=DEFAULT_MEM_POOL_MAX_BYTES):
        self.n_answers, self.n_questions, self.n_targets = n_answers, n_questions, n_targets
        self.init_amount = init_amount
        self.prec_type, self.prec_exponent, self.prec_mantissa = prec_type, prec_exponent, prec_mantissa
        self.mem_pool_max_bytes = mem_pool_max_bytes

    def to_c(self) -> CiEngineDefinition:
        c = CiEngineDefinition()
        c.nAnswers, c.nQuestions, c.nTargets = self.n_answers, self.n_questions, self.n_targets
        c.precType, c.precExponent, c.precMantissa = self.prec_type.value, self.prec_exponent, self.prec_mantissa
        c.initAmount, c.memPoolMaxBytes = self.init_amount, self.mem_pool_max_bytes
        return c


class EngineDimensions:
    def __init__(self, n_answers: int, n_questions: int, n_targets: int):
        self.n_answers, self.n_questions, self.n_targets = n_answers, n_questions, n_targets

    def __repr__(self):
        return f"[nAnswers={self.n_answers}, nQuestions={self.n_questions}, nTargets={self.n_targets}]"


INVALID_PQA_ID = -1


def _prec_value(precision) -> int:
    """PrecisionType, its integer, or None (0: the file's / the engine's own) as the C ABI's precType."""
    if precision is None:
        return 0
    return int(precision.value if isinstance(precision, PrecisionType) else precision)


def read_kb_header(file_path: str):
    """(PrecisionType, EngineDimensions, questions asked) of a .kb file: its first 40 bytes."""
    import struct

    with open(file_path, "rb") as f:
        raw = f.read(40)
    if len(raw) != 40:
        raise PqaException("%s is too short for a .kb header" % file_path)
    prec, k, q, t, asked = struct.unpack("<QqqqQ", raw)
    return PrecisionType(prec & 0xF), EngineDimensions(k, q, t), asked


class AddQuestionParam:  # reference ProbQA.py:381-387
    def __init__(self, init_amount=1.0):
        self.i_question = INVALID_PQA_ID
        self.init_amount = init_amount

    def __repr__(self):
        return "[i_question=%d, init_amount=%f]" % (self.i_question, self.init_amount)


class AddTargetParam:  # reference ProbQA.py:390-396
    def __init__(self, init_amount=1.0):
        self.i_target = INVALID_PQA_ID
        self.init_amount = init_amount

    def __repr__(self):
        return "[i_target=%d, init_amount=%f]" % (self.i_target, self.init_amount)


class PqaError:
    """Owns a native PqaError* (reference ProbQA.py:399-420)."""

    @staticmethod
    def factor(c_err) -> Optional["PqaError"]:
        if not c_err:
            return None
        return PqaError(c_err)

    def __init__(self, c_err):
        self.c_err = ctypes.c_void_p(c_err) if not isinstance(c_err, ctypes.c_void_p) else c_err

    def __del__(self):
        if self.c_err and _lib is not None:
            _lib.CiReleasePqaError(self.c_err)
            self.c_err = None

    def __repr__(self):
        return self.to_string(True)

    def to_string(self, with_params: bool) -> str:
        p = _lib.PqaError_ToString(self.c_err, 1 if with_params else 0)
        try:
            return ctypes.cast(p, ctypes.c_char_p).value.decode("utf-8", "replace")
        finally:
            _lib.CiReleaseString(p)


class _ErrSlot(__import__("threading").local):
    """The `void **ppError` argument of the value-returning calls, one per thread (ctypes releases the GIL inside a call): allocating
    a fresh c_void_p and its reference for every NextQuestion is a quarter of a microsecond of a 21 us step."""

    def __init__(self):
        self.err = ctypes.c_void_p()
        self.ref = ctypes.byref(self.err)


_err_slot = _ErrSlot()


def _check(c_err, throw: bool = True) -> Optional[PqaError]:
    if not c_err:       # (the common case of every call: nothing to wrap)
        return None
    err = PqaError.factor(c_err)
    if err and throw:
        raise PqaException(err.to_string(True))
    return err


def host_register(address: int, n_bytes: int) -> int:
    """Make host memory (e.g. a shared-memory segment) writable by this process's GPU; returns its device address."""
    load_library()
    dev = ctypes.c_void_p()
    _check(_lib.PqaHip_HostRegister(ctypes.c_void_p(address), n_bytes, ctypes.byref(dev)))
    return dev.value


def host_unregister(address: int) -> None:
    if _lib is not None:
        _lib.PqaHip_HostUnregister(ctypes.c_void_p(address))


def pick_when_all(address: int, world: int, stride: int, flag_value: int, timeout_s: float = 30.0):
    """Host half of the shared-memory exchange: wait for all flags, then the exact global pick -> (priority, index)."""
    load_library()
    pri, idx = ctypes.c_double(), ctypes.c_int64()
    _check(_lib.PqaHip_PickWhenAll(ctypes.c_void_p(address), world, stride, flag_value, timeout_s,
                                   ctypes.byref(pri), ctypes.byref(idx)))
    return pri.value, idx.value


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(_pdbl)


_RECORD = np.dtype([("id", np.int64), ("value", np.float64)])   # CiRatedTarget, CiRatedQuestion


def _pair(index: int, value: float) -> Tuple[int, float]:
    return index, value


class PqaEngine:
    """Reference ProbQA.py:423-741 plus the additive MI355X methods."""

    def __init__(self, c_engine):
        self.c_engine = ctypes.c_void_p(c_engine)

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "c_engine", None) and _lib is not None:
            _lib.CiReleasePqaEngine(self.c_engine)
            self.c_engine = None

    # ---- id mapping ---------------------------------------------------------------------------------------------
    def __call_id_mapping(self, fn, ids: List[int]) -> List[int]:
        arr = (ctypes.c_int64 * len(ids))(*ids)
        fn(self.c_engine, len(ids), arr)
        return list(arr)

    def question_perm_from_comp(self, ids): return self.__call_id_mapping(_lib.PqaEngine_QuestionPermFromComp, ids)
    def question_comp_from_perm(self, ids): return self.__call_id_mapping(_lib.PqaEngine_QuestionCompFromPerm, ids)
    def target_perm_from_comp(self, ids): return self.__call_id_mapping(_lib.PqaEngine_TargetPermFromComp, ids)
    def target_comp_from_perm(self, ids): return self.__call_id_mapping(_lib.PqaEngine_TargetCompFromPerm, ids)
    def quiz_perm_from_comp(self, ids): return self.__call_id_mapping(_lib.PqaEngine_QuizPermFromComp, ids)
    def quiz_comp_from_perm(self, ids): return self.__call_id_mapping(_lib.PqaEngine_QuizCompFromPerm, ids)

    def ensure_perm_quiz_greater(self, bound: int) -> bool:
        return _lib.PqaEngine_EnsurePermQuizGreater(self.c_engine, bound) != 0

    def remap_quiz_perm_id(self, src_id: int, dest_id: int, throw: bool = True) -> bool:
        ok = _lib.PqaEngine_RemapQuizPermId(self.c_engine, src_id, dest_id) != 0
        if not ok and throw:
            raise PqaException(f"Failed to remap quiz permanent ID {src_id} to {dest_id}")
        return ok

    @staticmethod
    def to_c_answered_questions(answered_questions: List[AnsweredQuestion]):
        n = len(answered_questions)
        arr = (CiAnsweredQuestion * max(n, 1))()
        for i, aq in enumerate(answered_questions):
            arr[i].iQuestion, arr[i].iAnswer = aq.i_question, aq.i_answer
        return arr, n

    # ---- reference operations -----------------------------------------------------------------------------------
    def train(self, answered_questions: List[AnsweredQuestion], i_target: int, amount: float = 1.0,
              throw: bool = True) -> Optional[PqaError]:
        arr, n = self.to_c_answered_questions(answered_questions)
        return _check(_lib.PqaEngine_Train(self.c_engine, n, arr, i_target, amount), throw)

    def get_total_questions_asked(self) -> int:
        c_err = ctypes.c_void_p()
        res = _lib.PqaEngine_GetTotalQuestionsAsked(self.c_engine, ctypes.byref(c_err))
        _check(c_err.value)
        return res

    def copy_dims(self) -> EngineDimensions:
        d = CiEngineDimensions()
        if _lib.PqaEngine_CopyDims(self.c_engine, ctypes.byref(d)) == 0:
            raise PqaException("PqaEngine_CopyDims() failed")
        return EngineDimensions(d.nAnswers, d.nQuestions, d.nTargets)

    def start_quiz(self) -> int:
        c_err = ctypes.c_void_p()
        i_quiz = _lib.PqaEngine_StartQuiz(self.c_engine, ctypes.byref(c_err))
        _check(c_err.value)
        return i_quiz

    def resume_quiz(self, answered_questions: List[AnsweredQuestion]) -> int:
        arr, n = self.to_c_answered_questions(answered_questions)
        c_err = ctypes.c_void_p()
        i_quiz = _lib.PqaEngine_ResumeQuiz(self.c_engine, ctypes.byref(c_err), n, arr)
        _check(c_err.value)
        return i_quiz

    def next_question(self, i_quiz: int) -> int:
        slot = _err_slot
        q = _lib.PqaEngine_NextQuestion(self.c_engine, slot.ref, i_quiz)
        if slot.err.value:
            _check(slot.err.value)
        return q

    def record_answer(self, i_quiz: int, i_answer: int, throw: bool = True) -> Optional[PqaError]:
        return _check(_lib.PqaEngine_RecordAnswer(self.c_engine, i_quiz, i_answer), throw)

    def get_active_question_id(self, i_quiz: int) -> int:
        c_err = ctypes.c_void_p()
        q = _lib.PqaEngine_GetActiveQuestionId(self.c_engine, ctypes.byref(c_err), i_quiz)
        _check(c_err.value)
        return q

    def set_active_question(self, i_quiz: int, i_question: int, throw: bool = True) -> Optional[PqaError]:
        return _check(_lib.PqaEngine_SetActiveQuestion(self.c_engine, i_quiz, i_question), throw)

    def list_top_targets(self, i_quiz: int, max_count: int) -> List[RatedTarget]:
        arr = (CiRatedTarget * max(max_count, 1))()
        c_err = ctypes.c_void_p()
        n = _lib.PqaEngine_ListTopTargets(self.c_engine, ctypes.byref(c_err), i_quiz, max_count, arr)
        if c_err.value:
            _check(c_err.value)
        if n == 1:      # (the learner loop's ListTopTargets(1))
            return [RatedTarget(arr[0].iTarget, arr[0].prob)]
        return [RatedTarget(arr[i].iTarget, arr[i].prob) for i in range(n)]

    def record_quiz_target(self, i_quiz: int, i_target: int, amount: float = 1.0, throw: bool = True):
        return _check(_lib.PqaEngine_RecordQuizTarget(self.c_engine, i_quiz, i_target, amount), throw)

    def release_quiz(self, i_quiz: int, throw: bool = True):
        return _check(_lib.PqaEngine_ReleaseQuiz(self.c_engine, i_quiz), throw)

    def save_kb(self, file_path: str, b_double_buffer: bool, throw: bool = True):
        return _check(_lib.PqaEngine_SaveKB(self.c_engine, file_path.encode(), 1 if b_double_buffer else 0), throw)

    def save_kb_as(self, file_path: str, precision: Optional["PrecisionType"], throw: bool = True):
        """save_kb in a chosen precision (PrecisionType.FLOAT / .DOUBLE; None = the engine's own: the bytes save_kb writes).  The rows are
        converted on the device on their way out.  Whole engines (one device, or the one-process sharded engine)."""
        return _check(_lib.PqaHip_SaveKBAs(self.c_engine, file_path.encode(), _prec_value(precision)), throw)

    def save_kb_shard(self, file_path: str, precision: Optional["PrecisionType"] = None, throw: bool = True):
        """This shard's part of a save, in place: its two blocks of rows at their offsets of `file_path`, which is not emptied; the
        shard that holds question 0 also writes header, vB and trailer.  Complete once every shard has returned (dist.save_kb)."""
        return _check(_lib.PqaHip_SaveKBShard(self.c_engine, file_path.encode(), _prec_value(precision)), throw)

    def start_maintenance(self, force_quizzes: bool, throw: bool = True):
        return _check(_lib.PqaEngine_StartMaintenance(self.c_engine, force_quizzes), throw)

    def finish_maintenance(self, throw: bool = True):
        return _check(_lib.PqaEngine_FinishMaintenance(self.c_engine), throw)

    def add_qs_ts(self, add_questions: List["AddQuestionParam"], add_targets: List["AddTargetParam"],
                  throw: bool = True) -> Optional[PqaError]:
        cq = (CiAddQorTParam * max(len(add_questions), 1))()
        ct = (CiAddQorTParam * max(len(add_targets), 1))()
        for i, p in enumerate(add_questions):
            cq[i].index, cq[i].initAmount = p.i_question, p.init_amount
        for i, p in enumerate(add_targets):
            ct[i].index, ct[i].initAmount = p.i_target, p.init_amount
        err = _check(_lib.PqaEngine_AddQsTs(self.c_engine, len(add_questions), cq, len(add_targets), ct), throw)
        for i, p in enumerate(add_questions):
            p.i_question = cq[i].index
        for i, p in enumerate(add_targets):
            p.i_target = ct[i].index
        return err

    def remove_questions(self, question_ids: List[int], throw: bool = True) -> Optional[PqaError]:
        arr = (ctypes.c_int64 * max(len(question_ids), 1))(*question_ids)
        return _check(_lib.PqaEngine_RemoveQuestions(self.c_engine, len(question_ids), arr), throw)

    def remove_targets(self, target_ids: List[int], throw: bool = True) -> Optional[PqaError]:
        arr = (ctypes.c_int64 * max(len(target_ids), 1))(*target_ids)
        return _check(_lib.PqaEngine_RemoveTargets(self.c_engine, len(target_ids), arr), throw)

    def compact(self) -> Tuple[List[int], List[int]]:
        n_q, n_t = ctypes.c_int64(), ctypes.c_int64()
        p_q, p_t = _pi64(), _pi64()
        _check(_lib.PqaEngine_Compact(self.c_engine, ctypes.byref(n_q), ctypes.byref(p_q), ctypes.byref(n_t),
                                      ctypes.byref(p_t)))
        try:
            return [p_q[i] for i in range(n_q.value)], [p_t[i] for i in range(n_t.value)]
        finally:
            _lib.CiReleaseCompaction(p_q)
            _lib.CiReleaseCompaction(p_t)

    # ---- Compact on a shard that a process of its own drives (include/PqaHipExt.h; probqa_amd/dist.py: compact) ------------------------
    def compact_plan(self) -> Tuple[int, int, List[Tuple[int, int]], bool]:
        """What a compaction would do, on the host alone: (questions afterwards, targets afterwards, the whole-question moves as
        (dst, src) pairs of GLOBAL ids, whether THIS shard would be left without a question)."""
        n_q, n_t, n_m, empty = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint8()
        p_m = _pi64()
        _check(_lib.PqaHip_CompactPlan(self.c_engine, ctypes.byref(n_q), ctypes.byref(n_t), ctypes.byref(n_m), ctypes.byref(p_m),
                                       ctypes.byref(empty)))
        try:
            return n_q.value, n_t.value, [(p_m[2 * i], p_m[2 * i + 1]) for i in range(n_m.value)], bool(empty.value)
        finally:
            _lib.CiReleaseCompaction(p_m)

    def question_block_slot_bytes(self) -> int:
        """Bytes of one slot of a block package: the K + 1 rows of a question at the pitch of the current number of targets."""
        return _lib.PqaHip_QuestionBlockSlotBytes(self.c_engine)

    def pack_question_blocks(self, questions: List[int], dst: int, flag: int = 0, flag_value: int = 0) -> None:
        """Enqueue (no synchronisation) the copy of those of the questions (GLOBAL ids) this engine holds into their slots of the
        package at device-visible address `dst`; `flag` (an address, 0 = none) receives `flag_value` once they are visible."""
        arr = (ctypes.c_int64 * max(len(questions), 1))(*questions)
        _check(_lib.PqaHip_PackQuestionBlocks(self.c_engine, len(questions), arr, ctypes.c_void_p(dst or None), ctypes.c_void_p(flag or None),
                                              flag_value))

    def compact_from_blocks(self, blocks: int = 0, slot_bytes: int = 0, emptied_rank: int = -1) -> Tuple[List[int], List[int]]:
        """compact() with the questions that move in from other shards read from the package at device-visible address `blocks` (slot i:
        the source of move i of compact_plan).  emptied_rank: the ranks' vote (-1: no shard would be left empty)."""
        n_q, n_t = ctypes.c_int64(), ctypes.c_int64()
        p_q, p_t = _pi64(), _pi64()
        _check(_lib.PqaEngine_CompactFromBlocks(self.c_engine, ctypes.c_void_p(blocks or None), slot_bytes, emptied_rank, ctypes.byref(n_q),
                                                ctypes.byref(p_q), ctypes.byref(n_t), ctypes.byref(p_t)))
        try:
            return [p_q[i] for i in range(n_q.value)], [p_t[i] for i in range(n_t.value)]
        finally:
            _lib.CiReleaseCompaction(p_q)
            _lib.CiReleaseCompaction(p_t)

    def shutdown(self, save_file_path: Optional[str] = None, throw: bool = True):
        p = save_file_path.encode() if save_file_path else None
        return _check(_lib.PqaEngine_Shutdown(self.c_engine, p), throw)

    def clear_old_quizzes(self, max_count: int, max_age_sec: float, throw: bool = True):
        return _check(_lib.PqaEngine_ClearOldQuizzes(self.c_engine, max_count, max_age_sec), throw)

    # ---- additive (include/PqaHipExt.h) -----------------------------------------------------------------------------
    def set_option(self, name: str, value: int):
        _check(_lib.PqaHip_SetOption(self.c_engine, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        return _lib.PqaHip_GetOption(self.c_engine, name.encode())

    def eval_kernel_name(self) -> str:
        return _lib.PqaHip_EvalKernelName(self.c_engine).decode()

    def set_kb(self, A: np.ndarray, D: np.ndarray, B: np.ndarray):
        A = np.ascontiguousarray(A, dtype=np.float64)
        D = np.ascontiguousarray(D, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        _check(_lib.PqaHip_SetKB(self.c_engine, _dptr(A), _dptr(D), _dptr(B)))

    def get_kb(self, n_local_questions: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        d = self.copy_dims()
        q = n_local_questions if n_local_questions is not None else d.n_questions
        A = np.empty((q, d.n_answers, d.n_targets)); D = np.empty((q, d.n_targets)); B = np.empty(d.n_targets)
        _check(_lib.PqaHip_GetKB(self.c_engine, _dptr(A), _dptr(D), _dptr(B)))
        return A, D, B

    def fill_synthetic(self, n_train: float, noise_amp: float, seed: int):
        _check(_lib.PqaHip_FillSynthetic(self.c_engine, n_train, noise_amp, seed))

    def set_target_gaps(self, targets: List[int]):
        arr = (ctypes.c_int64 * max(len(targets), 1))(*targets)
        _check(_lib.PqaHip_SetTargetGaps(self.c_engine, len(targets), arr))

    def set_question_gaps(self, questions: List[int]):
        arr = (ctypes.c_int64 * max(len(questions), 1))(*questions)
        _check(_lib.PqaHip_SetQuestionGaps(self.c_engine, len(questions), arr))

    def eval_priorities(self, i_quiz: int, n_local_questions: Optional[int] = None) -> np.ndarray:
        n = n_local_questions if n_local_questions is not None else self.copy_dims().n_questions
        out = np.empty(n, dtype=np.float64)
        _check(_lib.PqaEngine_EvalPriorities(self.c_engine, i_quiz, _dptr(out), n))
        return out

    def next_question_argmax(self, i_quiz: int) -> int:
        slot = _err_slot
        q = _lib.PqaEngine_NextQuestionArgmax(self.c_engine, slot.ref, i_quiz)
        if slot.err.value:
            _check(slot.err.value)
        return q

    def next_question_argmax_batch(self, quizzes) -> List[int]:
        """Argmax NextQuestion of several distinct quizzes with one launch; -1 for a quiz that has run out of questions."""
        n = len(quizzes)
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        out = (ctypes.c_int64 * max(n, 1))()
        _check(_lib.PqaEngine_NextQuestionArgmaxBatch(self.c_engine, n, qs, out))
        return list(out[:n])

    def next_question_sampled_batch(self, quizzes, rnds) -> List[int]:
        """The reference's selector for several distinct quizzes with one sweep and one selector launch: entry i is what
        next_question_sampled(quizzes[i], rnds[i]) selects; -1 for a quiz that has run out of questions."""
        n = len(quizzes)
        if len(rnds) != n:
            raise ValueError("one random number per quiz")
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        rs = (ctypes.c_uint64 * max(n, 1))(*[int(r) for r in rnds])
        out = (ctypes.c_int64 * max(n, 1))()
        _check(_lib.PqaEngine_NextQuestionSampledBatch(self.c_engine, n, qs, rs, out))
        return list(out[:n])

    def next_question_batch(self, quizzes) -> List[int]:
        """NextQuestion of several distinct quizzes in one call, by the engine's `select` option: the argmax batch, or the sampled
        batch with random numbers drawn from the engine's generator in batch order."""
        n = len(quizzes)
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        out = (ctypes.c_int64 * max(n, 1))()
        _check(_lib.PqaEngine_NextQuestionBatch(self.c_engine, n, qs, out))
        return list(out[:n])

    def select_argmax_batch(self, quizzes) -> np.ndarray:
        """This engine's (shard's) winners of a batch: array [n, 2] of (priority, GLOBAL question index or -1)."""
        n = len(quizzes)
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        out = (CiHipSelection * max(n, 1))()
        _check(_lib.PqaHip_SelectArgmaxBatch(self.c_engine, n, qs, out))
        return np.array([(out[i].priority, out[i].iQuestion) for i in range(n)], dtype=np.float64).reshape(n, 2)

    # ---- the Among calls: evaluate and select over a listed set of questions per quiz (GLOBAL ids; for the call, every question
    # outside a quiz's list counts as asked)
    @staticmethod
    def _among_args(quizzes, lists):
        n = len(quizzes)
        if len(lists) != n:
            raise ValueError("one list of question ids per quiz")
        flat = [int(q) for ids in lists for q in ids]
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        counts = (ctypes.c_int64 * max(n, 1))(*[len(ids) for ids in lists])
        ids = (ctypes.c_int64 * max(len(flat), 1))(*flat)
        return n, qs, counts, ids, len(flat)

    def eval_priorities_among_batch(self, quizzes, lists) -> List[np.ndarray]:
        """The priorities of every quiz's listed questions from one launch over the (quiz, question) pairs: entry i is parallel to
        lists[i]; 0 for a gap, an asked question, or a question another process's shard holds."""
        n, qs, counts, ids, total = self._among_args(quizzes, lists)
        out = np.zeros(max(total, 1), dtype=np.float64)
        _check(_lib.PqaEngine_EvalPrioritiesAmongBatch(self.c_engine, n, qs, counts, ids, _dptr(out)))
        ends = np.cumsum([len(x) for x in lists]) if n else []
        return [out[e - len(x):e].copy() for e, x in zip(ends, lists)]

    def select_argmax_among_batch(self, quizzes, lists) -> np.ndarray:
        """This engine's (shard's) winners among the lists: array [n, 2] of (priority, GLOBAL question id or -1); no bookkeeping."""
        n, qs, counts, ids, _ = self._among_args(quizzes, lists)
        out = (CiHipSelection * max(n, 1))()
        _check(_lib.PqaHip_SelectArgmaxAmongBatch(self.c_engine, n, qs, counts, ids, out))
        return np.array([(out[i].priority, out[i].iQuestion) for i in range(n)], dtype=np.float64).reshape(n, 2)

    def next_question_argmax_among_batch(self, quizzes, lists) -> List[int]:
        """Argmax NextQuestion of several distinct quizzes, each among its list; -1 for a quiz whose list holds no eligible question."""
        n, qs, counts, ids, _ = self._among_args(quizzes, lists)
        out = (ctypes.c_int64 * max(n, 1))()
        _check(_lib.PqaEngine_NextQuestionArgmaxAmongBatch(self.c_engine, n, qs, counts, ids, out))
        return list(out[:n])

    def next_question_sampled_among_batch(self, quizzes, rnds, lists) -> List[int]:
        """The reference's selector for several distinct quizzes, each among its list (skip bits: gaps | asked | not listed)."""
        n, qs, counts, ids, _ = self._among_args(quizzes, lists)
        if len(rnds) != n:
            raise ValueError("one random number per quiz")
        rs = (ctypes.c_uint64 * max(n, 1))(*[int(r) for r in rnds])
        out = (ctypes.c_int64 * max(n, 1))()
        _check(_lib.PqaEngine_NextQuestionSampledAmongBatch(self.c_engine, n, qs, counts, ids, rs, out))
        return list(out[:n])

    def next_question_among_batch(self, quizzes, lists) -> List[int]:
        """NextQuestion of several distinct quizzes, each among its list, by the engine's `select` option."""
        n, qs, counts, ids, _ = self._among_args(quizzes, lists)
        out = (ctypes.c_int64 * max(n, 1))()
        _check(_lib.PqaEngine_NextQuestionAmongBatch(self.c_engine, n, qs, counts, ids, out))
        return list(out[:n])

    def next_question_argmax_among(self, i_quiz: int, ids) -> int:
        return self.next_question_argmax_among_batch([i_quiz], [list(ids)])[0]

    def next_question_sampled_among(self, i_quiz: int, rnd: int, ids) -> int:
        return self.next_question_sampled_among_batch([i_quiz], [rnd], [list(ids)])[0]

    def eval_priorities_among(self, i_quiz: int, ids) -> np.ndarray:
        return self.eval_priorities_among_batch([i_quiz], [list(ids)])[0]

    def eval_priorities_batch(self, quizzes, n_local_questions: Optional[int] = None) -> np.ndarray:
        """Priority vectors [len(quizzes), Q] of several distinct quizzes from one sweep that reads the cube once."""
        n = len(quizzes)
        nq = n_local_questions if n_local_questions is not None else self.copy_dims().n_questions
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        out = np.zeros((n, nq), dtype=np.float64)
        _check(_lib.PqaEngine_EvalPrioritiesBatch(self.c_engine, n, qs, _dptr(out)))
        return out

    def enqueue_select_argmax_flag(self, i_quiz: int, out_dev: int, flag_dev: int, flag_value: int) -> None:
        _check(_lib.PqaHip_EnqueueSelectArgmaxFlag(self.c_engine, i_quiz, ctypes.c_void_p(out_dev),
                                                   ctypes.c_void_p(flag_dev), flag_value))

    def select_through_slots(self, i_quiz: int, slots_host: int, slots_dev: int, rank: int, world: int, stride: int,
                             flag_value: int, timeout_s: float = 30.0):
        """One step of the shared-memory exchange (enqueue_select_argmax_flag + pick_when_all) -> (priority, index)."""
        pri, idx = ctypes.c_double(), ctypes.c_int64()
        _check(_lib.PqaHip_SelectThroughSlots(self.c_engine, i_quiz, ctypes.c_void_p(slots_host), ctypes.c_void_p(slots_dev),
                                              rank, world, stride, flag_value, timeout_s, ctypes.byref(pri), ctypes.byref(idx)))
        return pri.value, idx.value

    def select_argmax_rccl(self, i_quiz: int, nccl_comm: int, world: int):
        """This shard's winner all-gathered over the caller's RCCL communicator (an ncclComm_t as an integer) -> (priority, index)."""
        pri, idx = ctypes.c_double(), ctypes.c_int64()
        _check(_lib.PqaHip_SelectArgmaxRccl(self.c_engine, i_quiz, ctypes.c_void_p(nccl_comm), world, ctypes.byref(pri), ctypes.byref(idx)))
        return pri.value, idx.value

    def log2hot(self, x: np.ndarray) -> np.ndarray:
        """The device's Log2Hot over an array (the per-element function of the sweep)."""
        xin = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(xin)
        _check(_lib.PqaHip_Log2Hot(self.c_engine, _dptr(xin), _dptr(out), xin.size))
        return out

    def next_question_sampled(self, i_quiz: int, rnd: int) -> int:
        c_err = ctypes.c_void_p()
        q = _lib.PqaEngine_NextQuestionSampled(self.c_engine, ctypes.byref(c_err), i_quiz, rnd)
        _check(c_err.value)
        return q

    def get_priors(self, i_quiz: int) -> np.ndarray:
        out = np.empty(self.copy_dims().n_targets, dtype=np.float64)
        _check(_lib.PqaHip_GetPriors(self.c_engine, i_quiz, _dptr(out), out.size))
        return out

    def get_stream(self) -> int:
        return _lib.PqaHip_GetStream(self.c_engine) or 0

    def set_stream(self, stream: int):
        _check(_lib.PqaHip_SetStream(self.c_engine, ctypes.c_void_p(stream)))

    def synchronize(self):
        _check(_lib.PqaHip_Synchronize(self.c_engine))

    def quiesce(self):
        """Everything this engine put on the device has finished; a resident sweep kernel stays (include/PqaHipExt.h)."""
        _check(_lib.PqaHip_Quiesce(self.c_engine))

    def enqueue_select_argmax(self, i_quiz: int, out_ptr: int = 0):
        _check(_lib.PqaHip_EnqueueSelectArgmax(self.c_engine, i_quiz, ctypes.c_void_p(out_ptr)))

    def enqueue_eval(self, i_quiz: int):
        _check(_lib.PqaHip_EnqueueEval(self.c_engine, i_quiz))

    def prior_device_ptr(self, i_quiz: int) -> Tuple[int, int]:
        dev = ctypes.c_void_p()
        ld = ctypes.c_int64()
        _check(_lib.PqaHip_GetPriorDevicePtr(self.c_engine, i_quiz, ctypes.byref(dev), ctypes.byref(ld)))
        return dev.value or 0, ld.value

    def record_answer_batch(self, quizzes, answers):
        """RecordAnswer of several quizzes (each with an active question) in one launch."""
        n = len(quizzes)
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        ans = (ctypes.c_int64 * max(n, 1))(*answers)
        _check(_lib.PqaEngine_RecordAnswerBatch(self.c_engine, n, qs, ans))

    def start_quiz_batch(self, n: int) -> List[int]:
        """n new quizzes, one launch for their priors."""
        out = (ctypes.c_int64 * max(n, 1))()
        _check(_lib.PqaEngine_StartQuizBatch(self.c_engine, n, out))
        return list(out[:n])

    def resume_quiz_batch(self, lists) -> List[int]:
        """ResumeQuiz for every list of answered questions in `lists`, one launch per chunk; all or none."""
        n = len(lists)
        counts = (ctypes.c_int64 * max(n, 1))(*[len(l) for l in lists])
        flat = [aq for l in lists for aq in l]
        arr, _ = self.to_c_answered_questions(flat)
        out = (ctypes.c_int64 * max(n, 1))()
        _check(_lib.PqaEngine_ResumeQuizBatch(self.c_engine, n, counts, arr, out))
        return list(out[:n])

    # ---- row packages: ResumeQuiz on a shard that a process of its own drives (include/PqaHipExt.h) ----------------------
    def answer_row_slot_bytes(self) -> int:
        """Bytes of one slot of a row package: the sA row and the mD row of one answered question, in the cube's element type."""
        return _lib.PqaHip_AnswerRowSlotBytes(self.c_engine)

    def pack_answer_rows(self, answered_questions: List[AnsweredQuestion], dst: int, flag: int = 0, flag_value: int = 0) -> None:
        """Enqueue (no synchronisation) the copy of the rows of those answered questions this engine holds into their slots of the
        package at device-visible address `dst`; `flag` (an address, 0 = none) receives `flag_value` once they are visible."""
        arr, n = self.to_c_answered_questions(answered_questions)
        _check(_lib.PqaHip_PackAnswerRows(self.c_engine, n, arr, ctypes.c_void_p(dst), ctypes.c_void_p(flag or None), flag_value))

    def resume_quiz_from_rows(self, answered_questions: List[AnsweredQuestion], rows: int) -> int:
        """resume_quiz with the rows of the questions other shards hold read from the package at device-visible address `rows`."""
        arr, n = self.to_c_answered_questions(answered_questions)
        c_err = ctypes.c_void_p()
        i_quiz = _lib.PqaEngine_ResumeQuizFromRows(self.c_engine, ctypes.byref(c_err), n, arr, ctypes.c_void_p(rows or None))
        _check(c_err.value)
        return i_quiz

    def resume_quiz_batch_from_rows(self, lists, rows: int) -> List[int]:
        """resume_quiz_batch likewise; the package's slots count through the answered questions of all lists, in order."""
        n = len(lists)
        counts = (ctypes.c_int64 * max(n, 1))(*[len(l) for l in lists])
        arr, _ = self.to_c_answered_questions([aq for l in lists for aq in l])
        out = (ctypes.c_int64 * max(n, 1))()
        _check(_lib.PqaEngine_ResumeQuizBatchFromRows(self.c_engine, n, counts, arr, ctypes.c_void_p(rows or None), out))
        return list(out[:n])

    # ---- a page of answers per quiz in one launch (include/PqaHipExt.h: PqaEngine_RecordAnswerPageBatch) ------------------
    def _record_pages(self, quizzes, pages, likelihoods: bool, rows: Optional[int]):
        quizzes, pages = list(quizzes), [list(p) for p in pages]
        if len(quizzes) != len(pages):
            raise ValueError("one page per quiz")
        n = len(quizzes)
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        counts = (ctypes.c_int64 * max(n, 1))(*[len(p) for p in pages])
        arr, total = self.to_c_answered_questions([aq for p in pages for aq in p])
        out = (ctypes.c_double * max(total, 1))() if likelihoods else None
        if rows is None:
            _check(_lib.PqaEngine_RecordAnswerPageBatch(self.c_engine, n, qs, counts, arr, out))
        else:
            _check(_lib.PqaEngine_RecordAnswerPageBatchFromRows(self.c_engine, n, qs, counts, arr, out, ctypes.c_void_p(rows or None)))
        if not likelihoods:
            return None
        res, at = [], 0
        for p in pages:
            res.append(list(out[at:at + len(p)]))
            at += len(p)
        return res

    def record_answer_page_batch(self, quizzes, pages, likelihoods: bool = False):
        """Quiz quizzes[i] receives the answers of pages[i] (a list of AnsweredQuestion, GLOBAL question ids; given as
        resume_quiz_batch takes its lists), in order, in one launch per 256 quizzes: what set_active_question + record_answer per
        answer leave, bit for bit.  All or none.  likelihoods: returns, per quiz, each step's total -- the predictive probability of
        the answer that was given -- instead of None."""
        return self._record_pages(quizzes, pages, likelihoods, None)

    def record_answer_page(self, i_quiz: int, page, likelihoods: bool = False):
        """record_answer_page_batch for one quiz: None, or the list of its steps' likelihoods."""
        res = self._record_pages([i_quiz], [page], likelihoods, None)
        return res[0] if likelihoods else None

    def record_answer_page_batch_from_rows(self, quizzes, pages, rows: int, likelihoods: bool = False):
        """record_answer_page_batch on a shard, with the rows of the questions other shards hold read from the package at
        device-visible address `rows`; its slots count through the answers of all pages, in order (pack_answer_rows)."""
        return self._record_pages(quizzes, pages, likelihoods, rows or 0)

    # ---- selection parts: the sampled selector on a shard that a process of its own drives (include/PqaHipExt.h) ----------
    def sampled_part_bytes(self) -> int:
        """Bytes of one selection part: a function of the whole question count and eval_subtasks alone."""
        return _lib.PqaHip_SampledPartBytes(self.c_engine)

    def pack_sampled_parts(self, quizzes, dst: int, flag: int = 0, flag_value: int = 0) -> None:
        """Enqueue (no synchronisation) the batched sweep for these distinct quizzes and the launch that writes part i to
        dst + i * sampled_part_bytes(), a device-visible 16-byte aligned address; `flag` (an address, 0 = none) receives
        `flag_value` once the parts are visible."""
        n = len(quizzes)
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        _check(_lib.PqaHip_PackSampledParts(self.c_engine, n, qs, ctypes.c_void_p(dst or None), ctypes.c_void_p(flag or None), flag_value))

    def sampled_pick_from_parts(self, quizzes, rnds, parts: int, rank: int, world: int) -> np.ndarray:
        """This rank's picks from the gathered parts (world x len(quizzes), rank-major, at device-visible address `parts`): array
        [n, 2] of (grand total, GLOBAL question or -1 where the chosen subtask lies whole on another rank)."""
        n = len(quizzes)
        if len(rnds) != n:
            raise ValueError("one random number per quiz")
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        rs = (ctypes.c_uint64 * max(n, 1))(*[int(r) for r in rnds])
        out = (CiHipSelection * max(n, 1))()
        _check(_lib.PqaHip_SampledPickFromParts(self.c_engine, n, qs, rs, ctypes.c_void_p(parts or None), rank, world, out))
        return np.array([(out[i].priority, out[i].iQuestion) for i in range(n)], dtype=np.float64).reshape(n, 2)

    def take_sampled_picks(self, quizzes, picks) -> List[int]:
        """The agreed GLOBAL picks become the quizzes' active questions (host only): the reference's fallback over the whole
        question axis for a pick that is a gap or was asked, one question asked counted per quiz; -1 for a quiz with none left."""
        n = len(quizzes)
        if len(picks) != n:
            raise ValueError("one pick per quiz")
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        ps = (ctypes.c_int64 * max(n, 1))(*[int(p) for p in picks])
        out = (ctypes.c_int64 * max(n, 1))()
        _check(_lib.PqaEngine_TakeSampledPicks(self.c_engine, n, qs, ps, out))
        return list(out[:n])

    # ---- posterior packages: RecordAnswer for many quizzes on a shard that a process of its own drives (include/PqaHipExt.h) ----
    def posterior_slot_bytes(self) -> int:
        """Bytes of one slot of a posterior package: a function of the target count alone."""
        return _lib.PqaHip_PosteriorSlotBytes(self.c_engine)

    def pack_answer_posteriors(self, quizzes, answers, dst: int, flag: int = 0, flag_value: int = 0) -> None:
        """Enqueue (no synchronisation, no change of any quiz) the posteriors that answers[i] to the active question of quizzes[i]
        would leave, for the quizzes whose active question this engine holds, into their slots of the package at device-visible
        16-byte aligned address `dst`; `flag` (an address, 0 = none) receives `flag_value` once they are visible."""
        n = len(quizzes)
        if len(answers) != n:
            raise ValueError("one answer per quiz")
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        ans = (ctypes.c_int64 * max(n, 1))(*answers)
        _check(_lib.PqaHip_PackAnswerPosteriors(self.c_engine, n, qs, ans, ctypes.c_void_p(dst or None), ctypes.c_void_p(flag or None), flag_value))

    def record_answer_batch_from_posteriors(self, quizzes, answers, posteriors: int) -> None:
        """RecordAnswer's bookkeeping for the batch of this engine's latest pack_answer_posteriors, every quiz's posterior taken
        from its slot of the combined package at device-visible address `posteriors`."""
        n = len(quizzes)
        if len(answers) != n:
            raise ValueError("one answer per quiz")
        qs = (ctypes.c_int64 * max(n, 1))(*quizzes)
        ans = (ctypes.c_int64 * max(n, 1))(*answers)
        _check(_lib.PqaEngine_RecordAnswerBatchFromPosteriors(self.c_engine, n, qs, ans, ctypes.c_void_p(posteriors or None)))

    def train_batch(self, records, throw: bool = True) -> Optional[PqaError]:
        """Train for every (answered_questions, i_target, amount) of `records` in one call: the KB consecutive `train` calls
        would leave; all or none."""
        counts = np.array([len(r[0]) for r in records], dtype=np.int64)
        aqs = np.array([(aq.i_question, aq.i_answer) for r in records for aq in r[0]], dtype=np.int64).reshape(-1, 2)
        targets = np.array([r[1] for r in records], dtype=np.int64)
        amounts = np.array([r[2] for r in records], dtype=np.float64)
        return self.train_batch_arrays(counts, aqs, targets, amounts, throw)

    def train_batch_arrays(self, counts, aqs, targets, amounts, throw: bool = True) -> Optional[PqaError]:
        """train_batch over numpy arrays: counts, targets int64 [n], amounts float64 [n], aqs int64 [sum(counts), 2] of
        (question, answer) -- no Python object per record."""
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        targets = np.ascontiguousarray(targets, dtype=np.int64)
        amounts = np.ascontiguousarray(amounts, dtype=np.float64)
        aqs = np.ascontiguousarray(aqs, dtype=np.int64).reshape(-1, 2)
        n = len(counts)
        if len(targets) != n or len(amounts) != n:
            raise ValueError("counts, targets and amounts must have the same length")
        p_aqs = aqs.ctypes.data_as(_pAQ) if aqs.shape[0] > 0 else None
        return _check(_lib.PqaEngine_TrainBatch(self.c_engine, n, counts.ctypes.data_as(_pi64), p_aqs, targets.ctypes.data_as(_pi64),
                                                amounts.ctypes.data_as(_pdbl)), throw)

    def record_quiz_target_batch(self, quizzes, targets, amounts, throw: bool = True) -> Optional[PqaError]:
        """RecordQuizTarget for every (quizzes[i], targets[i], amounts[i]) in one call; all or none."""
        quizzes = np.ascontiguousarray(quizzes, dtype=np.int64)
        targets = np.ascontiguousarray(targets, dtype=np.int64)
        amounts = np.ascontiguousarray(amounts, dtype=np.float64)
        n = len(quizzes)
        if len(targets) != n or len(amounts) != n:
            raise ValueError("quizzes, targets and amounts must have the same length")
        return _check(_lib.PqaEngine_RecordQuizTargetBatch(self.c_engine, n, quizzes.ctypes.data_as(_pi64), targets.ctypes.data_as(_pi64),
                                                           amounts.ctypes.data_as(_pdbl)), throw)

    # ---- the batched listings: one decoder of their records, one caller of their entries ------------------------------------------
    @staticmethod
    def _records(arr, counts, n: int, max_count: int, make_record) -> list:
        """Entry i's counts[i] records, from arr[i * max_count] on, each as make_record(id, value)."""
        rec = np.frombuffer(arr, dtype=_RECORD)
        return [[make_record(k, v) for k, v in zip(r["id"].tolist(), r["value"].tolist())]
                for r in (rec[i * max_count:i * max_count + int(counts[i])] for i in range(n))]

    def _list_batch(self, entry, record_type, make_record, ids, max_count: int, *package) -> list:
        """entry(engine, n, ids, [package,] max_count, records, counts) for the quizzes or sources `ids` -> their n listings."""
        src = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        n = len(src)
        counts = np.zeros(max(n, 1), dtype=np.int64)
        arr = (record_type * max(n * max_count, 1))()
        _check(entry(self.c_engine, n, src.ctypes.data_as(_pi64), *package, max_count, arr, counts.ctypes.data_as(_pi64)))
        return self._records(arr, counts, n, max_count, make_record)

    def list_top_targets_batch(self, quizzes, max_count: int) -> List[List[RatedTarget]]:
        """ListTopTargets of several quizzes with one launch sequence; no posterior leaves the device."""
        return self._list_batch(_lib.PqaEngine_ListTopTargetsBatch, CiRatedTarget, RatedTarget, quizzes, max_count)

    def list_top_targets_among_batch(self, quizzes, lists, max_count: int, list_of=None) -> Tuple[List[List[RatedTarget]], List[float]]:
        """The best targets of several quizzes (a quiz may repeat) WITHIN LISTED SETS of targets, and the posterior's total over each
        quiz's set: quiz i takes lists[list_of[i]], or lists[i] without list_of.  Probability descending, target id ascending among
        equal probabilities, whatever a list's order; the probabilities are the posterior's own, nothing is renormalised -- divide by
        the mass to do so.  The cost follows the lists, not the number of targets."""
        n = len(quizzes)
        qs = np.ascontiguousarray(quizzes, dtype=np.int64)
        lens = np.array([len(x) for x in lists], dtype=np.int64)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if len(lists) and lens.sum() else np.zeros(1), dtype=np.int64)
        lof = None if list_of is None else np.ascontiguousarray(list_of, dtype=np.int64)
        if lof is not None and len(lof) != n:
            raise ValueError("one list index per quiz")
        counts = np.zeros(max(n, 1), dtype=np.int64)
        mass = np.zeros(max(n, 1), dtype=np.float64)
        arr = (CiRatedTarget * max(n * max_count, 1))()
        _check(_lib.PqaEngine_ListTopTargetsAmongBatch(self.c_engine, n, qs.ctypes.data_as(_pi64), None if lof is None else lof.ctypes.data_as(_pi64), len(lists),
                                                       lens.ctypes.data_as(_pi64), ids.ctypes.data_as(_pi64), max_count, arr, counts.ctypes.data_as(_pi64),
                                                       mass.ctypes.data_as(_pdbl)))
        return self._records(arr, counts, n, max_count, RatedTarget), [float(m) for m in mass[:n]]

    def list_top_targets_among(self, i_quiz: int, targets, max_count: int) -> Tuple[List[RatedTarget], float]:
        got, mass = self.list_top_targets_among_batch([i_quiz], [list(targets)], max_count)
        return got[0], mass[0]

    # ---- what each answer would do to a quiz (include/PqaHipExt.h: PqaEngine_PreviewAnswersBatch) ----
    def preview_answers_batch(self, pairs, max_count: int) -> List[List[AnswerPreview]]:
        """For every (quiz, GLOBAL question) of `pairs`, per answer k what recording k would leave: the answer's likelihood, the
        entropy of the would-be posterior in bits and its best max_count (<= 256) targets -- RecordAnswer's own bits, probability
        descending, target id ascending among equals.  Read-only: no quiz changes.  A quiz may appear in several pairs.  On a shard
        engine the pairs whose question another rank holds come back as zeros (dist.preview_answers_batch merges the ranks)."""
        pr = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        n, k = len(pr), self.copy_dims().n_answers
        quizzes, questions = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        rows = max(n * k, 1)
        likelihood, entropy = np.zeros(rows, dtype=np.float64), np.zeros(rows, dtype=np.float64)
        counts = np.zeros(rows, dtype=np.int64)
        arr = (CiRatedTarget * max(n * k * max_count, 1))()
        _check(_lib.PqaEngine_PreviewAnswersBatch(self.c_engine, n, quizzes.ctypes.data_as(_pi64), questions.ctypes.data_as(_pi64), max_count,
                                                  likelihood.ctypes.data_as(_pdbl), entropy.ctypes.data_as(_pdbl), arr, counts.ctypes.data_as(_pi64)))
        targets = self._records(arr, counts, n * k, max_count, RatedTarget)
        return [[AnswerPreview(float(likelihood[r]), float(entropy[r]), targets[r]) for r in range(i * k, (i + 1) * k)] for i in range(n)]

    def preview_answers(self, i_quiz: int, i_question: int, max_count: int) -> List[AnswerPreview]:
        return self.preview_answers_batch([(i_quiz, i_question)], max_count)[0]

    # ---- where a quiz stands (include/PqaHipExt.h: PqaEngine_QuizStatusBatch, PqaEngine_RankTargetsBatch) ----
    def quiz_status_batch(self, quizzes, levels=()) -> List[QuizStatus]:
        """Per quiz (a quiz may repeat) the entropy of its posterior in bits -- the bits preview_answers_batch promised for it --, its
        mass, its best target, the number of candidates (targets that are no gaps with p > 0) and, per level (at most 16, shared by
        the call), the number and the mass of the candidates with p >= level.  Read-only: no quiz changes, no posterior leaves the
        device.  What a stopping rule needs, and the H_now of a question's gain H_now - sum_k likelihood_k * H_k."""
        qs = np.ascontiguousarray(quizzes, dtype=np.int64).reshape(-1)
        lv = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
        n, m = len(qs), len(lv)
        status = (CiHipQuizStatus * max(n, 1))()
        counts = np.zeros(max(n * m, 1), dtype=np.int64)
        mass = np.zeros(max(n * m, 1), dtype=np.float64)
        _check(_lib.PqaEngine_QuizStatusBatch(self.c_engine, n, qs.ctypes.data_as(_pi64), m, lv.ctypes.data_as(_pdbl) if m else None, status,
                                              counts.ctypes.data_as(_pi64), mass.ctypes.data_as(_pdbl)))
        return [QuizStatus(status[i].entropy, status[i].mass, status[i].topProb, status[i].iTopTarget, status[i].nCandidates,
                           [int(c) for c in counts[i * m:(i + 1) * m]], [float(x) for x in mass[i * m:(i + 1) * m]]) for i in range(n)]

    def quiz_status(self, i_quiz: int, levels=()) -> QuizStatus:
        return self.quiz_status_batch([i_quiz], levels)[0]

    def rank_targets_batch(self, pairs) -> List[Tuple[int, float]]:
        """For every (quiz, target) of `pairs` (rank, prob): the number of candidates that come before the target by probability
        descending, target id ascending among equals -- its index in list_top_targets_among and in the fast listing -- or -1 for a
        gap or a probability that is not > 0, and the posterior's own value at the target.  Read-only: no quiz changes."""
        pr = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        n = len(pr)
        quizzes, targets = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        prob = np.zeros(max(n, 1), dtype=np.float64)
        rank = np.zeros(max(n, 1), dtype=np.int64)
        _check(_lib.PqaEngine_RankTargetsBatch(self.c_engine, n, quizzes.ctypes.data_as(_pi64), targets.ctypes.data_as(_pi64), prob.ctypes.data_as(_pdbl),
                                               rank.ctypes.data_as(_pi64)))
        return [(int(rank[i]), float(prob[i])) for i in range(n)]

    def rank_target(self, i_quiz: int, i_target: int) -> Tuple[int, float]:
        return self.rank_targets_batch([(i_quiz, i_target)])[0]

    # ---- a quiz with each of its answers left out (include/PqaHipExt.h: PqaHip_GetQuizAnswers, PqaEngine_ReviewAnswersBatch) ----
    def get_quiz_answers(self, i_quiz: int) -> List[AnsweredQuestion]:
        """The answers the quiz holds, in the order RecordQuizTarget would train them, with GLOBAL question ids."""
        c_err = ctypes.c_void_p()
        n = _lib.PqaHip_GetQuizAnswers(self.c_engine, ctypes.byref(c_err), i_quiz, None, 0)
        _check(c_err.value)
        arr = (CiAnsweredQuestion * max(n, 1))()
        n = min(n, _lib.PqaHip_GetQuizAnswers(self.c_engine, ctypes.byref(c_err), i_quiz, arr, n))
        _check(c_err.value)
        return [AnsweredQuestion(arr[i].iQuestion, arr[i].iAnswer) for i in range(n)]

    def review_answers_batch(self, pairs, max_count: int) -> List[AnswerPreview]:
        """For every (quiz, position) of `pairs` the quiz as if the answer at that position had never been given: the left-out
        answer's likelihood under the posterior of the others, that posterior's entropy in bits and its best max_count (<= 256)
        targets -- ResumeQuiz's own bits over the remaining answers.  Read-only: no quiz changes.  A dead row has NaN for both numbers
        and no targets."""
        return self.review_answers_batch_from_rows(pairs, max_count, None, None)

    def review_answers(self, i_quiz: int, max_count: int) -> List[AnswerPreview]:
        """review_answers_batch for every position of one quiz."""
        return self.review_answers_batch([(i_quiz, i) for i in range(len(self.get_quiz_answers(i_quiz)))], max_count)

    def review_answers_batch_from_rows(self, pairs, max_count: int, rows, row_first) -> List[AnswerPreview]:
        """review_answers_batch on a shard that a process of its own drives: pair i's quiz has its answers' rows in slots
        row_first[i] ... of the package at device-visible address `rows` (pack_answer_rows).  row_first None: the plain call."""
        pr = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        n = len(pr)
        quizzes, positions = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        likelihood, entropy = np.zeros(max(n, 1), dtype=np.float64), np.zeros(max(n, 1), dtype=np.float64)
        counts = np.zeros(max(n, 1), dtype=np.int64)
        arr = (CiRatedTarget * max(n * max_count, 1))()
        head = (self.c_engine, n, quizzes.ctypes.data_as(_pi64), positions.ctypes.data_as(_pi64), max_count, likelihood.ctypes.data_as(_pdbl),
                entropy.ctypes.data_as(_pdbl), arr, counts.ctypes.data_as(_pi64))
        if row_first is None:
            _check(_lib.PqaEngine_ReviewAnswersBatch(*head))
        else:
            first = np.ascontiguousarray(row_first, dtype=np.int64).reshape(-1)
            if len(first) != n:
                raise ValueError("row_first names %d pairs, the call has %d" % (len(first), n))
            _check(_lib.PqaEngine_ReviewAnswersBatchFromRows(*head, ctypes.c_void_p(rows or None), first.ctypes.data_as(_pi64)))
        targets = self._records(arr, counts, n, max_count, RatedTarget)
        return [AnswerPreview(float(likelihood[i]), float(entropy[i]), targets[i]) for i in range(n)]

    # ---- targets that answer like a given one (include/PqaHipExt.h: PqaEngine_EvalTargetSimilarity and its neighbours) ----
    def eval_target_similarity(self, sources) -> np.ndarray:
        """sim(sources[i], t) for every target t as an [S, T] array: the mean over the questions that are not gaps of
        sum_k sqrt(p_qk(s) p_qk(t)) -- 1 for targets no quiz can tell apart, 0 at gaps.  Reads only the knowledge base: regular
        and maintenance mode."""
        src = np.ascontiguousarray(sources, dtype=np.int64).reshape(-1)
        t = self.copy_dims().n_targets
        out = np.zeros((len(src), t), dtype=np.float64)
        _check(_lib.PqaEngine_EvalTargetSimilarity(self.c_engine, len(src), src.ctypes.data_as(_pi64), _dptr(out), t))
        return out

    def list_similar_targets_batch(self, sources, max_count: int) -> List[List[RatedTarget]]:
        """Per source the targets most like it, the source itself and the gaps left out: similarity descending, target id
        ascending among equal values; the values are eval_target_similarity's bits.  Any number of sources, ids may repeat."""
        return self._list_batch(_lib.PqaEngine_ListSimilarTargetsBatch, CiRatedTarget, RatedTarget, sources, max_count)

    def list_similar_targets(self, source: int, max_count: int) -> List[RatedTarget]:
        return self.list_similar_targets_batch([source], max_count)[0]

    def pack_target_similarity_sums(self, sources, ptr: int, flag_ptr: int = 0, flag_value: int = 0) -> None:
        """Enqueue (no synchronisation) this engine's part of the similarity of up to 256 sources -- the sums over the questions
        it holds -- into the package at device-visible 16-byte aligned address `ptr`, slots at posterior_slot_bytes(); the
        ranks' packages are summed.  `flag_ptr` (an address, 0 = none) receives `flag_value` once the slots are visible."""
        src = np.ascontiguousarray(sources, dtype=np.int64).reshape(-1)
        _check(_lib.PqaHip_PackTargetSimilaritySums(self.c_engine, len(src), src.ctypes.data_as(_pi64), ctypes.c_void_p(ptr or None),
                                                    ctypes.c_void_p(flag_ptr or None), flag_value))

    def list_similar_targets_from_sums(self, sources, ptr: int, max_count: int) -> List[List[RatedTarget]]:
        """list_similar_targets_batch from the summed package at device-visible address `ptr`."""
        return self._list_batch(_lib.PqaEngine_ListSimilarTargetsFromSums, CiRatedTarget, RatedTarget, sources, max_count, ctypes.c_void_p(ptr or None))

    # ---- questions whose answers a given one predicts (include/PqaHipExt.h: PqaEngine_EvalQuestionRedundancy and its neighbours) ----
    def eval_question_redundancy(self, sources) -> np.ndarray:
        """I(sources[i], q) for every question q as an [S, Q] array: the mutual information in bits between the answers to the two
        questions for a target drawn from the prior -- 0 for independent questions and at gaps, the same for a question and its
        negation.  Reads only the knowledge base: regular and maintenance mode."""
        src = np.ascontiguousarray(sources, dtype=np.int64).reshape(-1)
        q = self.copy_dims().n_questions
        out = np.zeros((len(src), q), dtype=np.float64)
        _check(_lib.PqaEngine_EvalQuestionRedundancy(self.c_engine, len(src), src.ctypes.data_as(_pi64), _dptr(out), q))
        return out

    def list_redundant_questions_batch(self, sources, max_count: int) -> List[List[Tuple[int, float]]]:
        """Per source the questions whose answers it predicts best as (question, bits), the source itself and the gaps left out: bits
        descending, question id ascending among equal values; the values are eval_question_redundancy's bits.  Any number of
        sources, ids may repeat."""
        return self._list_batch(_lib.PqaEngine_ListRedundantQuestionsBatch, CiRatedQuestion, _pair, sources, max_count)

    def list_redundant_questions(self, source: int, max_count: int) -> List[Tuple[int, float]]:
        return self.list_redundant_questions_batch([source], max_count)[0]

    def question_weight_slot_bytes(self) -> int:
        """Bytes of a slot of a question-weight package: nAnswers rows of RoundLdT(nTargets) doubles; the same on every rank."""
        return _lib.PqaHip_QuestionWeightSlotBytes(self.c_engine)

    def pack_question_weights(self, sources, ptr: int, flag_ptr: int = 0, flag_value: int = 0) -> None:
        """Enqueue (no synchronisation) the weighted answer rows of those of up to 256 sources (GLOBAL ids) that this engine holds
        into the package at device-visible 16-byte aligned address `ptr`, slots of question_weight_slot_bytes(); the slots of
        other ranks' sources are not touched, and the ranks' zero-filled packages are summed.  `flag_ptr` (an address, 0 = none)
        receives `flag_value` once the slots are visible."""
        src = np.ascontiguousarray(sources, dtype=np.int64).reshape(-1)
        _check(_lib.PqaHip_PackQuestionWeights(self.c_engine, len(src), src.ctypes.data_as(_pi64), ctypes.c_void_p(ptr or None),
                                               ctypes.c_void_p(flag_ptr or None), flag_value))

    def eval_question_redundancy_from_weights(self, sources, ptr: int, n_local_questions: Optional[int] = None) -> np.ndarray:
        """eval_question_redundancy over the questions THIS engine holds from the summed package at device-visible address `ptr`:
        an [S, local questions] array, column j question q_first + j (a shard: give n_local_questions, as for eval_priorities)."""
        src = np.ascontiguousarray(sources, dtype=np.int64).reshape(-1)
        q = n_local_questions if n_local_questions is not None else self.copy_dims().n_questions
        out = np.zeros((len(src), q), dtype=np.float64)
        _check(_lib.PqaEngine_EvalQuestionRedundancyFromWeights(self.c_engine, len(src), src.ctypes.data_as(_pi64), ctypes.c_void_p(ptr or None), _dptr(out), q))
        return out

    def list_redundant_questions_from_weights(self, sources, ptr: int, max_count: int) -> List[List[Tuple[int, float]]]:
        """list_redundant_questions_batch over the questions THIS engine holds from the summed package at device-visible address
        `ptr`; GLOBAL ids.  The ranks' lists are merged by dist.merge_top_questions."""
        return self._list_batch(_lib.PqaEngine_ListRedundantQuestionsFromWeights, CiRatedQuestion, _pair, sources, max_count, ctypes.c_void_p(ptr or None))

    # ---- questions that tell listed targets apart (include/PqaHipExt.h: PqaEngine_EvalTargetSeparation and its neighbour) ----
    @staticmethod
    def _groups(groups) -> Tuple[np.ndarray, np.ndarray]:
        """(counts, targets one group after another) of a list of groups of targets, as the separation calls take them"""
        lens = np.array([len(g) for g in groups], dtype=np.int64)
        flat = np.concatenate([np.asarray(g, dtype=np.int64).reshape(-1) for g in groups]) if len(groups) and lens.sum() else np.zeros(0, dtype=np.int64)
        return np.ascontiguousarray(np.append(lens, 0)), np.ascontiguousarray(np.append(flat, 0))   # (never empty: a pointer to pass)

    def eval_target_separation(self, groups) -> np.ndarray:
        """sep(groups[g], q) for every question q THIS engine holds as a [G, local questions] array (column j: question q_first + j): the
        Jensen-Shannon divergence in bits of the answer distributions of the group's 2 .. 64 targets (a repeated id counts twice) under
        equal weights -- 0 where they answer alike and at gaps, log2 n where no two share an answer; a row of zeros for a group with a
        gap member.  Reads only the knowledge base: regular and maintenance mode, whole engines and shards."""
        counts, targets = self._groups(groups)
        q = self.get_option("local_questions")
        out = np.zeros((len(groups), q), dtype=np.float64)
        _check(_lib.PqaEngine_EvalTargetSeparation(self.c_engine, len(groups), counts.ctypes.data_as(_pi64), targets.ctypes.data_as(_pi64), _dptr(out), q))
        return out

    def list_separating_questions_batch(self, groups, max_count: int) -> List[List[Tuple[int, float]]]:
        """Per group the questions THIS engine holds that tell its targets apart best as (question, bits), the gaps and what separates
        nothing left out: bits descending, question id ascending among equal values; GLOBAL ids; the values are
        eval_target_separation's bits.  Any number of groups."""
        counts, targets = self._groups(groups)
        return self._list_batch(_lib.PqaEngine_ListSeparatingQuestionsBatch, CiRatedQuestion, _pair, counts[:-1], max_count, targets.ctypes.data_as(_pi64))

    def list_separating_questions(self, targets, max_count: int) -> List[Tuple[int, float]]:
        return self.list_separating_questions_batch([list(targets)], max_count)[0]

    # ---- what every question would tell a quiz (include/PqaHipExt.h: PqaEngine_EvalQuestionGainsBatch and its neighbour) ----
    def eval_question_gains_batch(self, quizzes) -> np.ndarray:
        """gain(quizzes[i], q) for every question q THIS engine holds as an [n, local questions] array (column j: question q_first + j):
        the information gain in bits -- the mutual information between the answer to q and the target for a target drawn from the
        quiz's posterior.  0 at gaps and for a question every candidate answers alike, at most log2 nAnswers; an asked question is
        evaluated like any other.  Changes no quiz; regular mode; whole engines and shards.  A quiz may repeat."""
        qs = np.ascontiguousarray(quizzes, dtype=np.int64).reshape(-1)
        q = self.get_option("local_questions")
        out = np.zeros((len(qs), q), dtype=np.float64)
        _check(_lib.PqaEngine_EvalQuestionGainsBatch(self.c_engine, len(qs), qs.ctypes.data_as(_pi64), _dptr(out), q))
        return out

    def list_informative_questions_batch(self, quizzes, max_count: int) -> List[List[Tuple[int, float]]]:
        """Per quiz the questions THIS engine holds that would tell it most as (question, bits), the gaps, the quiz's asked questions and
        what gains nothing left out: bits descending, question id ascending among equal values; GLOBAL ids; the values are
        eval_question_gains_batch's bits.  Entry 0 is the most informative question: follow with set_active_question to ask it."""
        return self._list_batch(_lib.PqaEngine_ListInformativeQuestionsBatch, CiRatedQuestion, _pair, quizzes, max_count)

    def list_informative_questions(self, quiz: int, max_count: int) -> List[Tuple[int, float]]:
        return self.list_informative_questions_batch([quiz], max_count)[0]

    # ---- question pages (include/PqaHipExt.h: PqaEngine_EvalConditionalGainsBatch and its neighbour) ----
    @staticmethod
    def _given_sets(n: int, given):
        """(counts pointer, ids pointer, keep-alive) of the quizzes' given sets; None: every set is empty (two NULL pointers)"""
        if given is None:
            return None, None, ()
        assert len(given) == n, "one given set per quiz"
        counts, ids = PqaEngine._groups(given)
        return counts.ctypes.data_as(_pi64), ids.ctypes.data_as(_pi64), (counts, ids)

    def eval_conditional_gains_batch(self, quizzes, given=None) -> np.ndarray:
        """CG(q | given[i]) for every question q of the engine as an [n, questions] array: what q tells quizzes[i] about the target in
        bits once the answers to the questions of given[i] (GLOBAL ids, in listed order) are known -- the answer combinations of the
        set weighted by their probabilities under the quiz's posterior.  given=None or an empty set: eval_question_gains_batch's row
        bit for bit.  At most 256 answer combinations a quiz.  Changes no quiz; regular mode; whole engines."""
        qs = np.ascontiguousarray(quizzes, dtype=np.int64).reshape(-1)
        counts, ids, keep = self._given_sets(len(qs), given)
        q = self.get_option("local_questions")
        out = np.zeros((len(qs), q), dtype=np.float64)
        _check(_lib.PqaEngine_EvalConditionalGainsBatch(self.c_engine, len(qs), qs.ctypes.data_as(_pi64), counts, ids, _dptr(out), q))
        del keep
        return out

    def list_question_page_batch(self, quizzes, page_size: int, given=None) -> List[List[Tuple[int, float]]]:
        """Per quiz a page of up to page_size questions as (question, bits) in pick order, filled greedily: each step takes the question
        that tells most GIVEN the set so far (given[i], then the page's earlier picks) among those that are no gaps, not asked and
        not in the set; bits are eval_conditional_gains_batch's for that prefix, and they add up to the page's joint information.
        Changes no quiz: follow with set_active_question and record_answer per question the user answers."""
        qs = np.ascontiguousarray(quizzes, dtype=np.int64).reshape(-1)
        counts, ids, keep = self._given_sets(len(qs), given)
        out = self._list_batch(_lib.PqaEngine_ListQuestionPageBatch, CiRatedQuestion, _pair, qs, page_size, counts, ids)
        del keep
        return out

    def list_question_page(self, quiz: int, page_size: int, given=()) -> List[Tuple[int, float]]:
        return self.list_question_page_batch([quiz], page_size, [list(given)])[0]

    # ... and across shards that separate processes drive: the given questions' blocks travel as a block package (dist.py runs the exchange)
    def pack_given_blocks(self, questions: List[int], dst: int, flag: int = 0, flag_value: int = 0) -> None:
        """pack_question_blocks in REGULAR mode, for the given questions of the two calls below: enqueue (no synchronisation) the copy of
        those of the questions (GLOBAL ids) this engine holds into their slots (question_block_slot_bytes each) of the package at
        device-visible address `dst`; a gap is refused."""
        arr = (ctypes.c_int64 * max(len(questions), 1))(*questions)
        _check(_lib.PqaHip_PackGivenBlocks(self.c_engine, len(questions), arr, ctypes.c_void_p(dst or None), ctypes.c_void_p(flag or None), flag_value))

    def _block_args(self, quizzes, given, block_questions, blocks_ptr):
        qs = np.ascontiguousarray(quizzes, dtype=np.int64).reshape(-1)
        counts, ids, keep = self._given_sets(len(qs), given)
        named = np.ascontiguousarray(list(block_questions), dtype=np.int64).reshape(-1)
        slot = self.question_block_slot_bytes() if (len(named) or blocks_ptr) else 0
        args = (len(qs), qs.ctypes.data_as(_pi64), counts, ids, len(named), named.ctypes.data_as(_pi64) if len(named) else None, ctypes.c_void_p(blocks_ptr or None), slot)
        return qs, args, (keep, named)

    def eval_conditional_gains_batch_from_blocks(self, quizzes, given, block_questions=(), blocks_ptr: int = 0) -> np.ndarray:
        """eval_conditional_gains_batch for the questions THIS engine holds, as an [n, local questions] array: a given question the
        engine does not hold is read from the slot of the package at device-visible address `blocks_ptr` that block_questions (GLOBAL
        ids, distinct) names.  The whole engine's bits; whole engines and shards."""
        qs, args, keep = self._block_args(quizzes, given, block_questions, blocks_ptr)
        q = self.get_option("local_questions")
        out = np.zeros((len(qs), q), dtype=np.float64)
        _check(_lib.PqaEngine_EvalConditionalGainsBatchFromBlocks(self.c_engine, *args, _dptr(out), q))
        del keep
        return out

    def select_page_step_from_blocks(self, quizzes, given, block_questions=(), blocks_ptr: int = 0) -> np.ndarray:
        """One step of a page for the questions THIS engine holds: array [n, 2] of (bits, GLOBAL question id or -1) -- the question that
        tells quizzes[i] most given given[i] among those that are no gaps, not asked and not in the set; the bits are
        eval_conditional_gains_batch_from_blocks'.  dist.merge_page_step merges the ranks' records."""
        qs, args, keep = self._block_args(quizzes, given, block_questions, blocks_ptr)
        out = (CiHipSelection * max(len(qs), 1))()
        _check(_lib.PqaHip_SelectPageStepFromBlocks(self.c_engine, *args, out))
        del keep
        return np.array([(out[i].priority, out[i].iQuestion) for i in range(len(qs))], dtype=np.float64).reshape(len(qs), 2)

    def list_top_questions(self, i_quiz: int, max_count: int) -> List[Tuple[int, float]]:
        """The quiz's best next questions as (question, priority), by descending priority (ascending question among equal priorities):
        eval_priorities' values, listed on the device.  GLOBAL ids; changes no quiz state -- follow with set_active_question and
        record_answer to take one."""
        held = max(min(max_count, self.copy_dims().n_questions), 1)   # (an engine lists at most the questions there are)
        arr = (CiRatedQuestion * held)()
        c_err = ctypes.c_void_p()
        n = _lib.PqaEngine_ListTopQuestions(self.c_engine, ctypes.byref(c_err), i_quiz, max_count, arr)
        if c_err.value:
            _check(c_err.value)
        return [(arr[i].iQuestion, arr[i].priority) for i in range(n)]

    def list_top_questions_batch(self, quizzes, max_count: int) -> List[List[Tuple[int, float]]]:
        """list_top_questions of up to 256 distinct quizzes behind one batched sweep (eval_priorities_batch's values)."""
        return self._list_batch(_lib.PqaEngine_ListTopQuestionsBatch, CiRatedQuestion, _pair, quizzes, max_count)

    def record_answer_remote(self, i_quiz: int, i_answer: int):
        _check(_lib.PqaHip_RecordAnswerRemote(self.c_engine, i_quiz, i_answer))


class PqaEngineFactory:
    """Reference ProbQA.py:743-783."""

    def __init__(self):
        load_library()
        self.c_factory = ctypes.c_void_p(_lib.CiGetPqaEngineFactory())

    def create_cpu_engine(self, eng_def: EngineDefinition) -> Tuple[Optional[PqaEngine], Optional[PqaError]]:
        c_def = eng_def.to_c()
        c_err = ctypes.c_void_p()
        c_engine = _lib.PqaEngineFactory_CreateCpuEngine(self.c_factory, ctypes.byref(c_err), ctypes.byref(c_def))
        return (PqaEngine(c_engine) if c_engine else None), PqaError.factor(c_err.value)

    def create_hip_engine(self, eng_def: EngineDefinition, q_first: int = 0, q_total: Optional[int] = None,
                          device: int = -1) -> PqaEngine:
        c_def = eng_def.to_c()
        shard = CiHipShard(q_first, q_total if q_total is not None else eng_def.n_questions, device, 0)
        c_err = ctypes.c_void_p()
        c_engine = _lib.PqaEngineFactory_CreateHipEngineSharded(self.c_factory, ctypes.byref(c_err),
                                                                ctypes.byref(c_def), ctypes.byref(shard))
        _check(c_err.value)
        return PqaEngine(c_engine)

    def load_cpu_engine(self, file_path: str, mem_pool_max_bytes: int = EngineDefinition.DEFAULT_MEM_POOL_MAX_BYTES):
        c_err = ctypes.c_void_p()
        c_engine = _lib.PqaEngineFactory_LoadCpuEngine(self.c_factory, ctypes.byref(c_err), file_path.encode(),
                                                       mem_pool_max_bytes)
        return (PqaEngine(c_engine) if c_engine else None), PqaError.factor(c_err.value)

    def load_hip_engine(self, file_path: str, precision: Optional[PrecisionType] = None, q_first: int = 0, n_local: Optional[int] = None,
                        q_total: Optional[int] = None, device: int = -1) -> PqaEngine:
        """Load a .kb file into an engine of `precision` (None: the file's), whatever the file's own -- the rows are converted on the
        device.  n_local given: a shard holding questions [q_first, q_first + n_local) of the file on `device` (q_total: None, or the
        file's question count, checked).  Raises PqaException; no engine exists then."""
        c_err = ctypes.c_void_p()
        shard = None
        if n_local is not None:
            shard = ctypes.byref(CiHipShard(q_first, q_total if q_total is not None else 0, device, 0))
        elif q_first != 0 or q_total is not None or device != -1:
            raise ValueError("q_first, q_total and device describe a shard: give n_local")
        c_engine = _lib.PqaEngineFactory_LoadHipEngineAs(self.c_factory, ctypes.byref(c_err), file_path.encode(), _prec_value(precision), shard,
                                                         n_local if n_local is not None else 0)
        _check(c_err.value)
        return PqaEngine(c_engine)


class MaintenanceLock:  # reference ProbQA.py:786-796
    def __init__(self, engine: PqaEngine, force_quizzes: bool):
        self.engine, self.force_quizzes = engine, force_quizzes

    def __enter__(self):
        self.engine.start_maintenance(self.force_quizzes)

    def __exit__(self, exc_type, exc_value, exc_trace):
        self.engine.finish_maintenance()
