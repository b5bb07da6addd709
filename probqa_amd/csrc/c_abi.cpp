// c_abi.cpp -- the extern "C" surface of libPqaCore.so.
// Every entry that takes an engine is one call of a shim of c_abi_shims.h -- reference ProbQA/PqaCore/PqaCInterop.cpp:45-408
// (AssignPqaError / ReturnPqaError and its three null-handle conventions: return an error object, set *ppError, or log and return a
// value) with the exception barrier inside --, every factory entry one call of CreateEngine / LoadEngine (EngineOf); declarations are in include/PqaCInterop.h
// and include/PqaHipExt.h.
#include <dlfcn.h>
#include <sched.h>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "c_abi_shims.h"
#include "hip_engine.h"
#include "review_plan.h"
#include "status_plan.h"
#include "sampled_part.h"

using pqa::AQ;
using pqa::ErrCode;
using pqa::Error;
using pqa::HipEngine;
using pqa::IEngine;
using namespace pqa::abi;

static_assert(sizeof(CiEngineDefinition) == 48, "POD layout must match reference PqaCInterop.h:10-19");
static_assert(offsetof(CiEngineDefinition, _precType) == 24 && offsetof(CiEngineDefinition, _precExponent) == 26 &&
                  offsetof(CiEngineDefinition, _precMantissa) == 28 && offsetof(CiEngineDefinition, _initAmount) == 32 &&
                  offsetof(CiEngineDefinition, _memPoolMaxBytes) == 40, "POD layout");
static_assert(sizeof(CiAnsweredQuestion) == sizeof(AQ) && sizeof(CiRatedTarget) == 16 && sizeof(CiAddQorTParam) == 16, "POD layout");
static_assert(sizeof(pqa::RatedTargetDev) == sizeof(CiRatedTarget) && offsetof(pqa::RatedTargetDev, prob) == offsetof(CiRatedTarget, _prob), "POD layout");
static_assert(sizeof(CiHipSelection) == sizeof(pqa::SelectResult), "selection record");

namespace {

struct Factory { int unused; };
Factory gFactory;  // process-global singleton, never freed (reference PqaCore/PqaEngineFactorySelector.cpp:11-15)

void ReleaseEngineSideTables(void *pvEngine);   // (what c_abi.cpp keeps per engine handle: the RCCL exchange buffers)
Error NotImpl(const char *feature) {
  return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + feature,
                      std::string(feature) + " is not built in the MI355X engine yet.");
}
char *DupString(const std::string &s) {
  char *p = new char[s.size() + 1];
  std::memcpy(p, s.c_str(), s.size() + 1);
  return p;
}

// PQA_DEVICES=i[,j,...]: empty when unset or malformed (a malformed value is reported and ignored)
std::vector<int> DevicesFromEnvironment() {
  std::vector<int> devices;
  const char *v = std::getenv("PQA_DEVICES");
  if (!v) return devices;
  const char *p = v;
  bool ok = *p != 0;
  while (ok && *p) {
    char *end = nullptr;
    const long d = std::strtol(p, &end, 10);
    if (end == p || d < 0 || d > 1023) { ok = false; break; }
    devices.push_back((int)d);
    p = end;
    if (*p == ',') p++; else if (*p != 0) ok = false;
  }
  if (!ok) {
    if (*v) std::fprintf(stderr, "PqaCore: ignoring PQA_DEVICES=%s (expected a comma-separated list of device ordinals)\n", v);
    devices.clear();
  }
  return devices;
}

// The factory's create entries, one call of EngineOf.
// PQA_DEVICES=i[,j,...] (unchanged wrappers cannot name a device): one ordinal = that device; several = one shard of
// the question axis per listed device (an ordinal may repeat: several shards on one device), behind this one engine handle
void *CreateEngine(void *pvFactory, void **ppError, const CiEngineDefinition *pEngDef, const CiHipShard *pShard) {
  return EngineOf(pvFactory, ppError, [&](Error &err) -> IEngine * {
    if (pEngDef == nullptr) {
      err = Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the engine definition.");
      return nullptr;
    }
    std::vector<int> devices;
    if (pShard == nullptr) devices = DevicesFromEnvironment();
    if (devices.size() >= 2) return pqa::CreateShardedEngine(err, *pEngDef, devices);
    CiHipShard whole;
    if (devices.size() == 1) {
      whole._qFirst = 0; whole._qTotal = pEngDef->_nQuestions; whole._device = devices[0]; whole._reserved = 0;
      pShard = &whole;
    }
    return HipEngine::Create(err, *pEngDef, pShard);
  });
}

// The factory's load entries likewise: .kb files whole or per shard, in the file's precision (precType 0) or another.
// PQA_DEVICES as above, here by hipSetDevice; a shard names its own device.
void *LoadEngine(void *pvFactory, void **ppError, const char *filePath, uint8_t precType, const CiHipShard *pShard, int64_t nLocalQuestions) {
  return EngineOf(pvFactory, ppError, [&](Error &err) -> IEngine * {
    if (precType != 0 && precType != 1 && precType != 3) {
      err = Error::MakeP(ErrCode::NotImplemented, "Feature=precType " + std::to_string((int)precType), "A .kb file is loaded as TPqaPrecisionType::Float or ::Double.");
      return nullptr;
    }
    const std::vector<int> devices = DevicesFromEnvironment();
    if (pShard != nullptr && !devices.empty()) {
      err = Error::Make(ErrCode::WrongMode, "A shard names its own device: PqaEngineFactory_LoadHipEngineAs with pShard is not combined with PQA_DEVICES.");
      return nullptr;
    }
    if (devices.size() >= 2) return pqa::LoadShardedEngine(err, filePath, devices, precType);
    if (devices.size() == 1 && hipSetDevice(devices[0]) != hipSuccess) {
      (void)hipGetLastError();
      err = Error::MakeP(ErrCode::IndexOutOfRange, "device=" + std::to_string(devices[0]), "No such HIP device (PQA_DEVICES).");
      return nullptr;
    }
    return HipEngine::LoadAs(err, filePath, precType, pShard, nLocalQuestions);
  });
}

}  // namespace

extern "C" {

PQACORE_API void CiDebugBreak(void) { /* reference requests a debugger; nothing to do here */ }

// The process-wide default logger (reference SRPlatform/SRDefaultLogger.cpp:47-83): a file logger once Logger_Init has named
// it, the debug stream (here: stderr) until then.  A second initialisation is an error, reported as an owned C string -- and so is
// an exception, by its text.
PQACORE_API uint8_t Logger_Init(void **ppStrErr, const char *baseName) {
  char *text = nullptr;
  bool done = false;
  Error err = Guarded([&] {
    const std::string failure = pqa::DefaultLogger::Init(baseName);
    done = failure.empty();
    if (!done) text = DupString(failure);
    return Error();
  });
  if (!err.ok()) {
    done = false;
    (void)Guarded([&] { text = DupString(err.message + " " + err.params); return Error(); });
  }
  if (ppStrErr) *ppStrErr = text; else delete[] text;
  return done ? 1 : 0;
}

PQACORE_API void CiReleaseString(void *pvString) { delete[] static_cast<char *>(pvString); }

PQACORE_API void *CiGetPqaEngineFactory(void) { return &gFactory; }

PQACORE_API void *PqaEngineFactory_CreateCpuEngine(void *pvFactory, void **ppError, const CiEngineDefinition *pEngDef) {
  return CreateEngine(pvFactory, ppError, pEngDef, nullptr);
}
PQACORE_API void *PqaEngineFactory_CreateHipEngine(void *pvFactory, void **ppError, const CiEngineDefinition *pEngDef) {
  return CreateEngine(pvFactory, ppError, pEngDef, nullptr);
}
PQACORE_API void *PqaEngineFactory_CreateHipEngineSharded(void *pvFactory, void **ppError,
                                                          const CiEngineDefinition *pEngDef, const CiHipShard *pShard) {
  return CreateEngine(pvFactory, ppError, pEngDef, pShard);
}

// (memPoolMaxBytes: the device engine has no host memory pool to size)
PQACORE_API void *PqaEngineFactory_LoadCpuEngine(void *pvFactory, void **ppError, const char *filePath, uint64_t /* memPoolMaxBytes */) {
  return LoadEngine(pvFactory, ppError, filePath, 0, nullptr, 0);
}
PQACORE_API void *PqaEngineFactory_LoadHipEngine(void *pvFactory, void **ppError, const char *filePath, uint64_t /* memPoolMaxBytes */) {
  return LoadEngine(pvFactory, ppError, filePath, 0, nullptr, 0);
}
// ---- .kb files per shard and in either precision (PqaHipExt.h)
PQACORE_API void *PqaEngineFactory_LoadHipEngineAs(void *pvFactory, void **ppError, const char *filePath, uint8_t precType, const CiHipShard *pShard,
                                                   int64_t nLocalQuestions) {
  return LoadEngine(pvFactory, ppError, filePath, precType, pShard, nLocalQuestions);
}
PQACORE_API void *PqaHip_SaveKBAs(void *pvEngine, const char *filePath, uint8_t precType) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.SaveKBAs(filePath, precType); });
}
PQACORE_API void *PqaHip_SaveKBShard(void *pvEngine, const char *filePath, uint8_t precType) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.SaveKBShard(filePath, precType); });
}

PQACORE_API void CiReleasePqaError(void *pvErr) { delete static_cast<Error *>(pvErr); }

PQACORE_API void *PqaError_ToString(void *pvError, const uint8_t withParams) {
  const Error *pErr = static_cast<Error *>(pvError);
  return GuardedValue<char *>(nullptr, nullptr, [&](Error &) { return DupString(pErr ? pErr->ToString(withParams != 0) : "[Success] message=[]"); });
}

PQACORE_API void CiReleasePqaEngine(void *pvEngine) {
  if (pvEngine) ReleaseEngineSideTables(pvEngine);
  delete AsEngine(pvEngine);
}

PQACORE_API void *PqaEngine_Train(void *pvEngine, int64_t nQuestions, const CiAnsweredQuestion *const pAQs,
                                  const int64_t iTarget, const double amount) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.Train(nQuestions, reinterpret_cast<const AQ *>(pAQs), iTarget, amount); });
}

PQACORE_API uint8_t PqaEngine_QuestionPermFromComp(void *pvEngine, const int64_t count, int64_t *pIds) {
  return LoggedOf<uint8_t>(pvEngine, 0, [&](IEngine &e) { return e.MapIds(0, true, count, pIds); });
}
PQACORE_API uint8_t PqaEngine_QuestionCompFromPerm(void *pvEngine, const int64_t count, int64_t *pIds) {
  return LoggedOf<uint8_t>(pvEngine, 0, [&](IEngine &e) { return e.MapIds(0, false, count, pIds); });
}
PQACORE_API uint8_t PqaEngine_TargetPermFromComp(void *pvEngine, const int64_t count, int64_t *pIds) {
  return LoggedOf<uint8_t>(pvEngine, 0, [&](IEngine &e) { return e.MapIds(1, true, count, pIds); });
}
PQACORE_API uint8_t PqaEngine_TargetCompFromPerm(void *pvEngine, const int64_t count, int64_t *pIds) {
  return LoggedOf<uint8_t>(pvEngine, 0, [&](IEngine &e) { return e.MapIds(1, false, count, pIds); });
}
PQACORE_API uint8_t PqaEngine_QuizPermFromComp(void *pvEngine, const int64_t count, int64_t *pIds) {
  return LoggedOf<uint8_t>(pvEngine, 0, [&](IEngine &e) { return e.MapIds(2, true, count, pIds); });
}
PQACORE_API uint8_t PqaEngine_QuizCompFromPerm(void *pvEngine, const int64_t count, int64_t *pIds) {
  return LoggedOf<uint8_t>(pvEngine, 0, [&](IEngine &e) { return e.MapIds(2, false, count, pIds); });
}
PQACORE_API uint8_t PqaEngine_EnsurePermQuizGreater(void *pvEngine, const int64_t bound) {
  return LoggedOf<uint8_t>(pvEngine, 0, [&](IEngine &e) { return e.EnsurePermQuizGreater(bound); });
}
PQACORE_API uint8_t PqaEngine_RemapQuizPermId(void *pvEngine, const int64_t srcPermId, const int64_t destPermId) {
  return LoggedOf<uint8_t>(pvEngine, 0, [&](IEngine &e) { return e.RemapQuizPermId(srcPermId, destPermId); });
}

PQACORE_API uint64_t PqaEngine_GetTotalQuestionsAsked(void *pvEngine, void **ppError) {
  return ValueOf<uint64_t>(pvEngine, ppError, 0, [&](IEngine &e, Error &err) { return e.GetTotalQuestionsAsked(err); });
}

PQACORE_API uint8_t PqaEngine_CopyDims(void *pvEngine, CiEngineDimensions *pDims) {
  return LoggedOf<uint8_t>(pvEngine, 0, [&](IEngine &e) { e.CopyDims(pDims); return 1; });
}

PQACORE_API int64_t PqaEngine_StartQuiz(void *pvEngine, void **ppError) {
  return ValueOf<int64_t>(pvEngine, ppError, -1, [&](IEngine &e, Error &err) { return e.StartQuiz(err); });
}

PQACORE_API int64_t PqaEngine_ResumeQuiz(void *pvEngine, void **ppError, const int64_t nAnswered,
                                         const CiAnsweredQuestion *const pAQs) {
  return ValueOf<int64_t>(pvEngine, ppError, -1, [&](IEngine &e, Error &err) { return e.ResumeQuiz(err, nAnswered, reinterpret_cast<const AQ *>(pAQs)); });
}

PQACORE_API int64_t PqaEngine_NextQuestion(void *pvEngine, void **ppError, const int64_t iQuiz) {
  return ValueOf<int64_t>(pvEngine, ppError, -1, [&](IEngine &e, Error &err) { return e.NextQuestion(err, iQuiz); });
}

PQACORE_API void *PqaEngine_RecordAnswer(void *pvEngine, const int64_t iQuiz, const int64_t iAnswer) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.RecordAnswer(iQuiz, iAnswer); });
}

PQACORE_API void *PqaEngine_ClearOldQuizzes(void *pvEngine, const int64_t maxCount, const double maxAgeSec) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ClearOldQuizzes(maxCount, maxAgeSec); });
}

PQACORE_API int64_t PqaEngine_GetActiveQuestionId(void *pvEngine, void **ppError, const int64_t iQuiz) {
  return ValueOf<int64_t>(pvEngine, ppError, -1, [&](IEngine &e, Error &err) { return e.GetActiveQuestionId(err, iQuiz); });
}

PQACORE_API void *PqaEngine_SetActiveQuestion(void *pvEngine, const int64_t iQuiz, const int64_t iQuestion) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.SetActiveQuestion(iQuiz, iQuestion); });
}

PQACORE_API int64_t PqaEngine_ListTopTargets(void *pvEngine, void **ppError, const int64_t iQuiz,
                                             const int64_t maxCount, CiRatedTarget *pDest) {
  return ValueOf<int64_t>(pvEngine, ppError, -1, [&](IEngine &e, Error &err) { return e.ListTopTargets(err, iQuiz, maxCount, pDest); });
}

PQACORE_API void *PqaEngine_RecordQuizTarget(void *pvEngine, const int64_t iQuiz, const int64_t iTarget,
                                             const double amount) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.RecordQuizTarget(iQuiz, iTarget, amount); });
}

PQACORE_API void *PqaEngine_ReleaseQuiz(void *pvEngine, const int64_t iQuiz) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ReleaseQuiz(iQuiz); });
}

PQACORE_API void *PqaEngine_SaveKB(void *pvEngine, const char *const filePath, const uint8_t bDoubleBuffer) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.SaveKB(filePath, bDoubleBuffer != 0); });
}

PQACORE_API void *PqaEngine_StartMaintenance(void *pvEngine, const bool forceQuizzes) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.StartMaintenance(forceQuizzes); });
}
PQACORE_API void *PqaEngine_FinishMaintenance(void *pvEngine) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.FinishMaintenance(); });
}
PQACORE_API void *PqaEngine_AddQsTs(void *pvEngine, const int64_t nQuestions, CiAddQorTParam *pAddQuestionParams,
                                    const int64_t nTargets, CiAddQorTParam *pAddTargetParams) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.AddQsTs(nQuestions, pAddQuestionParams, nTargets, pAddTargetParams); });
}
PQACORE_API void *PqaEngine_RemoveQuestions(void *pvEngine, const int64_t nQuestions, const int64_t *pQIds) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.RemoveQuestions(nQuestions, pQIds); });
}
PQACORE_API void *PqaEngine_RemoveTargets(void *pvEngine, const int64_t nTargets, const int64_t *pTIds) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.RemoveTargets(nTargets, pTIds); });
}
PQACORE_API void *PqaEngine_Compact(void *pvEngine, int64_t *pnQuestions, int64_t const **const ppOldQuestions,
                                    int64_t *pnTargets, int64_t const **const ppOldTargets) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.Compact(pnQuestions, ppOldQuestions, pnTargets, ppOldTargets); });
}
PQACORE_API void CiReleaseCompaction(const int64_t *p) { std::free(const_cast<int64_t *>(p)); }

PQACORE_API void *PqaEngine_Shutdown(void *pvEngine, const char *const saveFilePath) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.Shutdown(saveFilePath); });
}
// BaseEngine::SetLogger (reference PqaCore/BaseEngine.cpp:252-258): nullptr selects the default logger -- that case is served.
// Any other value is a pointer to an SRPlat::ISRLogger, a C++ object of the MSVC ABI (SRPlatform/Interface/ISRLogger.h:11-25,
// virtual Log(Severity, const SRString&)): none of the C-ABI wrappers can make one (ProbQA.py and the .NET layer only call
// Logger_Init), and this library cannot call through a foreign vtable.
PQACORE_API void *PqaEngine_SetLogger(void *pvEngine, void *pSRLogger) {
  return ErrorOf(pvEngine, [&](IEngine &) { return pSRLogger ? NotImpl("SetLogger with a caller-supplied ISRLogger object (MSVC C++ ABI)") : Error(); });
}

// ---------------------------------------------------------------------------------------------------- PqaHipExt.h
PQACORE_API void *PqaHip_SetOption(void *pvEngine, const char *name, int64_t value) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.SetOption(name, value); });
}
PQACORE_API int64_t PqaHip_GetOption(void *pvEngine, const char *name) {
  return LoggedOf<int64_t>(pvEngine, -1, [&](IEngine &e) { return e.GetOption(name); });
}
PQACORE_API const char *PqaHip_EvalKernelName(void *pvEngine) {
  return LoggedOf<const char *>(pvEngine, "", [&](IEngine &e) { return e.EvalKernelName(); });
}
PQACORE_API void *PqaHip_SetKB(void *pvEngine, const double *pA, const double *pD, const double *pB) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.SetKB(pA, pD, pB); });
}
PQACORE_API void *PqaHip_GetKB(void *pvEngine, double *pA, double *pD, double *pB) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.GetKB(pA, pD, pB); });
}
PQACORE_API void *PqaHip_FillSynthetic(void *pvEngine, double nTrain, double noiseAmp, uint64_t seed) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.FillSynthetic(nTrain, noiseAmp, seed); });
}
PQACORE_API void *PqaHip_SetTargetGaps(void *pvEngine, int64_t n, const int64_t *pTargets) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.SetTargetGaps(n, pTargets); });
}
PQACORE_API void *PqaHip_SetQuestionGaps(void *pvEngine, int64_t n, const int64_t *pQuestions) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.SetQuestionGaps(n, pQuestions); });
}
PQACORE_API void *PqaEngine_EvalPriorities(void *pvEngine, const int64_t iQuiz, double *pOut, const int64_t n) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.EvalPriorities(iQuiz, pOut, n); });
}
PQACORE_API int64_t PqaEngine_NextQuestionArgmax(void *pvEngine, void **ppError, const int64_t iQuiz) {
  return ValueOf<int64_t>(pvEngine, ppError, -1, [&](IEngine &e, Error &err) { return e.NextQuestionArgmax(err, iQuiz); });
}
PQACORE_API int64_t PqaEngine_NextQuestionSampled(void *pvEngine, void **ppError, const int64_t iQuiz,
                                                  const uint64_t rnd) {
  return ValueOf<int64_t>(pvEngine, ppError, -1, [&](IEngine &e, Error &err) { return e.NextQuestionSampled(err, iQuiz, rnd); });
}
PQACORE_API void *PqaHip_GetPriors(void *pvEngine, const int64_t iQuiz, double *pOut, const int64_t n) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.GetPriors(iQuiz, pOut, n); });
}
PQACORE_API void *PqaEngine_NextQuestionArgmaxBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes,
                                                    int64_t *pQuestions) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.NextQuestionArgmaxBatch(nQuizzes, pQuizzes, pQuestions); });
}
PQACORE_API void *PqaEngine_NextQuestionSampledBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const uint64_t *pRnd,
                                                     int64_t *pQuestions) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.NextQuestionSampledBatch(nQuizzes, pQuizzes, pRnd, pQuestions); });
}
PQACORE_API void *PqaEngine_NextQuestionBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, int64_t *pQuestions) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.NextQuestionBatch(nQuizzes, pQuizzes, pQuestions); });
}
PQACORE_API void *PqaEngine_RecordAnswerBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pAnswers) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.RecordAnswerBatch(nQuizzes, pQuizzes, pAnswers); });
}
PQACORE_API void *PqaEngine_StartQuizBatch(void *pvEngine, const int64_t nQuizzes, int64_t *pQuizzes) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.StartQuizBatch(nQuizzes, pQuizzes); });
}
PQACORE_API void *PqaEngine_ResumeQuizBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pCounts, const CiAnsweredQuestion *pAQs,
                                            int64_t *pQuizzes) {
  static_assert(sizeof(CiAnsweredQuestion) == sizeof(AQ), "the answered questions are passed through as they are");
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ResumeQuizBatch(nQuizzes, pCounts, reinterpret_cast<const AQ *>(pAQs), pQuizzes); });
}
PQACORE_API void *PqaEngine_TrainBatch(void *pvEngine, const int64_t nRecords, const int64_t *pCounts, const CiAnsweredQuestion *pAQs,
                                       const int64_t *pTargets, const double *pAmounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.TrainBatch(nRecords, pCounts, reinterpret_cast<const AQ *>(pAQs), pTargets, pAmounts); });
}
PQACORE_API void *PqaEngine_RecordQuizTargetBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pTargets,
                                                  const double *pAmounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.RecordQuizTargetBatch(nQuizzes, pQuizzes, pTargets, pAmounts); });
}
PQACORE_API void *PqaEngine_ListTopTargetsBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t maxCount,
                                                CiRatedTarget *pDest, int64_t *pCounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ListTopTargetsBatch(nQuizzes, pQuizzes, maxCount, pDest, pCounts); });
}
PQACORE_API int64_t PqaEngine_ListTopQuestions(void *pvEngine, void **ppError, const int64_t iQuiz, const int64_t maxCount, CiRatedQuestion *pDest) {
  return ValueOf<int64_t>(pvEngine, ppError, -1, [&](IEngine &e, Error &err) { return e.ListTopQuestions(err, iQuiz, maxCount, pDest); });
}
PQACORE_API void *PqaEngine_ListTopQuestionsBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t maxCount,
                                                  CiRatedQuestion *pDest, int64_t *pCounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ListTopQuestionsBatch(nQuizzes, pQuizzes, maxCount, pDest, pCounts); });
}
PQACORE_API void *PqaEngine_ListTopTargetsAmongBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pListOf, const int64_t nLists,
                                                     const int64_t *pListCounts, const int64_t *pTargets, const int64_t maxCount, CiRatedTarget *pDest,
                                                     int64_t *pCounts, double *pMass) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ListTopTargetsAmongBatch(nQuizzes, pQuizzes, pListOf, nLists, pListCounts, pTargets, maxCount, pDest, pCounts, pMass); });
}
PQACORE_API void *PqaEngine_PreviewAnswersBatch(void *pvEngine, const int64_t nPairs, const int64_t *pQuizzes, const int64_t *pQuestions, const int64_t maxCount,
                                                double *pLikelihood, double *pEntropy, CiRatedTarget *pDest, int64_t *pCounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.PreviewAnswersBatch(nPairs, pQuizzes, pQuestions, maxCount, pLikelihood, pEntropy, pDest, pCounts); });
}
PQACORE_API void *PqaEngine_QuizStatusBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t nLevels, const double *pLevels,
                                            CiHipQuizStatus *pStatus, int64_t *pLevelCounts, double *pLevelMass) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.QuizStatusBatch(nQuizzes, pQuizzes, nLevels, pLevels, pStatus, pLevelCounts, pLevelMass); });
}
PQACORE_API void *PqaEngine_RankTargetsBatch(void *pvEngine, const int64_t nPairs, const int64_t *pQuizzes, const int64_t *pTargets, double *pProb, int64_t *pRank) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.RankTargetsBatch(nPairs, pQuizzes, pTargets, pProb, pRank); });
}
PQACORE_API int64_t PqaHip_GetQuizAnswers(void *pvEngine, void **ppError, const int64_t iQuiz, CiAnsweredQuestion *pDest, const int64_t capacity) {
  return ValueOf<int64_t>(pvEngine, ppError, -1, [&](IEngine &e, Error &err) { return e.GetQuizAnswers(err, iQuiz, reinterpret_cast<AQ *>(pDest), capacity); });
}
PQACORE_API void *PqaEngine_ReviewAnswersBatch(void *pvEngine, const int64_t nPairs, const int64_t *pQuizzes, const int64_t *pPositions, const int64_t maxCount,
                                               double *pLikelihood, double *pEntropy, CiRatedTarget *pDest, int64_t *pCounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ReviewAnswersBatch(nPairs, pQuizzes, pPositions, maxCount, pLikelihood, pEntropy, pDest, pCounts); });
}
PQACORE_API void *PqaEngine_ReviewAnswersBatchFromRows(void *pvEngine, const int64_t nPairs, const int64_t *pQuizzes, const int64_t *pPositions, const int64_t maxCount,
                                                       double *pLikelihood, double *pEntropy, CiRatedTarget *pDest, int64_t *pCounts, const void *pRows,
                                                       const int64_t *pRowFirst) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ReviewAnswersBatchFromRows(nPairs, pQuizzes, pPositions, maxCount, pLikelihood, pEntropy, pDest, pCounts, pRows, pRowFirst); });
}

PQACORE_API void *PqaEngine_EvalPrioritiesAmongBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                     const int64_t *pQuestions, double *pOut) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.EvalPrioritiesAmongBatch(nQuizzes, pQuizzes, pCounts, pQuestions, pOut); });
}
PQACORE_API void *PqaHip_SelectArgmaxAmongBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                const int64_t *pQuestions, CiHipSelection *pOut) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.SelectArgmaxAmongBatch(nQuizzes, pQuizzes, pCounts, pQuestions, pOut); });
}
PQACORE_API void *PqaEngine_NextQuestionArgmaxAmongBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                         const int64_t *pQuestions, int64_t *pPicked) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.NextQuestionArgmaxAmongBatch(nQuizzes, pQuizzes, pCounts, pQuestions, pPicked); });
}
PQACORE_API void *PqaEngine_NextQuestionSampledAmongBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                          const int64_t *pQuestions, const uint64_t *pRnd, int64_t *pPicked) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.NextQuestionSampledAmongBatch(nQuizzes, pQuizzes, pCounts, pQuestions, pRnd, pPicked); });
}
PQACORE_API void *PqaEngine_NextQuestionAmongBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                   const int64_t *pQuestions, int64_t *pPicked) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.NextQuestionAmongBatch(nQuizzes, pQuizzes, pCounts, pQuestions, pPicked); });
}
PQACORE_API void *PqaHip_SelectArgmaxBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, CiHipSelection *pOut) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.SelectArgmaxBatch(nQuizzes, pQuizzes, pOut); });
}
PQACORE_API void *PqaEngine_EvalPrioritiesBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, double *pOut) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.EvalPrioritiesBatch(nQuizzes, pQuizzes, pOut); });
}
PQACORE_API void *PqaHip_Log2Hot(void *pvEngine, const double *pIn, double *pOut, const int64_t n) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.Log2HotArray(pIn, pOut, n); });
}
PQACORE_API void *PqaHip_GetStream(void *pvEngine) {
  return LoggedOf<void *>(pvEngine, nullptr, [&](IEngine &e) { return e.GetStream(); });
}
PQACORE_API void *PqaHip_SetStream(void *pvEngine, void *hipStream) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.SetStream(static_cast<hipStream_t>(hipStream)); });
}
PQACORE_API void *PqaHip_Synchronize(void *pvEngine) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.Synchronize(); });
}
PQACORE_API void *PqaHip_Quiesce(void *pvEngine) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.Quiesce(); });
}
PQACORE_API void *PqaHip_EnqueueSelectArgmaxFlag(void *pvEngine, const int64_t iQuiz, void *pOut, void *pFlag,
                                                 const uint64_t flagValue) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.EnqueueSelectArgmaxFlag(iQuiz, pOut, pFlag, flagValue); });
}
// ---- ResumeQuiz on shards driven by processes of their own: the owners pack the answered questions' rows, every rank resumes
// from the exchanged package (hip_engine_resume.cpp)
PQACORE_API int64_t PqaHip_AnswerRowSlotBytes(void *pvEngine) {
  return LoggedOf<int64_t>(pvEngine, -1, [&](IEngine &e) { return e.AnswerRowSlotBytes(); });
}
PQACORE_API void *PqaHip_PackAnswerRows(void *pvEngine, const int64_t nAnswered, const CiAnsweredQuestion *pAQs, void *pDst, void *pFlag,
                                        const uint64_t flagValue) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.PackAnswerRows(nAnswered, reinterpret_cast<const AQ *>(pAQs), pDst, pFlag, flagValue); });
}
PQACORE_API int64_t PqaEngine_ResumeQuizFromRows(void *pvEngine, void **ppError, const int64_t nAnswered, const CiAnsweredQuestion *pAQs,
                                                 const void *pRows) {
  return ValueOf<int64_t>(pvEngine, ppError, -1, [&](IEngine &e, Error &err) { return e.ResumeQuizFromRows(err, nAnswered, reinterpret_cast<const AQ *>(pAQs), pRows); });
}
PQACORE_API void *PqaEngine_ResumeQuizBatchFromRows(void *pvEngine, const int64_t nQuizzes, const int64_t *pCounts, const CiAnsweredQuestion *pAQs,
                                                    const void *pRows, int64_t *pQuizzes) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ResumeQuizBatchFromRows(nQuizzes, pCounts, reinterpret_cast<const AQ *>(pAQs), pRows, pQuizzes); });
}
// ---- a page of answers per quiz in one launch (hip_engine_record_page.cpp); FromRows: other shards' rows from a row package
PQACORE_API void *PqaEngine_RecordAnswerPageBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                  const CiAnsweredQuestion *pAQs, double *pLikelihood) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.RecordAnswerPageBatch(nQuizzes, pQuizzes, pCounts, reinterpret_cast<const AQ *>(pAQs), pLikelihood); });
}
PQACORE_API void *PqaEngine_RecordAnswerPageBatchFromRows(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                          const CiAnsweredQuestion *pAQs, double *pLikelihood, const void *pRows) {
  return ErrorOf(pvEngine, [&](IEngine &e) {
    return e.RecordAnswerPageBatchFromRows(nQuizzes, pQuizzes, pCounts, reinterpret_cast<const AQ *>(pAQs), pLikelihood, pRows);
  });
}
// ---- the sampled selector on shards driven by processes of their own: every rank packs a selection part per quiz, picks from the
// gathered parts of all ranks and takes the agreed pick (hip_engine_parts.cpp)
PQACORE_API int64_t PqaHip_SampledPartBytes(void *pvEngine) {
  return LoggedOf<int64_t>(pvEngine, -1, [&](IEngine &e) { return e.SampledPartBytes(); });
}
PQACORE_API void *PqaHip_PackSampledParts(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, void *pDst, void *pFlag,
                                          const uint64_t flagValue) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.PackSampledParts(nQuizzes, pQuizzes, pDst, pFlag, flagValue); });
}
PQACORE_API void *PqaHip_SampledPickFromParts(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const uint64_t *pRnd,
                                              const void *pParts, const int64_t rank, const int64_t world, CiHipSelection *pOut) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.SampledPickFromParts(nQuizzes, pQuizzes, pRnd, pParts, rank, world, pOut); });
}
PQACORE_API void *PqaEngine_TakeSampledPicks(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pPicks,
                                             int64_t *pQuestions) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.TakeSampledPicks(nQuizzes, pQuizzes, pPicks, pQuestions); });
}
// ---- RecordAnswer for many quizzes on shards driven by processes of their own: the holders of the active questions pack the new
// posteriors without changing a quiz, every rank records from the combined package (hip_engine_record_parts.cpp)
PQACORE_API int64_t PqaHip_PosteriorSlotBytes(void *pvEngine) {
  return LoggedOf<int64_t>(pvEngine, -1, [&](IEngine &e) { return e.PosteriorSlotBytes(); });
}
PQACORE_API void *PqaHip_PackAnswerPosteriors(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pAnswers, void *pDst,
                                              void *pFlag, const uint64_t flagValue) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.PackAnswerPosteriors(nQuizzes, pQuizzes, pAnswers, pDst, pFlag, flagValue); });
}
PQACORE_API void *PqaEngine_RecordAnswerBatchFromPosteriors(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pAnswers,
                                                            const void *pPosteriors) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.RecordAnswerBatchFromPosteriors(nQuizzes, pQuizzes, pAnswers, pPosteriors); });
}
// ---- targets that answer like a given one (hip_engine_sources.cpp): a whole engine's matrix and listing, and the pair for shards
// driven by processes of their own -- every rank packs its questions' sums, every rank lists from the summed package
PQACORE_API void *PqaEngine_EvalTargetSimilarity(void *pvEngine, const int64_t nSources, const int64_t *pSources, double *pOut, const int64_t n) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.EvalTargetSimilarity(nSources, pSources, pOut, n); });
}
PQACORE_API void *PqaEngine_ListSimilarTargetsBatch(void *pvEngine, const int64_t nSources, const int64_t *pSources, const int64_t maxCount,
                                                    CiRatedTarget *pDest, int64_t *pCounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ListSimilarTargetsBatch(nSources, pSources, maxCount, pDest, pCounts); });
}
PQACORE_API void *PqaHip_PackTargetSimilaritySums(void *pvEngine, const int64_t nSources, const int64_t *pSources, void *pDst, void *pFlag,
                                                  const uint64_t flagValue) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.PackTargetSimilaritySums(nSources, pSources, pDst, pFlag, flagValue); });
}
PQACORE_API void *PqaEngine_ListSimilarTargetsFromSums(void *pvEngine, const int64_t nSources, const int64_t *pSources, const void *pSums,
                                                       const int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ListSimilarTargetsFromSums(nSources, pSources, pSums, maxCount, pDest, pCounts); });
}
// ---- questions whose answers a given one predicts (hip_engine_sources.cpp): a whole engine's rows and listing, and the calls for
// shards driven by processes of their own -- the owners pack their sources' weighted rows, every rank evaluates / lists its own
// questions from the summed package
PQACORE_API void *PqaEngine_EvalQuestionRedundancy(void *pvEngine, const int64_t nSources, const int64_t *pSources, double *pOut, const int64_t n) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.EvalQuestionRedundancy(nSources, pSources, pOut, n); });
}
PQACORE_API void *PqaEngine_ListRedundantQuestionsBatch(void *pvEngine, const int64_t nSources, const int64_t *pSources, const int64_t maxCount,
                                                        CiRatedQuestion *pDest, int64_t *pCounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ListRedundantQuestionsBatch(nSources, pSources, maxCount, pDest, pCounts); });
}
PQACORE_API int64_t PqaHip_QuestionWeightSlotBytes(void *pvEngine) {
  return LoggedOf<int64_t>(pvEngine, -1, [&](IEngine &e) { return e.QuestionWeightSlotBytes(); });
}
PQACORE_API void *PqaHip_PackQuestionWeights(void *pvEngine, const int64_t nSources, const int64_t *pSources, void *pDst, void *pFlag,
                                             const uint64_t flagValue) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.PackQuestionWeights(nSources, pSources, pDst, pFlag, flagValue); });
}
PQACORE_API void *PqaEngine_EvalQuestionRedundancyFromWeights(void *pvEngine, const int64_t nSources, const int64_t *pSources, const void *pWeights,
                                                              double *pOut, const int64_t n) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.EvalQuestionRedundancyFromWeights(nSources, pSources, pWeights, pOut, n); });
}
PQACORE_API void *PqaEngine_ListRedundantQuestionsFromWeights(void *pvEngine, const int64_t nSources, const int64_t *pSources, const void *pWeights,
                                                              const int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ListRedundantQuestionsFromWeights(nSources, pSources, pWeights, maxCount, pDest, pCounts); });
}
// ---- questions that tell listed targets apart (hip_engine_sources.cpp): a value needs the group's columns of one question's block and
// nothing else, so a shard driven by a process of its own answers for its questions directly -- no package, no pack call
PQACORE_API void *PqaEngine_EvalTargetSeparation(void *pvEngine, const int64_t nGroups, const int64_t *pGroupCounts, const int64_t *pTargets, double *pOut,
                                                 const int64_t n) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.EvalTargetSeparation(nGroups, pGroupCounts, pTargets, pOut, n); });
}
PQACORE_API void *PqaEngine_ListSeparatingQuestionsBatch(void *pvEngine, const int64_t nGroups, const int64_t *pGroupCounts, const int64_t *pTargets,
                                                         const int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ListSeparatingQuestionsBatch(nGroups, pGroupCounts, pTargets, maxCount, pDest, pCounts); });
}
PQACORE_API void *PqaEngine_EvalQuestionGainsBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, double *pOut, const int64_t n) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.EvalQuestionGainsBatch(nQuizzes, pQuizzes, pOut, n); });
}
PQACORE_API void *PqaEngine_ListInformativeQuestionsBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t maxCount,
                                                          CiRatedQuestion *pDest, int64_t *pCounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ListInformativeQuestionsBatch(nQuizzes, pQuizzes, maxCount, pDest, pCounts); });
}
// ---- question pages (hip_engine_page.cpp): the plain calls on whole engines only -- the branch rows need the given questions' blocks, which
// one rank holds --, the FromBlocks forms on shards that separate processes drive, the blocks in a package
PQACORE_API void *PqaEngine_EvalConditionalGainsBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts,
                                                      const int64_t *pGiven, double *pOut, const int64_t n) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.EvalConditionalGainsBatch(nQuizzes, pQuizzes, pGivenCounts, pGiven, pOut, n); });
}
PQACORE_API void *PqaEngine_ListQuestionPageBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven,
                                                  const int64_t pageSize, CiRatedQuestion *pDest, int64_t *pCounts) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.ListQuestionPageBatch(nQuizzes, pQuizzes, pGivenCounts, pGiven, pageSize, pDest, pCounts); });
}
PQACORE_API void *PqaHip_PackGivenBlocks(void *pvEngine, const int64_t nQuestions, const int64_t *pQuestions, void *pDst, void *pFlag, const uint64_t flagValue) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.PackGivenBlocks(nQuestions, pQuestions, pDst, pFlag, flagValue); });
}
PQACORE_API void *PqaEngine_EvalConditionalGainsBatchFromBlocks(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts,
                                                                const int64_t *pGiven, const int64_t nBlocks, const int64_t *pBlockQuestions, const void *pBlocks,
                                                                const int64_t slotBytes, double *pOut, const int64_t n) {
  return ErrorOf(pvEngine, [&](IEngine &e) {
    return e.EvalConditionalGainsBatchFromBlocks(nQuizzes, pQuizzes, pGivenCounts, pGiven, nBlocks, pBlockQuestions, pBlocks, slotBytes, pOut, n);
  });
}
PQACORE_API void *PqaHip_SelectPageStepFromBlocks(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven,
                                                  const int64_t nBlocks, const int64_t *pBlockQuestions, const void *pBlocks, const int64_t slotBytes,
                                                  CiHipSelection *pOut) {
  return ErrorOf(pvEngine, [&](IEngine &e) {
    return e.SelectPageStepFromBlocks(nQuizzes, pQuizzes, pGivenCounts, pGiven, nBlocks, pBlockQuestions, pBlocks, slotBytes, pOut);
  });
}
// Host memory (e.g. a shared-memory segment mapped by every rank) made writable by this process's GPU.
PQACORE_API void *PqaHip_HostRegister(void *pHost, const int64_t nBytes, void **ppDevice) {
  return ReturnErr(Guarded([&]() -> Error {
    if (!pHost || !ppDevice || nBytes <= 0) return Error::Make(ErrCode::NullArgument, "Bad arguments to PqaHip_HostRegister.");
    hipError_t he = hipHostRegister(pHost, (size_t)nBytes, hipHostRegisterMapped | hipHostRegisterPortable);
    if (he == hipSuccess) he = hipHostGetDevicePointer(ppDevice, pHost, 0);
    if (he != hipSuccess) return Error::MakeP(ErrCode::StdException, std::string("hip=") + hipGetErrorString(he), "hipHostRegister failed.");
    return Error();
  }));
}
PQACORE_API void *PqaHip_HostUnregister(void *pHost) {
  if (pHost) hipHostUnregister(pHost);
  return nullptr;
}
// The winner (kb_plan.h: BestPick) among `world` records {double priority; int64 index} that lie strideBytes apart.
static void PickOfRecords(const char *base, int64_t world, int64_t strideBytes, double *pPriority, int64_t *pIndex) {
  pqa::BestPick best;
  for (int64_t r = 0; r < world; r++) {
    double p;
    int64_t i;
    std::memcpy(&p, base + r * strideBytes, 8);
    std::memcpy(&i, base + r * strideBytes + 8, 8);
    best.Offer(p, i);
  }
  *pPriority = best.priority;
  *pIndex = best.index;
}
// Host-side half of the shared-memory exchange: spin until the flags of all `world` slots equal flagValue, then pick the
// winner (maximum priority, lowest index on ties, NaN never wins, -1 if no slot has an eligible question).  A slot is
// strideBytes long and starts with {double priority; int64 index; uint64 flag}.  Returns an error after timeoutSec.
static Error PickWhenAll(const void *pSlots, const int64_t world, const int64_t strideBytes, const uint64_t flagValue, const double timeoutSec,
                         double *pPriority, int64_t *pIndex) {
  if (!pSlots || !pPriority || !pIndex || world <= 0 || strideBytes < 24)
    return Error::Make(ErrCode::NullArgument, "Bad arguments to PqaHip_PickWhenAll.");
  const char *base = (const char *)pSlots;
  const auto t0 = std::chrono::steady_clock::now();
  for (int64_t r = 0; r < world; r++) {
    const volatile uint64_t *flag = (const volatile uint64_t *)(base + r * strideBytes + 16);
    uint64_t spins = 0;
    bool yielding = false;
    while (*flag != flagValue) {   // (a pure spin for the first 200 us -- the answer is a kernel's time away --, then the core is offered between looks)
      ++spins;
      if (!yielding) {
        __builtin_ia32_pause();
        if ((spins & 63) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) yielding = true;
        continue;
      }
      if ((spins & 0xFF) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeoutSec)
        return Error::MakeP(ErrCode::StdException, "rank=" + std::to_string(r), "Timed out waiting for a shard's selection.");
      sched_yield();
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  PickOfRecords(base, world, strideBytes, pPriority, pIndex);
  return Error();
}
PQACORE_API void *PqaHip_PickWhenAll(const void *pSlots, const int64_t world, const int64_t strideBytes,
                                     const uint64_t flagValue, const double timeoutSec, double *pPriority, int64_t *pIndex) {
  return ReturnErr(Guarded([&] { return PickWhenAll(pSlots, world, strideBytes, flagValue, timeoutSec, pPriority, pIndex); }));
}
// One step of the shared-memory exchange in one call: enqueue this shard's selection with its record and flag in slot `rank`
// of the host's slot array (pSlotsDev: the device-visible address of the same array), then wait for every rank and pick.
PQACORE_API void *PqaHip_SelectThroughSlots(void *pvEngine, const int64_t iQuiz, const void *pSlots, void *pSlotsDev,
                                            const int64_t rank, const int64_t world, const int64_t strideBytes,
                                            const uint64_t flagValue, const double timeoutSec, double *pPriority,
                                            int64_t *pIndex) {
  return ErrorOf(pvEngine, [&](IEngine &eng) -> Error {
    if (!pSlots || !pSlotsDev || rank < 0 || rank >= world || strideBytes < 24)
      return Error::Make(ErrCode::NullArgument, "Bad arguments to PqaHip_SelectThroughSlots.");
    char *mine = (char *)pSlotsDev + rank * strideBytes;
    Error e = eng.EnqueueSelectArgmaxFlag(iQuiz, mine, mine + 16, flagValue);
    if (!e.ok()) return e;
    return PickWhenAll(pSlots, world, strideBytes, flagValue, timeoutSec, pPriority, pIndex);
  });
}
// The shards' 16-byte winners gathered by ONE RCCL collective on the engine's stream, for a process-per-GPU host that owns an RCCL
// communicator and is not Python (probqa_amd/dist.py does the same through torch.distributed; north_star: "a single RCCL
// all-reduce" -- an all-gather of {priority, GLOBAL index} and the exact pick on every rank, so that ties break by the lowest
// index as in the reference's argmax).  RCCL is looked up at the first call (dlopen: libPqaCore.so itself does not link it).
namespace {
// The exchange buffers of one engine: 16 (world + 1) bytes on the ENGINE's device and their pinned mirror.  They live as long as the
// engine (ReleaseRcclBufs at CiReleasePqaEngine: an engine at a recycled address never meets an earlier engine's buffers), and `mu`
// is held over enqueue, all-gather, copy and pick, so that concurrent calls on one engine do not share them mid-flight.
struct RcclBufs {
  std::mutex mu;
  void *dSend = nullptr, *dRecv = nullptr, *hRecv = nullptr;
  int64_t world = 0;
  int device = -1;
  void Free() {
    if (dSend) { hipSetDevice(device); hipFree(dSend); }
    if (hRecv) hipHostFree(hRecv);
    dSend = dRecv = hRecv = nullptr;
    world = 0;
  }
};
std::mutex gRcclMu;
std::unordered_map<void *, std::shared_ptr<RcclBufs>> gRcclBufs;
void ReleaseRcclBufs(void *pvEngine) {
  std::shared_ptr<RcclBufs> b;
  {
    std::lock_guard<std::mutex> lk(gRcclMu);
    auto it = gRcclBufs.find(pvEngine);
    if (it == gRcclBufs.end()) return;
    b = std::move(it->second);
    gRcclBufs.erase(it);
  }
  if (!b) return;   // (a slot whose buffers were never made)
  std::lock_guard<std::mutex> lk(b->mu);   // (a call still inside finishes first)
  b->Free();
}
typedef int (*NcclAllGatherFn)(const void *, void *, size_t, int, void *, hipStream_t);
NcclAllGatherFn RcclAllGather() {
  static NcclAllGatherFn fn = [] {
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    return h ? reinterpret_cast<NcclAllGatherFn>(dlsym(h, "ncclAllGather")) : nullptr;
  }();
  return fn;
}
void ReleaseEngineSideTables(void *pvEngine) { ReleaseRcclBufs(pvEngine); }
}  // namespace
PQACORE_API void *PqaHip_SelectArgmaxRccl(void *pvEngine, const int64_t iQuiz, void *pNcclComm, const int64_t world, double *pPriority,
                                          int64_t *pIndex) {
  return ErrorOf(pvEngine, [&](IEngine &eng) -> Error {
    if (!pNcclComm || !pPriority || !pIndex || world < 1 || world > 4096)
      return Error::Make(ErrCode::NullArgument, "Bad arguments to PqaHip_SelectArgmaxRccl.");
    const NcclAllGatherFn allGather = RcclAllGather();
    if (allGather == nullptr) return Error::Make(ErrCode::StdException, "librccl.so (ncclAllGather) could not be loaded.");
    std::shared_ptr<RcclBufs> bufs;
    {
      std::lock_guard<std::mutex> lk(gRcclMu);
      std::shared_ptr<RcclBufs> &slot = gRcclBufs[pvEngine];
      if (!slot) slot = std::make_shared<RcclBufs>();
      bufs = slot;
    }
    RcclBufs &b = *bufs;
    std::lock_guard<std::mutex> held(b.mu);
    const int device = (int)eng.GetOption("device");
    if (device < 0 || eng.GetOption("shards") > 0) return Error::Make(ErrCode::StdException, "PqaHip_SelectArgmaxRccl is for an engine on ONE device (a shard of a process-per-GPU host).");
    if (hipSetDevice(device) != hipSuccess) return Error::Make(ErrCode::StdException, "PqaHip_SelectArgmaxRccl: the engine's device cannot be selected.");
    if (b.world != world || b.device != device) {   // (first call, or another communicator size: allocated on the engine's device, whatever the calling thread's was)
      b.Free();
      b.device = device;
      void *d = nullptr, *h = nullptr;
      if (hipMalloc(&d, (size_t)(world + 1) * 16) != hipSuccess || hipHostMalloc(&h, (size_t)world * 16, hipHostMallocDefault) != hipSuccess) {
        if (d) hipFree(d);
        (void)hipGetLastError();
        return Error::Make(ErrCode::StdException, "PqaHip_SelectArgmaxRccl: no memory for the exchange buffers.");
      }
      b.dSend = d; b.dRecv = static_cast<char *>(d) + 16; b.hRecv = h; b.world = world;
    }
    Error e = eng.EnqueueSelectArgmax(iQuiz, b.dSend);   // {priority, GLOBAL index} of this shard's winner, in stream order
    if (!e.ok()) return e;
    const hipStream_t stream = eng.GetStream();
    const int rc = allGather(b.dSend, b.dRecv, 16, /* ncclUint8 */ 1, pNcclComm, stream);
    if (rc != 0) return Error::MakeP(ErrCode::StdException, "ncclResult=" + std::to_string(rc), "ncclAllGather failed.");
    hipError_t he = hipMemcpyAsync(b.hRecv, b.dRecv, (size_t)world * 16, hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    if (he != hipSuccess) return Error::MakeP(ErrCode::StdException, hipGetErrorString(he), "PqaHip_SelectArgmaxRccl: the gathered winners did not arrive.");
    PickOfRecords(static_cast<const char *>(b.hRecv), world, 16, pPriority, pIndex);
    return Error();
  });
}
PQACORE_API void *PqaHip_EnqueueSelectArgmax(void *pvEngine, const int64_t iQuiz, void *pOut) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.EnqueueSelectArgmax(iQuiz, pOut); });
}
PQACORE_API void *PqaHip_EnqueueEval(void *pvEngine, const int64_t iQuiz) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.EnqueueEval(iQuiz); });
}
PQACORE_API void *PqaHip_GetPriorDevicePtr(void *pvEngine, const int64_t iQuiz, void **ppDev, int64_t *pLdT) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.GetPriorDevicePtr(iQuiz, ppDev, pLdT); });
}
PQACORE_API void *PqaHip_RecordAnswerRemote(void *pvEngine, const int64_t iQuiz, const int64_t iAnswer) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.RecordAnswerRemote(iQuiz, iAnswer); });
}

PQACORE_API void *PqaHip_CompactPlan(void *pvEngine, int64_t *pnQuestions, int64_t *pnTargets, int64_t *pnMoves, int64_t const **const ppMoves,
                                     uint8_t *pWouldBeEmpty) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.CompactPlanOf(pnQuestions, pnTargets, pnMoves, ppMoves, pWouldBeEmpty); });
}
PQACORE_API int64_t PqaHip_QuestionBlockSlotBytes(void *pvEngine) {
  return LoggedOf<int64_t>(pvEngine, -1, [&](IEngine &e) { return e.QuestionBlockSlotBytes(); });
}
PQACORE_API void *PqaHip_PackQuestionBlocks(void *pvEngine, const int64_t nQuestions, const int64_t *pQuestions, void *pDst, void *pFlag,
                                            const uint64_t flagValue) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.PackQuestionBlocks(nQuestions, pQuestions, pDst, pFlag, flagValue); });
}
PQACORE_API void *PqaEngine_CompactFromBlocks(void *pvEngine, const void *pBlocks, const int64_t slotBytes, const int64_t emptiedRank, int64_t *pnQuestions,
                                              int64_t const **const ppOldQuestions, int64_t *pnTargets, int64_t const **const ppOldTargets) {
  return ErrorOf(pvEngine, [&](IEngine &e) { return e.CompactFromBlocks(pBlocks, slotBytes, emptiedRank, pnQuestions, ppOldQuestions, pnTargets, ppOldTargets); });
}

static int64_t HostLogicProbe(const char *what, const int64_t *pIn, const int64_t nIn, int64_t *pOut, const int64_t nOut) {
  const std::string w(what ? what : "");
  if (nIn < 0 || nOut < 0 || (nIn > 0 && !pIn) || (nOut > 0 && !pOut)) return -1;
  if (w.compare(0, 12, "option_spec:") == 0) {   // a row of engine_options.h, by the option's name or as "#i" by its position
    const std::string key = w.substr(12);
    const pqa::OptionSpec *o = pqa::FindOption(key.c_str());
    if (key.size() > 1 && key[0] == '#') {
      char *end = nullptr;
      const long long i = std::strtoll(key.c_str() + 1, &end, 10);
      if (*end == 0 && i >= 0 && i < pqa::kOptionCount) o = &pqa::kOptions[i];
    }
    if (!o || nOut < 6) return -1;
    const int64_t row[6] = {o->lo, o->hi, pqa::EngineOptions().*o->field, o->flag, o->effects, o->env != nullptr};
    std::copy(row, row + 6, pOut);
    return 6;
  }
  if (w == "id_ledger") {
    pqa::IdLedger ledger;
    int64_t i = 0, nRes = 0;
    while (i < nIn) {
      if (i + 3 > nIn || nRes >= nOut) return -1;
      const int64_t op = pIn[i], a = pIn[i + 1], b = pIn[i + 2];
      i += 3;
      int64_t r;
      switch (op) {
        case 0: r = ledger.PermanentOf(a); break;
        case 1: r = ledger.SlotOf(a); break;
        case 2: r = ledger.RaiseFloor(a); break;
        case 3: r = ledger.Vacate(a); break;
        case 4: r = ledger.Reissue(a); break;
        case 5: r = ledger.Extend(a); break;
        case 6: r = ledger.Rename(a, b); break;
        case 7:
          if (a < 0 || b != a || i + a > nIn) return -1;
          r = ledger.Repack(a, pIn + i);
          i += a;
          break;
        case 8: {
          FILE *f = std::tmpfile();
          if (!f) return -1;
          pqa::IdLedger back;
          r = ledger.Write(f) && std::fseek(f, 0, SEEK_SET) == 0 && back.Read(f);
          std::fclose(f);
          if (r) ledger = back;
          break;
        }
        case 9: r = ledger.LiveSlots(); break;
        default: return -1;
      }
      pOut[nRes++] = r;
    }
    return nRes;
  }
  if (w == "kb_layout") {   // {K, Q, T, elem, qFirst, nLocal} -> {valid, window ok, sA offset, sA bytes, mD offset, mD bytes, vB offset, trailer offset}
    if (nIn != 6 || nOut < 8) return -1;
    const pqa::KbLayout lay(pIn[0], pIn[1], pIn[2], pIn[3]);
    const bool window = lay.HasWindow(pIn[4], pIn[5]);
    const int64_t row[8] = {lay.valid, window, window ? lay.SaOffset(pIn[4]) : -1, window ? pIn[5] * lay.K * lay.rowBytes : -1, window ? lay.MdOffset(pIn[4]) : -1,
                            window ? pIn[5] * lay.rowBytes : -1, lay.valid ? lay.vbOff : -1, lay.valid ? lay.trailerOff : -1};
    std::copy(row, row + 8, pOut);
    return 8;
  }
  if (w == "sampled_part") {   // {Q, nSub, qFirst, n} -> {bytes, first whole subtask, their count, piece 0's subtask (-1: none) and length, piece 1's}
    if (nIn != 4 || nOut < 7 || pIn[0] < 1 || pIn[1] < 1 || pIn[2] < 0 || pIn[3] < 1 || pIn[3] > pIn[0] - pIn[2]) return -1;
    const pqa::SampledSplit sp = pqa::sampled_split(pIn[0], pIn[1]);
    const pqa::SampledPartShape sh = pqa::sampled_part_shape(sp, pIn[2], pIn[3]);
    const int64_t row[7] = {pqa::sampled_part_bytes(sp), sh.firstWhole, sh.nWhole, sh.p0Sub, sh.p0Len, sh.p1Sub, sh.p1Len};
    std::copy(row, row + 7, pOut);
    return 7;
  }
  if (w == "let_go") {
    if (nIn < 4 || pIn[3] < 0 || nIn != 4 + 2 * pIn[3]) return -1;
    std::vector<pqa::QuizUsage> inUse;
    for (int64_t k = 0; k < pIn[3]; k++) inUse.push_back(pqa::QuizUsage{pIn[4 + 2 * k], (time_t)pIn[5 + 2 * k]});
    const std::vector<int64_t> ids = pqa::QuizzesToLetGo(inUse, (time_t)pIn[0], pIn[1], (double)pIn[2]);
    if ((int64_t)ids.size() + 1 > nOut) return -1;
    pOut[0] = (int64_t)ids.size();
    for (size_t k = 0; k < ids.size(); k++) pOut[1 + k] = ids[k];
    return (int64_t)ids.size() + 1;
  }
  // The maintenance plans and the shards' pick (kb_plan.h).  Lists travel as {n, then n words}; doubles as their bit patterns.
  int64_t at = 0, nRes = 0;
  auto list = [&](std::vector<int64_t> &v) {
    if (at >= nIn || pIn[at] < 0 || at + 1 + pIn[at] > nIn) return false;
    v.assign(pIn + at + 1, pIn + at + 1 + pIn[at]);
    at += 1 + pIn[at];
    return true;
  };
  auto gapList = [&](std::vector<int64_t> &v, int64_t limit) {   // ... within the dimension, each id once: what an engine's list is
    if (!list(v)) return false;
    std::vector<char> seen((size_t)std::max<int64_t>(limit, 0), 0);
    for (int64_t g : v) { if (g < 0 || g >= limit || seen[(size_t)g]) return false; seen[(size_t)g] = 1; }
    return true;
  };
  auto put = [&](const std::vector<int64_t> &v) {
    if (nRes + 1 + (int64_t)v.size() > nOut) return false;
    pOut[nRes++] = (int64_t)v.size();
    nRes = std::copy(v.begin(), v.end(), pOut + nRes) - pOut;
    return true;
  };
  std::vector<int64_t> qGaps, tGaps, qWords, tWords;
  if (w == "add_plan" || w == "compact_plan") {
    at = 2;
    if (nIn < 2 || !gapList(qGaps, pIn[0]) || !gapList(tGaps, pIn[1])) return -1;
    if (w == "compact_plan") {
      const pqa::CompactPlan plan = pqa::PlanCompact(qGaps, tGaps, pIn[0], pIn[1]);
      for (const auto &mv : plan.qMoves) { qWords.push_back(mv.first); qWords.push_back(mv.second); }
      return at == nIn && put(plan.oldQ) && put(plan.oldT) && put(qWords) ? nRes : -1;
    }
    if (!list(qWords) || !list(tWords) || at != nIn || nOut < 4) return -1;
    std::vector<CiAddQorTParam> aq(qWords.size()), atp(tWords.size());
    for (size_t i = 0; i < aq.size(); i++) std::memcpy(&aq[i]._initAmount, &qWords[i], 8);
    for (size_t i = 0; i < atp.size(); i++) std::memcpy(&atp[i]._initAmount, &tWords[i], 8);
    const pqa::AddPlan plan = pqa::PlanAdd(qGaps, tGaps, pIn[0], pIn[1], (int64_t)aq.size(), aq.data(), (int64_t)atp.size(), atp.data());
    if (!qWords.empty()) std::memcpy(qWords.data(), plan.qInit.data(), 8 * qWords.size());
    if (!tWords.empty()) std::memcpy(tWords.data(), plan.tInit.data(), 8 * tWords.size());
    pOut[0] = plan.nQReuse; pOut[1] = plan.nTReuse; pOut[2] = plan.newQ; pOut[3] = plan.newT;
    nRes = 4;
    return put(plan.qIds) && put(plan.tIds) && put(qWords) && put(tWords) ? nRes : -1;
  }
  if (w == "shard_compact") {   // {bounds, Q, T, question gaps, target gaps} -> {refused, new bounds, moves as {dst, src, dst's shard, src's shard}}
    std::vector<int64_t> bounds;
    if (!list(bounds) || bounds.empty() || at + 2 > nIn) return -1;
    const int64_t Q = pIn[at], T = pIn[at + 1];
    at += 2;
    for (size_t r = 0; r < bounds.size(); r++)
      if (bounds[r] <= (r == 0 ? 0 : bounds[r - 1])) return -1;   // ascending, no shard without a question
    if (bounds.back() != Q || !gapList(qGaps, Q) || !gapList(tGaps, T) || at != nIn || nOut < 1) return -1;
    const pqa::ShardCompactPlan s = pqa::PlanShardCompact(bounds, pqa::PlanCompact(qGaps, tGaps, Q, T));
    pOut[0] = s.refused;
    nRes = 1;
    return put(s.newBounds) && put(s.moves) ? nRes : -1;
  }
  if (w == "check_removal") {
    at = 1;
    if (nIn < 1 || !gapList(qGaps, pIn[0]) || !list(qWords) || at != nIn || nOut < 2) return -1;
    auto isGap = [&](int64_t id) { return std::find(qGaps.begin(), qGaps.end(), id) != qGaps.end(); };
    pOut[0] = pqa::FirstBadRemoval((int64_t)qWords.size(), qWords.data(), pIn[0], isGap);
    pOut[1] = (int64_t)pqa::CheckRemoval((int64_t)qWords.size(), qWords.data(), pIn[0], isGap, "").code;
    return 2;
  }
  if (w == "merge_top") {   // {maxCount, nLists, then per list n and n x {priority bits, index}} -> {n, then n x {priority bits, index}}
    if (nIn < 2 || pIn[1] < 0) return -1;
    std::vector<std::vector<pqa::RatedIndex>> recs;
    at = 2;
    for (int64_t l = 0; l < pIn[1]; l++) {
      if (at >= nIn || pIn[at] < 0 || pIn[at] > (nIn - at - 1) / 2) return -1;
      std::vector<pqa::RatedIndex> v((size_t)pIn[at]);
      for (size_t k = 0; k < v.size(); k++) { std::memcpy(&v[k].priority, &pIn[at + 1 + 2 * (int64_t)k], 8); v[k].index = pIn[at + 2 + 2 * (int64_t)k]; }
      at += 1 + 2 * pIn[at];
      recs.push_back(std::move(v));
    }
    if (at != nIn) return -1;
    std::vector<std::pair<const pqa::RatedIndex *, int64_t>> lists;
    for (const auto &v : recs) lists.emplace_back(v.data(), (int64_t)v.size());
    const std::vector<pqa::RatedIndex> best = pqa::MergeTop(lists, pIn[0]);
    if (1 + 2 * (int64_t)best.size() > nOut) return -1;
    pOut[0] = (int64_t)best.size();
    for (size_t k = 0; k < best.size(); k++) { std::memcpy(&pOut[1 + 2 * k], &best[k].priority, 8); pOut[2 + 2 * k] = best[k].index; }
    return 1 + 2 * (int64_t)best.size();
  }
  if (w == "rated_prefix") {   // {want, id base, n, then n x {value bits, eligible (0 / 1)}} -> {count, then the listed ids}: entry i has id base + i
    if (nIn < 3 || pIn[0] < 0 || pIn[2] < 0 || nIn != 3 + 2 * pIn[2]) return -1;
    const int64_t n = pIn[2];
    std::vector<double> v((size_t)n);
    for (int64_t i = 0; i < n; i++) {
      if (pIn[4 + 2 * i] != 0 && pIn[4 + 2 * i] != 1) return -1;
      std::memcpy(&v[(size_t)i], &pIn[3 + 2 * i], 8);
    }
    std::vector<pqa::RatedIndex> recs((size_t)std::min(pIn[0], n));
    std::vector<int64_t> idx;
    const int64_t c = pqa::RatedPrefix(v.data(), n, pIn[0], [&](int64_t i) { return pIn[4 + 2 * i] == 1; }, [&](int64_t i) { return pIn[1] + i; }, recs.data(), idx);
    if (1 + c > nOut) return -1;
    pOut[0] = c;
    for (int64_t k = 0; k < c; k++) pOut[1 + k] = recs[(size_t)k].index;
    return 1 + c;
  }
  if (w == "group_tiles") {   // {maxEntries, maxGroups, nGroups, then the groups' counts} -> {nTiles, then the first group of every tile, nGroups}
    if (nIn < 3 || pIn[0] < 1 || pIn[1] < 1 || pIn[2] < 0 || nIn != 3 + pIn[2]) return -1;
    for (int64_t g = 0; g < pIn[2]; g++)
      if (pIn[3 + g] < 0) return -1;
    const std::vector<int64_t> tiles = pqa::PlanGroupTiles(pIn[2], pIn + 3, pIn[0], pIn[1]);
    if (1 + (int64_t)tiles.size() > nOut) return -1;
    pOut[0] = (int64_t)tiles.size() - 1;
    for (size_t k = 0; k < tiles.size(); k++) pOut[1 + k] = tiles[k];
    return 1 + (int64_t)tiles.size();
  }
  if (w == "review_plan") {   // {ldT, rowCap, budgetBytes, ldsAnswers, nPairs, then nPairs x {quiz, its answer count}} -> {nChunks, then per chunk its count and its pairs}
    if (nIn < 5 || pIn[0] < 1 || pIn[1] < 1 || pIn[2] < 0 || pIn[3] < 0 || pIn[4] < 0 || nIn != 5 + 2 * pIn[4]) return -1;
    std::vector<int64_t> quizOf((size_t)pIn[4]), answersOf((size_t)pIn[4]);
    for (int64_t i = 0; i < pIn[4]; i++) {
      quizOf[(size_t)i] = pIn[5 + 2 * i];
      answersOf[(size_t)i] = pIn[6 + 2 * i];
      if (answersOf[(size_t)i] < 1) return -1;
    }
    const std::vector<std::vector<int64_t>> chunks = pqa::PlanReviewChunks(pIn[4], quizOf.data(), answersOf.data(), pIn[0], pIn[1], pIn[2], pIn[3]);
    if (nOut < 1) return -1;
    pOut[0] = (int64_t)chunks.size();
    nRes = 1;
    for (const std::vector<int64_t> &c : chunks)
      if (!put(c)) return -1;
    return nRes;
  }
  if (w == "status_plan") {   // {tileCap, nPairs, then the pairs' quizzes} -> {nTiles, then per tile its count and its pairs}
    if (nIn < 2 || pIn[0] < 1 || pIn[1] < 0 || nIn != 2 + pIn[1] || nOut < 1) return -1;
    const pqa::RankTiles plan = pqa::PlanRankTiles(pIn[1], pIn + 2, pIn[0]);
    pOut[0] = plan.Tiles();
    nRes = 1;
    for (int64_t i = 0; i < plan.Tiles(); i++)
      if (!put(std::vector<int64_t>(plan.order.begin() + (std::ptrdiff_t)plan.start[(size_t)i], plan.order.begin() + (std::ptrdiff_t)plan.start[(size_t)i + 1]))) return -1;
    return nRes;
  }
  if (w == "better_pick") {
    if (nIn % 2 != 0 || nOut < 2) return -1;
    double p;   // (the script is what the exchanges hold: records {priority, index})
    PickOfRecords(reinterpret_cast<const char *>(pIn), nIn / 2, 16, &p, &pOut[1]);
    std::memcpy(&pOut[0], &p, 8);
    return 2;
  }
  return -1;
}
PQACORE_API int64_t PqaHip_HostLogicProbe(const char *what, const int64_t *pIn, const int64_t nIn, int64_t *pOut, const int64_t nOut) {
  return GuardedValue<int64_t>(nullptr, -1, [&](Error &) { return HostLogicProbe(what, pIn, nIn, pOut, nOut); });
}

}  // extern "C"
