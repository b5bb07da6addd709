// engine_interface.h -- the error object and the engine interface the C ABI is written against (c_abi.cpp, c_abi_shims.h), apart
// from the engines themselves (hip_engine.h): only the two public C headers and the stream's handle type are needed, so the C
// boundary compiles on a host without HIP.
#pragma once

#include <cstdint>
#include <string>
#include <utility>

#include "../../include/PqaHipExt.h"

typedef struct ihipStream_t *hipStream_t;   // (the opaque handle as <hip/hip_runtime_api.h> declares it)

namespace pqa {

// Error codes of reference PqaCore/Interface/PqaErrors.h:12-40
enum class ErrCode : int64_t {
  None = 0, NotImplemented = 1, SRException = 2, StdException = 3, InsufficientEngineDimensions = 4,
  MaintenanceModeChangeInProgress = 5, MaintenanceModeAlreadyThis = 6, ObjectShutDown = 7, IndexOutOfRange = 8,
  Internal = 9, Aggregate = 10, NegativeCount = 11, NonPositiveAmount = 12, AbsentId = 13, WrongMode = 14,
  UnhandledCase = 15, I64Underflow = 16, QuestionsExhausted = 17, NoQuizActiveQuestion = 18, CantOpenFile = 19,
  FileOp = 20, QuizzesActive = 21, NullArgument = 22, WrongRuntimeType = 23, NotInitialized = 24
};

// PqaError (reference PqaCore/Interface/PqaErrors.h:56-91): code + message + stringified params
struct Error {
  ErrCode code = ErrCode::None;
  std::string message;
  std::string params;   // what IPqaErrorParams::ToString() would give; empty = nullptr params
  bool hasParams = false;
  bool ok() const { return code == ErrCode::None; }
  std::string ToString(bool withParams) const;  // reference PqaCore/PqaErrors.cpp:128-143
  static Error Make(ErrCode c, std::string msg) { Error e; e.code = c; e.message = std::move(msg); return e; }
  static Error MakeP(ErrCode c, std::string params, std::string msg) {
    Error e; e.code = c; e.message = std::move(msg); e.params = std::move(params); e.hasParams = true; return e;
  }
};
const char *ErrCodeName(ErrCode c);  // reference PqaCore/PqaErrors.cpp:13-62

struct AQ { int64_t iQuestion, iAnswer; };

// What the C ABI (c_abi.cpp) drives: one engine on one device (HipEngine), or the question axis of one knowledge base split
// over several devices of the process (ShardedEngine, sharded_engine.cpp) -- the reference's IPqaEngine surface
// (PqaCore/Interface/IPqaEngine.h:14-113) plus the additive calls of include/PqaHipExt.h.
class IEngine {
 public:
  virtual ~IEngine() {}
  virtual Error Train(int64_t nQuestions, const AQ *pAQs, int64_t iTarget, double amount) = 0;
  virtual uint64_t GetTotalQuestionsAsked(Error &err) = 0;
  virtual void CopyDims(CiEngineDimensions *pDims) const = 0;
  virtual int64_t StartQuiz(Error &err) = 0;
  virtual int64_t ResumeQuiz(Error &err, int64_t nAnswered, const AQ *pAQs) = 0;
  virtual int64_t NextQuestion(Error &err, int64_t iQuiz) = 0;
  virtual Error RecordAnswer(int64_t iQuiz, int64_t iAnswer) = 0;
  virtual int64_t GetActiveQuestionId(Error &err, int64_t iQuiz) = 0;
  virtual Error SetActiveQuestion(int64_t iQuiz, int64_t iQuestion) = 0;
  virtual int64_t ListTopTargets(Error &err, int64_t iQuiz, int64_t maxCount, CiRatedTarget *pDest) = 0;
  virtual Error RecordQuizTarget(int64_t iQuiz, int64_t iTarget, double amount) = 0;
  virtual Error ReleaseQuiz(int64_t iQuiz) = 0;
  virtual Error StartMaintenance(bool forceQuizzes) = 0;
  virtual Error FinishMaintenance() = 0;
  virtual Error Shutdown(const char *saveFilePath) = 0;
  virtual bool MapIds(int which, bool toPerm, int64_t count, int64_t *pIds) = 0;
  virtual bool EnsurePermQuizGreater(int64_t bound) = 0;
  virtual bool RemapQuizPermId(int64_t srcPermId, int64_t destPermId) = 0;
  virtual Error SaveKB(const char *filePath, bool doubleBuffer) = 0;
  virtual Error SaveKBAs(const char *filePath, uint8_t precType) = 0;      // (additive) in a chosen precision, whole engines
  virtual Error SaveKBShard(const char *filePath, uint8_t precType) = 0;   // (additive) a shard's part, in place
  virtual Error AddQsTs(int64_t nQuestions, CiAddQorTParam *pAqps, int64_t nTargets, CiAddQorTParam *pAtps) = 0;
  virtual Error RemoveQuestions(int64_t n, const int64_t *pQIds) = 0;
  virtual Error RemoveTargets(int64_t n, const int64_t *pTIds) = 0;
  virtual Error Compact(int64_t *pnQuestions, const int64_t **ppOldQuestions, int64_t *pnTargets, const int64_t **ppOldTargets) = 0;
  virtual Error ClearOldQuizzes(int64_t maxCount, double maxAgeSec) = 0;
  // ---- additive (PqaHipExt.h)
  virtual Error SetOption(const char *name, int64_t value) = 0;
  virtual int64_t GetOption(const char *name) const = 0;
  virtual const char *EvalKernelName() const = 0;
  virtual Error SetKB(const double *pA, const double *pD, const double *pB) = 0;
  virtual Error GetKB(double *pA, double *pD, double *pB) = 0;
  virtual Error FillSynthetic(double nTrain, double noiseAmp, uint64_t seed) = 0;
  virtual Error SetTargetGaps(int64_t n, const int64_t *ids) = 0;
  virtual Error SetQuestionGaps(int64_t n, const int64_t *ids) = 0;
  virtual Error EvalPriorities(int64_t iQuiz, double *pOut, int64_t n) = 0;
  virtual int64_t NextQuestionArgmax(Error &err, int64_t iQuiz) = 0;
  virtual int64_t NextQuestionSampled(Error &err, int64_t iQuiz, uint64_t rnd) = 0;
  virtual Error GetPriors(int64_t iQuiz, double *pOut, int64_t n) = 0;
  virtual Error NextQuestionArgmaxBatch(int64_t n, const int64_t *pQuizzes, int64_t *pOut) = 0;
  virtual Error NextQuestionSampledBatch(int64_t n, const int64_t *pQuizzes, const uint64_t *pRnd, int64_t *pOut) = 0;
  virtual Error NextQuestionBatch(int64_t n, const int64_t *pQuizzes, int64_t *pOut) = 0;
  virtual Error EvalPrioritiesBatch(int64_t n, const int64_t *pQuizzes, double *pOut) = 0;
  virtual Error SelectArgmaxBatch(int64_t n, const int64_t *pQuizzes, CiHipSelection *pOut) = 0;
  virtual Error Log2HotArray(const double *pIn, double *pOut, int64_t n) = 0;
  virtual hipStream_t GetStream() const = 0;
  virtual Error SetStream(hipStream_t s) = 0;
  virtual Error Synchronize() = 0;
  virtual Error Quiesce() = 0;
  virtual Error EnqueueSelectArgmax(int64_t iQuiz, void *pOut) = 0;
  virtual Error EnqueueSelectArgmaxFlag(int64_t iQuiz, void *pOut, void *pFlag, uint64_t flagValue) = 0;
  virtual Error EnqueueEval(int64_t iQuiz) = 0;
  virtual Error GetPriorDevicePtr(int64_t iQuiz, void **ppDev, int64_t *pLdT) = 0;
  virtual Error RecordAnswerRemote(int64_t iQuiz, int64_t iAnswer) = 0;
  virtual Error RecordAnswerBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pAnswers) = 0;
  virtual Error StartQuizBatch(int64_t n, int64_t *pQuizzes) = 0;
  virtual Error ResumeQuizBatch(int64_t n, const int64_t *pCounts, const AQ *pAQs, int64_t *pQuizzes) = 0;
  virtual Error TrainBatch(int64_t n, const int64_t *pCounts, const AQ *pAQs, const int64_t *pTargets, const double *pAmounts) = 0;
  virtual Error RecordQuizTargetBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pTargets, const double *pAmounts) = 0;
  virtual Error ListTopTargetsBatch(int64_t n, const int64_t *pQuizzes, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts) = 0;
  // the best targets within a listed set (include/PqaHipExt.h: PqaEngine_ListTopTargetsAmongBatch)
  virtual Error ListTopTargetsAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pListOf, int64_t nLists, const int64_t *pListCounts,
                                         const int64_t *pTargets, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts, double *pMass) = 0;
  virtual int64_t ListTopQuestions(Error &err, int64_t iQuiz, int64_t maxCount, CiRatedQuestion *pDest) = 0;
  virtual Error ListTopQuestionsBatch(int64_t n, const int64_t *pQuizzes, int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) = 0;
  virtual int64_t AnswerRowSlotBytes() const = 0;
  virtual Error PackAnswerRows(int64_t n, const AQ *pAQs, void *pDst, void *pFlag, uint64_t flagValue) = 0;
  virtual int64_t ResumeQuizFromRows(Error &err, int64_t nAnswered, const AQ *pAQs, const void *pRows) = 0;
  virtual Error ResumeQuizBatchFromRows(int64_t n, const int64_t *pCounts, const AQ *pAQs, const void *pRows, int64_t *pQuizzes) = 0;
  // a page of answers per quiz (include/PqaHipExt.h: PqaEngine_RecordAnswerPageBatch)
  virtual Error RecordAnswerPageBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const AQ *pAQs, double *pLikelihood) = 0;
  virtual Error RecordAnswerPageBatchFromRows(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const AQ *pAQs, double *pLikelihood,
                                              const void *pRows) = 0;
  // Compact on a shard that a process of its own drives: question blocks travel as a package.  The one-process sharded engine moves
  // its blocks itself: it plans and packs nothing, and compacts from no package as Compact does.
  virtual Error CompactPlanOf(int64_t *, int64_t *, int64_t *, const int64_t **, uint8_t *) { return NoBlocks("CompactPlan"); }
  virtual int64_t QuestionBlockSlotBytes() const { return -1; }
  virtual Error PackQuestionBlocks(int64_t, const int64_t *, void *, void *, uint64_t) { return NoBlocks("PackQuestionBlocks"); }
  virtual Error CompactFromBlocks(const void *pBlocks, int64_t, int64_t, int64_t *pnQuestions, const int64_t **ppOldQuestions, int64_t *pnTargets,
                                  const int64_t **ppOldTargets) {
    return pBlocks ? NoBlocks("CompactFromBlocks with a package") : Compact(pnQuestions, ppOldQuestions, pnTargets, ppOldTargets);
  }
  // The sampled selector across shards that separate processes drive (sampled_part.h): selection parts.  The one-process sharded
  // engine selects over its shards itself.
  virtual int64_t SampledPartBytes() const { return -1; }
  virtual Error PackSampledParts(int64_t, const int64_t *, void *, void *, uint64_t) { return NoParts("PackSampledParts"); }
  virtual Error SampledPickFromParts(int64_t, const int64_t *, const uint64_t *, const void *, int64_t, int64_t, CiHipSelection *) {
    return NoParts("SampledPickFromParts");
  }
  virtual Error TakeSampledPicks(int64_t, const int64_t *, const int64_t *, int64_t *) { return NoParts("TakeSampledPicks"); }
  // RecordAnswer for many quizzes across such shards: posterior packages.  The one-process sharded engine records over its shards
  // itself (RecordAnswerBatch).
  virtual int64_t PosteriorSlotBytes() const { return -1; }
  virtual Error PackAnswerPosteriors(int64_t, const int64_t *, const int64_t *, void *, void *, uint64_t) { return NoPosteriors("PackAnswerPosteriors"); }
  virtual Error RecordAnswerBatchFromPosteriors(int64_t, const int64_t *, const int64_t *, const void *) {
    return NoPosteriors("RecordAnswerBatchFromPosteriors");
  }
  // The Among calls: evaluate and select over a listed set of questions.  A process-per-GPU host merges its shards' winners itself
  // (PqaHip_SelectArgmaxAmongBatch); the one-process sharded engine does not offer them.
  virtual Error EvalPrioritiesAmongBatch(int64_t, const int64_t *, const int64_t *, const int64_t *, double *) { return NoAmong("EvalPrioritiesAmongBatch"); }
  virtual Error SelectArgmaxAmongBatch(int64_t, const int64_t *, const int64_t *, const int64_t *, CiHipSelection *) { return NoAmong("SelectArgmaxAmongBatch"); }
  virtual Error NextQuestionArgmaxAmongBatch(int64_t, const int64_t *, const int64_t *, const int64_t *, int64_t *) { return NoAmong("NextQuestionArgmaxAmongBatch"); }
  virtual Error NextQuestionSampledAmongBatch(int64_t, const int64_t *, const int64_t *, const int64_t *, const uint64_t *, int64_t *) {
    return NoAmong("NextQuestionSampledAmongBatch");
  }
  virtual Error NextQuestionAmongBatch(int64_t, const int64_t *, const int64_t *, const int64_t *, int64_t *) { return NoAmong("NextQuestionAmongBatch"); }
  // Targets that answer like a given one (include/PqaHipExt.h: PqaEngine_EvalTargetSimilarity and its neighbours); the one-process
  // sharded engine does not offer them.
  virtual Error EvalTargetSimilarity(int64_t, const int64_t *, double *, int64_t) { return NoSimilarity("EvalTargetSimilarity"); }
  virtual Error ListSimilarTargetsBatch(int64_t, const int64_t *, int64_t, CiRatedTarget *, int64_t *) { return NoSimilarity("ListSimilarTargetsBatch"); }
  virtual Error PackTargetSimilaritySums(int64_t, const int64_t *, void *, void *, uint64_t) { return NoSimilarity("PackTargetSimilaritySums"); }
  virtual Error ListSimilarTargetsFromSums(int64_t, const int64_t *, const void *, int64_t, CiRatedTarget *, int64_t *) {
    return NoSimilarity("ListSimilarTargetsFromSums");
  }
  // Questions whose answers a given one predicts (include/PqaHipExt.h: PqaEngine_EvalQuestionRedundancy and its neighbours); the
  // one-process sharded engine does not offer them.
  virtual Error EvalQuestionRedundancy(int64_t, const int64_t *, double *, int64_t) { return NoRedundancy("EvalQuestionRedundancy"); }
  virtual Error ListRedundantQuestionsBatch(int64_t, const int64_t *, int64_t, CiRatedQuestion *, int64_t *) { return NoRedundancy("ListRedundantQuestionsBatch"); }
  virtual int64_t QuestionWeightSlotBytes() const { return -1; }
  virtual Error PackQuestionWeights(int64_t, const int64_t *, void *, void *, uint64_t) { return NoRedundancy("PackQuestionWeights"); }
  virtual Error EvalQuestionRedundancyFromWeights(int64_t, const int64_t *, const void *, double *, int64_t) {
    return NoRedundancy("EvalQuestionRedundancyFromWeights");
  }
  virtual Error ListRedundantQuestionsFromWeights(int64_t, const int64_t *, const void *, int64_t, CiRatedQuestion *, int64_t *) {
    return NoRedundancy("ListRedundantQuestionsFromWeights");
  }
  // Questions that tell listed targets apart (include/PqaHipExt.h: PqaEngine_EvalTargetSeparation and its neighbour); the one-process
  // sharded engine does not offer them.
  virtual Error EvalTargetSeparation(int64_t, const int64_t *, const int64_t *, double *, int64_t) { return NoSeparation("EvalTargetSeparation"); }
  virtual Error ListSeparatingQuestionsBatch(int64_t, const int64_t *, const int64_t *, int64_t, CiRatedQuestion *, int64_t *) {
    return NoSeparation("ListSeparatingQuestionsBatch");
  }
  // What every answer to a question would do to a quiz (include/PqaHipExt.h: PqaEngine_PreviewAnswersBatch); the one-process sharded
  // engine does not offer it.
  virtual Error PreviewAnswersBatch(int64_t, const int64_t *, const int64_t *, int64_t, double *, double *, CiRatedTarget *, int64_t *) {
    return Error::MakeP(ErrCode::NotImplemented, "Feature=PreviewAnswersBatch on this engine",
                        "Answer previews are for whole engines and for shards that separate processes drive.");
  }
  // Where a quiz stands and where named targets stand in it (include/PqaHipExt.h: PqaEngine_QuizStatusBatch, PqaEngine_RankTargetsBatch):
  // every engine that holds posteriors answers -- whole engines, shards, and the one-process sharded engine through its shard 0.
  virtual Error QuizStatusBatch(int64_t, const int64_t *, int64_t, const double *, CiHipQuizStatus *, int64_t *, double *) {
    return Error::MakeP(ErrCode::NotImplemented, "Feature=QuizStatusBatch on this engine", "This engine does not report a quiz's status.");
  }
  virtual Error RankTargetsBatch(int64_t, const int64_t *, const int64_t *, double *, int64_t *) {
    return Error::MakeP(ErrCode::NotImplemented, "Feature=RankTargetsBatch on this engine", "This engine does not rank named targets.");
  }
  // What every question would tell a quiz, in bits (include/PqaHipExt.h: PqaEngine_EvalQuestionGainsBatch and its neighbour); the
  // one-process sharded engine does not offer them.
  virtual Error EvalQuestionGainsBatch(int64_t, const int64_t *, double *, int64_t) { return NoGains("EvalQuestionGainsBatch"); }
  virtual Error ListInformativeQuestionsBatch(int64_t, const int64_t *, int64_t, CiRatedQuestion *, int64_t *) { return NoGains("ListInformativeQuestionsBatch"); }
  // What every question would tell a quiz once a given set is answered, and a greedy page of questions (include/PqaHipExt.h:
  // PqaEngine_EvalConditionalGainsBatch and its neighbour): whole engines only.
  virtual Error EvalConditionalGainsBatch(int64_t, const int64_t *, const int64_t *, const int64_t *, double *, int64_t) { return NoPages("EvalConditionalGainsBatch"); }
  virtual Error ListQuestionPageBatch(int64_t, const int64_t *, const int64_t *, const int64_t *, int64_t, CiRatedQuestion *, int64_t *) {
    return NoPages("ListQuestionPageBatch");
  }
  // ... and their forms for a shard that a process of its own drives, the given questions' blocks in a block package (PqaHip_PackGivenBlocks,
  // PqaEngine_EvalConditionalGainsBatchFromBlocks, PqaHip_SelectPageStepFromBlocks); the one-process sharded engine does not offer them.
  virtual Error PackGivenBlocks(int64_t, const int64_t *, void *, void *, uint64_t) { return NoPages("PackGivenBlocks"); }
  virtual Error EvalConditionalGainsBatchFromBlocks(int64_t, const int64_t *, const int64_t *, const int64_t *, int64_t, const int64_t *, const void *, int64_t, double *,
                                                    int64_t) {
    return NoPages("EvalConditionalGainsBatchFromBlocks");
  }
  virtual Error SelectPageStepFromBlocks(int64_t, const int64_t *, const int64_t *, const int64_t *, int64_t, const int64_t *, const void *, int64_t, CiHipSelection *) {
    return NoPages("SelectPageStepFromBlocks");
  }
  // A quiz with each of its answers left out (include/PqaHipExt.h: PqaEngine_ReviewAnswersBatch) and the quiz's recorded answers; the
  // one-process sharded engine reads the answers and does not offer the review.
  virtual int64_t GetQuizAnswers(Error &err, int64_t iQuiz, AQ *pDest, int64_t capacity) = 0;
  virtual Error ReviewAnswersBatch(int64_t, const int64_t *, const int64_t *, int64_t, double *, double *, CiRatedTarget *, int64_t *) {
    return Error::MakeP(ErrCode::NotImplemented, "Feature=ReviewAnswersBatch on this engine",
                        "Answer reviews are for whole engines and for shards that separate processes drive.");
  }
  virtual Error ReviewAnswersBatchFromRows(int64_t n, const int64_t *pQuizzes, const int64_t *pPositions, int64_t maxCount, double *pLikelihood, double *pEntropy,
                                           CiRatedTarget *pDest, int64_t *pCounts, const void *, const int64_t *) {
    return ReviewAnswersBatch(n, pQuizzes, pPositions, maxCount, pLikelihood, pEntropy, pDest, pCounts);
  }

 protected:
  static Error NoPages(const char *what) {
    return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + what + " on this engine",
                        "Question pages need the given questions' blocks, which one rank holds: the plain calls are for whole engines, the FromBlocks forms "
                        "for shards that separate processes drive.");
  }

 private:
  static Error NoGains(const char *what) {
    return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + what + " on this engine",
                        "Question gains are for whole engines and for shards that separate processes drive.");
  }
  static Error NoSeparation(const char *what) {
    return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + what + " on this engine",
                        "Target separation is for whole engines and for shards that separate processes drive.");
  }
  static Error NoRedundancy(const char *what) {
    return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + what + " on this engine",
                        "Question redundancy is for whole engines and for shards that separate processes drive.");
  }
  static Error NoSimilarity(const char *what) {
    return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + what + " on this engine",
                        "Target similarity is for whole engines and for shards that separate processes drive.");
  }
  static Error NoAmong(const char *what) {
    return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + what + " on this engine",
                        "The Among calls are for whole engines and for shards that separate processes drive.");
  }
  static Error NoPosteriors(const char *what) {
    return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + what + " on this engine", "Posterior packages are for shards that separate processes drive.");
  }
  static Error NoParts(const char *what) {
    return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + what + " on this engine", "Selection parts are for shards that separate processes drive.");
  }
  static Error NoBlocks(const char *what) {
    return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + what + " on this engine", "Question block packages are for shards that separate processes drive.");
  }
};

}  // namespace pqa
