// hip_engine.h -- host side of the MI355X engine behind the PqaCore C ABI.
//
// Mirrors the reference's engine interface for the hot path (reference: ProbQA/PqaCore/Interface/IPqaEngine.h:14-112;
// behaviour of PqaCore/BaseEngine.cpp and PqaCore/CpuEngine.cpp for StartQuiz / ResumeQuiz / NextQuestion /
// RecordAnswer / active-question bookkeeping / quiz registry / error objects).  All arithmetic runs in the gfx950
// kernels of pqa_kernels.h; this file only owns device memory, the quiz table and the reference's error behaviour.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <cstdio>
#include <ctime>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/PqaHipExt.h"
#include "engine_interface.h"   // ErrCode, Error, AQ, IEngine
#include "pqa_kernels.h"
#include "combining.h"
#include "selection_host.h"   // the selection codes, PriorityView, TakePriorities, the host's selector and the finish over a snapshot
#include "kb_plan.h"
#include "engine_options.h"

namespace pqa {

// SRDefaultLogger (reference SRPlatform/SRDefaultLogger.cpp): stderr until Init names a file, that file afterwards.
struct DefaultLogger {
  enum class Severity : uint8_t { None = 0, Info, Warning, Error, Critical };   // ISRLogger::Severity
  static std::string Init(const char *baseName);   // "" on success, the error text otherwise
  static void Log(Severity sev, const std::string &message);
};

// The two-way map between the dense ("compact") ids the arrays are indexed by and the ids a caller may keep across edits of the
// knowledge base ("permanent": never reissued).  Behaviour of the reference's PermanentIdManager (PqaCore/PermanentIdManager.h)
// as its callers and the .kb format see it; the structure is this file's own: the forward table is the array the file stores,
// the reverse direction is a vector ordered by permanent id -- ids are issued in increasing order, so it grows at its end -- whose
// entries are only trusted when the forward table agrees (a vacated slot leaves its entry behind; it is swept out when half of
// the vector is such leftovers).
class IdLedger {
 public:
  static constexpr int64_t kNone = -1;                  // cInvalidPqaId
  int64_t PermanentOf(int64_t slot) const { return InRange(slot) ? _permOf[(size_t)slot] : kNone; }
  int64_t SlotOf(int64_t permanent) const;
  bool Write(FILE *f, bool withoutSlots = false) const; // {next id to issue, slot count, the forward table}: the file's layout
  bool Read(FILE *f);
  bool RaiseFloor(int64_t bound);                       // ids issued from now on exceed `bound`; false if they did already
  bool Vacate(int64_t slot);                            // the slot's permanent id is retired
  bool Reissue(int64_t slot);                           // a vacated slot gets the next permanent id
  bool Extend(int64_t nSlots);                          // new slots at the end, each under the next permanent id
  bool Repack(int64_t nSlots, const int64_t *from);     // slot i takes over what slot from[i] held; nothing else survives
  bool Rename(int64_t permanent, int64_t toPermanent);  // a live id is re-labelled with an unused id from the past
  int64_t LiveSlots() const { return _live; }
  void Clear() { _permOf.clear(); _byPerm.clear(); _live = 0; }

 private:
  struct Back { int64_t permanent, slot; };
  bool InRange(int64_t slot) const { return slot >= 0 && slot < (int64_t)_permOf.size(); }
  bool Live(const Back &b) const { return _permOf[(size_t)b.slot] == b.permanent; }
  size_t LowerBound(int64_t permanent) const;
  void Enter(int64_t permanent, int64_t slot);
  void Rebuild();
  int64_t _issueNext = 0;
  int64_t _live = 0;                 // slots that hold a permanent id
  std::vector<int64_t> _permOf;      // slot -> permanent id, kNone for a vacated slot
  std::vector<Back> _byPerm;         // ascending by permanent id; at most one entry per id
};

// Which quizzes a ClearOldQuizzes(maxCount, maxAgeSec) call lets go (behaviour of BaseEngine::ClearOldQuizzes): every quiz
// unused for longer than maxAgeSec, then the longest-unused of the rest until maxCount remain.  `quizzes` in registry order;
// the result in the order they are to be released (it decides which registry slots the next quizzes reuse first): the aged-out
// ones in registry order, then by age, the longest-unused first, equal ages by registry order.
struct QuizUsage { int64_t id; time_t lastUsage; };
std::vector<int64_t> QuizzesToLetGo(const std::vector<QuizUsage> &quizzes, time_t now, int64_t maxCount, double maxAgeSec);

// The frame of a .kb file around the arrays (layout: hip_engine_kb.cpp), one copy for the one-device and the sharded engine:
// KbHeader in front of them -- the file's first 40 bytes as they are -- and behind them the gap lists (i64 n, n ids: questions,
// targets) and PermanentIdManager x3 (questions, targets, quizzes saved empty).  KbFile closes what is still open when it goes.
uint64_t PackPrecision(uint64_t type, uint64_t mantissa, uint64_t exponent);   // PrecisionDefinition (8 B)
struct KbHeader {
  uint64_t precision;
  int64_t K, Q, T;             // EngineDimensions {nAnswers, nQuestions, nTargets}
  uint64_t nAsked;
  CiEngineDefinition Definition() const;   // (precision unpacked; _initAmount = 1: not stored, every count is read from the file)
};
Error FileErr(const char *path, const char *msg);   // FileOp, with the path
Error KbOverflowErr(const char *filePath, const char *array, uint64_t count);   // finite values of an array do not fit fp32
// precType of a save (0: own) -> the header's PrecisionDefinition and the bytes of the file's number type; of a load -> the definition
Error KbSavePrecision(uint8_t precType, uint8_t ownType, uint32_t ownMantissa, uint16_t ownExponent, uint64_t &packed, int &fileElem);
Error KbLoadDefinition(const KbHeader &h, uint8_t precType, CiEngineDefinition &def);
struct KbFile {
  FILE *f = nullptr;
  const char *path;
  Error opened;                // why there is no file: no name, or it cannot be opened -- what the header calls answer then
  struct InPlace {};
  KbFile(const char *filePath, bool write);
  KbFile(const char *filePath, InPlace);   // for writing, created where missing, NOT emptied: a shard's part of a save
  Error CheckHeader(const KbHeader &h, KbLayout &layout) const;   // the dimensions make sense and the arrays fit the file's size
  int64_t Size() const;
  Error Seek(int64_t offset);
  ~KbFile() { if (f) std::fclose(f); }
  Error WriteHeader(const KbHeader &h);
  Error ReadHeader(KbHeader &h);
  Error WriteTrailer(const std::vector<int64_t> &qGaps, const std::vector<int64_t> &tGaps, const IdLedger &questionIds,
                     const IdLedger &targetIds, const IdLedger &quizIds);
  Error ReadTrailer(int64_t Q, int64_t T, std::vector<int64_t> &qGaps, std::vector<int64_t> &tGaps, IdLedger &questionIds,
                    IdLedger &targetIds, IdLedger &quizIds);   // every gap id checked against its dimension
  Error FlushAndClose();
};

// What every maintenance-mode operation answers in another mode, and what a removal answers to bad arguments or to an id that is
// out of range, a gap already, or repeated within the call (kb_plan.h: FirstBadRemoval) -- nothing has changed then.
Error WrongModeErr(const char *what);
Error CheckAddArgs(int64_t nQuestions, const CiAddQorTParam *pAqps, int64_t nTargets, const CiAddQorTParam *pAtps);   // AddQsTs: counts, arrays
template <typename IsGap>
Error CheckRemoval(int64_t n, const int64_t *ids, int64_t limit, IsGap isGap, const char *msg) {
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "Counts must be non-negative.");
  if (n > 0 && !ids) return Error::Make(ErrCode::NullArgument, "Nullptr ids array.");
  const int64_t bad = FirstBadRemoval(n, ids, limit, isGap);
  return bad < 0 ? Error() : Error::MakeP(ErrCode::AbsentId, "id=" + std::to_string(ids[bad]), msg);
}

// A quiz's own lines of host-coherent pinned memory: what the kernels working for ONE quiz hand to the host without a copy --
// the posterior's best targets (listed by RecordAnswer's kernel ahead of the ListTopTargets that follows it) and their flag.
// Per quiz, so that the quizzes of different client threads never wait for each other's results.
constexpr int kQuizTop = 32;
struct QuizPinned {
  RatedTargetDev top[kQuizTop];
  int64_t nOut;
  uint64_t topFlag;
  uint64_t pad[6];
};

// The pinned result lines of a batched listing, records | counts[entries] | tail[entries]: written by the listing kernels, read behind a stream synchronise or polled.
// They only grow: Ensure synchronises `stream` before a block goes, zero-fills the new one (no listing has operation number 0), and leaves {nullptr, 0} where it fails.
struct ResultLines {
  RatedTargetDev *records = nullptr;
  int64_t capacity = 0, entries = 0;   // the records the block holds, and the counts (and tail entries) behind them
  hipError_t Ensure(hipStream_t stream, int64_t needRecords, size_t tailBytesPerEntry, int64_t nEntries, unsigned flags);
  int64_t *Counts() const { return reinterpret_cast<int64_t *>(records + capacity); }
  template <typename T> T *Tail() const { return reinterpret_cast<T *>(Counts() + entries); }
  void Free();
};

struct Quiz {
  time_t lastUsage = 0;                // reference BaseQuiz::OnUsage
  double *dPrior = nullptr;            // ldT doubles, device
  uint32_t *dAsked = nullptr;          // device bitmap over LOCAL questions
  std::vector<uint32_t> hAsked;        // host mirror
  std::vector<AQ> answers;             // global question ids
  int64_t activeQuestion = -1;         // global id (reference CEQuiz::_activeQuestion)
  uint64_t priorVersion = 0;           // bumped whenever the posterior changes
  uint64_t serial = 0;                 // unique per created quiz: a registry slot reused by a later quiz is not this quiz
  int lateStreak = 0;                  // selections in a row whose (lazily fixed) sweep had listed rows at the pole: from the third on, RecordAnswer's
                                       // speculative sweep gets its fix-up launched right behind it again (it will be needed, and runs while the client is elsewhere)
  bool noServer = false;               // the resident sweep has answered a step of this quiz with -4 (a row at the pole of the lack term:
                                       // pole_kernels.hip) -- from here on its selections are launched, with the fix behind them
  QuizPinned *pin = nullptr;           // this quiz's host-coherent result lines (pooled by the engine)
  void *dRowStage = nullptr;           // sharded engine without peer access: the two rows of an answered question another shard holds, copied here
  // the listing in pin->top: made by the kernel that published `topOp` to pin->topFlag, of the posterior `topVersion`
  uint64_t topOp = 0, topVersion = 0;
  int64_t topCount = 0;
  std::atomic<bool> updatePending{false};   // a RecordAnswer of this quiz waits in the engine's list of deferred updates
  // A client of a combined sweep is selecting for this quiz outside the engine's lock (SelectFromPriorities): the quiz object
  // stays until it is done (a ReleaseQuiz from another thread -- a client's error, IPqaEngine.h:44 -- waits).
  std::atomic<bool> inSelection{false};
};

class HipEngine : public IEngine {
 public:
  static HipEngine *Create(Error &err, const CiEngineDefinition &def, const CiHipShard *shard);
  ~HipEngine() override;

  // ---- reference IPqaEngine surface (names as in IPqaEngine.h)
  Error Train(int64_t nQuestions, const AQ *pAQs, int64_t iTarget, double amount) override;
  uint64_t GetTotalQuestionsAsked(Error &err) override;
  void CopyDims(CiEngineDimensions *pDims) const override;
  int64_t StartQuiz(Error &err) override;
  int64_t ResumeQuiz(Error &err, int64_t nAnswered, const AQ *pAQs) override;
  int64_t NextQuestion(Error &err, int64_t iQuiz) override;
  Error RecordAnswer(int64_t iQuiz, int64_t iAnswer) override;
  int64_t GetActiveQuestionId(Error &err, int64_t iQuiz) override;
  Error SetActiveQuestion(int64_t iQuiz, int64_t iQuestion) override;
  int64_t ListTopTargets(Error &err, int64_t iQuiz, int64_t maxCount, CiRatedTarget *pDest) override;
  Error RecordQuizTarget(int64_t iQuiz, int64_t iTarget, double amount) override;
  Error ReleaseQuiz(int64_t iQuiz) override;
  Error StartMaintenance(bool forceQuizzes) override;
  Error FinishMaintenance() override;
  Error Shutdown(const char *saveFilePath) override;
  // which: 0 questions, 1 targets, 2 quizzes; toPerm: compact -> permanent (reference BaseEngine.cpp:150-215)
  bool MapIds(int which, bool toPerm, int64_t count, int64_t *pIds) override;
  bool EnsurePermQuizGreater(int64_t bound) override;
  bool RemapQuizPermId(int64_t srcPermId, int64_t destPermId) override;
  Error SaveKB(const char *filePath, bool doubleBuffer) override;
  Error SaveKBAs(const char *filePath, uint8_t precType) override;
  Error SaveKBShard(const char *filePath, uint8_t precType) override;
  static HipEngine *Load(Error &err, const char *filePath);
  // precType 0: the file's; shard != nullptr: questions [shard->_qFirst, + nLocal) of the file on shard->_device
  static HipEngine *LoadAs(Error &err, const char *filePath, uint8_t precType, const CiHipShard *shard, int64_t nLocal);
  Error AddQsTs(int64_t nQuestions, CiAddQorTParam *pAqps, int64_t nTargets, CiAddQorTParam *pAtps) override;
  Error RemoveQuestions(int64_t n, const int64_t *pQIds) override;
  Error RemoveTargets(int64_t n, const int64_t *pTIds) override;
  Error Compact(int64_t *pnQuestions, const int64_t **ppOldQuestions, int64_t *pnTargets, const int64_t **ppOldTargets) override;
  // ---- maintenance on a shard that a process of its own drives (hip_engine_kb.cpp): AddQsTs / RemoveQuestions / RemoveTargets are
  // collective and replicated -- every rank makes the same call --; Compact moves whole question blocks between the ranks as a
  // BLOCK PACKAGE: slot i = the K + 1 rows of the source of question move i of the plan, T elements each at the pitch of the current T
  Error CompactPlanOf(int64_t *pnQuestions, int64_t *pnTargets, int64_t *pnMoves, const int64_t **ppMoves, uint8_t *pWouldBeEmpty) override;
  int64_t QuestionBlockSlotBytes() const override { return (_K + 1) * RoundLdT(_T, _elem) * (int64_t)_elem; }
  Error PackQuestionBlocks(int64_t n, const int64_t *pQuestions, void *pDst, void *pFlag, uint64_t flagValue) override;
  Error CompactFromBlocks(const void *pBlocks, int64_t slotBytes, int64_t emptiedRank, int64_t *pnQuestions, const int64_t **ppOldQuestions,
                          int64_t *pnTargets, const int64_t **ppOldTargets) override;
  Error ClearOldQuizzes(int64_t maxCount, double maxAgeSec) override;

  // ---- additive (PqaHipExt.h)
  Error SetOption(const char *name, int64_t value) override;
  int64_t GetOption(const char *name) const override;
  const char *EvalKernelName() const override;
  Error SetKB(const double *pA, const double *pD, const double *pB) override;
  Error GetKB(double *pA, double *pD, double *pB) override;
  Error FillSynthetic(double nTrain, double noiseAmp, uint64_t seed) override;
  Error SetTargetGaps(int64_t n, const int64_t *ids) override;
  Error SetQuestionGaps(int64_t n, const int64_t *ids) override;
  Error EvalPriorities(int64_t iQuiz, double *pOut, int64_t n) override;
  int64_t NextQuestionArgmax(Error &err, int64_t iQuiz) override;
  int64_t NextQuestionSampled(Error &err, int64_t iQuiz, uint64_t rnd) override;
  Error GetPriors(int64_t iQuiz, double *pOut, int64_t n) override;
  int64_t NextQuestionArgmaxGraph(Error &err, Quiz *q);
  Error NextQuestionArgmaxBatch(int64_t n, const int64_t *pQuizzes, int64_t *pOut) override;
  // the reference's selector (NextQuestionSampled) for many quizzes: one batched sweep, one selector launch behind it
  Error NextQuestionSampledBatch(int64_t n, const int64_t *pQuizzes, const uint64_t *pRnd, int64_t *pOut) override;
  Error NextQuestionBatch(int64_t n, const int64_t *pQuizzes, int64_t *pOut) override;   // by option "select", random numbers drawn in batch order
  Error EvalPrioritiesBatch(int64_t n, const int64_t *pQuizzes, double *pOut) override;
  Error SelectArgmaxBatch(int64_t n, const int64_t *pQuizzes, CiHipSelection *pOut) override;   // pOut[i][q], q < local question count
  Error Log2HotArray(const double *pIn, double *pOut, int64_t n) override;  // device log2hot over an array (tests)
  hipStream_t GetStream() const override { return _stream; }
  Error SetStream(hipStream_t s) override;
  Error Synchronize() override;
  Error Quiesce() override;
  Error EnqueueSelectArgmax(int64_t iQuiz, void *pOut) override;
  Error EnqueueSelectArgmaxFlag(int64_t iQuiz, void *pOut, void *pFlag, uint64_t flagValue) override;
  Error EnqueueEval(int64_t iQuiz) override;
  Error GetPriorDevicePtr(int64_t iQuiz, void **ppDev, int64_t *pLdT) override;
  Error RecordAnswerRemote(int64_t iQuiz, int64_t iAnswer) override;
  Error RecordAnswerBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pAnswers) override;
  Error StartQuizBatch(int64_t n, int64_t *pQuizzes) override;
  Error ResumeQuizBatch(int64_t n, const int64_t *pCounts, const AQ *pAQs, int64_t *pQuizzes) override;
  Error TrainBatch(int64_t n, const int64_t *pCounts, const AQ *pAQs, const int64_t *pTargets, const double *pAmounts) override;
  Error RecordQuizTargetBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pTargets, const double *pAmounts) override;
  Error ListTopTargetsBatch(int64_t n, const int64_t *pQuizzes, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts) override;
  // the best targets within a listed set, and the posterior's total over it (hip_engine_top_among.cpp)
  Error ListTopTargetsAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pListOf, int64_t nLists, const int64_t *pListCounts,
                                 const int64_t *pTargets, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts, double *pMass) override;
  // what every answer to a question would do to a quiz: likelihood, entropy and best targets of each would-be posterior (hip_engine_preview.cpp)
  Error PreviewAnswersBatch(int64_t nPairs, const int64_t *pQuizzes, const int64_t *pQuestions, int64_t maxCount, double *pLikelihood, double *pEntropy,
                            CiRatedTarget *pDest, int64_t *pCounts) override;
  // where a quiz stands -- entropy, mass, best target, candidates, the candidates above given levels -- and where named targets stand in
  // it: rank and probability (hip_engine_status.cpp)
  Error QuizStatusBatch(int64_t nQuizzes, const int64_t *pQuizzes, int64_t nLevels, const double *pLevels, CiHipQuizStatus *pStatus, int64_t *pLevelCounts,
                        double *pLevelMass) override;
  Error RankTargetsBatch(int64_t nPairs, const int64_t *pQuizzes, const int64_t *pTargets, double *pProb, int64_t *pRank) override;
  // what every question of this engine would tell a quiz: its information gain in bits, as rows and as a listing (hip_engine_gain.cpp)
  Error EvalQuestionGainsBatch(int64_t nQuizzes, const int64_t *pQuizzes, double *pOut, int64_t n) override;
  Error ListInformativeQuestionsBatch(int64_t nQuizzes, const int64_t *pQuizzes, int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) override;
  // what every question would tell a quiz once the answers to a given set of questions are known, and a page of questions filled
  // greedily by that number (hip_engine_page.cpp)
  Error EvalConditionalGainsBatch(int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven, double *pOut, int64_t n) override;
  Error ListQuestionPageBatch(int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven, int64_t pageSize, CiRatedQuestion *pDest,
                              int64_t *pCounts) override;
  // ... and on a shard that a process of its own drives: the given questions' blocks travel as a BLOCK PACKAGE (PackQuestionBlocks'
  // slots, packed in regular mode), the rank sweeps its own questions over the same branch rows, the host merges a page's steps
  Error PackGivenBlocks(int64_t n, const int64_t *pQuestions, void *pDst, void *pFlag, uint64_t flagValue) override;
  Error EvalConditionalGainsBatchFromBlocks(int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven, int64_t nBlocks,
                                            const int64_t *pBlockQuestions, const void *pBlocks, int64_t slotBytes, double *pOut, int64_t n) override;
  Error SelectPageStepFromBlocks(int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven, int64_t nBlocks,
                                 const int64_t *pBlockQuestions, const void *pBlocks, int64_t slotBytes, CiHipSelection *pOut) override;
  // a quiz's recorded answers, and the quiz with each of them left out: likelihood of the left-out answer, entropy and best targets of the
  // others' posterior (hip_engine_review.cpp)
  int64_t GetQuizAnswers(Error &err, int64_t iQuiz, AQ *pDest, int64_t capacity) override;
  Error ReviewAnswersBatch(int64_t nPairs, const int64_t *pQuizzes, const int64_t *pPositions, int64_t maxCount, double *pLikelihood, double *pEntropy,
                           CiRatedTarget *pDest, int64_t *pCounts) override;
  Error ReviewAnswersBatchFromRows(int64_t nPairs, const int64_t *pQuizzes, const int64_t *pPositions, int64_t maxCount, double *pLikelihood, double *pEntropy,
                                   CiRatedTarget *pDest, int64_t *pCounts, const void *pRows, const int64_t *pRowFirst) override;
  // the best next questions by priority (hip_engine_list.cpp): what EvalPriorities / EvalPrioritiesBatch return, listed on the device
  int64_t ListTopQuestions(Error &err, int64_t iQuiz, int64_t maxCount, CiRatedQuestion *pDest) override;
  Error ListTopQuestionsBatch(int64_t n, const int64_t *pQuizzes, int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) override;
  // ---- the Among calls (hip_engine_among.cpp): evaluate and select over a listed set of questions per quiz -- for the call, every
  // question outside the list counts as asked.  Quiz i's list: pCounts[i] GLOBAL ids from pQuestions[sum(pCounts[0..i))].
  Error EvalPrioritiesAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, double *pOut) override;
  Error SelectArgmaxAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, CiHipSelection *pOut) override;
  Error NextQuestionArgmaxAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, int64_t *pPicked) override;
  Error NextQuestionSampledAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, const uint64_t *pRnd,
                                      int64_t *pPicked) override;
  Error NextQuestionAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, int64_t *pPicked) override;
  // ---- a shard driven by a process of its own (hip_engine_resume.cpp): the rows of answered questions as a package -- slot i
  // = sA[q_i][k_i][0..ldT) then mD[q_i][0..ldT), in the cube's element type -- filled by the owners, consumed by every rank
  int64_t AnswerRowSlotBytes() const override { return 2 * _ldT * (int64_t)_elem; }
  Error PackAnswerRows(int64_t n, const AQ *pAQs, void *pDst, void *pFlag, uint64_t flagValue) override;
  int64_t ResumeQuizFromRows(Error &err, int64_t nAnswered, const AQ *pAQs, const void *pRows) override;
  Error ResumeQuizBatchFromRows(int64_t n, const int64_t *pCounts, const AQ *pAQs, const void *pRows, int64_t *pQuizzes) override;
  // ---- a page of answers per quiz in one launch (hip_engine_record_page.cpp): what SetActiveQuestion + RecordAnswer per answer
  // leave, bit for bit, with each step's total; FromRows: the rows of other shards' questions from a row package, as above
  Error RecordAnswerPageBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const AQ *pAQs, double *pLikelihood) override;
  Error RecordAnswerPageBatchFromRows(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const AQ *pAQs, double *pLikelihood,
                                      const void *pRows) override;
  // ---- the sampled selector across such shards (hip_engine_parts.cpp; layout: sampled_part.h): every rank packs a SELECTION PART per quiz
  // behind its batched sweep, the ranks all-gather the parts, every rank picks from all of them, the ranks agree on the one pick
  // that is not -1, and every rank takes it -- the fallback over the whole question axis, the active question, the count
  int64_t SampledPartBytes() const override;
  Error PackSampledParts(int64_t n, const int64_t *pQuizzes, void *pDst, void *pFlag, uint64_t flagValue) override;
  Error SampledPickFromParts(int64_t n, const int64_t *pQuizzes, const uint64_t *pRnd, const void *pParts, int64_t rank, int64_t world,
                             CiHipSelection *pOut) override;
  Error TakeSampledPicks(int64_t n, const int64_t *pQuizzes, const int64_t *pPicks, int64_t *pQuestions) override;
  // ---- RecordAnswer for many quizzes across such shards (hip_engine_record_parts.cpp): a POSTERIOR PACKAGE -- slot i = quiz i's
  // new posterior, T doubles at a pitch that depends on T alone -- filled by the holders of the active questions without changing
  // any quiz, summed over the ranks, consumed by every rank
  int64_t PosteriorSlotBytes() const override { std::lock_guard<EngineMutex> lk(_mu); return RoundLdT(_T, 8) * 8; }
  Error PackAnswerPosteriors(int64_t n, const int64_t *pQuizzes, const int64_t *pAnswers, void *pDst, void *pFlag, uint64_t flagValue) override;
  Error RecordAnswerBatchFromPosteriors(int64_t n, const int64_t *pQuizzes, const int64_t *pAnswers, const void *pPosteriors) override;
  // ---- the source queries (hip_engine_sources.cpp): targets that answer like a given one (sim(s, t)) and questions whose answers a
  // given one predicts (I(s, q)).  Eval / List on a whole engine; on a shard that a process of its own drives, its part of a package
  // that the ranks sum -- similarity: the sums over its questions; redundancy: its sources' weighted rows -- and Eval / List from the sum
  Error EvalTargetSimilarity(int64_t nSources, const int64_t *pSources, double *pOut, int64_t n) override;
  Error ListSimilarTargetsBatch(int64_t nSources, const int64_t *pSources, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts) override;
  Error PackTargetSimilaritySums(int64_t nSources, const int64_t *pSources, void *pDst, void *pFlag, uint64_t flagValue) override;
  Error ListSimilarTargetsFromSums(int64_t nSources, const int64_t *pSources, const void *pSums, int64_t maxCount, CiRatedTarget *pDest,
                                   int64_t *pCounts) override;
  Error EvalQuestionRedundancy(int64_t nSources, const int64_t *pSources, double *pOut, int64_t n) override;
  Error ListRedundantQuestionsBatch(int64_t nSources, const int64_t *pSources, int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) override;
  int64_t QuestionWeightSlotBytes() const override { std::lock_guard<EngineMutex> lk(_mu); return _K * RoundLdT(_T, 8) * 8; }
  Error PackQuestionWeights(int64_t nSources, const int64_t *pSources, void *pDst, void *pFlag, uint64_t flagValue) override;
  Error EvalQuestionRedundancyFromWeights(int64_t nSources, const int64_t *pSources, const void *pWeights, double *pOut, int64_t n) override;
  Error ListRedundantQuestionsFromWeights(int64_t nSources, const int64_t *pSources, const void *pWeights, int64_t maxCount, CiRatedQuestion *pDest,
                                          int64_t *pCounts) override;
  // ... and questions that tell listed targets apart (sep(G, q)): Eval / List on a whole engine AND on such a shard, for its own questions
  Error EvalTargetSeparation(int64_t nGroups, const int64_t *pGroupCounts, const int64_t *pTargets, double *pOut, int64_t n) override;
  Error ListSeparatingQuestionsBatch(int64_t nGroups, const int64_t *pGroupCounts, const int64_t *pTargets, int64_t maxCount, CiRatedQuestion *pDest,
                                     int64_t *pCounts) override;

  // ---- what a sharded engine needs from its shards (sharded_engine.cpp; implemented in hip_engine_shard.cpp)
  // An answer of a quiz as the sharded engine hands it to EVERY shard: the answered question in global numbering; for the shards
  // that do not hold it, its two rows where they are (the owner's cube: read in place over peer access, or -- `stage` -- copied
  // into the quiz's staging rows first).  `list`: this shard's kernel also lists the new posterior's best targets.
  struct ShardAnswer { int64_t iQuiz, qGlobal, iAnswer; const void *rowA, *rowD; int srcDevice; bool stage, list; };
  // Bookkeeping of RecordAnswer for each (CEQuiz::RecordAnswer, PqaCore/CEQuiz.h:77-122) and ONE launch for all the posteriors.
  Error ApplyAnswers(int64_t n, const ShardAnswer *answers);
  // A combined sweep for n distinct quizzes in two halves (the combining of concurrent NextQuestion calls, done by the sharded
  // engine over all its shards): EnqueueCombined validates, flushes, launches into batch context `ctx` (0 / 1) and snapshots the
  // quizzes' unavailable questions; CollectCombined waits for that launch -- without the engine's lock -- and gives per quiz the
  // shard's winner (argmax batches) or a view of its priority vector on the host (hostPriorities).
  struct CombinedFlight { uint64_t tag = 0; bool hostPriorities = false, quizMinor = false, tagged = false; int64_t Bp = 0, nQ = 0, n = 0; hipError_t he = hipSuccess; };
  Error EnqueueCombined(int ctx, int64_t n, const int64_t *pQuizzes, bool hostPriorities, CombinedFlight *flight,
                        std::vector<uint32_t> *unavailable /* n x UnavailableWordCount() words, local bit order */);
  Error CollectCombined(int ctx, const CombinedFlight &flight, CiHipSelection *winners, PriorityView *views);
  size_t UnavailableWordCount() const { return _hQGap.size(); }
  void SetExternalCallers(const std::atomic<int> *n) { _extCallers = n; }   // the sharded engine's count of client threads inside it
  Error FlushDeferred();   // launch whatever posterior updates are deferred (the sharded engine's training barrier)
  int Device() const { return _device; }
  int64_t FirstQuestion() const { return _qFirst; }
  int64_t LocalQuestions() const { return _Q; }
  int64_t RowLength() const { return _ldT; }
  bool OwnsQuestion(int64_t qGlobal) const { return qGlobal >= _qFirst && qGlobal < _qFirst + _Q; }
  const double *PriorityDevicePtr() const { return _dPriority; }   // filled by EnqueueEval, local question order
  void BumpQuestionsAsked(uint64_t n) { _nQuestionsAsked.fetch_add(n, std::memory_order_relaxed); }
  Error GetRowPointers(int64_t qGlobal, int64_t iAnswer, const void **ppA, const void **ppD);
  // rowDevices / stageRow (optional): the device each row lives on, and whether it is copied to this device first (no peer access)
  int64_t ResumeQuizRows(Error &err, int64_t nAnswered, const AQ *pAQs, const void *const *rows, const int *rowDevices = nullptr,
                         const char *stageRow = nullptr);
  // ResumeQuizBatch with the row pointers resolved by the sharded engine (2 sum(pCounts) of them, in entry order), staged as
  // ResumeQuizRows stages them
  Error ResumeQuizBatchRows(int64_t n, const int64_t *pCounts, const AQ *pAQs, const void *const *rows, const int *rowDevices,
                            const char *stageRow, int64_t *pQuizzes);
  // .kb arrays of this engine's questions at the file's current position (hip_engine_kb.cpp); the engine's lock is not taken
  // fileElem: bytes of the file's number type (0: the engine's); where it differs the rows pass through convert_rows_kernel
  Error IoRows(FILE *f, const char *filePath, bool mD, bool write, int fileElem = 0);
  Error IoVB(FILE *f, const char *filePath, bool write, int fileElem = 0);
  Error SetVBFromHost(const double *vb);
  void GetGapLists(std::vector<int64_t> &questionsGlobal, std::vector<int64_t> &targets) const {
    for (int64_t q : _questionGapList) questionsGlobal.push_back(q + _qFirst);
    targets = _targetGapList;
  }
  const IdLedger &TargetIds() const { return _targetIds; }
  void SetTargetIds(const IdLedger &l) { _targetIds = l; }
  void SetQuizIds(const IdLedger &l) { _quizIds = l; }
  void SetQuestionsAsked(uint64_t n) { _nQuestionsAsked.store(n); }
  uint8_t PrecisionType() const { return _precType; }
  uint32_t PrecMantissa() const { return _precMantissa; }
  uint16_t PrecExponent() const { return _precExponent; }
  Error UnavailableWords(int64_t iQuiz, std::vector<uint32_t> &words);
  // ListTopQuestions / ListTopQuestionsBatch in two halves likewise (the sharded engine has every shard's sweep and listing in flight
  // before it waits for the first): Enqueue* validates and launches, Collect* waits and hands over this shard's best
  // min(maxCount, local questions) per quiz, GLOBAL ids, pDest[i * stride + j], j < pCounts[i].  One listing at a time between the two.
  Error EnqueueTopQuestions(int64_t iQuiz, int64_t maxCount, bool haveDest);
  int64_t CollectTopQuestions(Error &err, CiRatedQuestion *pDest);
  Error EnqueueTopQuestionsBatch(int64_t n, const int64_t *pQuizzes, int64_t maxCount);
  Error CollectTopQuestionsBatch(int64_t n, int64_t stride, CiRatedQuestion *pDest, int64_t *pCounts);
  static Error CheckTopQuestionsBatchArgs(int64_t n, const int64_t *pQuizzes, int64_t maxCount, bool haveDest, bool haveCounts);   // what comes before the lock
  // a batched selection in two halves: every shard's sweep is in flight before the first one is waited for
  Error EnqueueBatch(int64_t n, const int64_t *pQuizzes, bool wantPriorities, uint64_t *pTag);
  Error CollectBatchSelections(int64_t n, uint64_t tag, CiHipSelection *pOut);
  Error CollectBatchPriorities(int64_t n, double *pOut);
  Error ValidateBatch(int64_t n, const int64_t *pQuizzes) { std::lock_guard<EngineMutex> lk(_mu); return ValidateBatchLocked(n, pQuizzes); }   // what EnqueueBatch would refuse; changes nothing
  Error ValidateTrain(int64_t nQuestions, const AQ *pAQs, int64_t iTarget, int64_t iQuiz);
  // The same for a whole TrainBatch (pQuizzes == nullptr) or RecordQuizTargetBatch (pCounts, pAQs unused); an error names its entry.
  // The argument checks that come before the lock are the static ones below, shared with the sharded engine.
  Error ValidateTrainBatch(int64_t n, const int64_t *pCounts, const AQ *pAQs, const int64_t *pTargets, const int64_t *pQuizzes);
  static Error CheckTrainBatchArgs(int64_t n, const int64_t *pCounts, const AQ *pAQs, const int64_t *pTargets, const double *pAmounts);
  static Error CheckQuizTargetBatchArgs(int64_t n, const int64_t *pQuizzes, const int64_t *pTargets, const double *pAmounts);
  bool IsRegularMode() const { return _mode == Mode::Regular; }
  bool IsMaintenanceMode() const { return _mode == Mode::Maintenance; }
  double InitAmount() const { return _initAmount; }
  const void *QuestionBlock(int64_t qLocal) const { return CubeAt(qLocal); }
  const void *RowPointer(int64_t qLocal, int64_t row) const { return CubeAt(qLocal, row); }   // row < K: sA[q][row][.]; row == K: mD[q][.]
  int64_t Answers() const { return _K; }
  int64_t CombinedBatchFor(int64_t waiting) const { return PreferredCombinedBatch(waiting); }
  const double *VBDevicePtr() const { return _dVB; }
  // a rebuilt shard takes its questions' rows from the old shards' cubes (in place, over peer access) ...
  Error AdoptRows(const std::vector<const void *> &srcBlocks, int64_t ldTsrc, const std::vector<int64_t> &colMap, const double *srcVB);
  // ... and initialises added target columns and questions as CpuEngine::AddQsTsSpec does (CpuEngine.cpp:497-567)
  Error ApplyFills(const std::vector<int64_t> &tIds, const std::vector<double> &tInit, const std::vector<int64_t> &qLocalIds,
                   const std::vector<double> &qInit);
  const IdLedger &QuizIds() const { return _quizIds; }

 private:
  HipEngine() = default;
  Error Init(const CiEngineDefinition &def, const CiHipShard *shard);
  KbView View() const;
  Quiz *UseQuiz(Error &err, int64_t iQuiz);                 // reference BaseEngine::UseQuiz, BaseEngine.cpp:399-419
  Error CheckRegular(const char *what) const;               // MaintenanceSwitch gate of BaseEngine.cpp:423-427 etc.
  int64_t CreateQuiz(Error &err, int64_t nAnswered, const AQ *pAQs, const void *const *rows, const double *srcPrior, int srcDevice,
                     hipEvent_t ready);  // CpuEngine::CreateQuizInternal
  void DestroyQuiz(Quiz *q);
  // gap/asked fallback + bookkeeping (CpuEngine.cpp:403-413) over the quiz's own bits and the gaps, or over a snapshot of both
  // (a combined sweep's, without the engine's lock: what is written is the quiz's own or atomic)
  int64_t FinishSelection(Error &err, Quiz *q, int64_t selLocal) { return FinishSelection(err, q, selLocal, _Q, _hQGap.data(), q->hAsked.data()); }
  int64_t FinishSelection(Error &err, Quiz *q, int64_t selLocal, int64_t nQ, const uint32_t *unavailable, const uint32_t *asked = nullptr);
  Error RecordAnswerImpl(int64_t iQuiz, int64_t iAnswer, bool remote);
  Error RecordAnswerLocked(int64_t iQuiz, int64_t iAnswer, bool remote, bool flushNow);
  // ---- batched ResumeQuiz (hip_engine_resume.cpp): the entries of a ResumeQuizBatch, of a drain's posted ResumeQuiz calls, or one
  // long-row ResumeQuiz.  rows (optional): the entry's 2 nAnswered row pointers, resolved by the sharded engine.
  struct ResumeEntry { int64_t nAnswered = 0; const AQ *pAQs = nullptr; const void *const *rows = nullptr; Error err; int64_t id = -1; Quiz *quiz = nullptr; };
  // allOrNone: any failing entry fails the call and no quiz is created (the entry's own error is in e[i].err); otherwise every
  // entry succeeds or fails on its own.  The ids are assigned in entry order once every launch has been checked.
  Error ResumeEntriesLocked(std::vector<ResumeEntry> &e, bool allOrNone);
  Error ResumeBatchEntriesLocked(int64_t n, const int64_t *pCounts, const AQ *pAQs, const void *const *rows, int64_t *pQuizzes);
  // a package's slots as row pointers (this engine's own questions: its cube); a package in host memory staged by option "rows_stage"
  Error PackageRowsLocked(int64_t total, const AQ *pAQs, const void *pRows, std::vector<const void *> &rows);
  Error EnsurePackList(int64_t words); // room for `words` 8-byte words in _dAqs and _hPack, the previous list's copy finished, the header zeroed
  Error SubmitPackList(int64_t words); // the copy of _hPack's first `words` words to _dAqs on the engine's stream, and the event behind it
  Error SubmitSources(int64_t n, const int64_t *pSources);   // EnsurePackList, the sources into _hPack[2 + i], MarkStreamBusy, SubmitPackList: they stay in _dAqs + 2
  int64_t *_hPack = nullptr;           // PackAnswerRows / PackQuestionBlocks: the pinned source of the pointer list, and the event behind the list's copy
  int64_t _hPackWords = 0;
  hipEvent_t _evPack = nullptr;
  // A device buffer {*p, have} that only grows: the engine's stream is synchronised before it is freed, a failed allocation leaves {nullptr, 0}
  hipError_t GrowDeviceBytes(void **p, size_t &have, size_t need);
  template <typename T> hipError_t GrowDevice(T **p, size_t &have, size_t need) { return GrowDeviceBytes(reinterpret_cast<void **>(p), have, need); }
  // Option "rows_stage", a package in registered host memory: p, or where its `bytes` were copied to (enqueued) in the growing buffer {*buf, have}, "rows_staged" counted; nullptr: err
  bool IsStagedHostMemory(const void *p) const;
  const void *StageHostPackage(const void *p, size_t bytes, void **buf, size_t &have, Error &err);
  void *_dRowStage = nullptr;          // the row and posterior packages' staging buffer
  size_t _rowStageBytes = 0;
  uint64_t _packCalls = 0, _packBytes = 0, _rowsStaged = 0;   // read-only "pack_calls", "pack_bytes", "rows_staged"
  hipError_t TakeQuizBuffers(Quiz *q);
  // the batch's device tables -- slots, statuses, asked bitmaps, row pointers, long-row sums, exponent scratch -- and their
  // pinned host mirror: grown to the largest chunk so far, reused by every batch after it
  char *_dResume = nullptr, *_hResume = nullptr;
  size_t _dResumeBytes = 0, _hResumeBytes = 0;
  uint64_t _resumeBatches = 0, _resumesBatched = 0;   // options "resume_batches", "resumes_batched": drains that ran posted ResumeQuiz calls, and those calls
  // ---- pages of answers (hip_engine_record_page.cpp): a chunk's tables -- slots | row pointers | local question indices, and behind
  // them on the device the likelihoods -- with their pinned source and the event behind its copy (nothing else waits for a chunk
  // without likelihoods), the pinned lines the likelihoods come back in, the events of option "time_sweeps".  They grow and stay.
  struct RecordPageStage {
    char *dTables = nullptr, *hTables = nullptr;
    size_t dBytes = 0, hBytes = 0;
    double *hLikelihood = nullptr;
    size_t hLikelihoodCount = 0;
    hipEvent_t evCopy = nullptr, ev[2] = {nullptr, nullptr};
  } _recPage;
  void FreeRecordPage();
  Error RecordPages(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const AQ *pAQs, double *pLikelihood, bool fromRows, const void *pRows);
  // read-only "record_page_calls", "page_answers", "page_launches", "record_page_device_ns" ("page_calls" and "page_device_ns" are the question pages')
  uint64_t _recPageCalls = 0, _recPageAnswers = 0, _recPageLaunches = 0, _recPageDeviceNs = 0;
  StartBatchInline *_startBatch = nullptr;   // StartQuizBatch: CreateQuiz queues the new quizzes' buffers here instead of launching
  // the steps of one training call in execution order, appended to `out`; scratch: the caller's, reused from call to call
  void AppendTrainSteps(int64_t n, const AQ *pAQs, bool fromQuiz, std::vector<TrainStep> &out, std::vector<int64_t> &scratch) const;
  void BuildTrainSteps(int64_t n, const AQ *pAQs, bool fromQuiz, std::vector<TrainStep> &steps, std::vector<int64_t> &chainStart) const;
  // ---- many trainings in one call (hip_engine_train.cpp)
  struct TrainRecord { const AQ *pAQs; int64_t n, iTarget; double amount; };
  struct TrainBulk;                    // host scratch, pinned and device staging, events: kept from call to call
  TrainBulk *_tb = nullptr;
  void FreeTrainBulk();
  Error ValidateTrainBatchLocked(int64_t n, const int64_t *pCounts, const AQ *pAQs, const int64_t *pTargets, const int64_t *pQuizzes);
  Error TrainRecordsLocked(const std::vector<TrainRecord> &recs, bool fromQuiz);
  uint64_t _trainBulkCalls = 0, _trainBulkRecords = 0, _trainBulkLaunches = 0, _trainBulkHostNs = 0, _trainBulkDeviceNs = 0;
  Error TrainLocked(int64_t nQuestions, const AQ *pAQs, int64_t iTarget, double amount, bool fromQuiz);
  Error ValidateTrainLocked(int64_t nQuestions, const AQ *pAQs, int64_t iTarget) const;
  Error UploadGaps();
  Error RemoveIds(int64_t n, const int64_t *ids, int64_t limit, std::vector<uint32_t> &gapBits, std::vector<int64_t> &gapList, IdLedger &ledger,
                  const char *absentMsg);   // RemoveQuestions / RemoveTargets: all ids validated, then flagged, listed and retired
  Error ReallocKB(int64_t newQ, int64_t newT, int64_t newQTotal);   // grow the device cube / vB / per-question buffers (newQ: this engine's questions)
  Error CompactLocked(bool fromBlocks, const void *pBlocks, int64_t slotBytes, int64_t emptiedRank, int64_t *pnQuestions,
                      const int64_t **ppOldQuestions, int64_t *pnTargets, const int64_t **ppOldTargets);
  bool IsShard() const { return _qTotal != _Q; }             // holds a part of the question axis (_qFirst + _Q <= _qTotal always)
  int64_t AssignQuiz(Quiz *q);                               // reference BaseEngine::AssignQuiz, BaseEngine.cpp:780-793
  void UnassignQuiz(int64_t iQuiz);

  enum class Mode { Regular, Maintenance, Shutdown };

  int64_t _K = 0, _Q = 0, _T = 0, _ldT = 0, _qFirst = 0, _qTotal = 0;
  double _initAmount = 1;
  int _device = 0;
  hipStream_t _stream = nullptr, _ownStream = nullptr;
  // the cube: [Q][K+1][ldT] elements of _elem bytes -- double for Double engines, float for Float engines (reference
  // PqaCore/Interface/PqaCommon.h:17-24; the reference instantiates Float for its GPU engine, PqaEngineBaseFactory.cpp:124-142).
  // Everything else (vB, the quizzes' posteriors, priorities) is fp64 in both.
  char *_dCube = nullptr;
  int _elem = 8;
  uint8_t _precType = 3;
  char *CubeAt(int64_t q, int64_t row = 0) const { return _dCube + ((size_t)(q * (_K + 1) + row) * (size_t)_ldT) * (size_t)_elem; }
  static int64_t RoundLdT(int64_t T, int elem) { const int64_t m = 128 / elem; return ((T + m - 1) / m) * m; }   // rows start on 128-byte lines
  double *_dVB = nullptr, *_dPriority = nullptr, *_dRunLength = nullptr, *_dPoleScratch = nullptr;
  size_t PoleScratchBytes(int64_t capQ) const { return (size_t)capQ * (size_t)(2 * _K + 2) * sizeof(double) + PoleListBytes(capQ); }
  uint32_t *_dTGap = nullptr, *_dQGap = nullptr;
  int64_t *_dExps = nullptr, *_dAqs = nullptr, *_dStatus = nullptr, *_dNOut = nullptr;
  int64_t _aqCapacity = 0;
  // ListTopTargets over rows of more than 16384 targets / for many quizzes at once (kb_kernels.hip: LaunchTopTargetsBatch): the two
  // buffers of candidate lists on the device, and the pinned lines a batch's results arrive in (records, then the counts)
  RatedTargetDev *_dTopScratch[2] = {nullptr, nullptr};
  size_t _topScratchBytes[2] = {0, 0};
  ResultLines _hTopBatch;
  Error EnsureTopScratch(int64_t nQuizzes, int64_t want);
  Error EnsureTopScratchRecords(int64_t need);   // (both buffers; the question listing shares them)
  // ListTopTargetsAmongBatch (hip_engine_top_among.cpp): one call's lists as staged -- offsets[nLists + 1] | ids (int32) on the device --,
  // the level-0 partial sums, the gathered posteriors of listings beyond 256 records, and the pinned result lines
  // (records | counts | masses).  The buffers grow and never shrink.
  struct TopAmongStage {
    std::vector<int64_t> stamp, offsets;
    std::vector<int32_t> ids;
    void *dLists = nullptr;
    double *dPartial = nullptr, *dGather = nullptr;
    size_t listBytes = 0, partialBytes = 0, gatherBytes = 0;
    ResultLines lines;
  } _topAmong;
  Error ValidateTopAmongLocked(int64_t n, const int64_t *pQuizzes, const int64_t *pListOf, int64_t nLists, const int64_t *pListCounts, const int64_t *pTargets,
                               int64_t maxCount, bool haveDest, bool haveCounts);
  // PreviewAnswersBatch (hip_engine_preview.cpp): the would-be posteriors of a chunk of up to kTopBatchQuizzes rows, _ldT doubles each (also
  // where a row that does not fit LDS is staged), the pinned result lines (records | counts | likelihood and entropy per row), the events of
  // option "time_sweeps".  The buffers grow and never shrink.
  struct PreviewStage {
    double *dRows = nullptr;
    size_t rowsBytes = 0;
    ResultLines lines;
    hipEvent_t ev[2] = {nullptr, nullptr};
  } _preview;
  Error ValidatePreviewLocked(int64_t nPairs, const int64_t *pQuizzes, const int64_t *pQuestions);
  uint64_t _previewCalls = 0, _previewPairs = 0, _previewDeviceNs = 0;   // read-only "preview_calls", "preview_pairs", "preview_device_ns"
  // QuizStatusBatch / RankTargetsBatch (hip_engine_status.cpp): the pinned result lines -- a chunk's status lines (kStatusLineWords words per
  // quiz, behind one unused record) and a chunk's {rank, probability} records --, the events of option "time_sweeps".  Allocated once.
  struct StatusStage {
    ResultLines lines, rankLines;
    hipEvent_t ev[2] = {nullptr, nullptr};
  } _status;
  Error ValidateStatusLocked(const char *what, int64_t n, const int64_t *pQuizzes, const int64_t *pTargets);
  uint64_t _statusCalls = 0, _statusQuizzes = 0, _rankCalls = 0, _rankPairs = 0, _statusDeviceNs = 0;   // read-only "status_calls", "status_quizzes", "rank_calls", "rank_pairs", "status_device_ns"
  // EvalQuestionGainsBatch / ListInformativeQuestionsBatch (hip_engine_gain.cpp): a chunk's rows of RedRowPitch() doubles on the device, the
  // slots that show them to the question listing, its pinned result lines, the host's copy of the rows for listings beyond 256 records, the
  // events of option "time_sweeps".  The buffers grow and never shrink.
  struct GainStage {
    double *dRows = nullptr;
    size_t rowsBytes = 0;
    QuizSlot *dSlots = nullptr;
    ResultLines lines;
    std::vector<double> rows;
    hipEvent_t ev[2] = {nullptr, nullptr};
  } _gain;
  Error AdmitGainsLocked(int64_t rowLength, int64_t n, const int64_t *pQuizzes);
  Error GainRowsLocked(int64_t first, int64_t m, const int64_t *pQuizzes);   // a chunk's rows into _gain.dRows, enqueued
  uint64_t _gainCalls = 0, _gainQuizzes = 0, _gainDeviceNs = 0;   // read-only "gain_calls", "gain_quizzes", "gain_device_ns"
  // EvalConditionalGainsBatch / ListQuestionPageBatch (hip_engine_page.cpp): a chunk's branch rows of _ldT doubles in two halves and their
  // masses, the gain sweep's rows for them, the quizzes' combined rows, exclusion bitmaps and sets, the slots that show the combined rows
  // to the question listing, the pinned lines a page's picks arrive in (step s of quiz j at record s * 256 + j; the expansions read them
  // on the device), the call's given sets as validated, the events of option "time_sweeps".  The buffers grow and never shrink.
  struct PageStage {
    double *dRows = nullptr, *dMasses = nullptr, *dGains = nullptr, *dCombined = nullptr;
    uint32_t *dExcl = nullptr;
    int32_t *dSet = nullptr;
    size_t rowsBytes = 0, massesBytes = 0, gainsBytes = 0, combinedBytes = 0, exclBytes = 0;
    QuizSlot *dSlots = nullptr;
    ResultLines lines;
    std::vector<int32_t> given;                  // LOCAL ids, one set after another (-1: a question another engine holds) ...
    std::vector<int64_t> givenSlot;              // ... and for those the slot of the call's block package (-1: this engine's own cube)
    std::vector<int64_t> givenFirst, largest;    // nQuizzes + 1; the quizzes' branch rows at their largest step
    const char *blocks = nullptr;                // the call's block package as the kernels read it (staged, where it was in host memory)
    hipEvent_t ev[2] = {nullptr, nullptr}, evHead = nullptr;   // evHead: behind the last launch before a chunk's first sweep
  } _page;
  // the block package of the FromBlocks forms (nullptr: the plain calls, which a shard refuses)
  struct PageBlocks { int64_t n; const int64_t *questions; const void *blocks; int64_t slotBytes; };
  Error AdmitPageLocked(const char *call, int64_t rowLength, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven,
                        int64_t pageSize, bool page, const PageBlocks *pkg = nullptr);
  Error EvalPageRows(const char *call, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven, const PageBlocks *pkg, double *pOut,
                     int64_t n);   // both Eval forms
  Error StagePageBlocksLocked(const PageBlocks &pkg);   // st.blocks <- the package, its needed slots copied to the device first under option "rows_stage"
  Error PageChunkLocked(int64_t first, int64_t m, const int64_t *pQuizzes, int64_t steps);   // a chunk's launches, enqueued
  // read-only "page_calls", "page_quizzes", "page_device_ns", "page_head_ns" (of the latter: the roots and the given sets' expansions, what comes before the first sweep)
  uint64_t _pageCalls = 0, _pageQuizzes = 0, _pageDeviceNs = 0, _pageHeadNs = 0;
  // ReviewAnswersBatch (hip_engine_review.cpp): per row of a chunk _ldT mantissas (then the divided row) and, behind all of them, _ldT
  // exponent sums; the ratios of the chunk's quizzes that do not stay in LDS; the pinned result lines (records | counts | likelihood and
  // entropy per row); the events of option "time_sweeps".  The buffers grow and never shrink.
  struct ReviewStage {
    double *dRows = nullptr, *dRatios = nullptr;
    size_t rowsBytes = 0, ratiosBytes = 0;
    ResultLines lines;
    hipEvent_t ev[2] = {nullptr, nullptr};
  } _review;
  Error ReviewAnswers(int64_t nPairs, const int64_t *pQuizzes, const int64_t *pPositions, int64_t maxCount, double *pLikelihood, double *pEntropy,
                      CiRatedTarget *pDest, int64_t *pCounts, bool fromRows, const void *pRows, const int64_t *pRowFirst);
  uint64_t _reviewCalls = 0, _reviewRows = 0, _reviewDeviceNs = 0;   // read-only "review_calls", "review_rows", "review_device_ns"
  // ListTopQuestions (hip_engine_list.cpp): what a listing in flight between its two halves is, and the host-coherent lines a batch's
  // results arrive in -- records, then counts, then one flag per quiz.  Between the halves _mu is free (the sharded engine has every
  // shard's listing in flight before it waits for the first), so the single and the batch listing keep a record each -- the single one
  // under the sharded engine's operation lock, the batch one under its batch context 0, as _ctx[0] is -- and a record refers to no
  // quiz: a list of more than 256 questions takes its copy of the priorities and of the asked bits in the first half.
  struct TopQFlight { int64_t n = 0, want = 0; uint64_t op = 0; bool onHost = false; std::vector<double> pri; std::vector<std::vector<uint32_t>> asked; };
  TopQFlight _topQ, _topQBatch;
  ResultLines _hTopQ;   // (mapped and coherent: the host polls its tail, one flag per quiz)
  Error EnqueueTopQuestionsLocked(Quiz *q, int64_t maxCount);
  int64_t CollectTopQuestionsLocked(Error &err, CiRatedQuestion *pDest);
  Error EnqueueTopQuestionsBatchLocked(int64_t n, const int64_t *pQuizzes, int64_t maxCount);
  Error CollectTopQuestionsBatchLocked(int64_t n, int64_t stride, CiRatedQuestion *pDest, int64_t *pCounts);
  int64_t TopQuestionsOfVector(const double *pri, const std::vector<uint32_t> &asked, int64_t want, CiRatedQuestion *pDest) const;   // the host's prefix, same order
  int64_t ListTopTargetsOnHost(Error &err, Quiz *q, int64_t want, CiRatedTarget *pDest, bool referenceOrder = false);
  // ListTopTargets = the fast listing with one entry more than asked for; where it shows equal probabilities, the reference's own
  // order among them (its per-worker heaps, reproduced on the device: kb_kernels.hip LaunchTopTargetsExact) -- option "top_exact"
  int64_t ListTopTargetsFast(Error &err, int64_t iQuiz, int64_t maxCount, CiRatedTarget *pDest);
  int64_t ListTopTargetsExact(Error &err, int64_t iQuiz, int64_t maxCount, CiRatedTarget *pDest);
  Error EnsureTopExactScratch(int64_t nQuizzes, int64_t want);
  void *_dTopExact = nullptr;
  size_t _topExactBytes = 0;
  uint64_t _topExactListings = 0;  // read-only option "top_exact_listings": listings that took the heaps' path
  // Released quizzes' device buffers, reused by the next StartQuiz / ResumeQuiz of the same dimensions: hipMalloc / hipFree
  // cost tens of microseconds and hipFree synchronises the device.  Reuse is ordered by the engine's stream.
  struct QuizBuffers { double *dPrior; uint32_t *dAsked; int64_t ldT; size_t askedWords; };
  std::vector<QuizBuffers> _quizBufferPool;
  struct GraphEntry { hipGraphExec_t exec; int64_t variant; hipStream_t stream; uint64_t kbVersion; };
  uint64_t _kbVersion = 0;
  std::unordered_map<Quiz *, GraphEntry> _graphs;  // option "use_graph"
  SelectResult *_dGraphScratch = nullptr;
  uint64_t *_dTagCell = nullptr;
  // The launched, graph-replayed and resident selections each report through a packed record of their OWN in _hPinned->own[]
  // (select_record.h: the record carries 32 bits of its launch's tag, there is no flag), each waiting for "its" tag: with one record
  // for all three a selection would find it already carrying its tag -- left by another path's earlier selection -- and return that
  // one's question (graph tag 1, then the resident sweep's first request, also 1: found by the soak of tools/stress_more.py, when
  // the paths shared a record and a flag).  The graph's tags keep the range of their own that told the flag's values apart then.
  static constexpr uint64_t kGraphFlagBase = 1ull << 40;
  uint64_t _graphTag = kGraphFlagBase + 1;
  uint64_t _serverTag = 0;   // of the resident sweep's last packed answer (NextSelectionTag)
  enum OwnCell { kOwnLaunched = 0, kOwnGraph = 1, kOwnResident = 2 };
  void DropQuizBufferPool();
  SelectResult *_dSel = nullptr;
  struct Pinned {  // host-coherent: written by kernels, polled / read by the host without copies
    SelectResult sel; uint64_t seq; int64_t status[2]; int64_t nOut;
    uint64_t opFlag;               // completion flag of the sampled selection kernel
    uint64_t topFlag;              // completion flag of whatever listed into top[] last
    RatedTargetDev top[256];
    int64_t nOutQ;                 // ListTopQuestions of one quiz: lines of its own, so that a ListTopTargets between its two halves
    uint64_t topQFlag;             // (sharded engine) lists into top[] without touching them
    RatedTargetDev topQ[256];
    PackedSelection own[3];        // the engine's own selections, by path (OwnCell); decoded into `sel` by WaitPacked
  };
  SelectResult *OwnRecord(OwnCell c) { return reinterpret_cast<SelectResult *>(&_hPinned->own[c]); }
  // (Pinned::top: listings of more than kQuizTop targets; up to kQuizTop the quiz's own lines are used, where RecordAnswer's
  //  kernel lists the new posterior's best targets ahead of the ListTopTargets for the same quiz and posterior)
  uint64_t _opSeq = 0;
  // ---- the quizzes' pinned lines: slabs of host-coherent memory, handed out per quiz, returned at its release
  std::vector<QuizPinned *> _pinSlabs, _pinFree;
  static constexpr int kPinSlab = 256;
  QuizPinned *TakePin();
  // ---- deferred posterior updates.  While several client threads are inside the engine, RecordAnswer only does its
  // bookkeeping and leaves the kernel to whoever next needs a posterior (ListTopTargets, NextQuestion, ...): that caller launches
  // ONE kernel for all the updates that have gathered (grid.x = update; prior_kernels.hip: record_answer_batch_kernel) instead
  // of one launch each.  Alone in the engine, RecordAnswer launches at once, as before.
  struct BatchCtx;
  struct PendingUpdate { Quiz *q; int64_t qLocal, iAnswer; const void *rowA = nullptr, *rowD = nullptr; bool list = true; };   // rowA: another shard's question
  std::vector<PendingUpdate> _pendingUpdates;
  Error FlushUpdates();                       // the caller holds _mu
  void MarkStreamBusy();
  uint64_t _flushes = 0, _flushedUpdates = 0, _maxFlush = 0;
  std::atomic<int> _activeCallers{0};         // client threads inside quiz-level calls right now
  const std::atomic<int> *_extCallers = nullptr;   // a shard: the client threads inside the sharded engine that drives it
  int Callers() const {
    const int own = _activeCallers.load(std::memory_order_relaxed);
    return _extCallers ? std::max(own, _extCallers->load(std::memory_order_relaxed)) : own;
  }
  bool Concurrent() const { return _opt.combine && Callers() > 1; }
  static int AllowedCpus();                   // the CPUs this process may use: the cgroup's quota (cpu.max) or the affinity mask
  bool ClientsFitCpus() const { return _opt.combineSpin && Callers() + 2 <= AllowedCpus(); }
  // ---- combining of concurrent NextQuestion calls (reference: every client's NextQuestion runs under a SHARED lock,
  // PqaCore/CpuEngine.cpp:357-361, Interface/IPqaEngine.h:44).  A caller posts its request; if a leader is at work it waits
  // for its result, otherwise it becomes the leader: it takes everything posted so far -- distinct quizzes -- and serves it
  // with ONE row-sharing / grid.y sweep (BatchSweep), selects per quiz, hands the results out and, if requests are waiting
  // again, passes the lead to the oldest of them.  One request: the single-quiz path, as before.
  struct SelRequest {
    int64_t iQuiz = -1;
    SelKind kind = SelKind::Argmax;    // (Sampled: with rnd)
    uint64_t rnd = 0;
    int64_t result = -1;
    Error err;
    std::atomic<int> state{kReqWaiting};   // (combining.h) kReqSelect: select for yourself from `view` (the leader does not do it for everybody)
    PriorityView view;                 // kReqSelect: this quiz's priority vector on the host
    BatchCtx *ctx = nullptr;           // kReqSelect: whose reader count is this request's to release
    uint64_t serial = 0;               // kReqSelect: the quiz the sweep ran for
    Quiz *quiz = nullptr;              // kReqSelect: held by inSelection
    std::vector<uint32_t> unavailable; // kReqSelect: the quiz's asked questions and the gaps as they were when the sweep was launched
    int64_t nQ = 0, nSub = 0;
  };
  int64_t SelectFromPriorities(SelRequest *r);     // the host-side selector + FinishSelection for one request of a combined sweep
  std::atomic<size_t> _pendingCount{0};            // == _pendingUpdates.size(), readable without the lock
  std::atomic<int64_t> _flushedSinceSweep{0};      // RecordAnswers launched since the newest combined sweep: their clients' NextQuestions are on their way
  std::atomic<int64_t> _sweepNsEwma{0};            // how long a follower of a combined sweep waits for its result (moving average): it sleeps most of that, then spins
  std::atomic<int64_t> _lastCombined{0};           // requests of the newest combined sweep: as many RecordAnswers are about to arrive
  int64_t Combine(Error &err, int64_t iQuiz, SelKind kind, uint64_t rnd);
  // ---- posted operations.  With dozens of client threads the engine's lock is not held long but changes hands through the
  // kernel every time: each RecordAnswer and ListTopTargets slept on it and was woken by the thread before it, one wake-up
  // latency per call, serially (64 threads: 200 us inside a RecordAnswer that works for 1).  So a call that finds the lock
  // taken does not queue on it: it posts its operation and sleeps on the operation's own word; whoever holds the lock runs
  // everything posted so far right before it lets go (combining.h: PostingLock) -- the RecordAnswers of a drain into the list of
  // deferred updates, ONE launch for all the posteriors its ListTopTargets ask for -- and wakes the posters, all at once.
  struct Flight;
  struct EngineMutex;
  enum class OpKind { RecordAnswer, ListTopTargets, LaunchBatch, StartQuiz, ReleaseQuiz, RecordQuizTarget, ResumeQuiz };
  struct PostedOp {   // (made as one of the records named after the kinds, below: each takes what its kind reads)
    const OpKind kind;
    int64_t iQuiz = -1, iAnswer = 0, maxCount = 0, iTarget = 0, nAnswered = 0;
    const AQ *aqs = nullptr;
    double amount = 0;
    bool remote = false;
    BatchCtx *ctx = nullptr;
    std::vector<SelRequest *> *batch = nullptr;
    Flight *flight = nullptr;
    Error err;
    static constexpr int64_t kTakeLockYourself = -2;   // ListTopTargets' result: a list longer than the quiz's lines hold -- the poster's own work
    int64_t result = 0;                // ListTopTargets: the number of targets to take from `pin` once it carries `flagOp`
    QuizPinned *pin = nullptr;
    uint64_t flagOp = 0;
    Quiz *quiz = nullptr;              // (the drain's own, between its two passes)
    uint64_t serial = 0;
    std::atomic<int> state{kOpPosted};
    PostedOp *next = nullptr;
   protected:
    explicit PostedOp(OpKind k) : kind(k) {}
  };
  struct RecordAnswerOp : PostedOp { RecordAnswerOp(int64_t quiz, int64_t answer, bool rem) : PostedOp(OpKind::RecordAnswer) { iQuiz = quiz; iAnswer = answer; remote = rem; } };
  struct ListTopTargetsOp : PostedOp { ListTopTargetsOp(int64_t quiz, int64_t count) : PostedOp(OpKind::ListTopTargets) { iQuiz = quiz; maxCount = count; } };   // (the launch)
  struct LaunchBatchOp : PostedOp { LaunchBatchOp(BatchCtx &c, std::vector<SelRequest *> &b, Flight &f) : PostedOp(OpKind::LaunchBatch) { ctx = &c; batch = &b; flight = &f; } };
  struct StartQuizOp : PostedOp { StartQuizOp() : PostedOp(OpKind::StartQuiz) {} };   // (result = the quiz)
  struct ReleaseQuizOp : PostedOp { explicit ReleaseQuizOp(int64_t quiz) : PostedOp(OpKind::ReleaseQuiz) { iQuiz = quiz; } };
  struct RecordQuizTargetOp : PostedOp { RecordQuizTargetOp(int64_t quiz, int64_t target, double amt) : PostedOp(OpKind::RecordQuizTarget) { iQuiz = quiz; iTarget = target; amount = amt; } };
  struct ResumeQuizOp : PostedOp { ResumeQuizOp(int64_t n, const AQ *list) : PostedOp(OpKind::ResumeQuiz) { nAnswered = n; aqs = list; } };   // (result = the quiz; the poster waits: the list stays valid)
  // The way in of every call that can be posted.  True: `op` was posted -- the engine is taken, or option "post_always" -- and its holder has run it.  False: `lk`
  // holds _mu (without option "combine" always, waited for): the call runs its direct form, which differs from the drained one on purpose (flushes at once, may wait, speculates).
  bool TakeOrPost(std::unique_lock<EngineMutex> &lk, PostedOp &op) {
    if (_opt.combine) return TryLockOrPost(_mu, lk, op, _opt.postAlways != 0);
    lk = std::unique_lock<EngineMutex>(_mu);
    return false;
  }
  uint64_t _postedOps = 0, _postedDrains = 0;
  void DrainPosted(PostedOp *ordered);             // (the engine's lock held: everything posted so far, in post order) -- in these stages:
  struct PostedCounts { int64_t trains = 0, starts = 0, resumes = 0; bool needFlush = false; };
  PostedCounts RunPostedInPlace(PostedOp *ordered);   // RecordAnswer and ReleaseQuiz as they come; the listings validated (needFlush: a deferred update); the rest counted
  void TrainPosted(PostedOp *ordered);             // the drain's RecordQuizTarget calls
  void StartPosted(PostedOp *ordered);             // its StartQuiz calls: one launch per kStartInline of them
  void ResumePosted(PostedOp *ordered, int64_t nResumes);
  void ListPosted(PostedOp *ordered, const Error &flushErr);   // the listings, each record handed back as it is done
  uint64_t _trainBatches = 0, _trainBatchCalls = 0;
  Error ReleaseQuizLocked(int64_t iQuiz, bool mayWait);
  Error RecordQuizTargetLocked(int64_t iQuiz, int64_t iTarget, double amount);
  int64_t PreferredCombinedBatch(int64_t m) const;
  struct Flight {                      // a combined sweep between its launch and its collection
    CombinedFlight cf;                 // the sweep itself: EnqueueCombinedLocked fills it, CollectCombined waits for it
    std::vector<SelRequest *> live;
    bool anySampled = false;
    std::chrono::steady_clock::time_point tA, tB, tC;
  };
  void LaunchBatch(BatchCtx &c, std::vector<SelRequest *> &batch, Flight &f);
  void LaunchBatchLocked(BatchCtx &c, std::vector<SelRequest *> &batch, Flight &f);
  bool CollectBatch(BatchCtx &c, std::vector<SelRequest *> &batch, Flight &f, SelRequest *own);   // true: `own` is to select for itself
  int64_t NextQuestionArgmaxLocked(Error &err, int64_t iQuiz);
  int64_t NextQuestionSampledLocked(Error &err, int64_t iQuiz, uint64_t rnd);
  int64_t SelectLocked(Error &err, int64_t iQuiz, SelKind kind, uint64_t rnd) { return kind == SelKind::Argmax ? NextQuestionArgmaxLocked(err, iQuiz) : NextQuestionSampledLocked(err, iQuiz, rnd); }
  std::mutex _rngMu;
  uint64_t _quizSerial = 0;
  uint64_t _combBatches = 0, _combRequests = 0, _combMaxBatch = 0;
  std::atomic<uint64_t> _combNs[7] = {{0}, {0}, {0}, {0}, {0}, {0}, {0}};
  volatile uint64_t *_pendingRecordFlag = nullptr;   // where _pendingRecordOp will appear
  // spin on a host-coherent flag until it holds `value` (the kernel's last store); falls back to the stream's status
  Error WaitFlag(volatile uint64_t *flag, uint64_t value, const char *what);
  // the same wait for a packed record (FusedSelect::packed; resident: one the resident sweep answers): until it carries `tag`, then
  // {priority, index + outBase or -1 / -3 / -4} into _hPinned->sel, where the callers look
  Error WaitPacked(SelectResult *record, uint64_t tag, int64_t outBase, const char *what, bool resident = false);
  Error WaitFlagNapping(volatile uint64_t *flag, uint64_t value, const char *what);   // for many waiters at once: a short spin, then naps
  SelectResult *_dSelScratch = nullptr;  // its per-workgroup winner records
  double *_dPriorScratch = nullptr;      // the long-row posterior kernels' subtask sums (KbView::priorScratch)
  hipEvent_t _evSweep[2] = {nullptr, nullptr};   // option "time_sweeps": around every launched fp64 sweep; read-only "last_sweep_ns"
  void TimerStart(hipEvent_t (&ev)[2]);   // the event-pair timer of that option: events created on first use; Stop waits for its event and adds to `ns`
  void TimerStop(hipEvent_t (&ev)[2], uint64_t &ns);
  mutable bool _sweepTimed = false;
  // batched selections (NextQuestionArgmaxBatch); allocated on first use
  static constexpr int64_t kMaxBatch = 256, kBatchGrid = 1024;
  // (sweepOut / sweepSeq: where the sweep of a sampled batch publishes its own winners, so that out / seq are the selector's
  //  behind it; rnd: that batch's random numbers, read by the selector where they are)
  struct BatchPinned {
    QuizSlot slots[kMaxBatch]; SelectResult out[kMaxBatch]; uint64_t seq[kMaxBatch];
    SelectResult sweepOut[kMaxBatch]; uint64_t sweepSeq[kMaxBatch]; uint64_t rnd[kMaxBatch];
  };
  // Everything ONE batched sweep in flight needs of its own: the staged slots and winner records, the scratch of the
  // row-sharing sweep (batch_kernels.hip; sized by its plan, grown on demand), the host copy of the priority vectors.  Two of
  // them: the batch calls of the ABI and the shards' halves use the first; the leaders of combined sweeps alternate, so that
  // the next sweep is launched while the previous one runs.
  struct BatchCtx : CombineCtx {         // (mu: taken before the engine's lock)
    BatchPinned *h = nullptr;
    QuizSlot *dSlots = nullptr;
    SelectResult *dScratch = nullptr;
    double *dPriority = nullptr;
    int64_t priorityQ = -1;
    void *dPT = nullptr; double *dAcc = nullptr; BatchRecord *dRecs = nullptr; double *dPriT = nullptr;
    size_t ptBytes = 0, accBytes = 0, recBytes = 0, priTBytes = 0, rerankBytes = 0;
    void *dRerank = nullptr;             // Float engines: the candidates of the fp64 re-rank and their priorities
    void *dPole = nullptr;               // Double engines: the batched sweeps' pole scratch (BatchPlan::pole)
    size_t poleBytes = 0;
    double *dSelGrand = nullptr, *dSelRun = nullptr;   // the batched sampled selector's totals and run lengths (select_kernels.hip)
    size_t selGrandBytes = 0, selRunBytes = 0;
    hipEvent_t evSel[2] = {nullptr, nullptr};          // around that selector's launch
    void *dAmong = nullptr;              // the Among calls' staging: list offsets per quiz | pairs | the gathered priorities
    size_t amongBytes = 0;
    uint32_t *dAmongMask = nullptr;      // ... and the quizzes' bitmaps asked | not listed, for the sampled selector
    size_t amongMaskBytes = 0;
    int lastBp = 0;
    double *hPri = nullptr;              // pinned: the batch's priority vectors for the host-side selector -- copied there behind the
    size_t hPriDoubles = 0;              // row-sharing sweep, or written there by the grid.y = quiz sweep itself as {priority, launch tag} records
    bool hPriCoherent = false;           // hPri is host-coherent mapped memory (the kernels write it) rather than a copy's destination
    hipEvent_t event = nullptr;
  };
  BatchCtx _ctx[2];
  Combiner<SelRequest, BatchCtx> _comb{_ctx};
  // wantPriorities: the row-sharing sweep with its priority matrix kept (EvalPrioritiesBatch).  hostPriorities: whichever form
  // suits the batch, and the quizzes' priority vectors copied into _hBatchPri (layout: *pQuizMinor) for the host's selector.
  Error BatchSweep(BatchCtx &c, int64_t n, const int64_t *pQuizzes, std::vector<Quiz *> &quizzes, bool wantPriorities, uint64_t tag,
                   bool hostPriorities = false, bool *pQuizMinor = nullptr, bool *pTagged = nullptr, bool devicePriorities = false);
  // devicePriorities: the batch's form as for an argmax batch, every quiz's priorities left on the device (its own vector or the
  // quiz-minor matrix: lastBp), the sweep's own winners published to sweepOut / sweepSeq -- for the selector launched behind it
  Error ValidateBatchLocked(int64_t n, const int64_t *pQuizzes);
  Error EnsureBatchStaging(BatchCtx &c);    // the pinned staging lines, the device slots and the winner records: the first batch allocates them
  Error EnsureBatchVectors(BatchCtx &c);    // the per-quiz priority vectors dPriority, (re)sized with the knowledge base
  // The Among calls (hip_engine_among.cpp).  AmongStage: one call's lists as the kernels take them -- the quizzes with a non-empty list in
  // batch order (slot j), their pairs back to back, and where pair p of the call's pQuestions went.
  struct AmongStage {
    std::vector<int64_t> entry;            // slot j -> batch entry i
    std::vector<int64_t> offsets;          // slot j's pairs: [offsets[j], offsets[j + 1])
    std::vector<ListedPair> pairs;
    std::vector<uint32_t> masks;           // sampled forms: slot j's asked | not listed, maskWords words each (bits past Q clear, as `asked`)
    std::vector<int64_t> stamp;            // validation: the batch entry (+ 1) that listed a question last
    int64_t local = 0;                     // pairs whose question this engine holds
  } _among;
  enum class AmongForm { Eval, Select, Argmax, Sampled };
  Error ValidateAmongLocked(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, bool haveOut);
  Error AmongLocked(AmongForm form, int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, const uint64_t *pRnd,
                    double *pPriorities, CiHipSelection *pSel, int64_t *pPicked);
  uint64_t _amongCalls = 0, _amongPairs = 0;   // read-only "among_calls", "among_pairs"
  // ---- The source queries (hip_engine_sources.cpp): three families over one skeleton.  A family's stage: the engine's own package of a
  // whole engine's calls (also where a host package is staged), the rows, the family's scratch, the slots that show the rows to the
  // question listing, the listing's pinned lines (records | counts), the host copy of listings beyond 256 records, the events of option
  // "time_sweeps" around a whole engine's sweeps, the counters.  The buffers grow and never shrink.  The entries (argument checks, lock,
  // refusals in the one order, chunks of kMaxBatch sources), their steps under the lock, and SourceRowsLocked, which a family does its own way.
  // The third family's sources are GROUPS of targets (separation): pGroupCounts beside pSources, which then holds the groups' targets one
  // after another; it has no package -- its "pack" stages a chunk's groups and tiles on the device --, so it has no pack / from-package
  // calls and works on a shard directly.
  struct SourceStage {
    const bool questions;   // the results are questions (redundancy, separation); otherwise targets (similarity)
    const bool groups;      // a source is a group of targets (separation); otherwise one id of the results' kind
    uint64_t &calls, &sources, &deviceNs;
    double *dPackage = nullptr, *dRows = nullptr, *dScratch[2] = {nullptr, nullptr};
    size_t packageBytes = 0, rowsBytes = 0, scratchBytes[2] = {0, 0};
    QuizSlot *dSlots = nullptr;
    ResultLines lines;
    std::vector<double> rows;
    hipEvent_t ev[2] = {nullptr, nullptr};
    std::vector<int64_t> offsets;               // groups: where a group's entries begin in the call's pSources, [nSources + 1]
    const int64_t *dGroupStart = nullptr, *dTileGroup = nullptr, *dTileWidth = nullptr, *dEntries = nullptr;   // ... the staged chunk (in _dAqs) ...
    int64_t nTiles = 0;                                                                  // ... and its tiles (kb_plan.h: PlanGroupTiles)
  };
  uint64_t _simCalls = 0, _simSources = 0, _simDeviceNs = 0, _redCalls = 0, _redSources = 0, _redDeviceNs = 0;   // read-only "similarity_calls", "..._sources", "..._device_ns", "redundancy_calls", ...
  uint64_t _sepCalls = 0, _sepGroups = 0, _sepDeviceNs = 0;                                                      // ... "separation_calls", "separation_groups", "separation_device_ns"
  SourceStage _sim{false, false, _simCalls, _simSources, _simDeviceNs}, _red{true, false, _redCalls, _redSources, _redDeviceNs},
      _sep{true, true, _sepCalls, _sepGroups, _sepDeviceNs};
  int64_t PackagePitch() const { return RoundLdT(_T, 8); }                 // doubles of a similarity slot (PosteriorSlotBytes() / 8), of a row of a question-weight slot
  int64_t RedRowPitch() const { return (_Q + 15) & ~(int64_t)15; }         // doubles of a row of redundancy results
  int64_t SourceRowPitch(const SourceStage &st) const { return st.questions ? RedRowPitch() : PackagePitch(); }
  int64_t SourceSlotDoubles(const SourceStage &st) const { return st.groups ? 0 : (st.questions ? _K : 1) * PackagePitch(); }
  // (pGroupCounts: the groups family's counts, nullptr for the others)
  Error EvalSources(SourceStage &st, const char *call, int64_t nSources, const int64_t *pGroupCounts, const int64_t *pSources, double *pOut, int64_t n);
  Error ListSources(SourceStage &st, const char *call, int64_t nSources, const int64_t *pGroupCounts, const int64_t *pSources, int64_t maxCount, RatedTargetDev *pDest,
                    int64_t *pCounts);
  Error PackSources(SourceStage &st, const char *call, int64_t nSources, const int64_t *pSources, void *pDst, void *pFlag, uint64_t flagValue);
  Error EvalSourcesFromPackage(SourceStage &st, const char *call, int64_t nSources, const int64_t *pSources, const void *pPackage, double *pOut, int64_t n);
  Error ListSourcesFromPackage(SourceStage &st, const char *call, int64_t nSources, const int64_t *pSources, const void *pPackage, int64_t maxCount, RatedTargetDev *pDest, int64_t *pCounts);
  Error AdmitSourcesLocked(const SourceStage &st, const char *call, bool wholeOnly, int64_t rowLength, int64_t n, const int64_t *pSources) const;
  Error AdmitGroupsLocked(const char *call, int64_t rowLength, int64_t n, const int64_t *pGroupCounts, const int64_t *pTargets) const;
  Error PackSourcesLocked(SourceStage &st, int64_t n, const int64_t *pSources, void *pDst, void *pFlag, uint64_t flagValue);
  static void GroupOffsets(SourceStage &st, int64_t nGroups, const int64_t *pGroupCounts);   // st.offsets of a call
  Error StageGroupsLocked(SourceStage &st, int64_t first, int64_t n, const int64_t *pTargets);   // the groups family's "pack": groups [first, first + n) of st.offsets
  Error StageSourcesLocked(SourceStage &st, int64_t n, const int64_t *pSources, const void *pPackage, const double **dPackage);
  Error SourceRowsOutLocked(SourceStage &st, int64_t n, double *pOut, int64_t rowLength);   // (synchronises the stream)
  Error ListSourcesLocked(SourceStage &st, int64_t n, const double *dPackage, int64_t maxCount, RatedTargetDev *pDest, int64_t *pCounts);
  Error SourceRowsLocked(SourceStage &st, int64_t n, const double *dPackage, bool zeroSelf);
  Error NextQuestionSampledBatchLocked(int64_t n, const int64_t *pQuizzes, const uint64_t *pRnd, int64_t *pOut);
  Error LaunchSampledBatch(BatchCtx &c, int64_t n, const uint64_t *pRnd, uint64_t tag);
  // The engine's latest pack of selection parts: what a pick must find unchanged -- the quizzes and their posteriors, the split, this
  // shard's range -- and where the pack kernel left the run lengths of the shard's whole subtasks.
  struct PartsPack {
    uint64_t seq = 0;                         // 0: nothing packed yet
    std::vector<int64_t> quizzes;
    std::vector<uint64_t> serials, versions;
    int64_t nSub = 0, qFirst = 0, nLocal = 0, qTotal = 0, runQuiz = 0, runStride = 0;
    uint64_t kbVersion = 0;
  } _parts;
  int64_t SampledSubtasks() const { return _opt.evalSubtasks ? _opt.evalSubtasks : 8 * _opt.workers; }   // reference PqaCore/CpuEngine.cpp:339
  uint64_t *_dPartsWords = nullptr;           // {arrival counter, pad}, then a stamp per quiz of a batch
  double *_dPartsRun = nullptr, *_dPartsGrand = nullptr, *_dPartsPickRun = nullptr;
  size_t _partsRunBytes = 0, _partsGrandBytes = 0, _partsPickRunBytes = 0;
  // The engine's latest pack of posteriors: what RecordAnswerBatchFromPosteriors must find unchanged -- the batch, and every quiz's
  // posterior and active question.
  struct PosteriorPack {
    bool valid = false;
    std::vector<int64_t> quizzes, answers, active;
    std::vector<uint64_t> serials, versions;
  } _postPack;
  double *_dPostScratch = nullptr;            // the owned entries' posteriors between their update and the pack launch: ldT doubles each
  size_t _postScratchBytes = 0;
  uint64_t _postPacks = 0, _postPacked = 0, _postTaken = 0;   // read-only "posterior_packs", "posteriors_packed", "posteriors_taken"
  uint64_t _sampledBatches = 0, _sampledBatchDeviceNs = 0;   // read-only "sampled_batches", "sampled_batch_device_ns" (the selector's launches between events)
  uint64_t _priorityHostBytes = 0;     // read-only "priority_host_bytes": priorities the batched sweeps delivered to the host
  Error WaitBatchFlags(BatchCtx &c, int64_t n, uint64_t tag);
  Error EnqueueBatchLocked(int64_t n, const int64_t *pQuizzes, bool wantPriorities, uint64_t *pTag);
  Error CollectBatchSelectionsLocked(int64_t n, uint64_t tag, CiHipSelection *pOut);
  Error CollectBatchPrioritiesLocked(int64_t n, double *pOut);
  std::vector<Quiz *> _batchQuizzes;   // the quizzes of the batch between its two halves
  void *_dClusterScratch = nullptr;   // exchange buffers of the long-row sweep (cluster_kernels.hip), grown on demand
  size_t _clusterScratchBytes = 0;
  bool UseClusterSweep() const;       // rows beyond the register shapes, automatic variant, shape supported
  Error LaunchSingleSweep(Quiz *q, const FusedSelect *fused);
  bool LazyFix() const;
  // (a quiz whose last late_eager selections all needed the fix gets it launched behind the sweep again)
  bool LazyFor(const Quiz *q) const { return LazyFix() && q->lateStreak < _opt.lateEager; }
  FusedSelect OwnLaunch(uint64_t tag) { return FusedSelect::OwnCell(_dSelScratch, OwnRecord(kOwnLaunched), &_hPinned->seq, tag); }
  FusedSelect GraphReplay() { return FusedSelect::Graph(_dGraphScratch, OwnRecord(kOwnGraph), &_hPinned->seq, _dTagCell); }
  Error RunLazyFix(Quiz *q, const FusedSelect &swept, const char *what);   // the single-quiz sweep of this engine's precision, on _stream
  // The tail of a launched synchronous selection: the packed answer into _hPinned->sel (WaitPacked; waitWhat: its text where it is not
  // `what`), the lazy pole fix where the sweep asks for it (lateStreak, _poleListPending), the error "<what> (incomplete sweep)".
  Error AwaitLaunched(Quiz *q, const FusedSelect &fs, uint64_t tag, const char *what, const char *waitWhat = nullptr);
  // The resident sweep's step for a quiz: posted with `flags`, waited for, checked.  *handedOver: it answered "redo with the fix" --
  // this quiz's selections are launched from here on (Quiz::noServer), the caller goes on to launch this one.
  Error AskResident(Quiz *q, int64_t flags, const char *what, bool *handedOver);
  Error CollectCombined(BatchCtx &c, const CombinedFlight &flight, CiHipSelection *winners, PriorityView *views);   // (the engine's own leaders: no HIP call where flags are waited for)
  PriorityView ViewOf(const BatchCtx &c, const CombinedFlight &flight, int64_t i) const;   // quiz i's vector as the sweep delivered it (flight.hostPriorities)
  // EnqueueCombined behind its argument checks, the lock and the flush: tag, sweep, event; `quizzes`: the batch's, for the caller's snapshot
  Error EnqueueCombinedLocked(BatchCtx &c, int64_t n, const int64_t *pQuizzes, bool hostPriorities, CombinedFlight *flight, std::vector<Quiz *> &quizzes);
  uint64_t _selSeq = 0;
  // Tag of the next fused launch: consecutive launches differ in the low 32 bits, and those are never 0 (the state of
  // freshly cleared records)
  uint64_t NextLaunchTag() {
    if ((uint32_t)++_selSeq == 0) ++_selSeq;
    return _selSeq;
  }
  Pinned *_hPinned = nullptr;
  std::vector<uint32_t> _hTGap, _hQGap;   // host mirrors; qgap over local questions, bits past size set
  int64_t _nTargetGaps = 0;
  int64_t _capQ = 0;                        // questions the device buffers are allocated for (>= _Q)
  std::vector<int64_t> _questionGapList, _targetGapList;  // LIFO, like reference PqaCore/GapTracker.h
  IdLedger _questionIds, _targetIds, _quizIds;
  // A shard: the question axis of the WHOLE knowledge base, replicated on every rank -- the gap list in the reference's LIFO order and
  // the permanent-id ledger, both over GLOBAL ids.  Fresh ids at Create, the file's trailer after a load; SetQuestionGaps,
  // RemoveQuestions, AddQsTs and CompactFromBlocks keep them current, SaveKBShard writes its trailer from them, and the question id
  // maps answer from the ledger.  (_questionGapList, _questionIds and _hQGap stay what they are on a whole engine: over LOCAL ids.)
  std::vector<int64_t> _globalQuestionGaps;
  IdLedger _globalQuestionIds;
  uint32_t _precMantissa = 0;
  uint16_t _precExponent = 0;
  std::vector<Quiz *> _quizzes;
  std::vector<int64_t> _quizGaps;
  // The engine's lock.  Taking it also marks the engine's stream as possibly busy: the resident sweep runs on its own
  // stream, so a request is posted only after whatever the other operations enqueued on `_stream` has finished
  // (ServerPost); the selection paths, which leave nothing running, restore the mark they found.
  // Releasing it runs the posted operations first (DrainPosted).
  struct EngineMutex : PostingLock<PostedOp, HipEngine> {
    // (a sleeping lock on purpose: the client threads of a server may outnumber the cores it is allowed -- the GPU boxes of
    //  this project give a container 16 of 256 hardware threads -- and spinning waiters, tried in round 3 as a test-and-set and
    //  as a ticket lock, burn that allowance: 64 client threads fell from 45 k to 13 k questions/s, 256 to 0.3 k)
    using PostingLock::PostingLock;
    bool busy = false, wasBusy = false;
    // (spinFirst -- set while the client threads are fewer than the CPUs the process may use: a bounded spin before sleeping; the
    //  holder is usually a microsecond of bookkeeping or one kernel launch away from releasing, and being woken through the kernel
    //  costs tens of microseconds.  With more clients than CPUs every spinning waiter takes time from a thread that has work.)
    std::atomic<bool> spinFirst{false};
    bool try_lock() {
      if (!PostingLock::try_lock()) return false;
      wasBusy = busy; busy = true;
      return true;
    }
    void lock() {
      if (spinFirst.load(std::memory_order_relaxed))
        for (int i = 0; i < 400; i++) {
          if (PostingLock::try_lock()) { wasBusy = busy; busy = true; return; }
          for (int j = 0; j < 4; j++) __builtin_ia32_pause();
        }
      PostingLock::lock(); wasBusy = busy; busy = true;
    }
    void lock_urgent() { lock(); }
  };
  struct UrgentLock {   // (RAII for lock_urgent, re-lockable like std::unique_lock)
    EngineMutex &mu;
    bool held = false;
    explicit UrgentLock(EngineMutex &m) : mu(m) { lock(); }
    ~UrgentLock() { if (held) unlock(); }
    void lock() { mu.lock_urgent(); held = true; }
    void unlock() { mu.unlock(); held = false; }
  };
  mutable EngineMutex _mu{this, &HipEngine::DrainPosted};
  std::atomic<uint64_t> _nQuestionsAsked{0};
  Mode _mode = Mode::Regular;
  EngineOptions _opt;        // every option of SetOption / GetOption (engine_options.h)
  void ApplyEnvironment();   // the PQA_* variables: defaults for unchanged wrappers
  TaggedPriority *_hHostPriority = nullptr;   // host-coherent, _hostPriorityCap records {priority, launch tag}
  std::vector<double> _hostRun;               // the vector the host-side selector works on
  Error CollectHostPriority(uint64_t tag, const Quiz *q);   // the launch's entries out of _hHostPriority into _hostRun (TakePriorities)
  int64_t _hostPriorityCap = 0;
  hipError_t EnsureHostPriority();
  int64_t ClusterFrom() const { return _elem == 8 ? _opt.clusterFrom : 16384; }   // rows longer than this take the cluster sweep (Float engines: their register shapes hold 16384 elements; not re-measured)
  // ---- the next sweep ahead of its request (option "speculate"): RecordAnswer enqueues, right behind its posterior kernel, the
  // sweep the NextQuestion that normally follows would launch -- the client's time between the two calls (the wrapper's own
  // overhead, ListTopTargets, a person reading the question) overlaps with it, and that NextQuestion only waits for the flag.
  // The result is used only if nothing has touched the quiz, the cube, the gaps or the hand-over buffers since (every such
  // operation drops it); the random number of the sampled selector is drawn when NextQuestion is called, as before.
  // what a speculative sweep leaves: the winner's record in _hPinned->sel; the priority vector in _hHostPriority; the priorities in _dPriority
  enum class SpecKind { None, ArgmaxRecord, HostPriorities, DevicePriorities };
  struct Speculation {
    Quiz *quiz = nullptr;
    uint64_t priorVersion = 0, tag = 0;
    SpecKind kind = SpecKind::None;
    int64_t variant = 0;
    hipStream_t stream = nullptr;
    FusedSelect fs{};        // the launch's own arguments: a speculative sweep is launched WITHOUT the pole fix-up behind it (lazyFix) --
                             // most of a quiz's last speculations are never used, and their fix-ups were the longest kernels of the loop
  } _spec;
  // A sweep launched with lazyFix whose answer nobody has looked at yet may have left entries in the engine's suspect list: the next
  // launch that uses the list empties it first (and the speculation that left them is dropped: its fix-up would find nothing)
  bool _poleListPending = false;
  Error SettlePoleList();
  int _specScore = 0;        // +1 per speculation used, -1 per speculation dropped: below -4 only every 32nd RecordAnswer speculates
  uint64_t _specProbe = 0, _specHits = 0, _specDropped = 0;
  bool Speculate(Quiz *q, int64_t updQuestion = -1, int64_t updAnswer = -1);
  uint64_t _fusedUpdates = 0;   // read-only "fused_updates": RecordAnswers whose update ran inside the sweep's launch (option "fuse_update")
  int64_t SpeculateFor(int64_t iQuiz);
  SpecKind TakeSpeculation(Quiz *q, std::initializer_list<SpecKind> accepted, uint64_t *pTag);
  void DropSpeculation() {
    if (_spec.quiz != nullptr) { _spec.quiz = nullptr; _specDropped++; if (_specScore > -8) _specScore--; }
  }
  int64_t _topWantRecent = 10;   // what ListTopTargets has been asked for lately (option "top_cache" resets it)
  // ---- resident sweep (option "server"; pqa_kernels.h: ServerMailbox)
  hipStream_t _serverStream = nullptr;
  ServerMailbox *_hMailbox = nullptr;     // pinned
  ServerCtl *_dServerCtl = nullptr;
  volatile uint64_t *_serverRequest = nullptr;   // the request line: host-visible device memory if the platform maps it, else the mailbox's
  bool _serverRequestInVram = false;
  uint64_t _serverReqSeq = 0;                    // the sequence number last written there (the line is never read by the host)
  bool _serverLaunched = false;           // a kernel instance has been launched and not yet seen to have left
  uint64_t _serverKb = 0, _serverPosted = 0;
  int64_t _serverVariant = 0;
  uint64_t _pendingRecordOp = 0;          // RecordAnswer's kernel is the newest work on _stream and publishes this op number
  bool ServerUsable() const;
  Error ServerPost(Quiz *q, SelectResult *out, uint64_t *flag, uint64_t flagValue, int64_t outBase);
  void StopServer();
  void ServerQuiesce();   // returns once the posted step (if any) has finished: before anything that writes what it reads
  SelectorRng _rng;         // NextQuestion's random numbers, drawn under _rngMu
};

// One knowledge base over several devices of this process (sharded_engine.cpp); devices.size() >= 2.
IEngine *CreateShardedEngine(Error &err, const CiEngineDefinition &def, const std::vector<int> &devices);
IEngine *LoadShardedEngine(Error &err, const char *filePath, const std::vector<int> &devices, uint8_t precType = 0);

}  // namespace pqa
