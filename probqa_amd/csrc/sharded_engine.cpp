// sharded_engine.cpp -- one knowledge base, its question axis split over several devices of ONE process, behind the same C ABI.
//
// every question's priority depends only on its own sA / mD rows and on the (small, replicated) posterior, so
// the sweep shards by question with no data-path collective; what the shards exchange per selection is 16 bytes each.
// PQA_DEVICES=0,1,...,7 makes PqaEngineFactory_CreateCpuEngine build this engine instead of a single-device one, so that the
// reference's unchanged wrappers -- which can only call PqaEngine_NextQuestion (PqaCInterop.cpp:261-267) -- reach all the GPUs
// of a node.  Shard s is a complete HipEngine over the contiguous question range SRPoolRunner::CalcSplit gives it
// (SRPlatform/Interface/SRPoolRunner.h:96-110), with replicas of vB, the gap bitmaps and every quiz's posterior.
//
//   NextQuestion           one client: every shard's sweep is enqueued on its own device and stream; each finisher writes {priority,
//                          GLOBAL index} and then the step number into this engine's pinned slots; the host picks when all have
//                          landed (maximum priority, lowest index on ties) -- no collective launch, no copies, no stream sync; the
//                          reference's sampled selector (CpuEngine.cpp:362-400) runs on the host over the shards' priority vectors,
//                          with the subtask split over the GLOBAL question range.
//                          Many clients (the reference serves them under a SHARED lock, CpuEngine.cpp:357-361; its published rate
//                          is the sum over its learner threads, PqaClient.cpp:238-245): the calls that arrive together are
//                          combined -- ONE batched sweep per shard for all their quizzes, all shards in flight at once, the
//                          per-quiz winners (or priority vectors) merged on the host by the clients themselves.
//   RecordAnswer           is recorded here and returns; before anything reads a posterior, ALL gathered answers go to EVERY shard
//                          in one call and one launch each: a shard computes the posterior itself -- for a question another shard
//                          holds it reads that question's two rows where they are, over peer access (xGMI), or from a staged copy
//                          when the devices cannot map each other -- so all replicas hold the same bits and nothing is copied
//                          or waited for between the shards.
//   ResumeQuiz             every shard computes the posterior from row POINTERS (the other shards' rows in place, or staged).
//   Train / RecordQuizTarget   every shard applies the steps that fall on its questions (and its vB replica); other shards' reads
//                          of those rows are ordered around it by events (no host synchronisation).
//   SaveKB / LoadCpuEngine the file orders its rows by question: every shard streams its own block (same byte layout as a whole-cube
//                          engine's file: a KB saved sharded loads unsharded and vice versa).
// One lock (_opMu) orders what must happen in the same order on every shard -- quiz registry changes, trainings, the launch of a
// combined sweep; it is never held while the GPU is waited for, and calls that find it taken post their operation and are served
// by its holder on the way out (combining.h: PostingLock).  Maintenance-mode edits of the dimensions rebuild the
// shards (Rebuild below).  Not sharded (NotImplemented on this engine): SetStream and the stream-ordered single-shard entry points.
#include "hip_engine_internal.h"

#include <unordered_set>

namespace pqa {

namespace {

Error NotSharded(const char *what) {
  return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + what + " on a sharded engine",
                      std::string(what) + " is not available when the question axis is split over several devices (PQA_DEVICES).");
}

struct alignas(64) Slot {          // one per shard, host-coherent pinned memory
  double priority;
  int64_t index;
  uint64_t flag;
};

}  // namespace

class ShardedEngine final : public IEngine {
 public:
  static ShardedEngine *Create(Error &err, const CiEngineDefinition &def, const std::vector<int> &devices);
  ~ShardedEngine() override;

  Error Train(int64_t n, const AQ *pAQs, int64_t iTarget, double amount) override;
  uint64_t GetTotalQuestionsAsked(Error &err) override { return _sh[0]->GetTotalQuestionsAsked(err); }
  void CopyDims(CiEngineDimensions *pDims) const override { _sh[0]->CopyDims(pDims); }
  int64_t StartQuiz(Error &err) override;
  int64_t ResumeQuiz(Error &err, int64_t nAnswered, const AQ *pAQs) override;
  Error ResumeQuizBatch(int64_t n, const int64_t *pCounts, const AQ *pAQs, int64_t *pQuizzes) override;
  Error TrainBatch(int64_t n, const int64_t *pCounts, const AQ *pAQs, const int64_t *pTargets, const double *pAmounts) override;
  Error RecordQuizTargetBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pTargets, const double *pAmounts) override;
  int64_t NextQuestion(Error &err, int64_t iQuiz) override;
  Error RecordAnswer(int64_t iQuiz, int64_t iAnswer) override;
  int64_t GetActiveQuestionId(Error &err, int64_t iQuiz) override;
  Error SetActiveQuestion(int64_t iQuiz, int64_t iQuestion) override;
  int64_t ListTopTargets(Error &err, int64_t iQuiz, int64_t maxCount, CiRatedTarget *pDest) override;
  Error RecordQuizTarget(int64_t iQuiz, int64_t iTarget, double amount) override;
  Error ReleaseQuiz(int64_t iQuiz) override;
  // A forced switch destroys the shards' quizzes (BaseEngine.cpp:650-668), a shutdown likewise: what this engine keeps per quiz goes too
  Error StartMaintenance(bool force) override {
    std::lock_guard<OpLock> lk(_opMu);
    Error e = FlushAnswers();
    if (!e.ok()) return e;
    e = AllLocked([&](HipEngine &sh) { return sh.StartMaintenance(force); });
    if (e.ok() && force) ForgetQuizzes();
    return e;
  }
  Error FinishMaintenance() override { return All([&](HipEngine &e) { return e.FinishMaintenance(); }); }
  Error Shutdown(const char *saveFilePath) override {
    if (saveFilePath && *saveFilePath) { Error e = SaveKB(saveFilePath, false); if (!e.ok()) return e; }   // BaseEngine.cpp:270-300
    std::lock_guard<OpLock> lk(_opMu);
    (void)FlushAnswers();
    Error e = AllLocked([&](HipEngine &sh) { return sh.Shutdown(nullptr); });
    if (e.ok()) ForgetQuizzes();
    return e;
  }
  bool MapIds(int which, bool toPerm, int64_t count, int64_t *pIds) override {
    if (which == 0) {   // questions: the global compact <-> permanent map lives here (the shards' own maps are over local ids)
      std::lock_guard<OpLock> lk(_opMu);
      bool ok = true;
      for (int64_t i = 0; i < count; i++) {
        pIds[i] = toPerm ? _questionIds.PermanentOf(pIds[i]) : _questionIds.SlotOf(pIds[i]);
        ok = ok && pIds[i] != -1;
      }
      return ok;
    }
    return _sh[0]->MapIds(which, toPerm, count, pIds);
  }
  bool EnsurePermQuizGreater(int64_t bound) override { std::lock_guard<OpLock> lk(_opMu); bool ok = true; for (auto &s : _sh) ok = s->EnsurePermQuizGreater(bound) && ok; return ok; }
  bool RemapQuizPermId(int64_t a, int64_t b) override { std::lock_guard<OpLock> lk(_opMu); bool ok = true; for (auto &s : _sh) ok = s->RemapQuizPermId(a, b) && ok; return ok; }
  Error SaveKB(const char *filePath, bool doubleBuffer) override;
  Error SaveKBAs(const char *filePath, uint8_t precType) override;
  Error SaveKBShard(const char *, uint8_t) override {
    return Error::MakeP(ErrCode::NotImplemented, "Feature=SaveKBShard of a one-process sharded engine", "Its shards are saved together: SaveKB / SaveKBAs.");
  }
  static ShardedEngine *Load(Error &err, const char *filePath, const std::vector<int> &devices, uint8_t precType = 0);
  Error AddQsTs(int64_t nQuestions, CiAddQorTParam *pAqps, int64_t nTargets, CiAddQorTParam *pAtps) override;
  Error RemoveQuestions(int64_t n, const int64_t *pQIds) override;
  Error RemoveTargets(int64_t n, const int64_t *pTIds) override;
  Error Compact(int64_t *pnQuestions, const int64_t **ppOldQuestions, int64_t *pnTargets, const int64_t **ppOldTargets) override;
  Error ClearOldQuizzes(int64_t maxCount, double maxAgeSec) override;

  Error SetOption(const char *name, int64_t value) override {
    const std::string n(name ? name : "");
    std::lock_guard<OpLock> lk(_opMu);
    Error e = FlushAnswers();
    if (!e.ok()) return e;
    if (n == "combine" || n == "combine_linger_us") {   // this engine's own combining (the shards are driven one call at a time)
      if (!AcceptOption(*FindOption(name), value)) return Error::Make(ErrCode::UnhandledCase, "Unknown option or value out of range: " + n);
      (n == "combine" ? _optCombine : _optLingerUs) = value;
      return Error();
    }
    e = AllLocked([&](HipEngine &sh) { return sh.SetOption(name, value); });
    if (!e.ok()) return e;   // (a value the shards refuse changes nothing here either)
    if (n == "select") _select = value;   // (kept here too: NextQuestion dispatches on it)
    if (n == "seed") _rng.Seed((uint64_t)value);
    return Error();
  }
  int64_t GetOption(const char *name) const override {
    const std::string n(name ? name : "");
    if (n == "shards") return (int64_t)_sh.size();
    if (n == "shards_in_flight_max") return _shardsInFlightMax;   // the most shards whose sweeps were enqueued before the first was waited for (newest call)
    if (n == "combine") return _optCombine;
    if (n == "combine_linger_us") return _optLingerUs;
    if (n == "combined_batches") return (int64_t)_combBatches.load();       // sweeps that served more than one NextQuestion call ...
    if (n == "combined_requests") return (int64_t)_combRequests.load();     // ... the calls they served ...
    if (n == "combined_max_batch") return (int64_t)_combMaxBatch.load();    // ... and the largest of them
    if (n == "posted_ops") return (int64_t)_postedOps.load();               // calls that found the engine taken and were run by its holder
    if (n == "answer_flushes") return (int64_t)_answerFlushes.load();       // hand-overs of gathered answers to the shards ...
    if (n == "answers_flushed") return (int64_t)_answersFlushed.load();     // ... the answers they carried ...
    if (n == "answer_max_flush") return (int64_t)_answerMaxFlush.load();    // ... and the most in one
    if (n == "update_max_flush") return (int64_t)_answerMaxFlush.load();    // (the one-device engine's name for it)
    if (n == "start_batches") return (int64_t)_startBatches.load();         // launches that started several quizzes
    if (n == "peer_access") return _peerAll ? 1 : 0;                        // every pair of this engine's devices maps each other's memory
    if (n == "staged_rows") return (int64_t)_stagedRows.load();             // rows of other shards' questions that were copied instead of read in place
    if (n == "train_barriers") return (int64_t)_trainBarriers.load();
    return _sh[0]->GetOption(name);
  }
  const char *EvalKernelName() const override { return _sh[0]->EvalKernelName(); }
  Error SetKB(const double *pA, const double *pD, const double *pB) override {   // (the gathered answers read the cube as it was when they were given)
    return All([&](HipEngine &sh) {
      const size_t q0 = (size_t)sh.FirstQuestion();
      return sh.SetKB(pA + q0 * (size_t)_K * (size_t)_T, pD + q0 * (size_t)_T, pB);
    });
  }
  Error GetKB(double *pA, double *pD, double *pB) override {
    return All([&](HipEngine &sh) {
      const size_t q0 = (size_t)sh.FirstQuestion();
      return sh.GetKB(pA ? pA + q0 * (size_t)_K * (size_t)_T : nullptr, pD ? pD + q0 * (size_t)_T : nullptr, &sh == _sh[0].get() ? pB : nullptr);
    });
  }
  Error FillSynthetic(double nTrain, double noiseAmp, uint64_t seed) override { return All([&](HipEngine &e) { return e.FillSynthetic(nTrain, noiseAmp, seed); }); }
  Error SetTargetGaps(int64_t n, const int64_t *ids) override { return All([&](HipEngine &e) { return e.SetTargetGaps(n, ids); }); }
  Error SetQuestionGaps(int64_t n, const int64_t *ids) override {
    std::lock_guard<OpLock> lk(_opMu);
    { Error fe = FlushAnswers(); if (!fe.ok()) return fe; }
    Error e = AllLocked([&](HipEngine &eng) { return eng.SetQuestionGaps(n, ids); });
    if (e.ok())
      for (int64_t i = 0; i < n; i++)
        if (std::find(_qGapList.begin(), _qGapList.end(), ids[i]) == _qGapList.end()) { _qGapList.push_back(ids[i]); _questionIds.Vacate(ids[i]); }
    RefreshGapBits();
    return e;
  }
  Error EvalPriorities(int64_t iQuiz, double *pOut, int64_t n) override {
    if (n != _Q) return Error::MakeP(ErrCode::IndexOutOfRange, "n=" + std::to_string(n), "Priority buffer length must equal the question count.");
    return All([&](HipEngine &sh) { return sh.EvalPriorities(iQuiz, pOut + sh.FirstQuestion(), sh.LocalQuestions()); });
  }
  int64_t NextQuestionArgmax(Error &err, int64_t iQuiz) override { return Combine(err, iQuiz, SelKind::Argmax, 0); }
  int64_t NextQuestionSampled(Error &err, int64_t iQuiz, uint64_t rnd) override { return Combine(err, iQuiz, SelKind::Sampled, rnd); }
  Error GetPriors(int64_t iQuiz, double *pOut, int64_t n) override {
    Error e = EnsureApplied(iQuiz);
    if (!e.ok()) return e;
    Touch(iQuiz);
    return _sh[0]->GetPriors(iQuiz, pOut, n);
  }
  Error NextQuestionArgmaxBatch(int64_t n, const int64_t *pQuizzes, int64_t *pOut) override;
  Error NextQuestionSampledBatch(int64_t n, const int64_t *pQuizzes, const uint64_t *pRnd, int64_t *pOut) override;
  Error NextQuestionBatch(int64_t n, const int64_t *pQuizzes, int64_t *pOut) override;
  Error ValidateSelectionBatch(int64_t n, const int64_t *pQuizzes);
  Error EnqueueBatchOnShards(int64_t n, const int64_t *pQuizzes, bool wantPriorities, std::vector<uint64_t> &tags);   // (under _opMu, the gathered answers first)
  Error EvalPrioritiesBatch(int64_t n, const int64_t *pQuizzes, double *pOut) override;
  Error SelectArgmaxBatch(int64_t n, const int64_t *pQuizzes, CiHipSelection *pOut) override;
  Error Log2HotArray(const double *pIn, double *pOut, int64_t n) override { return _sh[0]->Log2HotArray(pIn, pOut, n); }
  hipStream_t GetStream() const override { return _sh[0]->GetStream(); }
  Error SetStream(hipStream_t) override { return NotSharded("SetStream"); }
  Error Synchronize() override { return All([&](HipEngine &sh) { return sh.Synchronize(); }); }
  Error Quiesce() override { return All([&](HipEngine &sh) { return sh.Quiesce(); }); }
  Error EnqueueSelectArgmax(int64_t, void *) override { return NotSharded("EnqueueSelectArgmax"); }
  Error EnqueueSelectArgmaxFlag(int64_t, void *, void *, uint64_t) override { return NotSharded("EnqueueSelectArgmaxFlag"); }
  Error EnqueueEval(int64_t iQuiz) override { return All([&](HipEngine &sh) { return sh.EnqueueEval(iQuiz); }); }
  Error GetPriorDevicePtr(int64_t iQuiz, void **ppDev, int64_t *pLdT) override {
    Error e = EnsureApplied(iQuiz);
    if (!e.ok()) return e;
    return _sh[0]->GetPriorDevicePtr(iQuiz, ppDev, pLdT);
  }
  Error RecordAnswerRemote(int64_t, int64_t) override { return NotSharded("RecordAnswerRemote"); }
  // (row packages serve shards driven by processes of their own; this engine holds every question, so a package has nothing to add)
  int64_t AnswerRowSlotBytes() const override { return _sh[0]->AnswerRowSlotBytes(); }
  Error PackAnswerRows(int64_t, const AQ *, void *, void *, uint64_t) override { return NotSharded("PackAnswerRows"); }
  int64_t ResumeQuizFromRows(Error &err, int64_t nAnswered, const AQ *pAQs, const void *) override { return ResumeQuiz(err, nAnswered, pAQs); }
  Error ResumeQuizBatchFromRows(int64_t n, const int64_t *pCounts, const AQ *pAQs, const void *, int64_t *pQuizzes) override {
    return ResumeQuizBatch(n, pCounts, pAQs, pQuizzes);
  }
  Error RecordAnswerBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pAnswers) override {   // (gathered like any other answers: one hand-over to the shards)
    if (n > 0 && (!pQuizzes || !pAnswers)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
    for (int64_t i = 0; i < n; i++) { Error e = RecordAnswerDeferred(pQuizzes[i], pAnswers[i]); if (!e.ok()) return e; }
    return FlushNow();
  }
  // A page of answers per quiz: validated whole, in the one-device engine's order, then served position by position through the
  // gathered answers (one hand-over to the shards per position: the bits of the consecutive calls; no kernel of its own, no speed claimed)
  Error RecordAnswerPageBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const AQ *pAQs, double *pLikelihood) override;
  Error RecordAnswerPageBatchFromRows(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const AQ *pAQs, double *pLikelihood, const void *) override {
    return RecordAnswerPageBatch(n, pQuizzes, pCounts, pAQs, pLikelihood);   // (this engine holds every question: a package has nothing to add)
  }
  Error ListTopTargetsBatch(int64_t n, const int64_t *pQuizzes, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts) override {
    // every shard holds every quiz's whole posterior: the gathered answers reach the shards, then one of them lists
    Error e = FlushNow();
    if (!e.ok()) return e;
    return _sh[0]->ListTopTargetsBatch(n, pQuizzes, maxCount, pDest, pCounts);
  }
  Error ListTopTargetsAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pListOf, int64_t nLists, const int64_t *pListCounts,
                                 const int64_t *pTargets, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts, double *pMass) override {
    // the posteriors are replicated: the gathered answers reach the shards, a quiz whose replicas may differ is refused, shard 0 lists
    Error e = FlushNow();
    for (int64_t i = 0; e.ok() && i < n && pQuizzes; i++) e = FailedQuiz(pQuizzes[i]);
    if (!e.ok()) return e;
    e = _sh[0]->ListTopTargetsAmongBatch(n, pQuizzes, pListOf, nLists, pListCounts, pTargets, maxCount, pDest, pCounts, pMass);
    for (int64_t i = 0; e.ok() && i < n && pQuizzes; i++) Touch(pQuizzes[i]);
    return e;
  }
  // (as ListTopTargetsAmongBatch: replicated posteriors, shard 0 answers)
  Error QuizStatusBatch(int64_t n, const int64_t *pQuizzes, int64_t nLevels, const double *pLevels, CiHipQuizStatus *pStatus, int64_t *pLevelCounts,
                        double *pLevelMass) override {
    Error e = FlushNow();
    for (int64_t i = 0; e.ok() && i < n && pQuizzes; i++) e = FailedQuiz(pQuizzes[i]);
    if (!e.ok()) return e;
    e = _sh[0]->QuizStatusBatch(n, pQuizzes, nLevels, pLevels, pStatus, pLevelCounts, pLevelMass);
    for (int64_t i = 0; e.ok() && i < n && pQuizzes; i++) Touch(pQuizzes[i]);
    return e;
  }
  Error RankTargetsBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pTargets, double *pProb, int64_t *pRank) override {
    Error e = FlushNow();
    for (int64_t i = 0; e.ok() && i < n && pQuizzes; i++) e = FailedQuiz(pQuizzes[i]);
    if (!e.ok()) return e;
    e = _sh[0]->RankTargetsBatch(n, pQuizzes, pTargets, pProb, pRank);
    for (int64_t i = 0; e.ok() && i < n && pQuizzes; i++) Touch(pQuizzes[i]);
    return e;
  }
  int64_t GetQuizAnswers(Error &err, int64_t iQuiz, AQ *pDest, int64_t capacity) override {
    // every shard records every answer of every quiz: the gathered answers reach the shards, then one of them reads
    err = FlushNow();
    if (!err.ok()) return -1;
    return _sh[0]->GetQuizAnswers(err, iQuiz, pDest, capacity);
  }
  int64_t ListTopQuestions(Error &err, int64_t iQuiz, int64_t maxCount, CiRatedQuestion *pDest) override;
  Error ListTopQuestionsBatch(int64_t n, const int64_t *pQuizzes, int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) override;
  Error StartQuizBatch(int64_t n, int64_t *pQuizzes) override {
    if (n > 0 && !pQuizzes) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
    for (int64_t i = 0; i < n; i++) {
      Error e;
      pQuizzes[i] = StartQuiz(e);
      if (pQuizzes[i] < 0) { for (int64_t j = 0; j < i; j++) (void)ReleaseQuiz(pQuizzes[j]); return e; }
    }
    return Error();
  }

 private:
  ShardedEngine() = default;

  // ---- the engine's lock and its posted operations ---------------------------------------------------------------------------
  struct SelRequest;
  struct Flight;
  enum class OpKind {
    StartQuiz,          // result = the quiz
    ReleaseQuiz,        // (iQuiz)
    RecordQuizTarget,   // (iQuiz, iTarget, amount)
    Flush,              // hand the gathered answers to the shards
    LaunchBatch         // a leader's LaunchBatch(ctx, batch, flight)
  };
  struct Op {
    OpKind kind;
    explicit Op(OpKind k) : kind(k) {}
    int64_t iQuiz = -1, iTarget = -1;
    double amount = 0;
    Error err;
    int64_t result = -1;
    int ctx = 0;
    std::vector<SelRequest *> *batch = nullptr;
    Flight *flight = nullptr;
    std::atomic<int> state{kOpPosted};
    Op *next = nullptr;
  };
  using OpLock = PostingLock<Op, ShardedEngine>;   // (a sleeping lock; releasing it runs whatever was posted meanwhile: Execute)
  mutable OpLock _opMu{this, &ShardedEngine::Execute};
  void Execute(Op *ordered);           // (the lock held)
  void RunOrPost(Op &op) { if (_opMu.RunOrPost(op)) _postedOps.fetch_add(1, std::memory_order_relaxed); }

  template <typename F>
  Error All(F &&f) {   // (the gathered answers first: what follows reads or changes what they read)
    std::lock_guard<OpLock> lk(_opMu);
    Error fe = FlushAnswers();
    return fe.ok() ? AllLocked(f) : fe;
  }
  template <typename F>
  Error AllLocked(F &&f) { for (auto &s : _sh) { Error e = f(*s); if (!e.ok()) return e; } return Error(); }
  int OwnerOf(int64_t qGlobal) const {
    for (size_t s = 0; s < _sh.size(); s++) if (_sh[s]->OwnsQuestion(qGlobal)) return (int)s;
    return -1;
  }

  // ---- per-quiz state kept HERE (the shards keep the posterior, the asked bits and the answers): last use (BaseQuiz::OnUsage,
  // BaseEngine.cpp:417 -- ClearOldQuizzes is decided once for all shards), the active question (CEQuiz::_activeQuestion) and
  // whether an answer of the quiz is still among the gathered ones.  Read and written by the quiz's own client without a lock
  // (no concurrent calls on one quiz, IPqaEngine.h:44): a table of chunks that only grows, under _opMu.
  // failed: a hand-over of this quiz's answer did not reach every shard (FlushAnswers): the posterior replicas may differ, and every
  // later call on the quiz says so instead of selecting from one of them; released like any other quiz
  struct QuizRow {
    std::atomic<int64_t> lastUse{0}, active{-1};
    std::atomic<int> pending{0}, failed{0};
    void Clear() { lastUse.store(0); active.store(-1); pending.store(0); failed.store(0); }   // the quiz is not there (any more)
  };
  static constexpr int64_t kRowsPerChunk = 4096, kRowChunks = 8192;
  std::atomic<QuizRow *> _rows[kRowChunks] = {};
  std::atomic<int64_t> _registrySize{0};       // ids below this have been handed out at some time
  QuizRow *Row(int64_t id) const {
    if (id < 0 || id >= kRowsPerChunk * kRowChunks) return nullptr;
    QuizRow *c = _rows[id / kRowsPerChunk].load(std::memory_order_acquire);
    return c ? c + id % kRowsPerChunk : nullptr;
  }
  QuizRow *LiveRow(int64_t id) const { QuizRow *r = Row(id); return r && r->lastUse.load(std::memory_order_relaxed) != 0 ? r : nullptr; }
  QuizRow *EnsureRow(int64_t id) {             // (_opMu held)
    if (id < 0 || id >= kRowsPerChunk * kRowChunks) return nullptr;
    QuizRow *c = _rows[id / kRowsPerChunk].load(std::memory_order_acquire);
    if (!c) { c = new QuizRow[kRowsPerChunk]; _rows[id / kRowsPerChunk].store(c, std::memory_order_release); }
    if (id >= _registrySize.load(std::memory_order_relaxed)) _registrySize.store(id + 1, std::memory_order_relaxed);
    return c + id % kRowsPerChunk;
  }
  void Touch(int64_t iQuiz) { if (QuizRow *r = LiveRow(iQuiz)) r->lastUse.store((int64_t)NowStamp(), std::memory_order_relaxed); }
  static int64_t NowStamp() { const time_t t = time(nullptr); return t == 0 ? 1 : (int64_t)t; }
  void NewQuiz(int64_t id) { QuizRow *r = EnsureRow(id); if (r) { r->Clear(); r->lastUse.store(NowStamp()); } }
  void ForgetQuizzes() {
    { std::lock_guard<std::mutex> lk(_pendMu); _pending.clear(); _pendingCount.store(0); }
    for (int64_t id = 0; id < _registrySize.load(); id++) if (QuizRow *r = Row(id)) r->Clear();
  }
  // The error a call on quiz `iQuiz` gets when the quiz is not there or the mode is wrong: the shards' own (BaseEngine::UseQuiz,
  // BaseEngine.cpp:399-419; the MaintenanceSwitch gate), asked of shard 0 by a call that changes nothing.
  Error QuizError(int64_t iQuiz) { Error e; (void)_sh[0]->GetActiveQuestionId(e, iQuiz); return e; }
  QuizRow *UseQuiz(Error &err, int64_t iQuiz);

  // ---- the gathered answers ---------------------------------------------------------------------------------------------------
  struct PendingAnswer { int64_t iQuiz, qGlobal, iAnswer; };
  std::mutex _pendMu;
  std::vector<PendingAnswer> _pending;
  std::atomic<size_t> _pendingCount{0};
  std::atomic<int64_t> _answersSinceSweep{0}, _lastCombined{0};
  Error RecordAnswerDeferred(int64_t iQuiz, int64_t iAnswer);
  Error FlushAnswers();                 // (_opMu held) everything gathered so far: one ApplyAnswers per shard
  Error FlushNow() {                    // through the lock: when it returns, every hand-over begun before it has reached all shards
    Op op(OpKind::Flush);
    RunOrPost(op);
    return op.err;
  }
  // Before anything reads quiz `iQuiz`'s posterior on a shard: its answer -- if one is among the gathered ones, or in a hand-over
  // another thread is making right now (the quiz's flag falls only after the last shard has it) -- has reached the shards.
  Error FailedQuiz(int64_t iQuiz) const {
    QuizRow *r = LiveRow(iQuiz);
    if (r && r->failed.load(std::memory_order_acquire))
      return Error::MakeP(ErrCode::Internal, "quizId=" + std::to_string(iQuiz), "An answer of this quiz did not reach every shard: its posteriors may differ. Release the quiz.");
    return Error();
  }
  Error EnsureApplied(int64_t iQuiz) {
    QuizRow *r = LiveRow(iQuiz);
    Error e = r && r->pending.load(std::memory_order_acquire) ? FlushNow() : Error();
    return e.ok() ? FailedQuiz(iQuiz) : e;
  }
  std::vector<char> _qGapBit;           // per global question: a gap (mirror of _qGapList for RecordAnswer's check)
  void RefreshGapBits() { _qGapBit.assign((size_t)_Q, 0); for (int64_t g : _qGapList) if (g >= 0 && g < _Q) _qGapBit[(size_t)g] = 1; }

  // ---- other shards' rows: peer access, or staged copies; trainings are ordered around the reads by events -------------------
  bool _peerAll = true, _forceNoPeer = false;
  std::vector<char> _peer;              // [s * N + o]: shard s's device reads shard o's memory in place
  bool InPlace(size_t s, size_t o) const { return !_forceNoPeer && _peer[s * _sh.size() + o]; }
  std::vector<hipEvent_t> _readsDone, _trainDone;   // per shard: behind its reads of other shards' rows / behind its training kernels
  std::vector<char> _remoteReads;       // per shard: it has read other shards' rows since its last _readsDone
  std::vector<uint64_t> _trainEpoch;    // per shard: trainings it has run
  std::vector<uint64_t> _seenTrain;     // [s * N + o]: the training epoch of shard o that shard s's stream is ordered behind
  Error WaitForTraining(size_t s, size_t o);     // before shard s reads shard o's rows
  Error BeforeTraining();               // every shard's reads of other shards' rows so far are ordered before every shard's training
  Error AfterTraining();
  // A training on every shard (_opMu held).  The reference validates every answered question before any Add subtask runs
  // (CETrainSubtaskDistrib.h:26-45): a gap question owned by shard k must not leave shards 0..k-1 trained and their vB replicas
  // ahead -- so the gathered answers go out, EVERY shard validates, and only then every shard applies the steps that fall on its
  // own questions (and its vB replica), between the two barriers that order the other shards' reads of those rows around it.
  template <typename Validate, typename Apply>
  Error TrainOnAllShards(Validate &&validate, Apply &&apply) {
    Error e = FlushAnswers();
    if (!e.ok()) return e;
    for (auto &s : _sh) { e = validate(*s); if (!e.ok()) return e; }
    e = BeforeTraining();
    if (!e.ok()) return e;
    for (auto &s : _sh) { e = apply(*s); if (!e.ok()) break; }
    Error ae = AfterTraining();
    return e.ok() ? ae : e;
  }
  // The rows a resumed quiz (or a batch of them) reads, `total` answered questions in all: every shard computes the posterior itself
  // from row POINTERS, the rows of other shards' questions in place or staged.  ResolveRows: per answered question its owner and
  // its two rows (*iBad: the entry that was refused).  StageFor: before shard s reads them -- the owners' trainings are waited for,
  // and the rows it cannot read in place are marked for staging.
  struct ResumeRows { std::vector<const void *> rows; std::vector<int> rowDev, owners; std::vector<char> stage; };
  Error ResolveRows(int64_t total, const AQ *pAQs, ResumeRows &r, int64_t *iBad);
  Error StageFor(size_t s, ResumeRows &r, bool *allInPlace);
  std::atomic<uint64_t> _stagedRows{0}, _trainBarriers{0};

  // ---- one NextQuestion by itself ------------------------------------------------------------------------------------------------
  int64_t SelectArgmaxLocked(Error &err, int64_t iQuiz, double *pPriority);
  int64_t SelectSampledLocked(Error &err, int64_t iQuiz, uint64_t rnd);
  int64_t Commit(Error &err, int64_t iQuiz, int64_t qGlobal);

  // A quiz's asked-or-gap bitmap in GLOBAL numbering (64-bit packs, the bits past the last question set) out of the shards' 32-bit words
  // in local bit order (their ranges are not multiples of 32).  wordsOf(s): shard s's words, nullptr -> false.  `skip` is the caller's.
  template <typename WordsOf>
  bool GlobalSkip(WordsOf &&wordsOf, std::vector<uint64_t> &skip) const {
    skip.assign((size_t)((_Q + 63) / 64) + 1, 0);
    for (size_t s = 0; s < _sh.size(); s++) {
      const uint32_t *w = wordsOf(s);
      if (!w) return false;
      const int64_t q0 = _sh[s]->FirstQuestion(), nLocal = _sh[s]->LocalQuestions();
      for (int64_t k = 0; k < nLocal; k++)
        if ((w[(size_t)(k >> 5)] >> (k & 31)) & 1u) skip[(size_t)((q0 + k) >> 6)] |= 1ULL << ((q0 + k) & 63);
    }
    for (int64_t q = _Q; q < (int64_t)skip.size() * 64; q++) skip[(size_t)(q >> 6)] |= 1ULL << (q & 63);
    return true;
  }
  static bool Skipped(const std::vector<uint64_t> &skip, int64_t q) { return ((skip[(size_t)(q >> 6)] >> (q & 63)) & 1ULL) != 0; }
  // CpuEngine.cpp:403-407: a pick that is asked or a gap falls to BaseEngine::FindNearestQuestion, over the global bitmap
  static int64_t NearestFree(const std::vector<uint64_t> &skip, int64_t pick, int64_t nQ) {
    return pick >= 0 && Skipped(skip, pick) ? FindNearestInPacks(pick, nQ, [&](int64_t p) { return ~skip[(size_t)p]; }) : pick;
  }

  // ---- concurrent NextQuestion calls: combined (combining.h; as hip_engine_combine.cpp's Combine / LaunchBatch / CollectBatch) -------
  struct SelRequest {
    int64_t iQuiz = -1;
    SelKind kind = SelKind::Argmax;    // (Sampled: with rnd)
    uint64_t rnd = 0;
    int64_t result = -1;
    Error err;
    std::atomic<int> state{kReqWaiting};   // (combining.h) kReqSelect: select for yourself from `views`
    std::vector<PriorityView> views;   // kReqSelect: per shard, this quiz's priority vector on the host
    std::vector<uint64_t> skip;        // kReqSelect: asked questions and gaps in GLOBAL numbering as the sweeps saw them (64-bit packs)
    CombineCtx *ctx = nullptr;
  };
  struct Flight {
    std::vector<SelRequest *> live;    // the requests whose sweep is in flight
    std::vector<HipEngine::CombinedFlight> shard;
    std::vector<std::vector<uint32_t>> unavailable;   // per shard: live.size() x words
    bool anySampled = false;
  };
  CombineCtx _bctx[2];                 // (mu: one combined sweep at a time in a context, and the batch calls of the ABI in context 0)
  Combiner<SelRequest, CombineCtx> _comb{_bctx};
  std::mutex _rngMu;
  int64_t _optCombine = EngineOptions().combine, _optLingerUs = EngineOptions().lingerUs;   // "combine", "combine_linger_us": kept here, not in the shards
  std::atomic<int> _activeCallers{0};
  bool Concurrent() const { return _optCombine && _activeCallers.load(std::memory_order_relaxed) > 1; }
  int64_t Combine(Error &err, int64_t iQuiz, SelKind kind, uint64_t rnd);
  void LaunchBatch(int ctx, std::vector<SelRequest *> &batch, Flight &f);
  void LaunchBatchLocked(int ctx, std::vector<SelRequest *> &batch, Flight &f);
  bool CollectBatch(int ctx, std::vector<SelRequest *> &batch, Flight &f, SelRequest *own);
  int64_t SelectFromViews(SelRequest *r);
  void ServeAlone(SelRequest *r) {     // (_opMu held)
    r->err = FailedQuiz(r->iQuiz);
    if (!r->err.ok()) { r->result = -1; return; }
    r->result = r->kind == SelKind::Argmax ? SelectArgmaxAlone(r->err, r->iQuiz) : SelectSampledLocked(r->err, r->iQuiz, r->rnd);
  }
  int64_t SelectArgmaxAlone(Error &err, int64_t iQuiz) {
    const int64_t q = SelectArgmaxLocked(err, iQuiz, nullptr);
    if (!err.ok()) return -1;
    return Commit(err, iQuiz, q);
  }
  std::atomic<uint64_t> _combBatches{0}, _combRequests{0}, _combMaxBatch{0}, _postedOps{0}, _answerFlushes{0}, _answersFlushed{0},
      _answerMaxFlush{0}, _startBatches{0};

  std::vector<std::unique_ptr<HipEngine>> _sh;
  int64_t _K = 0, _Q = 0, _T = 0;
  int64_t _select = 0;
  Slot *_slots = nullptr;               // [shards], pinned + mapped: written by the sweeps' finishers, polled here
  uint64_t _step = 0;
  std::vector<double> _hostPriority;
  IdLedger _questionIds;                     // global question ids
  SelectorRng _rng;                          // seeded by Create
  int64_t _shardsInFlightMax = 0;
  // ---- maintenance-mode edits of the dimensions (CpuEngine.cpp:468-658, BaseEngine.cpp:721-873): the ids are worked out HERE,
  // over the global question axis, exactly as the unsharded engine works them out; the data moves by REBUILDING the shards --
  // new shards over SRPoolRunner::CalcSplit of the new question count, every new question taking its rows from wherever the old
  // shards hold them (in place over peer access, columns picked by the target map), all-or-nothing (the old shards stay until
  // the new ones are complete).
  std::vector<int64_t> _qGapList;           // global question gaps, LIFO like PqaCore/GapTracker.h (the shards keep bitmaps of their own)
  std::vector<int> _devices;
  Error Rebuild(int64_t newQ, int64_t newT, const std::vector<int64_t> &srcQ, const std::vector<int64_t> &srcT,
                const std::vector<int64_t> &qGaps, const std::vector<int64_t> &tGaps, const IdLedger &targetIds,
                const std::vector<int64_t> &fillT, const std::vector<double> &fillTInit, const std::vector<int64_t> &fillQ,
                const std::vector<double> &fillQInit);
  // Shard s of N over qTotal questions in all, from *first on (SRPoolRunner::CalcSplit, SRPlatform/Interface/SRPoolRunner.h:96-110:
  // the first qTotal % N shards hold one question more); *first moves to the next shard's.
  static HipEngine *NewShard(Error &err, CiEngineDefinition def, int64_t s, int64_t N, int64_t qTotal, int device, int64_t *first) {
    def._nQuestions = qTotal / N + (s < qTotal % N ? 1 : 0);
    const CiHipShard sh{*first, qTotal, device, 0};
    *first += def._nQuestions;
    return HipEngine::Create(err, def, &sh);
  }
  Error InitCrossShard();               // peer access between the devices, the ordering events
  void AdoptShards();                   // what every (re)built set of shards is told
  void ReleaseEverywhere(int64_t iQuiz, size_t nShards) {   // roll a partly created quiz back
    for (size_t s = 0; s < nShards; s++) (void)_sh[s]->ReleaseQuiz(iQuiz);
  }
};

ShardedEngine::~ShardedEngine() {
  for (size_t s = 0; s < _sh.size(); s++) {
    hipSetDevice(_sh[s]->Device());
    if (s < _readsDone.size() && _readsDone[s]) hipEventDestroy(_readsDone[s]);
    if (s < _trainDone.size() && _trainDone[s]) hipEventDestroy(_trainDone[s]);
  }
  _sh.clear();
  if (_slots) hipHostFree(_slots);
  for (auto &c : _rows) delete[] c.load();
}

// A list of operations under the lock (one, from a caller that found the lock free; or everything posted so far).  All of them are
// concurrent calls, so any order among them is a valid one: first the gathered answers go to the shards (whatever follows reads
// posteriors or the quizzes' answer lists), then the registry changes in their order, the quiz starts in ONE launch per shard, the
// trainings between their two barriers, and last the combined sweeps -- they are what the most clients wait for.
void ShardedEngine::Execute(Op *ordered) {
  Error flushErr = FlushAnswers();
  std::vector<Op *> starts, trains;
  for (Op *op = ordered; op != nullptr; op = op->next) {
    if (op->kind == OpKind::Flush) { op->err = flushErr; continue; }
    if (op->kind == OpKind::StartQuiz) { starts.push_back(op); continue; }
    if (op->kind == OpKind::RecordQuizTarget) { op->err = flushErr; trains.push_back(op); continue; }
    if (op->kind == OpKind::ReleaseQuiz) {   // every shard releases (a shard that has not got the quiz says so): the registries stay in step
      Error first;
      size_t released = 0;
      for (auto &s : _sh) { Error e = s->ReleaseQuiz(op->iQuiz); if (e.ok()) released++; else if (first.ok()) first = e; }
      // (some shards released and one refused -- a NextQuestion of the quiz selecting on another thread, the client's own error: the
      //  refusing shards are asked again until they agree, so that every shard's registry holds the same quizzes)
      for (int tries = 0; !first.ok() && released > 0 && released < _sh.size() && tries < 2000; tries++) {
        first = Error();
        released = 0;
        for (auto &s : _sh) {
          Error qe;
          (void)s->GetActiveQuestionId(qe, op->iQuiz);
          if (!qe.ok()) { released++; continue; }              // (this shard has let it go already)
          Error e = s->ReleaseQuiz(op->iQuiz);
          if (e.ok()) released++; else if (first.ok()) first = e;
        }
        if (!first.ok()) { struct timespec ts{0, 50000}; nanosleep(&ts, nullptr); }
      }
      if (first.ok()) if (QuizRow *r = Row(op->iQuiz)) r->Clear();
      op->err = first;
    }
  }
  if (!starts.empty()) {
    // the StartQuiz calls that arrived together: ONE launch per shard sets all their priors (prior_kernels.hip: start_quiz_batch_kernel)
    const int64_t k = (int64_t)starts.size();
    std::vector<int64_t> ids((size_t)k), got((size_t)k);
    Error err;
    size_t done = 0;
    for (; done < _sh.size() && err.ok(); done++) {
      std::vector<int64_t> &dst = done == 0 ? ids : got;
      err = _sh[done]->StartQuizBatch(k, dst.data());
      if (err.ok() && done > 0 && got != ids) {
        for (int64_t id : got) (void)_sh[done]->ReleaseQuiz(id);
        err = Error::Make(ErrCode::Internal, "The shards' quiz registries have diverged.");
      }
      if (!err.ok()) break;
    }
    if (!err.ok()) {
      for (size_t s = 0; s < done; s++) for (int64_t id : ids) (void)_sh[s]->ReleaseQuiz(id);   // all or nothing
      for (Op *op : starts) { op->err = err; op->result = -1; }
    } else {
      for (int64_t i = 0; i < k; i++) { NewQuiz(ids[(size_t)i]); starts[(size_t)i]->result = ids[(size_t)i]; }
      if (k > 1) _startBatches.fetch_add(1, std::memory_order_relaxed);
    }
  }
  if (!trains.empty()) {
    // RecordQuizTarget (BaseEngine.cpp:529-566, CpuEngine.cpp:442-466), every call with its own error: one that a shard refuses
    // is left out, the others train (no barriers when none is left)
    Error te = !flushErr.ok() ? flushErr : TrainOnAllShards(
        [&](HipEngine &sh) {
          bool any = false;
          for (Op *op : trains) {
            if (op->err.ok() && op->amount > 0) op->err = sh.ValidateTrain(0, nullptr, op->iTarget, op->iQuiz);
            any = any || op->err.ok();
          }
          return any ? Error() : trains[0]->err;
        },
        [&](HipEngine &sh) {
          for (Op *op : trains) {
            if (!op->err.ok()) continue;
            if (&sh == _sh[0].get()) Touch(op->iQuiz);
            op->err = sh.RecordQuizTarget(op->iQuiz, op->iTarget, op->amount);
          }
          return Error();
        });
    if (!te.ok()) for (Op *op : trains) if (op->err.ok()) op->err = te;
  }
  for (Op *op = ordered; op != nullptr; op = op->next)
    if (op->kind == OpKind::LaunchBatch) LaunchBatchLocked(op->ctx, *op->batch, *op->flight);
}

// ---- creation -------------------------------------------------------------------------------------------------------------------
ShardedEngine *ShardedEngine::Create(Error &err, const CiEngineDefinition &def, const std::vector<int> &devices) {
  std::unique_ptr<ShardedEngine> eng(new ShardedEngine());
  const int64_t N = (int64_t)devices.size();
  if (def._nQuestions < N) {
    err = Error::MakeP(ErrCode::InsufficientEngineDimensions, "[nQuestions=" + std::to_string(def._nQuestions) + " of " + std::to_string(N) + "]",
                       "Fewer questions than devices in PQA_DEVICES.");
    return nullptr;
  }
  eng->_K = def._nAnswers; eng->_Q = def._nQuestions; eng->_T = def._nTargets;
  eng->_devices = devices;
  for (int64_t s = 0, first = 0; s < N; s++) {
    HipEngine *e = NewShard(err, def, s, N, def._nQuestions, devices[(size_t)s], &first);
    if (!e) return nullptr;
    eng->_sh.emplace_back(e);
  }
  err = eng->InitCrossShard();
  if (!err.ok()) return nullptr;
  if (hipHostMalloc((void **)&eng->_slots, sizeof(Slot) * (size_t)N, hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable) != hipSuccess) {
    err = Error::Make(ErrCode::Internal, "Can't allocate the shards' selection slots.");
    return nullptr;
  }
  std::memset(eng->_slots, 0, sizeof(Slot) * (size_t)N);
  eng->_select = eng->_sh[0]->GetOption("select");
  {   // the selector's generator: from the system's entropy like the reference's (SRFastRandom.h:31-40), or PQA_SEED
    std::random_device rd;
    int64_t seed = (int64_t)(((uint64_t)rd() << 32) ^ rd());
    (void)SeedFromEnvironment(seed, false);   // (a value that is refused: every shard has said so already)
    eng->_rng.Seed((uint64_t)seed);
  }
  eng->_hostPriority.resize((size_t)def._nQuestions);
  eng->_questionIds.Extend(def._nQuestions);
  eng->RefreshGapBits();
  eng->AdoptShards();
  err = Error();
  return eng.release();
}

void ShardedEngine::AdoptShards() {
  for (auto &s : _sh) s->SetExternalCallers(&_activeCallers);
}

// Where the rows of another shard's question are read from.  Peer access is enabled between every pair of distinct devices; a pair
// that cannot map each other's memory (or PQA_FORCE_NO_PEER=1: every pair, a test hook that runs on one GPU) gets staged copies --
// hipMemcpyPeerAsync needs no peer access -- of the two rows an answer needs and of the rows ResumeQuiz reads; what has no staged
// form says so when it is called (the maintenance-mode rebuild of the shards reads whole question blocks in place).  The pair's
// state is decided here, once, and logged: nothing dereferences a pointer the device cannot reach.
Error ShardedEngine::InitCrossShard() {
  const size_t N = _sh.size();
  _peer.assign(N * N, 1);
  _peerAll = true;
  if (const char *v = std::getenv("PQA_FORCE_NO_PEER")) _forceNoPeer = *v && std::strcmp(v, "0") != 0;
  for (size_t a = 0; a < N; a++)
    for (size_t b = 0; b < N; b++) {
      const int da = _sh[a]->Device(), db = _sh[b]->Device();
      if (da == db) continue;
      int can = 0;
      bool ok = hipDeviceCanAccessPeer(&can, da, db) == hipSuccess && can;
      if (ok) {
        hipSetDevice(da);
        const hipError_t e = hipDeviceEnablePeerAccess(db, 0);
        ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
        (void)hipGetLastError();
      }
      if (!ok) {
        _peer[a * N + b] = 0;
        _peerAll = false;
        DefaultLogger::Log(DefaultLogger::Severity::Warning, "Device " + std::to_string(da) + " cannot map the memory of device " + std::to_string(db) +
                                                                 ": rows of its questions are copied instead of read in place (PQA_DEVICES).");
      }
    }
  if (_forceNoPeer) _peerAll = false;
  _readsDone.assign(N, nullptr);
  _trainDone.assign(N, nullptr);
  for (size_t s = 0; s < N; s++) {
    hipSetDevice(_sh[s]->Device());
    if (hipEventCreateWithFlags(&_readsDone[s], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&_trainDone[s], hipEventDisableTiming) != hipSuccess)
      return Error::Make(ErrCode::Internal, "Can't create the shards' ordering events.");
  }
  _remoteReads.assign(N, 0);
  _trainEpoch.assign(N, 0);
  _seenTrain.assign(N * N, 0);
  return Error();
}

// Shard s is about to read rows of shard o: not before o's training kernels so far have run.
Error ShardedEngine::WaitForTraining(size_t s, size_t o) {
  const size_t N = _sh.size();
  if (s == o || _seenTrain[s * N + o] == _trainEpoch[o]) return Error();
  hipSetDevice(_sh[s]->Device());
  if (hipStreamWaitEvent(_sh[s]->GetStream(), _trainDone[o], 0) != hipSuccess) return Error::Make(ErrCode::Internal, "hipStreamWaitEvent failed.");
  _seenTrain[s * N + o] = _trainEpoch[o];
  return Error();
}

// A training writes rows that other shards' posterior kernels may still be reading (they were launched before the training call
// arrived, so they must see the rows as they were): every shard that has read other shards' rows since its last event records
// one behind those reads, and every other shard's stream waits for it before its training kernel.
Error ShardedEngine::BeforeTraining() {
  const size_t N = _sh.size();
  bool any = false;
  for (size_t t = 0; t < N; t++) {
    if (!_remoteReads[t]) continue;
    any = true;
    hipSetDevice(_sh[t]->Device());
    if (hipEventRecord(_readsDone[t], _sh[t]->GetStream()) != hipSuccess) return Error::Make(ErrCode::Internal, "hipEventRecord failed.");
  }
  if (!any) return Error();
  _trainBarriers.fetch_add(1, std::memory_order_relaxed);
  for (size_t s = 0; s < N; s++) {
    hipSetDevice(_sh[s]->Device());
    for (size_t t = 0; t < N; t++)
      if (t != s && _remoteReads[t] && hipStreamWaitEvent(_sh[s]->GetStream(), _readsDone[t], 0) != hipSuccess)
        return Error::Make(ErrCode::Internal, "hipStreamWaitEvent failed.");
  }
  std::fill(_remoteReads.begin(), _remoteReads.end(), 0);
  return Error();
}

Error ShardedEngine::AfterTraining() {
  for (size_t s = 0; s < _sh.size(); s++) {
    hipSetDevice(_sh[s]->Device());
    if (hipEventRecord(_trainDone[s], _sh[s]->GetStream()) != hipSuccess) return Error::Make(ErrCode::Internal, "hipEventRecord failed.");
    _trainEpoch[s]++;
  }
  return Error();
}

// ---- quiz registry ----------------------------------------------------------------------------------------------------------------
int64_t ShardedEngine::StartQuiz(Error &err) {
  CallScope scope(_activeCallers);
  Op op(OpKind::StartQuiz);
  RunOrPost(op);
  err = op.err;
  return op.result;
}

Error ShardedEngine::ReleaseQuiz(int64_t iQuiz) {
  CallScope scope(_activeCallers);
  Op op(OpKind::ReleaseQuiz);
  op.iQuiz = iQuiz;
  RunOrPost(op);
  return op.err;
}

int64_t ShardedEngine::ResumeQuiz(Error &err, int64_t nAnswered, const AQ *pAQs) {
  if (nAnswered < 0) { err = Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nAnswered), "|nAnswered| must be non-negative."); return -1; }
  if (nAnswered == 0) return StartQuiz(err);   // BaseEngine.cpp:393-395
  if (pAQs == nullptr) { err = Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of answered questions."); return -1; }
  CallScope scope(_activeCallers);
  std::lock_guard<OpLock> lk(_opMu);
  err = FlushAnswers();
  if (!err.ok()) return -1;
  ResumeRows r;
  err = ResolveRows(nAnswered, pAQs, r, nullptr);
  if (!err.ok()) return -1;
  int64_t id = -1;
  for (size_t s = 0; s < _sh.size(); s++) {
    bool allInPlace = true;
    err = StageFor(s, r, &allInPlace);
    if (!err.ok()) { ReleaseEverywhere(id, s); return -1; }
    const int64_t got = _sh[s]->ResumeQuizRows(err, nAnswered, pAQs, r.rows.data(), allInPlace ? nullptr : r.rowDev.data(), allInPlace ? nullptr : r.stage.data());
    if (got < 0) { ReleaseEverywhere(id, s); return -1; }   // (e.g. out of memory on shard s: the earlier shards' quiz goes again)
    if (s == 0) id = got;
    else if (got != id) {
      (void)_sh[s]->ReleaseQuiz(got);
      ReleaseEverywhere(id, s);
      err = Error::Make(ErrCode::Internal, "The shards' quiz registries have diverged.");
      return -1;
    }
    // (ResumeQuiz synchronises the shard's stream: its reads of the other shards' rows are done when it returns)
  }
  NewQuiz(id);
  return id;
}

Error ShardedEngine::ResolveRows(int64_t total, const AQ *pAQs, ResumeRows &r, int64_t *iBad) {
  r.rows.resize(2 * (size_t)total);
  r.rowDev.resize(2 * (size_t)total);
  r.owners.resize((size_t)total);
  for (int64_t i = 0; i < total; i++) {
    if (iBad) *iBad = i;
    const int owner = OwnerOf(pAQs[i].iQuestion);
    if (owner < 0) return Error::MakeP(ErrCode::IndexOutOfRange, "subjIndex=" + std::to_string(pAQs[i].iQuestion), "Question index is not in KB range.");
    Error e = _sh[(size_t)owner]->GetRowPointers(pAQs[i].iQuestion, pAQs[i].iAnswer, &r.rows[2 * (size_t)i], &r.rows[2 * (size_t)i + 1]);
    if (!e.ok()) return e;
    r.owners[(size_t)i] = owner;
    r.rowDev[2 * (size_t)i] = r.rowDev[2 * (size_t)i + 1] = _sh[(size_t)owner]->Device();
  }
  return Error();
}

Error ShardedEngine::StageFor(size_t s, ResumeRows &r, bool *allInPlace) {
  r.stage.assign(2 * r.owners.size(), 0);
  *allInPlace = true;
  for (size_t i = 0; i < r.owners.size(); i++) {
    const size_t o = (size_t)r.owners[i];
    if (o == s) continue;
    Error e = WaitForTraining(s, o);
    if (!e.ok()) return e;
    if (!InPlace(s, o)) {
      *allInPlace = false;
      r.stage[2 * i] = r.stage[2 * i + 1] = 1;
      _stagedRows.fetch_add(2, std::memory_order_relaxed);
    }
  }
  return Error();
}

// ResumeQuizBatch: the row pointers resolved as ResumeQuiz resolves them, then every shard one batch (HipEngine::ResumeQuizBatchRows:
// a launch sequence per chunk).  The shards assign the same ids; all or none across the shards.
Error ShardedEngine::ResumeQuizBatch(int64_t n, const int64_t *pCounts, const AQ *pAQs, int64_t *pQuizzes) {
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "|nQuizzes| must be non-negative.");
  if (n > 0 && (!pCounts || !pQuizzes)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  int64_t total = 0;
  for (int64_t i = 0; i < n; i++) {
    if (pCounts[i] < 0)
      return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(pCounts[i]),
                          "Batch entry " + std::to_string(i) + ": |nAnswered| must be non-negative.");
    total += pCounts[i];
  }
  if (total > 0 && pAQs == nullptr) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of answered questions.");
  for (int64_t i = 0; i < n; i++) pQuizzes[i] = -1;
  if (n == 0) return Error();
  CallScope scope(_activeCallers);
  std::lock_guard<OpLock> lk(_opMu);
  Error err = FlushAnswers();
  if (!err.ok()) return err;
  ResumeRows r;
  int64_t iBad = 0;
  err = ResolveRows(total, pAQs, r, &iBad);
  if (!err.ok()) {
    int64_t entry = 0;   // (the quiz whose answered question was refused)
    for (int64_t end = pCounts[0]; end <= iBad; end += pCounts[entry]) entry++;
    err.message = "Batch entry " + std::to_string(entry) + ": " + err.message;
    return err;
  }
  std::vector<int64_t> ids((size_t)n);
  auto releaseAll = [&](size_t nShards) { for (int64_t i = 0; i < n; i++) if (pQuizzes[i] >= 0) ReleaseEverywhere(pQuizzes[i], nShards); };
  for (size_t s = 0; s < _sh.size(); s++) {
    bool allInPlace = true;
    err = StageFor(s, r, &allInPlace);
    if (!err.ok()) { releaseAll(s); return err; }
    err = _sh[s]->ResumeQuizBatchRows(n, pCounts, pAQs, r.rows.data(), allInPlace ? nullptr : r.rowDev.data(), allInPlace ? nullptr : r.stage.data(),
                                      s == 0 ? pQuizzes : ids.data());
    if (!err.ok()) { releaseAll(s); for (int64_t i = 0; i < n; i++) pQuizzes[i] = -1; return err; }
    if (s > 0 && !std::equal(ids.begin(), ids.end(), pQuizzes)) {
      for (int64_t i = 0; i < n; i++) (void)_sh[s]->ReleaseQuiz(ids[(size_t)i]);
      releaseAll(s);
      for (int64_t i = 0; i < n; i++) pQuizzes[i] = -1;
      return Error::Make(ErrCode::Internal, "The shards' quiz registries have diverged.");
    }
    // (every chunk of the batch synchronised the shard's stream: its reads of the other shards' rows are done)
  }
  for (int64_t i = 0; i < n; i++) NewQuiz(pQuizzes[i]);
  return Error();
}

// ClearOldQuizzes (behaviour: BaseEngine.cpp:814-873), decided once for all shards by the rule the one-device engine uses
// (QuizzesToLetGo, hip_engine_kb.cpp) over the usage times kept here.
Error ShardedEngine::ClearOldQuizzes(int64_t maxCount, double maxAgeSec) {
  if (maxCount < 0)
    return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(maxCount), "The number of quizzes to keep cannot be less than 0.");
  std::lock_guard<OpLock> lk(_opMu);
  if (!_sh[0]->IsRegularMode()) return Error();   // quizzes are not expected to exist in maintenance / shutdown mode
  Error first = FlushAnswers();
  std::vector<QuizUsage> inUse;
  for (int64_t id = 0; id < _registrySize.load(); id++)
    if (QuizRow *r = LiveRow(id)) inUse.push_back(QuizUsage{id, (time_t)r->lastUse.load()});   // (registry order)
  for (int64_t id : QuizzesToLetGo(inUse, time(nullptr), maxCount, maxAgeSec)) {
    if (QuizRow *r = Row(id)) r->Clear();
    for (auto &s : _sh) { Error e = s->ReleaseQuiz(id); if (!e.ok() && first.ok()) first = e; }
  }
  return first;
}

// ---- active question, answers, listings -----------------------------------------------------------------------------------------
ShardedEngine::QuizRow *ShardedEngine::UseQuiz(Error &err, int64_t iQuiz) {   // BaseEngine::UseQuiz: the quiz's row, its last use now
  QuizRow *r = _sh[0]->IsRegularMode() ? LiveRow(iQuiz) : nullptr;
  err = r ? Error() : QuizError(iQuiz);
  if (!r && err.ok() && !(r = LiveRow(iQuiz))) err = Error::Make(ErrCode::Internal, "The quiz tables have diverged.");
  if (r) r->lastUse.store(NowStamp(), std::memory_order_relaxed);
  return r;
}

int64_t ShardedEngine::GetActiveQuestionId(Error &err, int64_t iQuiz) {
  QuizRow *r = UseQuiz(err, iQuiz);
  return r ? r->active.load(std::memory_order_relaxed) : -1;
}

Error ShardedEngine::SetActiveQuestion(int64_t iQuiz, int64_t iQuestion) {
  Error err;
  if (QuizRow *r = UseQuiz(err, iQuiz)) r->active.store(iQuestion, std::memory_order_relaxed);   // unchecked, as reference PqaCore/BaseEngine.cpp:507-508
  return err;
}

// Everything NextQuestion does after the pick (CpuEngine.cpp:403-413): the question becomes the quiz's active question, the
// asked-questions counter moves once.
int64_t ShardedEngine::Commit(Error &err, int64_t iQuiz, int64_t qGlobal) {
  if (qGlobal < 0) { err = Error::Make(ErrCode::QuestionsExhausted, "Found no unasked question that is not in a gap."); return -1; }
  QuizRow *r = LiveRow(iQuiz);
  if (!r) { err = QuizError(iQuiz); return -1; }
  r->active.store(qGlobal, std::memory_order_relaxed);
  _sh[0]->BumpQuestionsAsked(1);
  err = Error();
  return qGlobal;
}

// RecordAnswer (BaseEngine.cpp:441-466, CEQuiz::RecordAnswer PqaCore/CEQuiz.h:77-122): validated and recorded here; the shards
// get it -- with everything else that has gathered -- before the next thing that reads a posterior.
Error ShardedEngine::RecordAnswerDeferred(int64_t iQuiz, int64_t iAnswer) {
  if (!_sh[0]->IsRegularMode()) return QuizError(iQuiz);
  if (iAnswer < 0 || iAnswer >= _K)  // reference PqaCore/BaseEngine.cpp:447-451
    return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(iAnswer, 0, _K - 1), "Answer index is not in the answer range.");
  QuizRow *r = LiveRow(iQuiz);
  if (!r) { Error e = QuizError(iQuiz); return e.ok() ? Error::Make(ErrCode::Internal, "The quiz tables have diverged.") : e; }
  { Error fe = FailedQuiz(iQuiz); if (!fe.ok()) return fe; }
  r->lastUse.store(NowStamp(), std::memory_order_relaxed);
  const int64_t aq = r->active.load(std::memory_order_relaxed);
  if (aq == -1)
    return Error::MakeP(ErrCode::NoQuizActiveQuestion, "answerId=" + std::to_string(iAnswer),
                        "An attempt to record an answer in a quiz that doesn't have an active question");
  if (aq < 0 || aq >= _Q || _qGapBit[(size_t)aq])
    return Error::MakeP(ErrCode::NoQuizActiveQuestion, "answerId=" + std::to_string(iAnswer),
                        "An attempt to record an answer in a quiz that has invalid active question");
  if (r->pending.load(std::memory_order_acquire)) {   // (a second answer of a quiz whose first is still among the gathered ones)
    Error e = FlushNow();
    if (!e.ok()) return e;
  }
  r->active.store(-1, std::memory_order_relaxed);
  r->pending.store(1, std::memory_order_release);
  {
    std::lock_guard<std::mutex> lk(_pendMu);
    _pending.push_back(PendingAnswer{iQuiz, aq, iAnswer});
    _pendingCount.store(_pending.size(), std::memory_order_release);
  }
  return Error();
}

Error ShardedEngine::RecordAnswer(int64_t iQuiz, int64_t iAnswer) {
  CallScope scope(_activeCallers);
  Error e = RecordAnswerDeferred(iQuiz, iAnswer);
  if (!e.ok()) return e;
  // Alone in the engine: the shards' kernels start now, under whatever the client does next.  Other clients inside: the answer
  // waits for the next call that needs a posterior -- which hands over all that have gathered by then, in one launch per shard.
  return Concurrent() ? Error() : FlushNow();
}

Error ShardedEngine::RecordAnswerPageBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const AQ *pAQs, double *pLikelihood) {
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "|nQuizzes| must be non-negative.");
  if (n > 0 && (!pQuizzes || !pCounts)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  int64_t total = 0, longest = 0;
  for (int64_t i = 0; i < n; i++) {
    if (pCounts[i] < 0)
      return Error::MakeP(ErrCode::NegativeCount, "entry=" + std::to_string(i) + " count=" + std::to_string(pCounts[i]), "A page's number of answers must be non-negative.");
    total += pCounts[i];
    longest = std::max(longest, pCounts[i]);
  }
  if (total > 0 && pAQs == nullptr) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of answered questions.");
  if (pLikelihood != nullptr) return NotSharded("RecordAnswerPageBatch with likelihoods");
  CallScope scope(_activeCallers);
  if (!_sh[0]->IsRegularMode()) return QuizError(n > 0 ? pQuizzes[0] : -1);
  for (int64_t i = 0; i < n; i++)
    if (pCounts[i] > kRecordPageMax)
      return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(i) + " " + RangeParams(pCounts[i], 0, kRecordPageMax), "A page holds at most 4096 answers.");
  for (int64_t i = 0; i < n; i++) {
    Error e = LiveRow(pQuizzes[i]) ? FailedQuiz(pQuizzes[i]) : QuizError(pQuizzes[i]);
    if (e.ok() && !LiveRow(pQuizzes[i])) e = Error::Make(ErrCode::Internal, "The quiz tables have diverged.");
    if (!e.ok()) {
      e.params = "entry=" + std::to_string(i) + " quizId=" + std::to_string(pQuizzes[i]) + (e.hasParams ? " " + e.params : std::string());
      e.hasParams = true;
      return e;
    }
  }
  {
    std::unordered_set<int64_t> seen;
    for (int64_t i = 0; i < n; i++)
      if (!seen.insert(pQuizzes[i]).second)
        return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(i) + " quizId=" + std::to_string(pQuizzes[i]), "A quiz appears twice in the call.");
  }
  for (int64_t i = 0, at = 0; i < n; i++)
    for (int64_t j = 0; j < pCounts[i]; j++, at++) {
      const int64_t id = pAQs[at].iQuestion;
      const std::string where = "entry=" + std::to_string(i) + " position=" + std::to_string(j) + " questionId=" + std::to_string(id);
      if (id < 0 || id >= _Q) return Error::MakeP(ErrCode::IndexOutOfRange, where + " " + RangeParams(id, 0, _Q - 1), "A page's question is out of range.");
      if (_qGapBit[(size_t)id]) return Error::MakeP(ErrCode::IndexOutOfRange, where, "A page's question is a gap.");
    }
  for (int64_t i = 0, at = 0; i < n; i++)
    for (int64_t j = 0; j < pCounts[i]; j++, at++)
      if (pAQs[at].iAnswer < 0 || pAQs[at].iAnswer >= _K)
        return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(i) + " position=" + std::to_string(j) + " " + RangeParams(pAQs[at].iAnswer, 0, _K - 1),
                            "Answer index is not in the answer range.");
  for (int64_t p = 0; p < longest; p++) {
    for (int64_t i = 0, at = 0; i < n; at += pCounts[i], i++) {
      if (pCounts[i] <= p) continue;
      QuizRow *r = LiveRow(pQuizzes[i]);
      if (!r) return QuizError(pQuizzes[i]);
      r->active.store(pAQs[at + p].iQuestion, std::memory_order_relaxed);
      Error e = RecordAnswerDeferred(pQuizzes[i], pAQs[at + p].iAnswer);
      if (!e.ok()) return e;
    }
    Error e = FlushNow();
    if (!e.ok()) return e;
  }
  return Error();
}

Error ShardedEngine::FlushAnswers() {
  std::vector<PendingAnswer> taken;
  {
    std::lock_guard<std::mutex> lk(_pendMu);
    taken.swap(_pending);
    _pendingCount.store(0, std::memory_order_release);
  }
  if (taken.empty()) return Error();
  const size_t N = _sh.size();
  _answerFlushes.fetch_add(1, std::memory_order_relaxed);
  _answersFlushed.fetch_add(taken.size(), std::memory_order_relaxed);
  _answersSinceSweep.fetch_add((int64_t)taken.size(), std::memory_order_relaxed);
  if (taken.size() > _answerMaxFlush.load(std::memory_order_relaxed)) _answerMaxFlush.store(taken.size(), std::memory_order_relaxed);
  std::vector<HipEngine::ShardAnswer> forShard(taken.size());
  Error first;
  for (size_t s = 0; s < N; s++) {
    for (size_t i = 0; i < taken.size(); i++) {
      const PendingAnswer &p = taken[i];
      const int owner = OwnerOf(p.qGlobal);
      HipEngine::ShardAnswer &a = forShard[i];
      a = HipEngine::ShardAnswer{p.iQuiz, p.qGlobal, p.iAnswer, nullptr, nullptr, -1, false, (size_t)(p.iQuiz % (int64_t)N) == s};
      if ((size_t)owner == s) continue;
      HipEngine &o = *_sh[(size_t)owner];
      a.rowA = o.RowPointer(p.qGlobal - o.FirstQuestion(), p.iAnswer);
      a.rowD = o.RowPointer(p.qGlobal - o.FirstQuestion(), _K);
      a.srcDevice = o.Device();
      a.stage = !InPlace(s, (size_t)owner);
      if (a.stage) _stagedRows.fetch_add(2, std::memory_order_relaxed);
      Error we = WaitForTraining(s, (size_t)owner);
      if (!we.ok() && first.ok()) first = we;
      _remoteReads[s] = 1;
    }
    Error e = _sh[s]->ApplyAnswers((int64_t)forShard.size(), forShard.data());
    if (!e.ok() && first.ok()) first = e;
  }
  // (a failure on any shard: which of the batch's answers that shard still applied is not known here -- every quiz of the batch is
  //  marked, and says so from now on)
  for (const PendingAnswer &p : taken)
    if (QuizRow *r = Row(p.iQuiz)) {
      if (!first.ok()) r->failed.store(1, std::memory_order_release);
      r->pending.store(0, std::memory_order_release);
    }
  return first;
}

int64_t ShardedEngine::ListTopTargets(Error &err, int64_t iQuiz, int64_t maxCount, CiRatedTarget *pDest) {
  CallScope scope(_activeCallers);
  QuizRow *r = LiveRow(iQuiz);
  if (r && r->pending.load(std::memory_order_acquire)) {
    // Group commit.  This quiz's answer is among the gathered ones, and the clients that got their questions from the same combined
    // sweep are recording theirs right now: a moment for them, so that ONE hand-over carries all of them.
    if (_optLingerUs > 0 && Concurrent()) {
      const size_t target = (size_t)std::max<int64_t>(2, std::min<int64_t>(_lastCombined.load(std::memory_order_relaxed), _activeCallers.load(std::memory_order_relaxed) - 1));
      const auto t0 = std::chrono::steady_clock::now();
      const auto limit = std::chrono::microseconds(_optLingerUs);
      for (;;) {
        const size_t have = _pendingCount.load(std::memory_order_relaxed);
        if (have == 0 || have >= target) break;   // (0: somebody has handed them over)
        for (int i = 0; i < 32; i++) _mm_pause();
        if (std::chrono::steady_clock::now() - t0 > limit) break;
      }
    }
    err = FlushNow();
    if (!err.ok()) return -1;
  }
  if (r) r->lastUse.store(NowStamp(), std::memory_order_relaxed);
  // (the shard whose kernel listed the new posterior's best targets with the update: FlushAnswers)
  return _sh[(size_t)(iQuiz >= 0 ? iQuiz % (int64_t)_sh.size() : 0)]->ListTopTargets(err, iQuiz, maxCount, pDest);
}

// ---- training -------------------------------------------------------------------------------------------------------------------
Error ShardedEngine::Train(int64_t n, const AQ *pAQs, int64_t iTarget, double amount) {
  std::lock_guard<OpLock> lk(_opMu);
  const bool checkable = n >= 0 && amount > 0 && (n == 0 || pAQs != nullptr);   // (else: shard 0 produces the reference's argument error, before any kernel)
  return TrainOnAllShards([&](HipEngine &sh) { return checkable ? sh.ValidateTrain(n, pAQs, iTarget, -1) : Error(); },
                          [&](HipEngine &sh) { return sh.Train(n, pAQs, iTarget, amount); });
}

// TrainBatch / RecordQuizTargetBatch: what Train does, once for the whole batch.
Error ShardedEngine::TrainBatch(int64_t n, const int64_t *pCounts, const AQ *pAQs, const int64_t *pTargets, const double *pAmounts) {
  Error e = HipEngine::CheckTrainBatchArgs(n, pCounts, pAQs, pTargets, pAmounts);
  if (!e.ok() || n == 0) return e;
  CallScope scope(_activeCallers);
  std::lock_guard<OpLock> lk(_opMu);
  return TrainOnAllShards([&](HipEngine &sh) { return sh.ValidateTrainBatch(n, pCounts, pAQs, pTargets, nullptr); },
                          [&](HipEngine &sh) { return sh.TrainBatch(n, pCounts, pAQs, pTargets, pAmounts); });
}

Error ShardedEngine::RecordQuizTargetBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pTargets, const double *pAmounts) {
  Error e = HipEngine::CheckQuizTargetBatchArgs(n, pQuizzes, pTargets, pAmounts);
  if (!e.ok() || n == 0) return e;
  CallScope scope(_activeCallers);
  std::lock_guard<OpLock> lk(_opMu);
  return TrainOnAllShards([&](HipEngine &sh) { return sh.ValidateTrainBatch(n, nullptr, nullptr, pTargets, pQuizzes); },
                          [&](HipEngine &sh) {
                            if (&sh == _sh[0].get()) for (int64_t i = 0; i < n; i++) Touch(pQuizzes[i]);
                            return sh.RecordQuizTargetBatch(n, pQuizzes, pTargets, pAmounts);
                          });
}

Error ShardedEngine::RecordQuizTarget(int64_t iQuiz, int64_t iTarget, double amount) {
  CallScope scope(_activeCallers);
  Op op(OpKind::RecordQuizTarget);
  op.iQuiz = iQuiz; op.iTarget = iTarget; op.amount = amount;
  RunOrPost(op);
  return op.err;
}

// ---- one NextQuestion by itself (_opMu held through the wait: nobody else is asking) ------------------------------------------------
int64_t ShardedEngine::SelectArgmaxLocked(Error &err, int64_t iQuiz, double *pPriority) {
  if (++_step == 0) ++_step;
  const uint64_t step = _step;
  for (size_t s = 0; s < _sh.size(); s++) {
    // the slots are mapped + portable: their host address is what every device sees
    err = _sh[s]->EnqueueSelectArgmaxFlag(iQuiz, &_slots[s].priority, &_slots[s].flag, step);
    if (!err.ok()) return -1;
  }
  Touch(iQuiz);
  SpinWait w;
  for (size_t s = 0; s < _sh.size(); s++) {
    volatile uint64_t *flag = &_slots[s].flag;
    while (*flag != step)
      if (!w.Tick(std::chrono::seconds(60))) {
        err = Error::MakeP(ErrCode::Internal, "shard=" + std::to_string(s), "Timed out waiting for a shard's selection.");
        return -1;
      }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  BestPick best;   // (kb_plan.h: maximum priority, lowest index on ties)
  for (size_t s = 0; s < _sh.size(); s++) {
    if (_slots[s].index == kSelIncomplete) { err = Error::Make(ErrCode::Internal, "A shard's sweep did not complete."); return -1; }
    best.Offer(_slots[s].priority, _slots[s].index);
  }
  CheckPriority(best.priority, best.index);   // (the reference's "Got priority=" warning, for the question that was selected)
  if (pPriority) *pPriority = best.priority;
  err = Error();
  return best.index;
}

// The reference's selector (PqaCore/CpuEngine.cpp:362-400) over the GLOBAL question range: the same per-subtask Kahan run
// lengths, grand totals and upper_bounds as select_sampled_wg_impl (pqa_device.h) runs on one device, here on the host over the
// shards' priority vectors -- with the same priorities, subtask count and random number it picks the question an unsharded
// engine picks.
int64_t ShardedEngine::SelectSampledLocked(Error &err, int64_t iQuiz, uint64_t rnd) {
  Touch(iQuiz);
  for (auto &s : _sh) { err = s->EnqueueEval(iQuiz); if (!err.ok()) return -1; }
  for (auto &s : _sh) {
    hipSetDevice(s->Device());
    if (hipMemcpyAsync(_hostPriority.data() + s->FirstQuestion(), s->PriorityDevicePtr(), (size_t)s->LocalQuestions() * sizeof(double),
                       hipMemcpyDeviceToHost, s->GetStream()) != hipSuccess) { err = Error::Make(ErrCode::Internal, "Copy of a shard's priorities failed."); return -1; }
  }
  for (auto &s : _sh) {
    hipSetDevice(s->Device());
    if (hipStreamSynchronize(s->GetStream()) != hipSuccess) { err = Error::Make(ErrCode::Internal, "A shard's sweep failed."); return -1; }
  }
  std::vector<uint64_t> skip;
  std::vector<uint32_t> words;
  if (!GlobalSkip([&](size_t s) { err = _sh[s]->UnavailableWords(iQuiz, words); return err.ok() ? words.data() : nullptr; }, skip)) return -1;
  const int64_t sel = SelectSampledHost(_hostPriority.data(), _Q, _sh[0]->GetOption("eval_subtasks"), rnd, [&](int64_t q) { return Skipped(skip, q); });
  return Commit(err, iQuiz, NearestFree(skip, sel, _Q));
}

int64_t ShardedEngine::NextQuestion(Error &err, int64_t iQuiz) {
  if (_select == 1) return Combine(err, iQuiz, SelKind::Argmax, 0);
  uint64_t rnd;
  { std::lock_guard<std::mutex> lk(_rngMu); rnd = _rng.Next(); }   // (drawn when the call arrives, whatever sweep serves it)
  return Combine(err, iQuiz, SelKind::Sampled, rnd);
}

// ---- concurrent NextQuestion calls ------------------------------------------------------------------------------------------------
// A caller posts its request; if a leader is at work it waits for its result, otherwise it becomes the leader: it takes everything
// posted so far -- distinct quizzes -- launches ONE batched sweep per shard for it (every shard's on its own device and stream, all
// in flight before the first is waited for), hands the lead to the oldest request still waiting as soon as the sweeps are
// launched, and then waits for its own.  Two batch contexts alternate, so that the next leader launches while this one's sweeps
// run.  One request alone takes the single-quiz path (the shards' fused argmax through the pinned slots).
int64_t ShardedEngine::Combine(Error &err, int64_t iQuiz, SelKind kind, uint64_t rnd) {
  CallScope scope(_activeCallers);
  SelRequest r;
  r.iQuiz = iQuiz; r.kind = kind; r.rnd = rnd;
  if (!_optCombine) {
    std::lock_guard<OpLock> lk(_opMu);
    err = FlushAnswers();
    if (!err.ok()) return -1;
    ServeAlone(&r);
    err = r.err;
    return r.result;
  }
  int st = _comb.Wait(r);
  if (st == kReqLead) {   // (the lead: nobody else led, or the leader before launched its batch and handed the lead to this, the oldest request)
    if (_optLingerUs > 0 && Concurrent()) _comb.Linger(_optLingerUs, _answersSinceSweep.load(std::memory_order_relaxed), _activeCallers);
    Flight f;
    st = _comb.Lead(
        r, 256, [this](int64_t m) { return _sh[0]->CombinedBatchFor(m); },
        [&](CombineCtx &c, std::vector<SelRequest *> &batch, std::chrono::steady_clock::time_point) {
          LaunchBatch((int)(&c - _bctx), batch, f);   // (under _opMu; what could not be launched has its error -- or its result, for a batch of one)
        },
        [&](CombineCtx &c, std::vector<SelRequest *> &batch) { return !f.live.empty() && CollectBatch((int)(&c - _bctx), batch, f, &r); });
  }
  if (st == kReqSelect) {   // the sweeps have run: this quiz's priorities are on the host, the selection is this thread's own work
    SelectFromViews(&r);
    r.ctx->readers.fetch_sub(1, std::memory_order_release);
  }
  err = r.err;
  return r.result;
}

void ShardedEngine::LaunchBatch(int ctx, std::vector<SelRequest *> &batch, Flight &f) {
  Op op(OpKind::LaunchBatch);
  op.ctx = ctx; op.batch = &batch; op.flight = &f;
  RunOrPost(op);
}

void ShardedEngine::LaunchBatchLocked(int ctx, std::vector<SelRequest *> &batch, Flight &f) {
  _answersSinceSweep.store(0, std::memory_order_relaxed);
  std::vector<SelRequest *> live;
  std::vector<int64_t> ids;
  const bool regular = _sh[0]->IsRegularMode();
  for (SelRequest *r : batch) {
    if (!regular || LiveRow(r->iQuiz) == nullptr) { r->err = QuizError(r->iQuiz); r->result = -1; if (r->err.ok()) r->err = Error::Make(ErrCode::Internal, "The quiz tables have diverged."); continue; }
    { Error fe = FailedQuiz(r->iQuiz); if (!fe.ok()) { r->err = fe; r->result = -1; continue; } }
    live.push_back(r);
    ids.push_back(r->iQuiz);
    f.anySampled = f.anySampled || r->kind == SelKind::Sampled;
  }
  if (live.empty()) return;
  if (live.size() == 1) { ServeAlone(live[0]); return; }
  const int64_t n = (int64_t)live.size();
  const size_t N = _sh.size();
  f.shard.assign(N, HipEngine::CombinedFlight());
  f.unavailable.assign(N, std::vector<uint32_t>());
  Error err;
  _shardsInFlightMax = 0;
  for (size_t s = 0; s < N && err.ok(); s++) {
    err = _sh[s]->EnqueueCombined(ctx, n, ids.data(), f.anySampled, &f.shard[s], f.anySampled ? &f.unavailable[s] : nullptr);
    if (err.ok()) _shardsInFlightMax++;
  }
  if (!err.ok()) {
    // (a shard refused the batch -- e.g. a quiz released under its own NextQuestion, the caller's error: every request by itself;
    //  the sweeps already launched run to their end unread)
    for (size_t s = 0; s < N; s++) if (f.shard[s].n > 0) (void)_sh[s]->CollectCombined(ctx, f.shard[s], nullptr, nullptr);
    for (SelRequest *r : live) ServeAlone(r);
    return;
  }
  for (SelRequest *r : live) Touch(r->iQuiz);
  _combBatches.fetch_add(1, std::memory_order_relaxed);
  _combRequests.fetch_add((uint64_t)n, std::memory_order_relaxed);
  if ((uint64_t)n > _combMaxBatch.load(std::memory_order_relaxed)) _combMaxBatch.store((uint64_t)n, std::memory_order_relaxed);
  _lastCombined.store(n, std::memory_order_relaxed);
  _bctx[ctx].inFlight.store(true, std::memory_order_relaxed);
  f.live.swap(live);
}

// Wait for every shard's sweep and hand the results out -- the engine open to the other clients' calls meanwhile.  Returns true if
// `own` is to select for itself.
bool ShardedEngine::CollectBatch(int ctx, std::vector<SelRequest *> &batch, Flight &f, SelRequest *own) {
  const int64_t n = (int64_t)f.live.size();
  const size_t N = _sh.size();
  CombineCtx &c = _bctx[ctx];
  std::vector<std::vector<CiHipSelection>> winners(N);
  std::vector<std::vector<PriorityView>> views(N);
  Error err;
  for (size_t s = 0; s < N; s++) {   // (every shard is waited for, whatever the others reported)
    winners[s].resize((size_t)n);
    views[s].resize((size_t)n);
    Error e = _sh[s]->CollectCombined(ctx, f.shard[s], winners[s].data(), views[s].data());
    if (!e.ok() && err.ok()) err = e;
  }
  c.inFlight.store(false, std::memory_order_relaxed);
  if (!err.ok()) {
    for (SelRequest *r : f.live) { r->err = err; r->result = -1; }
    return false;
  }
  if (f.anySampled) {
    // The priority vectors are on the host: every client selects for ITSELF (the O(Q) scalar Kahan steps of the reference's
    // selector run on as many cores as there are clients), the leader only for its own request.
    c.readers.fetch_add((int)n, std::memory_order_acq_rel);
    bool ownLive = false;
    for (int64_t i = 0; i < n; i++) {
      SelRequest *r = f.live[(size_t)i];
      r->views.resize(N);
      for (size_t s = 0; s < N; s++) r->views[s] = views[s][(size_t)i];
      GlobalSkip([&](size_t s) { return f.unavailable[s].data() + (size_t)i * _sh[s]->UnavailableWordCount(); }, r->skip);
      r->ctx = &c;
      if (r == own) { ownLive = true; continue; }
      Combiner<SelRequest, CombineCtx>::LetSelect(batch, r);
    }
    return ownLive;
  }
  // the kernels' choices: per quiz the best of the shards' winners
  for (int64_t i = 0; i < n; i++) {
    SelRequest *r = f.live[(size_t)i];
    BestPick best;
    for (size_t s = 0; s < N; s++) best.Offer(winners[s][(size_t)i]._priority, winners[s][(size_t)i]._iQuestion);
    r->result = Commit(r->err, r->iQuiz, best.index);
  }
  return false;
}

// One request of a combined sweep, after the sweeps: this quiz's priority vector out of the shards' host buffers into global order,
// then the selector (the reference's: SelectSampledHost; the argmax by the device's rule) and NextQuestion's bookkeeping -- on the
// client's own thread, no lock.
int64_t ShardedEngine::SelectFromViews(SelRequest *r) {
  const int64_t nQ = _Q;
  auto skipped = [&](int64_t q) { return Skipped(r->skip, q); };
  std::vector<double> run((size_t)nQ);
  for (size_t s = 0; s < _sh.size(); s++) {
    const int64_t q0 = _sh[s]->FirstQuestion();
    if (!TakePriorities(r->views[s], _sh[s]->LocalQuestions(), [&](int64_t k) { return skipped(q0 + k); }, run.data() + q0, std::chrono::seconds(30))) {
      r->err = Error::Make(ErrCode::Internal, "Timed out waiting for a shard's priority vector.");
      return r->result = -1;
    }
  }
  int64_t pick = -1;
  if (r->kind == SelKind::Sampled) {
    pick = SelectSampledHost(run.data(), nQ, _sh[0]->GetOption("eval_subtasks"), r->rnd, skipped);
  } else {
    BestPick best;
    for (int64_t q = 0; q < nQ; q++) if (!skipped(q)) best.Offer(run[(size_t)q], q);
    pick = best.index;
    if (pick >= 0) CheckPriority(run[(size_t)pick], pick);
  }
  return r->result = Commit(r->err, r->iQuiz, NearestFree(r->skip, pick, nQ));
}

// ---- the batch calls of the ABI -------------------------------------------------------------------------------------------------
// Every shard's batched sweep is enqueued -- on its own device and stream -- before the first one is waited for: on N devices a
// batch takes one shard's time, not N shards' (SRPoolRunner's subtasks run side by side too, SRPlatform/Interface/SRPoolRunner.h:96-110).
Error ShardedEngine::EnqueueBatchOnShards(int64_t n, const int64_t *pQuizzes, bool wantPriorities, std::vector<uint64_t> &tags) {
  tags.assign(_sh.size(), 0);
  std::lock_guard<OpLock> lk(_opMu);
  Error e = FlushAnswers();
  _shardsInFlightMax = 0;
  for (size_t s = 0; e.ok() && s < _sh.size(); s++) {
    e = _sh[s]->EnqueueBatch(n, pQuizzes, wantPriorities, &tags[s]);   // (validation fails on shard 0, before anything was launched)
    if (e.ok()) _shardsInFlightMax++;
  }
  for (int64_t i = 0; e.ok() && i < n && pQuizzes; i++) Touch(pQuizzes[i]);
  return e;
}

Error ShardedEngine::SelectArgmaxBatch(int64_t n, const int64_t *pQuizzes, CiHipSelection *pOut) {
  if (n > 0 && !pOut) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  std::lock_guard<std::mutex> ctxLock(_bctx[0].mu);   // (the shards' batch context 0: not while a combined sweep uses it)
  while (_bctx[0].readers.load(std::memory_order_acquire) != 0) _mm_pause();
  std::vector<uint64_t> tags;
  Error first = EnqueueBatchOnShards(n, pQuizzes, false, tags);
  if (!first.ok()) return first;
  std::vector<CiHipSelection> part((size_t)n);
  for (size_t s = 0; s < _sh.size(); s++) {
    Error e = _sh[s]->CollectBatchSelections(n, tags[s], part.data());
    if (!e.ok()) { if (first.ok()) first = e; continue; }   // (the other shards' launches are still waited for)
    for (int64_t i = 0; i < n; i++) {
      const CiHipSelection &c = part[(size_t)i];
      CiHipSelection &b = pOut[i];
      if (s == 0) { b = c; continue; }
      if (BetterPick(b._priority, b._iQuestion, c._priority, c._iQuestion)) b = c;
    }
  }
  return first;
}

Error ShardedEngine::NextQuestionArgmaxBatch(int64_t n, const int64_t *pQuizzes, int64_t *pOut) {
  if (n < 0 || n > 256) return Error::MakeP(ErrCode::IndexOutOfRange, "n=" + std::to_string(n), "Batch size is out of range.");
  if (n == 0) return Error();
  if (!pQuizzes || !pOut) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  std::vector<CiHipSelection> best((size_t)n);
  Error e = SelectArgmaxBatch(n, pQuizzes, best.data());
  if (!e.ok()) return e;
  for (int64_t i = 0; i < n; i++) {
    Error ce;
    pOut[i] = Commit(ce, pQuizzes[i], best[(size_t)i]._iQuestion);   // -1 + QuestionsExhausted: reported as -1 only
  }
  return Error();
}

// NextQuestionSampledBatch: the subtask split of the reference's selector runs over the GLOBAL question axis, so no shard can select
// by itself.  One batched sweep per shard (all in flight together), the priority vectors gathered on the host, then per quiz what
// SelectSampledLocked does: SelectSampledHost over the global vector, the nearest free question for a pick that is asked or a gap,
// the active question set.  Every shard validates the batch before anything is launched or changed.
Error ShardedEngine::ValidateSelectionBatch(int64_t n, const int64_t *pQuizzes) {
  if (n < 0 || n > 256) return Error::MakeP(ErrCode::IndexOutOfRange, "n=" + std::to_string(n), "Batch size is out of range.");
  if (n == 0) return Error();
  if (!pQuizzes) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  for (auto &s : _sh) { Error e = s->ValidateBatch(n, pQuizzes); if (!e.ok()) return e; }
  for (int64_t i = 0; i < n; i++) { Error e = FailedQuiz(pQuizzes[i]); if (!e.ok()) return e; }
  return Error();
}

Error ShardedEngine::NextQuestionSampledBatch(int64_t n, const int64_t *pQuizzes, const uint64_t *pRnd, int64_t *pOut) {
  Error e = ValidateSelectionBatch(n, pQuizzes);
  if (!e.ok() || n == 0) return e;
  if (!pRnd || !pOut) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  std::vector<double> pri((size_t)n * (size_t)_Q);
  e = EvalPrioritiesBatch(n, pQuizzes, pri.data());   // (flushes the gathered answers, touches the quizzes)
  if (!e.ok()) return e;
  std::lock_guard<OpLock> lk(_opMu);
  const int64_t nSub = _sh[0]->GetOption("eval_subtasks");
  std::vector<uint64_t> skip;
  std::vector<uint32_t> words;
  std::vector<int64_t> picks((size_t)n, -1);
  for (int64_t i = 0; i < n; i++) {
    if (!GlobalSkip([&](size_t s) { e = _sh[s]->UnavailableWords(pQuizzes[i], words); return e.ok() ? words.data() : nullptr; }, skip))
      return e;   // (nothing has changed yet)
    const int64_t sel = SelectSampledHost(pri.data() + (size_t)i * (size_t)_Q, _Q, nSub, pRnd[i], [&](int64_t q) { return Skipped(skip, q); });
    picks[(size_t)i] = NearestFree(skip, sel, _Q);
  }
  for (int64_t i = 0; i < n; i++) {
    Error ce;
    pOut[i] = Commit(ce, pQuizzes[i], picks[(size_t)i]);   // -1 + QuestionsExhausted: reported as -1 only
  }
  return Error();
}

Error ShardedEngine::NextQuestionBatch(int64_t n, const int64_t *pQuizzes, int64_t *pOut) {
  if (_select == 1) return NextQuestionArgmaxBatch(n, pQuizzes, pOut);
  Error e = ValidateSelectionBatch(n, pQuizzes);   // (a refused call draws nothing)
  if (!e.ok() || n == 0) return e;
  if (!pOut) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  std::vector<uint64_t> rnd((size_t)n);
  {
    std::lock_guard<std::mutex> lk(_rngMu);   // one number per quiz in batch order, as consecutive NextQuestion calls draw them
    for (int64_t i = 0; i < n; i++) rnd[(size_t)i] = _rng.Next();
  }
  return NextQuestionSampledBatch(n, pQuizzes, rnd.data(), pOut);
}

Error ShardedEngine::EvalPrioritiesBatch(int64_t n, const int64_t *pQuizzes, double *pOut) {
  std::lock_guard<std::mutex> ctxLock(_bctx[0].mu);
  while (_bctx[0].readers.load(std::memory_order_acquire) != 0) _mm_pause();
  std::vector<uint64_t> tags;
  Error first = EnqueueBatchOnShards(n, pQuizzes, true, tags);
  if (!first.ok()) return first;
  std::vector<double> part;
  for (auto &s : _sh) {
    part.resize((size_t)n * (size_t)s->LocalQuestions());
    Error e = s->CollectBatchPriorities(n, part.data());
    if (!e.ok()) return e;
    for (int64_t i = 0; i < n; i++)
      std::memcpy(pOut + (size_t)i * (size_t)_Q + (size_t)s->FirstQuestion(), part.data() + (size_t)i * (size_t)s->LocalQuestions(),
                  (size_t)s->LocalQuestions() * sizeof(double));
  }
  return Error();
}

// ---- ListTopQuestions: every shard lists the best maxCount of ITS questions -- all shards' sweeps and listings in flight before the
// first is waited for -- and the host merges the shards' lists under the listings' own order (kb_plan.h: MergeTop).  The best maxCount
// of the whole question axis are among the shards' best maxCount each.
int64_t ShardedEngine::ListTopQuestions(Error &err, int64_t iQuiz, int64_t maxCount, CiRatedQuestion *pDest) {
  std::lock_guard<OpLock> lk(_opMu);
  err = FlushAnswers();   // (the gathered answers first: the sweeps read the posteriors they change)
  if (err.ok()) err = FailedQuiz(iQuiz);
  if (!err.ok()) return -1;
  size_t launched = 0;
  _shardsInFlightMax = 0;
  for (; err.ok() && launched < _sh.size(); launched++) {   // (validation fails on shard 0, before anything was launched)
    err = _sh[launched]->EnqueueTopQuestions(iQuiz, maxCount, pDest != nullptr);
    if (err.ok()) _shardsInFlightMax++;
  }
  if (err.ok()) Touch(iQuiz);
  std::vector<std::vector<RatedIndex>> part(_sh.size());
  std::vector<std::pair<const RatedIndex *, int64_t>> lists;
  for (size_t s = 0; s < launched; s++) {   // (what was launched is waited for, whatever the others reported)
    part[s].resize((size_t)std::max<int64_t>(0, std::min<int64_t>(maxCount, _sh[s]->LocalQuestions())));
    Error e;
    const int64_t c = _sh[s]->CollectTopQuestions(e, reinterpret_cast<CiRatedQuestion *>(part[s].data()));
    if (!e.ok() && err.ok()) err = e;
    lists.emplace_back(part[s].data(), std::max<int64_t>(c, 0));
  }
  if (!err.ok()) return -1;
  const std::vector<RatedIndex> best = MergeTop(lists, maxCount);
  if (!best.empty()) std::memcpy(pDest, best.data(), best.size() * sizeof(RatedIndex));
  return (int64_t)best.size();
}

Error ShardedEngine::ListTopQuestionsBatch(int64_t n, const int64_t *pQuizzes, int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) {
  Error first = HipEngine::CheckTopQuestionsBatchArgs(n, pQuizzes, maxCount, pDest != nullptr, pCounts != nullptr);
  if (!first.ok()) return first;
  std::lock_guard<std::mutex> ctxLock(_bctx[0].mu);   // (the shards' batch context 0: not while a combined sweep uses it)
  while (_bctx[0].readers.load(std::memory_order_acquire) != 0) _mm_pause();
  size_t launched = 0;
  {
    std::lock_guard<OpLock> lk(_opMu);
    first = FlushAnswers();
    for (auto &s : _sh) { if (first.ok()) first = s->ValidateBatch(n, pQuizzes); }   // (every shard, before anything is launched)
    for (int64_t i = 0; first.ok() && i < n; i++) first = FailedQuiz(pQuizzes[i]);
    _shardsInFlightMax = 0;
    for (; first.ok() && launched < _sh.size(); launched++) {
      first = _sh[launched]->EnqueueTopQuestionsBatch(n, pQuizzes, maxCount);
      if (first.ok()) _shardsInFlightMax++;
    }
    for (int64_t i = 0; first.ok() && i < n; i++) Touch(pQuizzes[i]);
  }
  std::vector<std::vector<RatedIndex>> part(_sh.size());
  std::vector<std::vector<int64_t>> counts(_sh.size(), std::vector<int64_t>((size_t)std::max<int64_t>(n, 0), 0));
  std::vector<int64_t> stride(_sh.size(), 0);
  for (size_t s = 0; s < launched; s++) {
    stride[s] = std::max<int64_t>(0, std::min<int64_t>(maxCount, _sh[s]->LocalQuestions()));
    part[s].resize((size_t)(n * stride[s]));
    Error e = _sh[s]->CollectTopQuestionsBatch(n, stride[s], reinterpret_cast<CiRatedQuestion *>(part[s].data()), counts[s].data());
    if (!e.ok() && first.ok()) first = e;
  }
  if (!first.ok()) return first;
  for (int64_t i = 0; i < n; i++) {
    std::vector<std::pair<const RatedIndex *, int64_t>> lists;
    for (size_t s = 0; s < _sh.size(); s++) lists.emplace_back(part[s].data() + i * stride[s], counts[s][(size_t)i]);
    const std::vector<RatedIndex> best = MergeTop(lists, maxCount);
    if (!best.empty()) std::memcpy(pDest + i * maxCount, best.data(), best.size() * sizeof(RatedIndex));
    pCounts[i] = (int64_t)best.size();
  }
  return Error();
}

// ---- maintenance ------------------------------------------------------------------------------------------------------------
Error ShardedEngine::RemoveQuestions(int64_t n, const int64_t *pQIds) {   // BaseEngine.cpp:722-743; all ids validated before the first is removed
  std::lock_guard<OpLock> lk(_opMu);
  Error e = _sh[0]->IsMaintenanceMode() ? Error() : WrongModeErr("remove questions");
  if (!e.ok()) return e;
  e = CheckRemoval(n, pQIds, _Q, [&](int64_t iq) { return _qGapBit[(size_t)iq] != 0; }, "Question index is not in KB.");
  if (!e.ok()) return e;
  for (auto &s : _sh) { e = s->SetQuestionGaps(n, pQIds); if (!e.ok()) return e; }
  for (int64_t i = 0; i < n; i++) { _qGapList.push_back(pQIds[i]); _questionIds.Vacate(pQIds[i]); }
  RefreshGapBits();
  return Error();
}

Error ShardedEngine::RemoveTargets(int64_t n, const int64_t *pTIds) {   // BaseEngine.cpp:745-765
  std::lock_guard<OpLock> lk(_opMu);
  Error e = _sh[0]->IsMaintenanceMode() ? Error() : WrongModeErr("remove targets");
  if (!e.ok()) return e;
  // (the target axis is replicated: every shard validates and removes the same ids; shard 0 refuses a bad call before any other is asked)
  for (auto &s : _sh) { e = s->RemoveTargets(n, pTIds); if (!e.ok()) return e; }
  return Error();
}

// New shards for new dimensions.  srcQ[q'] / srcT[t']: the old global question / target whose data new q' / t' takes, -1 for none
// (a gap, or an id that fillQ / fillT initialise).  The registries that are not data -- gaps, id maps, options, mode -- are
// carried over.  On failure nothing has changed.
Error ShardedEngine::Rebuild(int64_t newQ, int64_t newT, const std::vector<int64_t> &srcQ, const std::vector<int64_t> &srcT,
                             const std::vector<int64_t> &qGaps, const std::vector<int64_t> &tGaps, const IdLedger &targetIds,
                             const std::vector<int64_t> &fillT, const std::vector<double> &fillTInit, const std::vector<int64_t> &fillQ,
                             const std::vector<double> &fillQInit) {
  const int64_t N = (int64_t)_sh.size();
  if (!_peerAll)   // (adopt_rows_kernel reads the old shards' question blocks in place)
    return Error::MakeP(ErrCode::NotImplemented, "Feature=maintenance-mode edits of the dimensions without peer access between the devices",
                        "Rebuilding the shards reads the old shards' rows in place: every listed device must map the others' memory (PQA_DEVICES).");
  if (newQ < N) return Error::MakeP(ErrCode::InsufficientEngineDimensions, "[nQuestions=" + std::to_string(newQ) + " of " + std::to_string(N) + "]",
                                    "Fewer questions than devices in PQA_DEVICES.");
  HipEngine &s0 = *_sh[0];
  CiEngineDefinition def;
  std::memset(&def, 0, sizeof(def));
  def._nAnswers = _K; def._nTargets = newT;
  def._precType = s0.PrecisionType(); def._precMantissa = s0.PrecMantissa(); def._precExponent = s0.PrecExponent();
  def._initAmount = s0.InitAmount();
  Error err;
  for (auto &s : _sh) { err = s->Synchronize(); if (!err.ok()) return err; }
  std::vector<std::unique_ptr<HipEngine>> fresh;
  for (int64_t s = 0, next = 0; s < N; s++) {
    HipEngine *e = NewShard(err, def, s, N, newQ, _devices[(size_t)s], &next);
    if (!e) return err;
    fresh.emplace_back(e);
    const int64_t first = e->FirstQuestion(), nLocal = e->LocalQuestions();
    // its questions' rows, from wherever the old shards hold them
    std::vector<const void *> blocks((size_t)nLocal, nullptr);
    for (int64_t q = 0; q < nLocal; q++) {
      const int64_t old = srcQ[(size_t)(first + q)];
      if (old < 0) continue;
      const int owner = OwnerOf(old);
      blocks[(size_t)q] = _sh[(size_t)owner]->QuestionBlock(old - _sh[(size_t)owner]->FirstQuestion());
    }
    err = e->AdoptRows(blocks, s0.RowLength(), srcT, _sh[(size_t)s]->VBDevicePtr());   // (vB: the replica on the same device)
    if (!err.ok()) return err;
    std::vector<int64_t> localQ;
    std::vector<double> localInit;
    for (size_t i = 0; i < fillQ.size(); i++)
      if (fillQ[i] >= first && fillQ[i] < first + nLocal) { localQ.push_back(fillQ[i] - first); localInit.push_back(fillQInit[i]); }
    err = e->ApplyFills(fillT, fillTInit, localQ, localInit);
    if (!err.ok()) return err;
    err = e->SetQuestionGaps((int64_t)qGaps.size(), qGaps.data());
    if (err.ok()) err = e->SetTargetGaps((int64_t)tGaps.size(), tGaps.data());
    if (!err.ok()) return err;
    e->SetTargetIds(targetIds);
    e->SetQuizIds(_sh[(size_t)s]->QuizIds());
    Error ae;
    e->SetQuestionsAsked(s == 0 ? s0.GetTotalQuestionsAsked(ae) : 0);
    for (const char *opt : {"select", "workers", "eval_subtasks", "eval_variant", "bug_compat", "top_cache", "speculate", "host_sampled",
                            "fused_sampled", "batch_min", "batch_qb", "batch_tile", "batch_groups", "batch_tail", "batch_form", "cluster_form", "cluster_shape", "rerank", "combine", "server", "use_graph",
                            "pole_fix", "pole_lazy", "late_eager", "long_row_form", "fuse_update", "combine_spin", "combine_linger_us", "post_always", "server_idle_us"}) {
      const int64_t v = _sh[(size_t)s]->GetOption(opt);
      if (v >= 0) (void)e->SetOption(opt, std::string(opt) == "eval_subtasks" && v == 8 * _sh[(size_t)s]->GetOption("workers") ? 0 : v);
    }
    err = e->StartMaintenance(false);
    if (!err.ok()) return err;
  }
  // ---- commit
  _sh.swap(fresh);
  _Q = newQ;
  _T = newT;
  _qGapList = qGaps;
  _hostPriority.assign((size_t)newQ, 0.0);
  ForgetQuizzes();
  RefreshGapBits();
  AdoptShards();
  std::fill(_remoteReads.begin(), _remoteReads.end(), 0);   // (every old shard was synchronised above; the new ones start clean)
  std::fill(_trainEpoch.begin(), _trainEpoch.end(), 0);
  std::fill(_seenTrain.begin(), _seenTrain.end(), 0);
  return Error();
}

Error ShardedEngine::AddQsTs(int64_t nQuestions, CiAddQorTParam *pAqps, int64_t nTargets, CiAddQorTParam *pAtps) {
  std::lock_guard<OpLock> lk(_opMu);
  Error e = _sh[0]->IsMaintenanceMode() ? Error() : WrongModeErr("add questions/targets");
  if (e.ok()) e = CheckAddArgs(nQuestions, pAqps, nTargets, pAtps);
  if (!e.ok()) return e;
  // CpuEngine::AddQsTsSpec, reference PqaCore/CpuEngine.cpp:468-575, over the GLOBAL ids (kb_plan.h)
  std::vector<int64_t> tGapList, tmp;
  _sh[0]->GetGapLists(tmp, tGapList);
  const AddPlan plan = PlanAdd(_qGapList, tGapList, _Q, _T, nQuestions, pAqps, nTargets, pAtps);
  const std::vector<int64_t> &qIds = plan.qIds, &tIds = plan.tIds;
  const int64_t nQReuse = plan.nQReuse, nTReuse = plan.nTReuse, newQ = plan.newQ, newT = plan.newT;
  std::vector<int64_t> srcQ((size_t)newQ, -1), srcT((size_t)newT, -1);
  for (int64_t q = 0; q < _Q; q++) srcQ[(size_t)q] = q;      // (a gap's rows travel too: they are nobody's)
  for (int64_t t = 0; t < _T; t++) srcT[(size_t)t] = t;
  for (int64_t id : qIds) if (id < _Q) srcQ[(size_t)id] = -1;   // re-initialised below
  std::vector<int64_t> qGaps(_qGapList.begin(), _qGapList.end() - nQReuse), tGaps(tGapList.begin(), tGapList.end() - nTReuse);
  IdLedger targetIds = _sh[0]->TargetIds();
  for (int64_t i = 0; i < nTReuse; i++) targetIds.Reissue(tIds[(size_t)i]);
  targetIds.Extend(newT);                                           // :541-542
  IdLedger questionIds = _questionIds;
  for (int64_t i = 0; i < nQReuse; i++) questionIds.Reissue(qIds[(size_t)i]);
  questionIds.Extend(newQ);
  // (the rebuilt shards mark their remaining gaps themselves: their own id maps are over local ids and are not consulted)
  e = Rebuild(newQ, newT, srcQ, srcT, qGaps, tGaps, targetIds, tIds, plan.tInit, qIds, plan.qInit);
  if (!e.ok()) return e;
  _questionIds = questionIds;
  for (int64_t i = 0; i < nQuestions; i++) pAqps[i]._index = qIds[(size_t)i];
  for (int64_t j = 0; j < nTargets; j++) pAtps[j]._index = tIds[(size_t)j];
  return Error();
}

Error ShardedEngine::Compact(int64_t *pnQuestions, const int64_t **ppOldQuestions, int64_t *pnTargets, const int64_t **ppOldTargets) {
  std::lock_guard<OpLock> lk(_opMu);
  Error e = _sh[0]->IsMaintenanceMode() ? Error() : WrongModeErr("compact the KB");
  if (!e.ok()) return e;
  if (!pnQuestions || !ppOldQuestions || !pnTargets || !ppOldTargets) return Error::Make(ErrCode::NullArgument, "Nullptr output.");
  // CpuEngine::CompactSpec, CpuEngine.cpp:577-658, over the global axes (kb_plan.h); the data moves by rebuilding the shards
  std::vector<int64_t> tGapList, tmp;
  _sh[0]->GetGapLists(tmp, tGapList);
  const CompactPlan plan = PlanCompact(_qGapList, tGapList, _Q, _T);
  const int64_t nQ = (int64_t)plan.oldQ.size(), nT = (int64_t)plan.oldT.size();
  if (nQ < (int64_t)_sh.size())
    return Error::MakeP(ErrCode::InsufficientEngineDimensions, "[nQuestions=" + std::to_string(nQ) + " of " + std::to_string(_sh.size()) + "]",
                        "Fewer questions than devices in PQA_DEVICES would remain.");
  IdLedger targetIds = _sh[0]->TargetIds(), questionIds = _questionIds;
  targetIds.Repack(nT, plan.oldT.data());
  questionIds.Repack(nQ, plan.oldQ.data());
  e = Rebuild(nQ, nT, plan.oldQ, plan.oldT, {}, {}, targetIds, {}, {}, {}, {});
  if (!e.ok()) return e;
  _questionIds = questionIds;
  *pnQuestions = nQ; *pnTargets = nT;
  *ppOldQuestions = MallocCopy(plan.oldQ); *ppOldTargets = MallocCopy(plan.oldT);
  return Error();
}

// ---- .kb file (layout of reference PqaCore/BaseEngine.cpp:323-385 + PqaCore/CpuEngine.cpp:664-688, see hip_engine_kb.cpp): the
// file orders its rows by question, so the shards' blocks follow each other -- every shard streams its own rows through its
// own staging buffer; vB, the target gaps and the target / quiz id maps are replicas (shard 0's are written).
Error ShardedEngine::SaveKB(const char *filePath, bool doubleBuffer) {
  (void)doubleBuffer;
  return SaveKBAs(filePath, 0);
}
// precType 0: the engine's own; another type: every shard's rows pass through the converting kernel on their way out
Error ShardedEngine::SaveKBAs(const char *filePath, uint8_t precType) {
  std::lock_guard<OpLock> lk(_opMu);
  Error e = FlushAnswers();
  if (!e.ok()) return e;
  for (auto &s : _sh) { e = s->Synchronize(); if (!e.ok()) return e; }   // (also parks resident sweeps)
  HipEngine &s0 = *_sh[0];
  uint64_t precision = 0;
  int fe = 0;
  e = KbSavePrecision(precType, s0.PrecisionType(), s0.PrecMantissa(), s0.PrecExponent(), precision, fe);
  if (!e.ok()) return e;
  KbFile file(filePath, true);
  const uint64_t nAsked = s0.GetTotalQuestionsAsked(e);
  e = file.WriteHeader(KbHeader{precision, _K, _Q, _T, nAsked});
  for (size_t s = 0; e.ok() && s < _sh.size(); s++) e = _sh[s]->IoRows(file.f, filePath, false, true, fe);
  for (size_t s = 0; e.ok() && s < _sh.size(); s++) e = _sh[s]->IoRows(file.f, filePath, true, true, fe);
  if (e.ok()) e = s0.IoVB(file.f, filePath, true, fe);
  std::vector<int64_t> tGaps, tmp;
  s0.GetGapLists(tmp, tGaps);
  if (e.ok()) e = file.WriteTrailer(_qGapList, tGaps, _questionIds, s0.TargetIds(), s0.QuizIds());
  return e.ok() ? file.FlushAndClose() : e;
}

ShardedEngine *ShardedEngine::Load(Error &err, const char *filePath, const std::vector<int> &devices, uint8_t precType) {
  KbFile file(filePath, false);
  KbHeader h;
  err = file.ReadHeader(h);
  if (!err.ok()) return nullptr;
  KbLayout lay;
  err = file.CheckHeader(h, lay);
  if (!err.ok()) return nullptr;
  CiEngineDefinition def;
  err = KbLoadDefinition(h, precType, def);   // (precType 0: the file's own)
  if (!err.ok()) return nullptr;
  const int fe = (int)lay.elem;
  std::unique_ptr<ShardedEngine> eng(Create(err, def, devices));
  if (!eng) return nullptr;
  for (size_t s = 0; err.ok() && s < eng->_sh.size(); s++) err = eng->_sh[s]->IoRows(file.f, filePath, false, false, fe);
  for (size_t s = 0; err.ok() && s < eng->_sh.size(); s++) err = eng->_sh[s]->IoRows(file.f, filePath, true, false, fe);
  if (err.ok()) err = eng->_sh[0]->IoVB(file.f, filePath, false, fe);
  std::vector<double> vb((size_t)h.T);   // shard 0's vB (already in the engine's number type) to the other replicas
  if (err.ok()) err = eng->_sh[0]->GetKB(nullptr, nullptr, vb.data());
  for (size_t i = 1; err.ok() && i < eng->_sh.size(); i++) err = eng->_sh[i]->SetVBFromHost(vb.data());
  if (!err.ok()) return nullptr;
  eng->_sh[0]->SetQuestionsAsked(h.nAsked);
  std::vector<int64_t> tGaps;
  IdLedger targetIds, quizIds;
  err = file.ReadTrailer(h.Q, h.T, eng->_qGapList, tGaps, eng->_questionIds, targetIds, quizIds);
  if (!err.ok()) return nullptr;
  eng->RefreshGapBits();
  for (auto &s : eng->_sh) {
    err = s->SetQuestionGaps((int64_t)eng->_qGapList.size(), eng->_qGapList.data());
    if (err.ok()) err = s->SetTargetGaps((int64_t)tGaps.size(), tGaps.data());
    if (!err.ok()) return nullptr;
    s->SetTargetIds(targetIds);
    s->SetQuizIds(quizIds);
  }
  return eng.release();
}

IEngine *LoadShardedEngine(Error &err, const char *filePath, const std::vector<int> &devices, uint8_t precType) {
  return ShardedEngine::Load(err, filePath, devices, precType);
}

IEngine *CreateShardedEngine(Error &err, const CiEngineDefinition &def, const std::vector<int> &devices) {
  return ShardedEngine::Create(err, def, devices);
}

}  // namespace pqa
