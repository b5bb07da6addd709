// hip_engine_list.cpp -- HipEngine: ListTopQuestions / ListTopQuestionsBatch (hip_engine.h), the question-side twin of ListTopTargets.
// The priorities are the ones PqaEngine_EvalPriorities / PqaEngine_EvalPrioritiesBatch return -- the same sweep, launched the same way,
// the pole fix behind it redoing every listed question -- and they stay on the device: the listing kernels (kb_kernels.hip:
// LaunchTopQuestions) go on the engine's stream right behind them and write records, counts and flags into host-coherent memory, which
// the host polls.  Lists of more than 256 questions are bulk exports: the priority vector is copied and the prefix taken on the host
// under the same order (as ListTopTargetsOnHost is for targets).
// Nothing of a quiz changes: no active question, no counter.  Towards the resident sweep, the speculative sweep and the pole list the
// calls do what EvalPriorities / EvalPrioritiesBatch do (StopServer, LaunchSingleSweep's SettlePoleList, BatchSweep).
#include "hip_engine_internal.h"

namespace pqa {
static_assert(sizeof(CiRatedQuestion) == sizeof(RatedTargetDev) && sizeof(CiRatedQuestion) == sizeof(RatedIndex) && sizeof(CiRatedQuestion) == 16,
              "the kernels' records are the caller's");

namespace {
Error TopQuestionsArgs(int64_t maxCount, bool haveDest) {   // (the codes ListTopTargetsBatch answers with)
  if (maxCount < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(maxCount), "|maxCount| must be non-negative.");
  if (maxCount > 0 && !haveDest) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the destination.");
  return Error();
}
}  // namespace

// The host's listing of a priority vector: the eligible questions with a priority > 0 by (priority descending, question ascending).
int64_t HipEngine::TopQuestionsOfVector(const double *pri, const std::vector<uint32_t> &asked, int64_t want, CiRatedQuestion *pDest) const {
  std::vector<int64_t> idx;
  return RatedPrefix(pri, _Q, want, [&](int64_t i) { return !BitTest(_hQGap, i) && !BitTest(asked, i); }, [&](int64_t i) { return _qFirst + i; }, pDest, idx);
}

// ---- one quiz: the engine's own priority vector and pinned lines -------------------------------------------------------------------
Error HipEngine::EnqueueTopQuestionsLocked(Quiz *q, int64_t maxCount) {
  const int64_t want = std::min<int64_t>(maxCount, _Q);
  _topQ = TopQFlight{};
  if (want <= 0) return Error();
  hipSetDevice(_device);
  Error err = FlushUpdates();   // (a deferred RecordAnswer of the quiz: the priorities are its new posterior's)
  if (!err.ok()) return err;
  const bool onHost = want > 256;
  if (!onHost) {
    err = EnsureTopScratchRecords(TopQuestionsScratchRecords(_Q, want));
    if (!err.ok()) return err;
  }
  StopServer();   // a launched sweep has no room beside the resident one and would wait for it to idle out
  err = LaunchSingleSweep(q, nullptr);
  if (!err.ok()) return err;
  uint64_t op = 0;
  if (!onHost) {
    TopQuestions a{};
    a.priority = _dPriority; a.asked = q->dAsked; a.qgap = _dQGap; a.nQuizzes = 1; a.Q = _Q;
    op = ++_opSeq;
    HIP_TRY(LaunchTopQuestions(a, want, _dTopScratch[0], _dTopScratch[1], _hPinned->topQ, &_hPinned->nOutQ, &_hPinned->topQFlag, op, _stream));
  } else {   // (the bulk export: the vector and the asked bits as they are now -- the next sweep of any quiz overwrites _dPriority)
    _topQ.pri.resize((size_t)_Q);
    HIP_TRY(hipMemcpyAsync(_topQ.pri.data(), _dPriority, (size_t)_Q * sizeof(double), hipMemcpyDeviceToHost, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
    _topQ.asked.assign(1, q->hAsked);
  }
  _topQ.n = 1; _topQ.want = want; _topQ.op = op; _topQ.onHost = onHost;
  return Error();
}

int64_t HipEngine::CollectTopQuestionsLocked(Error &err, CiRatedQuestion *pDest) {
  const TopQFlight f = std::move(_topQ);
  _topQ = TopQFlight{};
  if (f.n == 0) return 0;
  hipSetDevice(_device);
  if (f.onHost) return TopQuestionsOfVector(f.pri.data(), f.asked[0], f.want, pDest);
  err = WaitFlag(&_hPinned->topQFlag, f.op, "ListTopQuestions");
  if (!err.ok()) return -1;
  const int64_t n = std::max<int64_t>(0, std::min<int64_t>(_hPinned->nOutQ, f.want));
  for (int64_t i = 0; i < n; i++) {
    pDest[i]._iQuestion = _qFirst + _hPinned->topQ[i].iTarget;
    pDest[i]._priority = _hPinned->topQ[i].prob;
  }
  return n;
}

Error HipEngine::EnqueueTopQuestions(int64_t iQuiz, int64_t maxCount, bool haveDest) {
  std::lock_guard<EngineMutex> lk(_mu);
  _topQ = TopQFlight{};
  Error err = CheckRegular("list top questions");
  if (!err.ok()) return err;
  Quiz *q = UseQuiz(err, iQuiz);
  if (!q) return err;
  err = TopQuestionsArgs(maxCount, haveDest);
  if (!err.ok()) return err;
  return EnqueueTopQuestionsLocked(q, maxCount);
}

int64_t HipEngine::CollectTopQuestions(Error &err, CiRatedQuestion *pDest) {
  std::lock_guard<EngineMutex> lk(_mu);
  return CollectTopQuestionsLocked(err, pDest);
}

int64_t HipEngine::ListTopQuestions(Error &err, int64_t iQuiz, int64_t maxCount, CiRatedQuestion *pDest) {
  std::lock_guard<EngineMutex> lk(_mu);
  err = CheckRegular("list top questions");
  if (!err.ok()) return -1;
  Quiz *q = UseQuiz(err, iQuiz);
  if (!q) return -1;
  err = TopQuestionsArgs(maxCount, pDest != nullptr);
  if (err.ok()) err = EnqueueTopQuestionsLocked(q, maxCount);
  if (!err.ok()) return -1;
  return CollectTopQuestionsLocked(err, pDest);
}

// ---- many quizzes: the batched sweep's priorities where it left them ------------------------------------------------------------------
// The sweep is EvalPrioritiesBatch's (BatchSweep with the priorities wanted), whichever form option "batch_form" and the batch give it:
// grid.y = quiz leaves every quiz's own vector, the row-sharing and (quiz, chunk) sweeps the quiz-minor matrix (BatchCtx::lastBp).
Error HipEngine::EnqueueTopQuestionsBatchLocked(int64_t n, const int64_t *pQuizzes, int64_t maxCount) {
  _topQBatch = TopQFlight{};
  Error err = ValidateBatchLocked(n, pQuizzes);   // (mode, size, ids: before anything is launched or written)
  if (!err.ok()) return err;
  const int64_t want = std::min<int64_t>(maxCount, _Q);
  if (n == 0 || want <= 0) return Error();
  hipSetDevice(_device);
  const bool onHost = want > 256;
  int64_t *hCounts = nullptr;
  uint64_t *hFlags = nullptr;
  if (!onHost) {
    err = EnsureTopScratchRecords(n * TopQuestionsScratchRecords(_Q, want));
    if (!err.ok()) return err;
    HIP_TRY(_hTopQ.Ensure(_stream, n * want, sizeof(uint64_t), kMaxBatch, hipHostMallocMapped | hipHostMallocCoherent));   // records | counts | flags
    hCounts = _hTopQ.Counts();
    hFlags = _hTopQ.Tail<uint64_t>();
  }
  uint64_t tag = 0;
  err = EnqueueBatchLocked(n, pQuizzes, true, &tag);
  if (!err.ok()) return err;
  uint64_t op = 0;
  if (!onHost) {
    const BatchCtx &c = _ctx[0];
    TopQuestions a{};
    a.slots = c.dSlots; a.priority = c.lastBp > 0 ? c.dPriT : nullptr; a.qgap = _dQGap; a.nQuizzes = (int)n; a.Bp = c.lastBp; a.Q = _Q;
    op = ++_opSeq;
    HIP_TRY(LaunchTopQuestions(a, want, _dTopScratch[0], _dTopScratch[1], _hTopQ.records, hCounts, hFlags, op, _stream));
  }
  if (onHost) for (int64_t i = 0; i < n; i++) _topQBatch.asked.push_back(_batchQuizzes[(size_t)i]->hAsked);
  _topQBatch.n = n; _topQBatch.want = want; _topQBatch.op = op; _topQBatch.onHost = onHost;
  return Error();
}

Error HipEngine::CollectTopQuestionsBatchLocked(int64_t n, int64_t stride, CiRatedQuestion *pDest, int64_t *pCounts) {
  const TopQFlight f = std::move(_topQBatch);
  _topQBatch = TopQFlight{};
  for (int64_t i = 0; i < n; i++) pCounts[i] = 0;
  if (f.n == 0) return Error();
  if (f.n != n || stride < f.want) return Error::Make(ErrCode::Internal, "No listing of this batch is in flight.");
  hipSetDevice(_device);
  if (f.onHost) {
    std::vector<double> pri((size_t)n * (size_t)_Q);
    Error err = CollectBatchPrioritiesLocked(n, pri.data());
    if (!err.ok()) return err;
    for (int64_t i = 0; i < n; i++) pCounts[i] = TopQuestionsOfVector(pri.data() + (size_t)i * (size_t)_Q, f.asked[(size_t)i], f.want, pDest + i * stride);
    return Error();
  }
  const int64_t *hCounts = _hTopQ.Counts();
  volatile uint64_t *hFlags = _hTopQ.Tail<volatile uint64_t>();
  for (int64_t i = 0; i < n; i++) {   // (the quizzes' last merges retire together: the first wait is the long one)
    Error err = WaitFlag(&hFlags[i], f.op, "ListTopQuestionsBatch");
    if (!err.ok()) return err;
  }
  for (int64_t i = 0; i < n; i++) {
    const int64_t c = std::max<int64_t>(0, std::min<int64_t>(hCounts[i], f.want));
    const RatedTargetDev *rec = _hTopQ.records + i * f.want;
    CiRatedQuestion *dst = pDest + i * stride;
    for (int64_t j = 0; j < c; j++) { dst[j]._iQuestion = _qFirst + rec[j].iTarget; dst[j]._priority = rec[j].prob; }
    pCounts[i] = c;
  }
  return Error();
}

namespace {
Error TopQuestionsBatchArgs(int64_t n, const int64_t *pQuizzes, int64_t maxCount, bool haveDest, bool haveCounts) {   // (ListTopTargetsBatch's)
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "|nQuizzes| must be non-negative.");
  if (maxCount < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(maxCount), "|maxCount| must be non-negative.");
  if (n > 0 && (!pQuizzes || !haveCounts || (maxCount > 0 && !haveDest))) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  return Error();
}
}  // namespace
Error HipEngine::CheckTopQuestionsBatchArgs(int64_t n, const int64_t *pQuizzes, int64_t maxCount, bool haveDest, bool haveCounts) {
  return TopQuestionsBatchArgs(n, pQuizzes, maxCount, haveDest, haveCounts);
}

Error HipEngine::EnqueueTopQuestionsBatch(int64_t n, const int64_t *pQuizzes, int64_t maxCount) {
  std::lock_guard<EngineMutex> lk(_mu);
  return EnqueueTopQuestionsBatchLocked(n, pQuizzes, maxCount);
}

Error HipEngine::CollectTopQuestionsBatch(int64_t n, int64_t stride, CiRatedQuestion *pDest, int64_t *pCounts) {
  std::lock_guard<EngineMutex> lk(_mu);
  return CollectTopQuestionsBatchLocked(n, stride, pDest, pCounts);
}

Error HipEngine::ListTopQuestionsBatch(int64_t n, const int64_t *pQuizzes, int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) {
  Error err = TopQuestionsBatchArgs(n, pQuizzes, maxCount, pDest != nullptr, pCounts != nullptr);
  if (!err.ok()) return err;
  std::lock_guard<std::mutex> selLk(_ctx[0].mu);   // (this context's staging buffers: not while a leader's combined sweep uses them)
  std::lock_guard<EngineMutex> lk(_mu);
  err = EnqueueTopQuestionsBatchLocked(n, pQuizzes, maxCount);
  if (!err.ok() || n == 0) return err;
  return CollectTopQuestionsBatchLocked(n, maxCount, pDest, pCounts);
}

}  // namespace pqa
