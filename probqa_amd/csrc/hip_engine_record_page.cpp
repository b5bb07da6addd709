// hip_engine_record_page.cpp -- HipEngine::RecordAnswerPageBatch / RecordAnswerPageBatchFromRows (hip_engine.h, include/PqaHipExt.h): a
// page of answers per quiz in one launch, where a client today calls SetActiveQuestion + RecordAnswer once per answer.
//   * validation: everything a call can be refused for, in the header's order, before any quiz changes or anything is launched;
//   * the quizzes with a non-empty page run in chunks of up to kRecordPageChunk, in the manner of ResumeEntriesLocked: the chunk's
//     tables -- slots | row pointers | local question indices -- in one pinned block, one copy, ONE launch (prior_kernels.hip:
//     record_answer_page_kernel), and, only when the caller wants the likelihoods, their copy back and one synchronisation.  Without
//     them nothing waits for the device, as in FlushUpdates: the posteriors, the asked bits and the listings are ordered on the stream;
//   * the host's bookkeeping of a chunk -- answers, asked bits, active question, versions, the listing's record -- follows its launch.
// Row pointers are the {sA[q][a], mD[q]} pairs of a resumed quiz (PackageRowsLocked): this engine's own cube, or the slots of a row
// package for the questions another shard holds.
#include "hip_engine_internal.h"

#include <unordered_set>

namespace pqa {

namespace {
inline size_t Align256(size_t x) { return (x + 255) & ~(size_t)255; }
}  // namespace

void HipEngine::FreeRecordPage() {
  RecordPageStage &st = _recPage;
  hipFree(st.dTables);
  if (st.hTables) hipHostFree(st.hTables);
  if (st.hLikelihood) hipHostFree(st.hLikelihood);
  if (st.evCopy) hipEventDestroy(st.evCopy);
  if (st.ev[0]) { hipEventDestroy(st.ev[0]); hipEventDestroy(st.ev[1]); }
  st = RecordPageStage();
}

Error HipEngine::RecordAnswerPageBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const AQ *pAQs, double *pLikelihood) {
  return RecordPages(n, pQuizzes, pCounts, pAQs, pLikelihood, false, nullptr);
}
Error HipEngine::RecordAnswerPageBatchFromRows(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const AQ *pAQs, double *pLikelihood,
                                               const void *pRows) {
  return RecordPages(n, pQuizzes, pCounts, pAQs, pLikelihood, true, pRows);
}

Error HipEngine::RecordPages(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const AQ *pAQs, double *pLikelihood, bool fromRows, const void *pRows) {
  // ---- 1, 2: counts and buffers
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "|nQuizzes| must be non-negative.");
  if (n > 0 && (!pQuizzes || !pCounts)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  int64_t total = 0;
  for (int64_t i = 0; i < n; i++) {
    if (pCounts[i] < 0)
      return Error::MakeP(ErrCode::NegativeCount, "entry=" + std::to_string(i) + " count=" + std::to_string(pCounts[i]), "A page's number of answers must be non-negative.");
    total += pCounts[i];
  }
  if (total > 0 && pAQs == nullptr) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of answered questions.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  // ---- 3: the mode, as RecordAnswerBatch answers it
  Error err = CheckRegular("record an answer");
  if (!err.ok()) return err;
  // ---- 4: the fixed limit of a page
  for (int64_t i = 0; i < n; i++)
    if (pCounts[i] > kRecordPageMax)
      return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(i) + " " + RangeParams(pCounts[i], 0, kRecordPageMax), "A page holds at most 4096 answers.");
  // ---- 5, 6: the quizzes, each once
  std::vector<Quiz *> quizzes((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    const int64_t id = pQuizzes[i];
    const bool there = id >= 0 && id < (int64_t)_quizzes.size() && _quizzes[(size_t)id] != nullptr;
    const time_t usedBefore = there ? _quizzes[(size_t)id]->lastUsage : 0;
    if (!(quizzes[(size_t)i] = UseQuiz(err, id))) {
      err.params = "entry=" + std::to_string(i) + " quizId=" + std::to_string(id) + (err.hasParams ? " " + err.params : std::string());
      err.hasParams = true;
      return err;
    }
    if (pCounts[i] == 0) quizzes[(size_t)i]->lastUsage = usedBefore;   // (an empty page is no use of the quiz)
  }
  {
    std::unordered_set<int64_t> seen;
    for (int64_t i = 0; i < n; i++)
      if (!seen.insert(pQuizzes[i]).second)
        return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(i) + " quizId=" + std::to_string(pQuizzes[i]), "A quiz appears twice in the call.");
  }
  // ---- 7, 8: questions over the whole knowledge base's axis (another shard's gaps are known here too), then answers
  std::unordered_set<int64_t> foreignGaps;
  if (IsShard()) foreignGaps.insert(_globalQuestionGaps.begin(), _globalQuestionGaps.end());
  bool anyForeign = false;
  for (int64_t i = 0, at = 0; i < n; i++)
    for (int64_t j = 0; j < pCounts[i]; j++, at++) {
      const int64_t id = pAQs[at].iQuestion;
      const std::string where = "entry=" + std::to_string(i) + " position=" + std::to_string(j) + " questionId=" + std::to_string(id);
      if (id < 0 || id >= _qTotal) return Error::MakeP(ErrCode::IndexOutOfRange, where + " " + RangeParams(id, 0, _qTotal - 1), "A page's question is out of range.");
      const bool own = OwnsQuestion(id);
      if (own ? BitTest(_hQGap, id - _qFirst) : foreignGaps.count(id) != 0) return Error::MakeP(ErrCode::IndexOutOfRange, where, "A page's question is a gap.");
      anyForeign = anyForeign || !own;
    }
  for (int64_t i = 0, at = 0; i < n; i++)
    for (int64_t j = 0; j < pCounts[i]; j++, at++) {
      const int64_t ia = pAQs[at].iAnswer;
      if (ia < 0 || ia >= _K)
        return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(i) + " position=" + std::to_string(j) + " " + RangeParams(ia, 0, _K - 1),
                            "Answer index is not in the answer range.");
    }
  if (anyForeign && !fromRows)
    return Error::MakeP(ErrCode::NotImplemented, "Feature=RecordAnswerPageBatch across separately driven shards",
                        "An answered question belongs to another shard: its rows are not reachable from this engine alone "
                        "(PqaEngine_RecordAnswerPageBatchFromRows takes them from a row package; PQA_DEVICES / the sharded engine of one process resolves them).");
  if (anyForeign && pRows == nullptr) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the row package.");
  _recPageCalls++;
  _recPageAnswers += (uint64_t)total;
  if (total == 0) return Error();

  // ---- engine state: the deferred answers first, the resident sweep's step finished, a speculation of one of the quizzes dropped
  hipSetDevice(_device);
  err = FlushUpdates();
  if (!err.ok()) return err;
  ServerQuiesce();
  for (int64_t i = 0; i < n; i++)
    if (pCounts[i] > 0 && _spec.quiz == quizzes[(size_t)i]) DropSpeculation();
  std::vector<const void *> rows;
  err = PackageRowsLocked(total, pAQs, pRows, rows);   // (a host package is staged behind this, under option "rows_stage")
  if (!err.ok()) return err;

  const KbView kb = View();
  const int64_t nLoose = std::max<int64_t>(1, _opt.workers - 1);   // reference PqaCore/CEQuiz.h:98, PqaCore/BaseCpuEngine.cpp:22
  const int64_t topCount = _T <= 16384 ? std::min<int64_t>(std::min<int64_t>(std::min<int64_t>(_opt.topCache, _topWantRecent), kQuizTop), _T) : 0;
  RecordPageStage &st = _recPage;
  struct Entry { int64_t i, first; };   // a quiz with a non-empty page: its batch entry and where its answers begin in pAQs
  std::vector<Entry> chunk;
  int64_t next = 0, at = 0;
  bool waited = false;
  for (;;) {
    chunk.clear();
    size_t nAnswers = 0;
    for (; next < n && (int64_t)chunk.size() < kRecordPageChunk; at += pCounts[next], next++)
      if (pCounts[next] > 0) { chunk.push_back(Entry{next, at}); nAnswers += (size_t)pCounts[next]; }
    if (chunk.empty()) break;
    const size_t m = chunk.size();
    const size_t offRows = Align256(m * sizeof(RecordPageSlot));
    const size_t offLocal = offRows + Align256(2 * nAnswers * sizeof(void *));
    const size_t hostBytes = offLocal + Align256(nAnswers * sizeof(int32_t));
    const size_t devBytes = hostBytes + (pLikelihood ? Align256(nAnswers * sizeof(double)) : 0);   // the likelihoods stay behind the copied tables
    if (devBytes > st.dBytes) {
      hipFree(st.dTables);   // (waits for whatever still reads them)
      st.dTables = nullptr;
      st.dBytes = 0;
      HIP_TRY(hipMalloc((void **)&st.dTables, devBytes));
      st.dBytes = devBytes;
    }
    // the pinned block is not rewritten while an earlier chunk's copy of it is still under way
    if (st.evCopy == nullptr) HIP_TRY(hipEventCreateWithFlags(&st.evCopy, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(st.evCopy));
    if (hostBytes > st.hBytes) {
      if (st.hTables) hipHostFree(st.hTables);
      st.hTables = nullptr;
      st.hBytes = 0;
      HIP_TRY(hipHostMalloc((void **)&st.hTables, hostBytes, hipHostMallocDefault));
      st.hBytes = hostBytes;
    }
    if (pLikelihood && nAnswers > st.hLikelihoodCount) {
      if (st.hLikelihood) hipHostFree(st.hLikelihood);
      st.hLikelihood = nullptr;
      st.hLikelihoodCount = 0;
      HIP_TRY(hipHostMalloc((void **)&st.hLikelihood, nAnswers * sizeof(double), hipHostMallocDefault));
      st.hLikelihoodCount = nAnswers;
    }
    RecordPageSlot *slots = reinterpret_cast<RecordPageSlot *>(st.hTables);
    const void **hRows = reinterpret_cast<const void **>(st.hTables + offRows);
    int32_t *hLocal = reinterpret_cast<int32_t *>(st.hTables + offLocal);
    size_t done = 0;
    for (size_t k = 0; k < m; k++) {
      const Entry &x = chunk[k];
      Quiz *q = quizzes[(size_t)x.i];
      const int64_t count = pCounts[x.i];
      slots[k] = RecordPageSlot{q->dPrior, q->dAsked, (void *)q->pin, _opSeq + 1 + (uint64_t)k,
                                reinterpret_cast<const void *const *>(st.dTables + offRows + 2 * done * sizeof(void *)),
                                reinterpret_cast<const int32_t *>(st.dTables + offLocal + done * sizeof(int32_t)),
                                pLikelihood ? reinterpret_cast<double *>(st.dTables + hostBytes + done * sizeof(double)) : nullptr, count};
      for (int64_t j = 0; j < count; j++, done++) {
        const AQ &aq = pAQs[x.first + j];
        hRows[2 * done] = rows[2 * (size_t)(x.first + j)];
        hRows[2 * done + 1] = rows[2 * (size_t)(x.first + j) + 1];
        hLocal[done] = OwnsQuestion(aq.iQuestion) ? (int32_t)(aq.iQuestion - _qFirst) : -1;
      }
    }
    MarkStreamBusy();
    HIP_TRY(hipMemcpyAsync(st.dTables, st.hTables, hostBytes, hipMemcpyHostToDevice, _stream));
    HIP_TRY(hipEventRecord(st.evCopy, _stream));
    TimerStart(st.ev);
    HIP_TRY(LaunchRecordAnswerPage(kb, reinterpret_cast<const RecordPageSlot *>(st.dTables), (int64_t)m, nLoose, topCount, _stream));
    _recPageLaunches++;
    // ---- the chunk's bookkeeping (CEQuiz::RecordAnswer, PqaCore/CEQuiz.h:77-122, per answer): the launch is on the stream
    for (size_t k = 0; k < m; k++) {
      const Entry &x = chunk[k];
      Quiz *q = quizzes[(size_t)x.i];
      for (int64_t j = 0; j < pCounts[x.i]; j++) {
        const AQ &aq = pAQs[x.first + j];
        q->answers.push_back(aq);
        if (OwnsQuestion(aq.iQuestion)) BitSet(q->hAsked, aq.iQuestion - _qFirst, true);
        q->priorVersion++;
      }
      q->activeQuestion = -1;
      q->topOp = _opSeq + 1 + (uint64_t)k; q->topVersion = q->priorVersion; q->topCount = topCount;
    }
    _opSeq += (uint64_t)m;
    TimerStop(st.ev, _recPageDeviceNs);
    if (pLikelihood) {
      HIP_TRY(hipMemcpyAsync(st.hLikelihood, st.dTables + hostBytes, nAnswers * sizeof(double), hipMemcpyDeviceToHost, _stream));
      HIP_TRY(hipStreamSynchronize(_stream));
      waited = true;
      size_t from = 0;
      for (size_t k = 0; k < m; k++) {
        std::memcpy(pLikelihood + chunk[k].first, st.hLikelihood + from, (size_t)pCounts[chunk[k].i] * sizeof(double));
        from += (size_t)pCounts[chunk[k].i];
      }
    }
  }
  if (anyForeign && !waited) {   // the package is the caller's until the call returns: the launches have read it by then
    HIP_TRY(hipStreamSynchronize(_stream));
    waited = true;
  }
  if (waited) {   // (the stream has just been synchronised)
    _mu.busy = false;
    _pendingRecordOp = 0;
  }
  return Error();
}

}  // namespace pqa
