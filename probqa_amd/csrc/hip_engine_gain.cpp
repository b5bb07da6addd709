// hip_engine_gain.cpp -- HipEngine::EvalQuestionGainsBatch and HipEngine::ListInformativeQuestionsBatch (hip_engine.h,
// include/PqaHipExt.h): what every question of this engine would tell a quiz, in bits -- the mutual information between the answer and
// the target for a target drawn from the quiz's posterior (gain_kernels.hip has the definition).
//   * validation: everything a call can be refused for, in the header's order, before anything is launched or written;
//   * a call runs in chunks of up to kTopBatchQuizzes quizzes: the chunk's posteriors as launch arguments, ONE sweep of the cube per tile
//     of quizzes (LaunchQuestionGains) into rows[quiz][RedRowPitch()] on the device;
//   * Eval copies the rows out; List shows them to the question listing through slots that carry each quiz's own asked bitmap
//     (LaunchGainSlots, LaunchTopQuestions) for up to 256 records a quiz, and beyond that copies them and takes the prefix here in the
//     same order: gain descending, question ascending; gaps, the quiz's asked questions and what is not > 0 are no candidates.
// Nothing of a quiz changes: the posteriors and asked bits are only read.  A shard answers for the questions it holds -- every shard
// holds every posterior whole, so there is no package.
#include "hip_engine_internal.h"

namespace pqa {

// What both calls can be refused for under the lock: the row length (rowLength >= 0), the mode, an unknown quiz.
Error HipEngine::AdmitGainsLocked(int64_t rowLength, int64_t n, const int64_t *pQuizzes) {
  if (rowLength >= 0 && rowLength != _Q)
    return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(rowLength, _Q, _Q), "Gain row length must equal the question count.");
  return ValidateStatusLocked("question gains", n, pQuizzes, nullptr);
}

Error HipEngine::GainRowsLocked(int64_t first, int64_t m, const int64_t *pQuizzes) {
  Error err;
  TopBatchPriors pr;
  for (int64_t j = 0; j < m; j++) {
    const Quiz *q = UseQuiz(err, pQuizzes[first + j]);
    if (!q) return err;
    pr.prior[j] = q->dPrior;
  }
  HIP_TRY(GrowDevice(&_gain.dRows, _gain.rowsBytes, (size_t)m * (size_t)RedRowPitch() * sizeof(double)));
  MarkStreamBusy();
  HIP_TRY(LaunchQuestionGains(View(), pr, m, _gain.dRows, RedRowPitch(), _stream));
  return Error();
}

Error HipEngine::EvalQuestionGainsBatch(int64_t nQuizzes, const int64_t *pQuizzes, double *pOut, int64_t n) {
  if (nQuizzes < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nQuizzes), "|nQuizzes| must be non-negative.");
  if (nQuizzes > 0 && (!pQuizzes || !pOut)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the quizzes or the gain buffer.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = AdmitGainsLocked(n, nQuizzes, pQuizzes);
  if (!err.ok() || nQuizzes == 0) return err;
  _gainCalls++;
  _gainQuizzes += (uint64_t)nQuizzes;
  hipSetDevice(_device);
  err = FlushUpdates();   // (the quizzes' deferred answers: their posteriors are read below)
  if (!err.ok()) return err;
  if (_serverLaunched) StopServer();   // a launched kernel has no room beside the resident sweep and would wait for it to idle out
  for (int64_t first = 0; first < nQuizzes; first += kTopBatchQuizzes) {
    const int64_t m = std::min<int64_t>(kTopBatchQuizzes, nQuizzes - first);
    TimerStart(_gain.ev);
    err = GainRowsLocked(first, m, pQuizzes);
    if (!err.ok()) return err;
    TimerStop(_gain.ev, _gainDeviceNs);
    HIP_TRY(hipMemcpy2DAsync(pOut + first * n, (size_t)n * sizeof(double), _gain.dRows, (size_t)RedRowPitch() * sizeof(double), (size_t)n * sizeof(double), (size_t)m,
                             hipMemcpyDeviceToHost, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  _pendingRecordOp = 0;
  return Error();
}

Error HipEngine::ListInformativeQuestionsBatch(int64_t nQuizzes, const int64_t *pQuizzes, int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) {
  if (nQuizzes < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nQuizzes), "|nQuizzes| must be non-negative.");
  if (maxCount < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(maxCount), "|maxCount| must be non-negative.");
  if (nQuizzes > 0 && (!pQuizzes || !pCounts || (maxCount > 0 && !pDest))) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = AdmitGainsLocked(-1, nQuizzes, pQuizzes);
  if (!err.ok() || nQuizzes == 0) return err;
  _gainCalls++;
  _gainQuizzes += (uint64_t)nQuizzes;
  for (int64_t i = 0; i < nQuizzes; i++) pCounts[i] = 0;
  if (maxCount == 0) return Error();
  hipSetDevice(_device);
  err = FlushUpdates();
  if (!err.ok()) return err;
  if (_serverLaunched) StopServer();

  GainStage &st = _gain;
  const int64_t want = std::min<int64_t>(maxCount, _Q), pitch = RedRowPitch();
  for (int64_t first = 0; first < nQuizzes; first += kTopBatchQuizzes) {
    const int64_t m = std::min<int64_t>(kTopBatchQuizzes, nQuizzes - first);
    CiRatedQuestion *dest = pDest + first * maxCount;
    TimerStart(st.ev);
    err = GainRowsLocked(first, m, pQuizzes);
    if (!err.ok()) return err;
    if (want > 256) {
      TimerStop(st.ev, _gainDeviceNs);
      st.rows.resize((size_t)(m * pitch));
      HIP_TRY(hipMemcpyAsync(st.rows.data(), st.dRows, (size_t)(m * pitch) * sizeof(double), hipMemcpyDeviceToHost, _stream));
      HIP_TRY(hipStreamSynchronize(_stream));
      for (int64_t j = 0; j < m; j++) {
        const Quiz *q = UseQuiz(err, pQuizzes[first + j]);
        if (!q) return err;
        pCounts[first + j] = TopQuestionsOfVector(st.rows.data() + j * pitch, q->hAsked, want, dest + j * maxCount);
      }
      continue;
    }
    err = EnsureTopScratchRecords(m * TopQuestionsScratchRecords(_Q, want));
    if (!err.ok()) return err;
    HIP_TRY(st.lines.Ensure(_stream, (int64_t)kTopBatchQuizzes * want, 0, kTopBatchQuizzes, hipHostMallocDefault));
    if (!st.dSlots) HIP_TRY(hipMalloc((void **)&st.dSlots, (size_t)kTopBatchQuizzes * sizeof(QuizSlot)));
    GainAsked asked;
    for (int64_t j = 0; j < m; j++) {
      const Quiz *q = UseQuiz(err, pQuizzes[first + j]);
      if (!q) return err;
      asked.asked[j] = q->dAsked;
    }
    HIP_TRY(LaunchGainSlots(st.dSlots, st.dRows, pitch, asked, m, _stream));
    TopQuestions a{};
    a.slots = st.dSlots; a.qgap = _dQGap; a.nQuizzes = (int)m; a.Q = _Q;
    HIP_TRY(LaunchTopQuestions(a, want, _dTopScratch[0], _dTopScratch[1], st.lines.records, st.lines.Counts(), nullptr, 0, _stream));
    TimerStop(st.ev, _gainDeviceNs);
    HIP_TRY(hipStreamSynchronize(_stream));
    for (int64_t j = 0; j < m; j++) {
      const int64_t c = std::max<int64_t>(0, std::min<int64_t>(st.lines.Counts()[j], want));
      const RatedTargetDev *rec = st.lines.records + j * want;
      for (int64_t x = 0; x < c; x++) { dest[j * maxCount + x]._iQuestion = _qFirst + rec[x].iTarget; dest[j * maxCount + x]._priority = rec[x].prob; }
      pCounts[first + j] = c;
    }
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  _pendingRecordOp = 0;
  return Error();
}

}  // namespace pqa
