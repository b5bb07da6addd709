// hip_engine_among.cpp -- HipEngine: the Among calls (hip_engine.h, include/PqaHipExt.h): evaluate and select over a LISTED set of
// questions per quiz.  "Among a list L" means: for this call only, every question outside L counts as asked -- the quiz's priority
// vector is the sweep's with zeros outside L, and the selection is the existing selector over it with the skip bits
// gaps | asked | not listed.
// One launch of eval_listed_kernel (among_kernels.hip) evaluates all (quiz, question) pairs of the call into the batch context's
// per-quiz priority vectors (BatchCtx::dPriority), the pole fix behind it on Double engines; then, by the form of the call:
//   EvalPrioritiesAmongBatch            a gather of the pairs' priorities and ONE copy of sum(pCounts) doubles to the host;
//   SelectArgmaxAmongBatch,             listed_argmax_kernel over each quiz's pairs -- maximum priority, lowest id among equals --
//   NextQuestionArgmaxAmongBatch        whose records the host polls;
//   NextQuestionSampledAmongBatch       the vectors zeroed first, the quizzes' bitmaps asked | not listed uploaded, and the batched
//                                       sampled selector as it is (LaunchSampledBatch over the quizzes' own vectors) -- the
//                                       reference's fallback (FinishSelection) runs over the same bitmap, so it never leaves the list.
// Nothing of size Q crosses to the host.  The calls write only into the batch context's buffers, never into a quiz's own state or the
// engine's single-quiz vector; towards the resident sweep, the speculative sweep and the single-quiz pole list they do what
// EvalPrioritiesBatch does (FlushUpdates, StopServer).  A quiz with an empty list takes no part in the launches: its pick is -1.
#include "hip_engine_internal.h"

namespace pqa {

// Everything a call can be refused for, before anything is launched, drawn or written.
Error HipEngine::ValidateAmongLocked(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, bool haveOut) {
  Error err = ValidateBatchLocked(n, pQuizzes);   // (mode, batch size, quiz ids: as EvalPrioritiesBatch / NextQuestionSampledBatch)
  if (!err.ok() || n == 0) return err;
  if (!pCounts || !haveOut) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  int64_t total = 0;
  for (int64_t i = 0; i < n; i++) {
    if (pCounts[i] < 0) return Error::MakeP(ErrCode::NegativeCount, "entry=" + std::to_string(i) + " count=" + std::to_string(pCounts[i]), "A list's length must be non-negative.");
    total += pCounts[i];
  }
  if (total > 0 && !pQuestions) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  std::vector<int64_t> &stamp = _among.stamp;
  stamp.assign((size_t)_qTotal, 0);
  int64_t at = 0;
  for (int64_t i = 0; i < n; i++)
    for (int64_t k = 0; k < pCounts[i]; k++, at++) {
      const int64_t id = pQuestions[at];
      const std::string where = "entry=" + std::to_string(i) + " position=" + std::to_string(k) + " questionId=" + std::to_string(id);
      if (id < 0 || id >= _qTotal) return Error::MakeP(ErrCode::IndexOutOfRange, where + " " + RangeParams(id, 0, _qTotal - 1), "A listed question is out of range.");
      if (stamp[(size_t)id] == i + 1) return Error::MakeP(ErrCode::IndexOutOfRange, where, "A question appears twice in one quiz's list.");
      stamp[(size_t)id] = i + 1;
    }
  return Error();
}

Error HipEngine::AmongLocked(AmongForm form, int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, const uint64_t *pRnd,
                             double *pPriorities, CiHipSelection *pSel, int64_t *pPicked) {
  int64_t total = 0;
  if (n > 0 && n <= kMaxBatch && pCounts)
    for (int64_t i = 0; i < n; i++) total += pCounts[i] > 0 ? pCounts[i] : 0;
  const bool haveOut = form == AmongForm::Eval ? (pPriorities != nullptr || total == 0) : form == AmongForm::Select ? pSel != nullptr : pPicked != nullptr;
  Error err = ValidateAmongLocked(n, pQuizzes, pCounts, pQuestions, haveOut && (form != AmongForm::Sampled || pRnd != nullptr));
  if (!err.ok() || n == 0) return err;
  hipSetDevice(_device);
  err = FlushUpdates();
  if (!err.ok()) return err;
  BatchCtx &c = _ctx[0];
  err = EnsureBatchStaging(c);
  if (err.ok()) err = EnsureBatchVectors(c);
  if (!err.ok()) return err;

  // ---- the lists as the kernels take them: the quizzes with a non-empty list are the launch's slots, in batch order
  AmongStage &st = _among;
  st.entry.clear(); st.offsets.clear(); st.pairs.clear(); st.local = 0;
  _batchQuizzes.assign((size_t)n, nullptr);
  for (int64_t i = 0, at = 0; i < n; at += pCounts[i], i++) {
    _batchQuizzes[(size_t)i] = UseQuiz(err, pQuizzes[i]);
    if (!_batchQuizzes[(size_t)i]) return err;
    if (pCounts[i] == 0) continue;
    const int32_t j = (int32_t)st.entry.size();
    st.entry.push_back(i);
    st.offsets.push_back((int64_t)st.pairs.size());
    for (int64_t k = 0; k < pCounts[i]; k++) {
      const int64_t id = pQuestions[at + k];
      const bool own = OwnsQuestion(id);   // (another process's shard holds the others: skipped here, priority 0)
      st.pairs.push_back(ListedPair{j, own ? (int32_t)(id - _qFirst) : -1});
      st.local += own ? 1 : 0;
    }
  }
  st.offsets.push_back((int64_t)st.pairs.size());
  const int64_t nz = (int64_t)st.entry.size(), nPairs = (int64_t)st.pairs.size();
  _amongCalls++;
  _amongPairs += (uint64_t)st.local;
  for (int64_t i = 0; i < n; i++) {
    if (pSel) pSel[i] = CiHipSelection{0.0, -1};
    if (pPicked) pPicked[i] = -1;
  }
  if (nz == 0) return Error();

  const size_t offBytes = ((size_t)(nz + 1) * sizeof(int64_t) + 15) / 16 * 16, pairBytes = (size_t)nPairs * sizeof(ListedPair);
  HIP_TRY(GrowDevice(&c.dAmong, c.amongBytes, offBytes + pairBytes + (form == AmongForm::Eval ? (size_t)nPairs * sizeof(double) : 0)));
  int64_t *dOffsets = static_cast<int64_t *>(c.dAmong);
  ListedPair *dPairs = reinterpret_cast<ListedPair *>(static_cast<char *>(c.dAmong) + offBytes);
  double *dGather = reinterpret_cast<double *>(static_cast<char *>(c.dAmong) + offBytes + pairBytes);
  HIP_TRY(hipMemcpyAsync(dOffsets, st.offsets.data(), (size_t)(nz + 1) * sizeof(int64_t), hipMemcpyHostToDevice, _stream));
  HIP_TRY(hipMemcpyAsync(dPairs, st.pairs.data(), pairBytes, hipMemcpyHostToDevice, _stream));

  // ---- the sampled forms: every slot's bitmap asked | not listed, and its vector zero outside the list
  const bool sampled = form == AmongForm::Sampled;
  const size_t maskWords = _hQGap.size();
  if (sampled) {
    st.masks.assign((size_t)nz * maskWords, ~0u);
    for (const ListedPair &lp : st.pairs)
      if (lp.q >= 0) st.masks[(size_t)lp.b * maskWords + ((size_t)lp.q >> 5)] &= ~(1u << (lp.q & 31));
    for (int64_t j = 0; j < nz; j++) {
      const std::vector<uint32_t> &asked = _batchQuizzes[(size_t)st.entry[(size_t)j]]->hAsked;
      for (size_t w = 0; w < maskWords && w < asked.size(); w++) st.masks[(size_t)j * maskWords + w] |= asked[w];
    }
    HIP_TRY(GrowDevice(&c.dAmongMask, c.amongMaskBytes, st.masks.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(c.dAmongMask, st.masks.data(), st.masks.size() * sizeof(uint32_t), hipMemcpyHostToDevice, _stream));
    HIP_TRY(hipMemsetAsync(c.dPriority, 0, (size_t)nz * (size_t)_Q * sizeof(double), _stream));
  }
  for (int64_t j = 0; j < nz; j++) {
    const Quiz *q = _batchQuizzes[(size_t)st.entry[(size_t)j]];
    c.h->slots[j] = QuizSlot{q->dPrior, sampled ? c.dAmongMask + (size_t)j * maskWords : q->dAsked, c.dPriority + (size_t)j * (size_t)_Q,
                             &c.h->out[j], &c.h->seq[j], nullptr};
  }
  HIP_TRY(hipMemcpyAsync(c.dSlots, c.h->slots, (size_t)nz * sizeof(QuizSlot), hipMemcpyHostToDevice, _stream));
  StopServer();   // a launched sweep has no room beside the resident one and would wait for it to idle out
  c.lastBp = 0;   // (the quizzes' priorities are their own vectors in dPriority)

  // ---- the listed sweep, the pole fix behind it (Double engines, option pole_fix): list and records in the batch's pole scratch
  const KbView kb = View();
  const size_t poleBytes = EvalListedPoleBytes(kb, nPairs);
  if (poleBytes > c.poleBytes) {
    HIP_TRY(GrowDevice(&c.dPole, c.poleBytes, poleBytes));
    HIP_TRY(hipMemsetAsync(c.dPole, 0, kBatchPoleClear, _stream));   // (the head, once: every launch leaves it cleared)
  }
  HIP_TRY(LaunchEvalListed(kb, c.dSlots, (int)nz, dPairs, nPairs, poleBytes > 0 ? c.dPole : nullptr, _stream));

  if (form == AmongForm::Eval) {   // sum(pCounts) doubles cross to the host
    HIP_TRY(LaunchListedGather(c.dSlots, dPairs, nPairs, dGather, _stream));
    _priorityHostBytes += (size_t)nPairs * sizeof(double);
    HIP_TRY(hipMemcpyAsync(pPriorities, dGather, (size_t)nPairs * sizeof(double), hipMemcpyDeviceToHost, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
    return Error();
  }
  const uint64_t tag = NextLaunchTag();
  if (sampled) {
    std::vector<uint64_t> rnd((size_t)nz);
    for (int64_t j = 0; j < nz; j++) rnd[(size_t)j] = pRnd[st.entry[(size_t)j]];
    err = LaunchSampledBatch(c, nz, rnd.data(), tag);
    if (!err.ok()) return err;
  } else {
    HIP_TRY(LaunchListedArgmax(kb, c.dSlots, (int)nz, dOffsets, dPairs, 0, tag, _stream));
  }
  err = WaitBatchFlags(c, nz, tag);
  if (!err.ok()) return err;
  for (int64_t j = 0; j < nz; j++) {
    const int64_t i = st.entry[(size_t)j];
    const SelectResult r = c.h->out[j];
    CheckPriority(r.priority, sampled ? -1 : r.index);   // (the sampled selector reports the grand total, not a priority)
    if (form == AmongForm::Select) {
      pSel[i]._priority = r.index < 0 ? 0.0 : r.priority;
      pSel[i]._iQuestion = r.index < 0 ? -1 : r.index + _qFirst;
      continue;
    }
    Error e;   // -1 + QuestionsExhausted: reported as -1 only
    pPicked[i] = sampled ? FinishSelection(e, _batchQuizzes[(size_t)i], r.index, _Q, _hQGap.data(), st.masks.data() + (size_t)j * maskWords)
                         : FinishSelection(e, _batchQuizzes[(size_t)i], r.index < 0 ? kSelNone : r.index);
  }
  return Error();
}

Error HipEngine::EvalPrioritiesAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, double *pOut) {
  std::lock_guard<std::mutex> selLk(_ctx[0].mu);   // (this context's staging buffers: not while a leader's combined sweep uses them)
  std::lock_guard<EngineMutex> lk(_mu);
  return AmongLocked(AmongForm::Eval, n, pQuizzes, pCounts, pQuestions, nullptr, pOut, nullptr, nullptr);
}

Error HipEngine::SelectArgmaxAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, CiHipSelection *pOut) {
  std::lock_guard<std::mutex> selLk(_ctx[0].mu);
  std::lock_guard<EngineMutex> lk(_mu);
  return AmongLocked(AmongForm::Select, n, pQuizzes, pCounts, pQuestions, nullptr, nullptr, pOut, nullptr);
}

Error HipEngine::NextQuestionArgmaxAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, int64_t *pPicked) {
  std::lock_guard<std::mutex> selLk(_ctx[0].mu);
  std::lock_guard<EngineMutex> lk(_mu);
  return AmongLocked(AmongForm::Argmax, n, pQuizzes, pCounts, pQuestions, nullptr, nullptr, nullptr, pPicked);
}

Error HipEngine::NextQuestionSampledAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, const uint64_t *pRnd,
                                               int64_t *pPicked) {
  std::lock_guard<std::mutex> selLk(_ctx[0].mu);
  std::lock_guard<EngineMutex> lk(_mu);
  return AmongLocked(AmongForm::Sampled, n, pQuizzes, pCounts, pQuestions, pRnd, nullptr, nullptr, pPicked);
}

// What a server calls: by option "select".  select = 0: one number per quiz from the engine's generator, in batch order, as
// NextQuestionBatch draws them -- after the whole call has been validated, so that a refused call draws nothing.
Error HipEngine::NextQuestionAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pCounts, const int64_t *pQuestions, int64_t *pPicked) {
  std::lock_guard<std::mutex> selLk(_ctx[0].mu);
  std::lock_guard<EngineMutex> lk(_mu);
  if (_opt.select == 1) return AmongLocked(AmongForm::Argmax, n, pQuizzes, pCounts, pQuestions, nullptr, nullptr, nullptr, pPicked);
  Error err = ValidateAmongLocked(n, pQuizzes, pCounts, pQuestions, pPicked != nullptr);
  if (!err.ok() || n == 0) return err;
  std::vector<uint64_t> rnd((size_t)n);
  {
    std::lock_guard<std::mutex> rk(_rngMu);
    for (int64_t i = 0; i < n; i++) rnd[(size_t)i] = _rng.Next();
  }
  return AmongLocked(AmongForm::Sampled, n, pQuizzes, pCounts, pQuestions, rnd.data(), nullptr, nullptr, pPicked);
}

}  // namespace pqa
