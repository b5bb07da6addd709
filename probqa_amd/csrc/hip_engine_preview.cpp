// hip_engine_preview.cpp -- HipEngine::PreviewAnswersBatch (hip_engine.h, include/PqaHipExt.h): for many (quiz, question) pairs, what each
// of the K answers would do to the quiz -- its likelihood, the entropy of the posterior it would leave, and that posterior's best targets.
//   * validation: everything a call can be refused for, in the header's order, before anything is launched or written;
//   * a ROW is one (pair, answer); rows are independent, so the call runs in chunks of up to kTopBatchQuizzes rows wherever the pairs'
//     boundaries fall.  Per chunk: the quizzes' posteriors and the rows' sA / mD pointers through the pack list, ONE launch that leaves the
//     would-be posteriors in engine scratch and the likelihoods and entropies in the host-coherent result lines (preview_kernels.hip),
//     then the batched listing over the scratch rows (kb_kernels.hip: LaunchTopTargetsBatch) -- records and counts into the same lines.
// Nothing of size T crosses to the host and nothing of a quiz changes: the posteriors are only read.
// A shard that a process of its own drives answers for the pairs whose question it holds and leaves zeros for the others.
#include "hip_engine_internal.h"

namespace pqa {

static_assert(sizeof(PreviewRow) == 3 * sizeof(int64_t), "the rows travel in the answered-question buffer");

Error HipEngine::ValidatePreviewLocked(int64_t nPairs, const int64_t *pQuizzes, const int64_t *pQuestions) {
  Error err = CheckRegular("preview answers");
  if (!err.ok()) return err;
  for (int64_t i = 0; i < nPairs; i++)
    if (!UseQuiz(err, pQuizzes[i])) {
      err.params = "entry=" + std::to_string(i) + " quizId=" + std::to_string(pQuizzes[i]) + (err.hasParams ? " " + err.params : std::string());
      err.hasParams = true;
      return err;
    }
  for (int64_t i = 0; i < nPairs; i++) {
    const int64_t id = pQuestions[i];
    const std::string where = "entry=" + std::to_string(i) + " questionId=" + std::to_string(id);
    if (id < 0 || id >= _qTotal) return Error::MakeP(ErrCode::IndexOutOfRange, where + " " + RangeParams(id, 0, _qTotal - 1), "A previewed question is out of range.");
    if (OwnsQuestion(id) && BitTest(_hQGap, id - _qFirst)) return Error::MakeP(ErrCode::IndexOutOfRange, where, "A previewed question is a gap.");
  }
  return Error();
}

Error HipEngine::PreviewAnswersBatch(int64_t nPairs, const int64_t *pQuizzes, const int64_t *pQuestions, int64_t maxCount, double *pLikelihood, double *pEntropy,
                                     CiRatedTarget *pDest, int64_t *pCounts) {
  if (nPairs < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nPairs), "|nPairs| must be non-negative.");
  if (maxCount < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(maxCount), "|maxCount| must be non-negative.");
  if (maxCount > 256) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(maxCount, 0, 256), "A preview lists at most 256 targets per answer.");
  if (nPairs > 0 && (!pQuizzes || !pQuestions || (maxCount > 0 && (!pDest || !pCounts)))) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = ValidatePreviewLocked(nPairs, pQuizzes, pQuestions);
  if (!err.ok() || nPairs == 0) return err;
  // ---- the rows this engine holds, in call order; every other row is zeros
  const int64_t nRowsAll = nPairs * _K;
  struct Held { const double *prior; int64_t qLocal, row; };   // row: the pair's first row in the call
  std::vector<Held> held;
  for (int64_t i = 0; i < nPairs; i++) {
    const Quiz *q = UseQuiz(err, pQuizzes[i]);
    if (!q) return err;
    if (OwnsQuestion(pQuestions[i])) held.push_back(Held{q->dPrior, pQuestions[i] - _qFirst, i * _K});
  }
  _previewCalls++;
  _previewPairs += (uint64_t)held.size();
  for (int64_t r = 0; r < nRowsAll; r++) {
    if (pLikelihood) pLikelihood[r] = 0.0;
    if (pEntropy) pEntropy[r] = 0.0;
    if (pCounts) pCounts[r] = 0;
  }
  if (held.empty() || (maxCount == 0 && !pLikelihood && !pEntropy)) return Error();
  hipSetDevice(_device);
  err = FlushUpdates();   // (the pairs' quizzes' deferred answers: their posteriors are read below)
  if (!err.ok()) return err;
  if (_serverLaunched) StopServer();   // a launched kernel has no room beside the resident sweep and would wait for it to idle out

  const KbView kb = View();
  const int64_t nLoose = std::max<int64_t>(1, _opt.workers - 1);   // RecordAnswer's split: reference PqaCore/CEQuiz.h:98, PqaCore/BaseCpuEngine.cpp:22
  const int64_t nRows = (int64_t)held.size() * _K, group = std::min<int64_t>(nRows, kTopBatchQuizzes), want = std::min<int64_t>(maxCount, _T);
  const bool list = maxCount > 0;
  PreviewStage &st = _preview;
  if (list || !PreviewStagesInLds(kb, nLoose)) HIP_TRY(GrowDevice(&st.dRows, st.rowsBytes, (size_t)(group * _ldT) * sizeof(double)));
  if (list) {
    err = EnsureTopScratch(group, want);
    if (!err.ok()) return err;
  }
  HIP_TRY(st.lines.Ensure(_stream, std::max<int64_t>(1, group * want), 2 * sizeof(double), kTopBatchQuizzes, hipHostMallocDefault));   // records | counts | likelihoods, entropies
  RatedTargetDev *const hLines = st.lines.records;
  int64_t *const hCounts = st.lines.Counts();
  double *const hLikelihood = st.lines.Tail<double>(), *const hEntropy = hLikelihood + kTopBatchQuizzes;
  TopBatchPriors pr;
  for (int64_t first = 0; first < nRows; first += group) {
    const int64_t m = std::min<int64_t>(group, nRows - first);
    // the list: {arrival counter, pad} and then a PreviewRow per row of the chunk
    const int64_t words = 2 + 3 * m;
    err = EnsurePackList(words);
    if (!err.ok()) return err;
    PreviewRow *rows = reinterpret_cast<PreviewRow *>(_hPack + 2);
    for (int64_t j = 0; j < m; j++) {
      const Held &h = held[(size_t)((first + j) / _K)];
      rows[j] = PreviewRow{h.prior, CubeAt(h.qLocal, (first + j) % _K), CubeAt(h.qLocal, _K)};
      pr.prior[j] = st.dRows + j * _ldT;
    }
    MarkStreamBusy();
    err = SubmitPackList(words);
    if (!err.ok()) return err;
    TimerStart(st.ev);
    HIP_TRY(LaunchPreviewRows(kb, reinterpret_cast<const PreviewRow *>(_dAqs + 2), m, nLoose, st.dRows, _ldT, list, hLikelihood, hEntropy, _stream));
    if (list) HIP_TRY(LaunchTopTargetsBatch(kb, pr, m, want, _dTopScratch[0], _dTopScratch[1], hLines, hCounts, nullptr, 0, _stream));
    TimerStop(st.ev, _previewDeviceNs);
    HIP_TRY(hipStreamSynchronize(_stream));
    for (int64_t j = 0; j < m; j++) {
      const int64_t r = held[(size_t)((first + j) / _K)].row + (first + j) % _K;
      if (pLikelihood) pLikelihood[r] = hLikelihood[j];
      if (pEntropy) pEntropy[r] = hEntropy[j];
      if (!list) continue;
      const int64_t c = std::max<int64_t>(0, std::min<int64_t>(hCounts[j], want));
      pCounts[r] = c;
      std::memcpy(pDest + r * maxCount, hLines + j * want, (size_t)c * sizeof(RatedTargetDev));
    }
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  _pendingRecordOp = 0;
  return Error();
}

}  // namespace pqa
