// hip_engine_review.cpp -- HipEngine::GetQuizAnswers and HipEngine::ReviewAnswersBatch / ReviewAnswersBatchFromRows (hip_engine.h,
// include/PqaHipExt.h): for many (quiz, position) pairs, the quiz as if the answer at that position had never been given -- the
// likelihood of the left-out answer under the posterior of the others, that posterior's entropy and its best targets.
//   * validation: everything a call can be refused for, in the header's order, before anything is launched or written;
//   * a ROW is one pair.  The rows go in chunks (review_plan.h: a quiz's rows together where they fit, at most kTopBatchQuizzes rows,
//     the chunk's scratch within kReviewBudget).  Per chunk: the quizzes' row pointers, their requests and the rows' left-out row pairs
//     through the pack list; the chains kernel (a workgroup per tile of targets and distinct quiz: ratios once, prefix once) and the rows
//     kernel (a workgroup per row: ResumeQuiz's normalisation, entropy, likelihood) of review_kernels.hip; the batched listing over the
//     divided rows (kb_kernels.hip: LaunchTopTargetsBatch); one synchronisation.
// Nothing of size T crosses to the host and nothing of a quiz changes: the review reads the knowledge base and Quiz::answers only.
#include "hip_engine_internal.h"
#include "review_plan.h"

namespace pqa {

namespace {
// Scratch a chunk may take (rows' mantissas and exponent sums, spilled ratios): as hip_engine_resume.cpp's kResumeExpsBudget
constexpr int64_t kReviewBudget = (int64_t)64 << 20;
static_assert(sizeof(ReviewRow) == 3 * sizeof(int64_t) && sizeof(ReviewQuiz) == 5 * sizeof(int64_t) && sizeof(ReviewRequest) == sizeof(int64_t),
              "the tables travel in the pack list as 8-byte words");
}  // namespace

int64_t HipEngine::GetQuizAnswers(Error &err, int64_t iQuiz, AQ *pDest, int64_t capacity) {
  if (capacity < 0) {
    err = Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(capacity), "|capacity| must be non-negative.");
    return -1;
  }
  if (capacity > 0 && pDest == nullptr) {
    err = Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the answers' destination.");
    return -1;
  }
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  const Quiz *q = UseQuiz(err, iQuiz);
  if (!q) return -1;
  const int64_t n = (int64_t)q->answers.size();
  std::copy(q->answers.begin(), q->answers.begin() + (std::ptrdiff_t)std::min(n, capacity), pDest);
  return n;
}

Error HipEngine::ReviewAnswersBatch(int64_t nPairs, const int64_t *pQuizzes, const int64_t *pPositions, int64_t maxCount, double *pLikelihood, double *pEntropy,
                                    CiRatedTarget *pDest, int64_t *pCounts) {
  return ReviewAnswers(nPairs, pQuizzes, pPositions, maxCount, pLikelihood, pEntropy, pDest, pCounts, false, nullptr, nullptr);
}

Error HipEngine::ReviewAnswersBatchFromRows(int64_t nPairs, const int64_t *pQuizzes, const int64_t *pPositions, int64_t maxCount, double *pLikelihood,
                                            double *pEntropy, CiRatedTarget *pDest, int64_t *pCounts, const void *pRows, const int64_t *pRowFirst) {
  return ReviewAnswers(nPairs, pQuizzes, pPositions, maxCount, pLikelihood, pEntropy, pDest, pCounts, true, pRows, pRowFirst);
}

Error HipEngine::ReviewAnswers(int64_t nPairs, const int64_t *pQuizzes, const int64_t *pPositions, int64_t maxCount, double *pLikelihood, double *pEntropy,
                               CiRatedTarget *pDest, int64_t *pCounts, bool fromRows, const void *pRows, const int64_t *pRowFirst) {
  if (nPairs < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nPairs), "|nPairs| must be non-negative.");
  if (maxCount < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(maxCount), "|maxCount| must be non-negative.");
  if (maxCount > 256) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(maxCount, 0, 256), "A review lists at most 256 targets per row.");
  if (nPairs > 0 && (!pQuizzes || !pPositions || (fromRows && !pRowFirst) || (maxCount > 0 && (!pDest || !pCounts))))
    return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = CheckRegular("review answers");
  if (!err.ok()) return err;
  std::vector<const Quiz *> quizOf((size_t)nPairs);
  std::vector<int64_t> answersOf((size_t)nPairs);
  for (int64_t i = 0; i < nPairs; i++) {
    quizOf[(size_t)i] = UseQuiz(err, pQuizzes[i]);
    if (!quizOf[(size_t)i]) {
      err.params = "entry=" + std::to_string(i) + " quizId=" + std::to_string(pQuizzes[i]) + (err.hasParams ? " " + err.params : std::string());
      err.hasParams = true;
      return err;
    }
    answersOf[(size_t)i] = (int64_t)quizOf[(size_t)i]->answers.size();
  }
  for (int64_t i = 0; i < nPairs; i++) {
    const int64_t n = answersOf[(size_t)i], at = pPositions[i];
    if (at < 0 || at >= n)
      return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(i) + " position=" + std::to_string(at) + " " + RangeParams(at, 0, n - 1),
                          "A reviewed position is not among the quiz's answers.");
    if (fromRows && pRowFirst[i] < 0)
      return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(i) + " rowFirst=" + std::to_string(pRowFirst[i]), "A package slot is negative.");
  }
  // an answered question another shard holds: its rows come in a package or not at all.  The left-out answer's rows are needed for
  // the likelihood alone.
  bool anyForeign = false;
  for (int64_t i = 0; i < nPairs; i++) {
    const std::vector<AQ> &aqs = quizOf[(size_t)i]->answers;
    for (int64_t j = 0; j < (int64_t)aqs.size(); j++) {
      if (OwnsQuestion(aqs[(size_t)j].iQuestion) || (j == pPositions[i] && !pLikelihood)) continue;
      anyForeign = true;
      if (!fromRows)
        return Error::MakeP(ErrCode::NotImplemented, "Feature=ResumeQuiz across separately driven shards",
                            "An answered question belongs to another shard: its rows are not reachable from this engine alone "
                            "(PqaEngine_ReviewAnswersBatchFromRows takes them from a package).");
    }
  }
  if (anyForeign && pRows == nullptr) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the row package.");
  if (nPairs == 0) return Error();
  _reviewCalls++;
  _reviewRows += (uint64_t)nPairs;
  if (maxCount == 0 && !pLikelihood && !pEntropy) return Error();
  hipSetDevice(_device);
  if (_serverLaunched) StopServer();   // a launched kernel has no room beside the resident sweep and would wait for it to idle out

  // ---- the package's slots: one pointer pair per slot that holds another engine's question (a host package staged first, option "rows_stage")
  std::vector<const void *> slotRows;
  if (anyForeign) {
    int64_t nSlots = 0;
    for (int64_t i = 0; i < nPairs; i++) nSlots = std::max(nSlots, pRowFirst[i] + answersOf[(size_t)i]);
    std::vector<AQ> slotAQ((size_t)nSlots, AQ{_qFirst, 0});   // (a slot nothing foreign lies in counts as this engine's own: neither staged nor read)
    for (int64_t i = 0; i < nPairs; i++)
      for (int64_t j = 0; j < answersOf[(size_t)i]; j++)
        if (!OwnsQuestion(quizOf[(size_t)i]->answers[(size_t)j].iQuestion)) slotAQ[(size_t)(pRowFirst[i] + j)] = quizOf[(size_t)i]->answers[(size_t)j];
    err = PackageRowsLocked(nSlots, slotAQ.data(), pRows, slotRows);
    if (!err.ok()) return err;
  }
  auto rowPair = [&](int64_t pair, int64_t j, const void *&rowA, const void *&rowD) {
    const AQ aq = quizOf[(size_t)pair]->answers[(size_t)j];
    if (OwnsQuestion(aq.iQuestion)) {
      rowA = CubeAt(aq.iQuestion - _qFirst, aq.iAnswer);
      rowD = CubeAt(aq.iQuestion - _qFirst, _K);
    } else if (anyForeign) {
      rowA = slotRows[2 * (size_t)(pRowFirst[pair] + j)];
      rowD = slotRows[2 * (size_t)(pRowFirst[pair] + j) + 1];
    } else {
      rowA = rowD = nullptr;   // (a left-out answer of another shard without a likelihood asked for: never read)
    }
  };

  // ---- the chunks, and the scratch of the largest
  const std::vector<std::vector<int64_t>> chunks = PlanReviewChunks(nPairs, pQuizzes, answersOf.data(), _ldT, kTopBatchQuizzes, kReviewBudget, kReviewLdsAnswers);
  struct ChunkQuiz { int64_t first, count; };   // a run of the chunk's pairs that share a quiz
  auto quizRuns = [&](const std::vector<int64_t> &chunk) {
    std::vector<ChunkQuiz> runs;
    for (size_t j = 0; j < chunk.size(); j++)
      if (j == 0 || pQuizzes[chunk[j]] != pQuizzes[chunk[j - 1]]) runs.push_back(ChunkQuiz{(int64_t)j, 1});
      else runs.back().count++;
    return runs;
  };
  int64_t maxRows = 0, maxSpill = 0;
  for (const std::vector<int64_t> &chunk : chunks) {
    maxRows = std::max<int64_t>(maxRows, (int64_t)chunk.size());
    int64_t spill = 0;
    for (const ChunkQuiz &r : quizRuns(chunk)) spill += ReviewSpillBytes(answersOf[(size_t)chunk[(size_t)r.first]], _ldT, kReviewLdsAnswers);
    maxSpill = std::max(maxSpill, spill);
  }
  const KbView kb = View();
  const bool list = maxCount > 0;
  const int64_t want = std::min<int64_t>(maxCount, _T);
  ReviewStage &st = _review;
  HIP_TRY(GrowDevice(&st.dRows, st.rowsBytes, (size_t)(maxRows * ReviewRowBytes(_ldT))));
  if (maxSpill > 0) HIP_TRY(GrowDevice(&st.dRatios, st.ratiosBytes, (size_t)maxSpill));
  if (list) {
    err = EnsureTopScratch(maxRows, want);
    if (!err.ok()) return err;
  }
  HIP_TRY(st.lines.Ensure(_stream, std::max<int64_t>(1, maxRows * want), 2 * sizeof(double), kTopBatchQuizzes, hipHostMallocDefault));   // records | counts | likelihoods, entropies
  RatedTargetDev *const hLines = st.lines.records;
  int64_t *const hCounts = st.lines.Counts();
  double *const hLikelihood = st.lines.Tail<double>(), *const hEntropy = hLikelihood + kTopBatchQuizzes;
  TopBatchPriors pr;
  for (const std::vector<int64_t> &chunk : chunks) {
    const int64_t m = (int64_t)chunk.size();
    const std::vector<ChunkQuiz> runs = quizRuns(chunk);
    const int64_t nq = (int64_t)runs.size();
    int64_t nPointers = 0, ldsAnswers = 0;
    for (const ChunkQuiz &r : runs) {
      const int64_t n = answersOf[(size_t)chunk[(size_t)r.first]];
      nPointers += 2 * n;
      if (n <= kReviewLdsAnswers) ldsAnswers = std::max(ldsAnswers, n);
    }
    // the list: {arrival counter, pad}, a ReviewRow per row, a ReviewQuiz per distinct quiz, a ReviewRequest per row, the quizzes' row pointers
    const int64_t offRows = 2, offQuizzes = offRows + 3 * m, offRequests = offQuizzes + 5 * nq, offPointers = offRequests + m, words = offPointers + nPointers;
    err = EnsurePackList(words);
    if (!err.ok()) return err;
    ReviewRow *rows = reinterpret_cast<ReviewRow *>(_hPack + offRows);
    ReviewQuiz *quizzes = reinterpret_cast<ReviewQuiz *>(_hPack + offQuizzes);
    ReviewRequest *requests = reinterpret_cast<ReviewRequest *>(_hPack + offRequests);
    const void **pointers = reinterpret_cast<const void **>(_hPack + offPointers);
    double *const dMants = st.dRows;
    int64_t *const dExps = reinterpret_cast<int64_t *>(st.dRows + maxRows * _ldT);
    int64_t atPointer = 0, atSpill = 0;
    for (int64_t k = 0; k < nq; k++) {
      const ChunkQuiz &r = runs[(size_t)k];
      const int64_t lead = chunk[(size_t)r.first], n = answersOf[(size_t)lead];
      // the requests of this quiz, position ascending (rows of equal positions in chunk order)
      std::vector<int64_t> order((size_t)r.count);
      for (int64_t j = 0; j < r.count; j++) order[(size_t)j] = r.first + j;
      std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return pPositions[chunk[(size_t)x]] < pPositions[chunk[(size_t)y]]; });
      for (int64_t j = 0; j < r.count; j++) requests[r.first + j] = ReviewRequest{(int32_t)pPositions[chunk[(size_t)order[(size_t)j]]], (int32_t)order[(size_t)j]};
      for (int64_t j = 0; j < n; j++) rowPair(lead, j, pointers[atPointer + 2 * j], pointers[atPointer + 2 * j + 1]);
      // (a left-out answer of another shard whose rows nobody needs: then it is the quiz's only requested position, its ratio enters
      //  no chain that is written, and the chains kernel divides some rows of this engine's in its place)
      for (int64_t j = 0; j < n; j++)
        if (pointers[atPointer + 2 * j] == nullptr) {
          pointers[atPointer + 2 * j] = CubeAt(0, 0);
          pointers[atPointer + 2 * j + 1] = CubeAt(0, _K);
        }
      const int64_t spill = ReviewSpillBytes(n, _ldT, kReviewLdsAnswers);
      quizzes[k] = ReviewQuiz{reinterpret_cast<const void *const *>(_dAqs + offPointers + atPointer), reinterpret_cast<const ReviewRequest *>(_dAqs + offRequests + r.first),
                              spill > 0 ? st.dRatios + atSpill / (int64_t)sizeof(double) : nullptr, n, r.count};
      atPointer += 2 * n;
      atSpill += spill;
    }
    for (int64_t j = 0; j < m; j++) {
      const int64_t pair = chunk[(size_t)j];
      rows[j].nRemaining = answersOf[(size_t)pair] - 1;
      rowPair(pair, pPositions[pair], rows[j].rowA, rows[j].rowD);
      pr.prior[j] = dMants + j * _ldT;
    }
    MarkStreamBusy();
    err = SubmitPackList(words);
    if (!err.ok()) return err;
    TimerStart(st.ev);
    HIP_TRY(LaunchReviewChains(kb, reinterpret_cast<const ReviewQuiz *>(_dAqs + offQuizzes), nq, ldsAnswers, _opt.bugCompat != 0, dMants, dExps, _ldT, _stream));
    HIP_TRY(LaunchReviewRows(kb, reinterpret_cast<const ReviewRow *>(_dAqs + offRows), m, _opt.workers, dMants, dExps, _ldT, pLikelihood ? hLikelihood : nullptr,
                             pEntropy ? hEntropy : nullptr, _stream));
    if (list) HIP_TRY(LaunchTopTargetsBatch(kb, pr, m, want, _dTopScratch[0], _dTopScratch[1], hLines, hCounts, nullptr, 0, _stream));
    TimerStop(st.ev, _reviewDeviceNs);
    HIP_TRY(hipStreamSynchronize(_stream));
    for (int64_t j = 0; j < m; j++) {
      const int64_t r = chunk[(size_t)j];
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
