// hip_engine_status.cpp -- HipEngine::QuizStatusBatch and HipEngine::RankTargetsBatch (hip_engine.h, include/PqaHipExt.h): where a quiz
// stands -- entropy, mass, best target, number of candidates and the candidates above given levels -- and where named targets stand in it.
//   * validation: everything a call can be refused for, in the header's order, before anything is launched or written;
//   * a status call runs in chunks of up to kTopBatchQuizzes quizzes: ONE launch per chunk (status_kernels.hip: LaunchQuizStatus), a
//     workgroup per quiz, a line of kStatusLineWords words per quiz in the host-coherent result lines, one synchronisation;
//   * a rank call groups its pairs into tiles of up to kRankTile named targets of one quiz (status_plan.h) and runs in chunks of up to
//     kTopBatchQuizzes tiles: the tiles and their targets through the pack list, ONE launch (LaunchRankTargets), a {rank, probability}
//     record per pair in the result lines, one synchronisation, the records scattered back to the pairs' places in the call.
// Nothing of size T crosses to the host and nothing of a quiz changes: the posteriors are only read.  A quiz's outputs depend on that
// quiz (and the levels) alone.  Every shard holds every posterior whole, so a shard answers like a whole engine.
#include "hip_engine_internal.h"
#include "status_plan.h"

#include <cmath>

namespace pqa {

static_assert(sizeof(RankTile) == 2 * sizeof(int64_t), "the tiles travel in the answered-question buffer, two words each");
static_assert(sizeof(CiHipQuizStatus) == 40, "the status record of include/PqaHipExt.h");

// What both calls can be refused for once their counts and buffers have passed: the mode, an unknown quiz, a target out of range.
Error HipEngine::ValidateStatusLocked(const char *what, int64_t n, const int64_t *pQuizzes, const int64_t *pTargets) {
  Error err = CheckRegular(what);
  if (!err.ok()) return err;
  for (int64_t i = 0; i < n; i++)
    if (!UseQuiz(err, pQuizzes[i])) {
      err.params = "entry=" + std::to_string(i) + " quizId=" + std::to_string(pQuizzes[i]) + (err.hasParams ? " " + err.params : std::string());
      err.hasParams = true;
      return err;
    }
  for (int64_t i = 0; pTargets && i < n; i++) {
    const int64_t id = pTargets[i];
    if (id < 0 || id >= _T)
      return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(i) + " targetId=" + std::to_string(id) + " " + RangeParams(id, 0, _T - 1),
                          "A named target is out of range.");
  }
  return Error();
}

Error HipEngine::QuizStatusBatch(int64_t nQuizzes, const int64_t *pQuizzes, int64_t nLevels, const double *pLevels, CiHipQuizStatus *pStatus, int64_t *pLevelCounts,
                                 double *pLevelMass) {
  if (nQuizzes < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nQuizzes), "|nQuizzes| must be non-negative.");
  if (nLevels < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nLevels), "|nLevels| must be non-negative.");
  if (nLevels > kStatusLevels) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(nLevels, 0, kStatusLevels), "A status call takes at most 16 levels.");
  if ((nQuizzes > 0 && (!pQuizzes || !pStatus)) || (nLevels > 0 && (!pLevels || (nQuizzes > 0 && !pLevelCounts && !pLevelMass))))
    return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  StatusLevels lv{};
  lv.n = (int32_t)nLevels;
  for (int64_t j = 0; j < nLevels; j++) {
    if (std::isnan(pLevels[j])) return Error::MakeP(ErrCode::IndexOutOfRange, "level=" + std::to_string(j), "A level is not a number.");
    lv.level[j] = pLevels[j];
  }
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = ValidateStatusLocked("quiz status", nQuizzes, pQuizzes, nullptr);
  if (!err.ok() || nQuizzes == 0) return err;
  _statusCalls++;
  _statusQuizzes += (uint64_t)nQuizzes;
  hipSetDevice(_device);
  err = FlushUpdates();   // (the quizzes' deferred answers: their posteriors are read below)
  if (!err.ok()) return err;
  if (_serverLaunched) StopServer();   // a launched kernel has no room beside the resident sweep and would wait for it to idle out

  const KbView kb = View();
  StatusStage &st = _status;
  HIP_TRY(st.lines.Ensure(_stream, 1, (size_t)kStatusLineWords * sizeof(int64_t) - sizeof(int64_t), kTopBatchQuizzes, hipHostMallocDefault));
  int64_t *const hLines = st.lines.Counts();   // kTopBatchQuizzes lines of kStatusLineWords words
  TopBatchPriors pr;
  for (int64_t first = 0; first < nQuizzes; first += kTopBatchQuizzes) {
    const int64_t m = std::min<int64_t>(kTopBatchQuizzes, nQuizzes - first);
    for (int64_t j = 0; j < m; j++) {
      const Quiz *q = UseQuiz(err, pQuizzes[first + j]);
      if (!q) return err;
      pr.prior[j] = q->dPrior;
    }
    MarkStreamBusy();
    TimerStart(st.ev);
    HIP_TRY(LaunchQuizStatus(kb, pr, m, lv, hLines, _stream));
    TimerStop(st.ev, _statusDeviceNs);
    HIP_TRY(hipStreamSynchronize(_stream));
    for (int64_t j = 0; j < m; j++) {
      const int64_t *line = hLines + j * kStatusLineWords;
      CiHipQuizStatus &s = pStatus[first + j];
      std::memcpy(&s._entropy, line + 0, 8);
      std::memcpy(&s._mass, line + 1, 8);
      std::memcpy(&s._topProb, line + 2, 8);
      s._iTopTarget = line[3];
      s._nCandidates = line[4];
      if (pLevelCounts) std::memcpy(pLevelCounts + (first + j) * nLevels, line + kStatusLineCounts, (size_t)nLevels * sizeof(int64_t));
      if (pLevelMass) std::memcpy(pLevelMass + (first + j) * nLevels, line + kStatusLineMasses, (size_t)nLevels * sizeof(double));
    }
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  _pendingRecordOp = 0;
  return Error();
}

Error HipEngine::RankTargetsBatch(int64_t nPairs, const int64_t *pQuizzes, const int64_t *pTargets, double *pProb, int64_t *pRank) {
  if (nPairs < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nPairs), "|nPairs| must be non-negative.");
  if (nPairs > 0 && (!pQuizzes || !pTargets || !pProb || !pRank)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = ValidateStatusLocked("rank targets", nPairs, pQuizzes, pTargets);
  if (!err.ok() || nPairs == 0) return err;
  _rankCalls++;
  _rankPairs += (uint64_t)nPairs;
  hipSetDevice(_device);
  err = FlushUpdates();
  if (!err.ok()) return err;
  if (_serverLaunched) StopServer();

  const KbView kb = View();
  const RankTiles plan = PlanRankTiles(nPairs, pQuizzes, kRankTile);
  StatusStage &st = _status;
  HIP_TRY(st.rankLines.Ensure(_stream, (int64_t)kTopBatchQuizzes * kRankTile, 0, 0, hipHostMallocDefault));
  RatedTargetDev *const hRecords = st.rankLines.records;
  for (int64_t first = 0; first < plan.Tiles(); first += kTopBatchQuizzes) {
    const int64_t m = std::min<int64_t>(kTopBatchQuizzes, plan.Tiles() - first);
    const int64_t base = plan.start[(size_t)first], nIds = plan.start[(size_t)(first + m)] - base;
    // the list: {arrival counter, pad}, a RankTile per tile of the chunk, then the chunk's named targets as int32
    const int64_t words = 2 + 2 * m + (nIds + 1) / 2;
    err = EnsurePackList(words);
    if (!err.ok()) return err;
    RankTile *tiles = reinterpret_cast<RankTile *>(_hPack + 2);
    int32_t *ids = reinterpret_cast<int32_t *>(_hPack + 2 + 2 * m);
    for (int64_t j = 0; j < m; j++) {
      const int64_t a = plan.start[(size_t)(first + j)], b = plan.start[(size_t)(first + j + 1)];
      const Quiz *q = UseQuiz(err, pQuizzes[plan.order[(size_t)a]]);
      if (!q) return err;
      tiles[j] = RankTile{q->dPrior, (int32_t)(a - base), (int32_t)(b - a)};
    }
    for (int64_t k = 0; k < nIds; k++) ids[k] = (int32_t)pTargets[plan.order[(size_t)(base + k)]];
    if (nIds & 1) ids[nIds] = 0;
    MarkStreamBusy();
    err = SubmitPackList(words);
    if (!err.ok()) return err;
    TimerStart(st.ev);
    HIP_TRY(LaunchRankTargets(kb, reinterpret_cast<const RankTile *>(_dAqs + 2), m, reinterpret_cast<const int32_t *>(_dAqs + 2 + 2 * m), hRecords, _stream));
    TimerStop(st.ev, _statusDeviceNs);
    HIP_TRY(hipStreamSynchronize(_stream));
    for (int64_t k = 0; k < nIds; k++) {
      const int64_t i = plan.order[(size_t)(base + k)];
      pRank[i] = hRecords[k].iTarget;
      pProb[i] = hRecords[k].prob;
    }
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  _pendingRecordOp = 0;
  return Error();
}

}  // namespace pqa
