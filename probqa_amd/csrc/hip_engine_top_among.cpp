// hip_engine_top_among.cpp -- HipEngine::ListTopTargetsAmongBatch (hip_engine.h, include/PqaHipExt.h): the best targets of many quizzes
// WITHIN A LISTED SET each, and the posterior's total over the set.  The lists are given once and the quizzes point at them.
//   * validation: everything a call can be refused for, before anything is launched or written (a stamp vector over T finds a target
//     twice in one list, as ValidateAmongLocked's over Q);
//   * staging, once per call: offsets[nLists + 1] | the ids as int32 (T < 2^31), one copy each; the buffers grow and never shrink;
//   * a quiz whose min(maxCount, its list's length) is at most 256 -- in groups of 256 quizzes: the gathering level 0 over a grid of
//     (chunks of the group's longest list, quiz), the partial sums added per quiz in a fixed order, the merges (kb_kernels.hip:
//     LaunchTopTargetsAmong); per quiz, records, a count and a mass come back in the host-coherent result lines;
//   * a quiz beyond that: the posteriors of its LIST gathered (sum of the lists' lengths doubles, never T per quiz) and selected here
//     under the same order -- probability descending, target ascending.
// Which of the two a quiz takes depends on maxCount and its own list only, so its records and its mass are the same bits whatever else
// is in the batch.  Nothing of a quiz changes.
#include "hip_engine_internal.h"

namespace pqa {

Error HipEngine::ValidateTopAmongLocked(int64_t n, const int64_t *pQuizzes, const int64_t *pListOf, int64_t nLists, const int64_t *pListCounts,
                                        const int64_t *pTargets, int64_t maxCount, bool haveDest, bool haveCounts) {
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "|nQuizzes| must be non-negative.");
  if (nLists < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nLists), "|nLists| must be non-negative.");
  if (maxCount < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(maxCount), "|maxCount| must be non-negative.");
  if ((n > 0 && (!pQuizzes || !haveCounts || (maxCount > 0 && !haveDest))) || (nLists > 0 && !pListCounts))
    return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  Error err = CheckRegular("list top targets among");
  if (!err.ok()) return err;
  if (!pListOf && nLists != n)
    return Error::MakeP(ErrCode::IndexOutOfRange, "nLists=" + std::to_string(nLists) + " nQuizzes=" + std::to_string(n),
                        "Without |pListOf| quiz i takes list i: there must be as many lists as quizzes.");
  int64_t total = 0;
  for (int64_t l = 0; l < nLists; l++) {
    if (pListCounts[l] < 0) return Error::MakeP(ErrCode::NegativeCount, "list=" + std::to_string(l) + " count=" + std::to_string(pListCounts[l]), "A list's length must be non-negative.");
    total += pListCounts[l];
  }
  if (total > 0 && !pTargets) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  for (int64_t i = 0; i < n; i++) {
    if (pListOf && (pListOf[i] < 0 || pListOf[i] >= nLists))
      return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(i) + " " + RangeParams(pListOf[i], 0, nLists - 1), "A quiz's list index is out of range.");
    if (!UseQuiz(err, pQuizzes[i])) {
      err.params = "entry=" + std::to_string(i) + " quizId=" + std::to_string(pQuizzes[i]) + (err.hasParams ? " " + err.params : std::string());
      err.hasParams = true;
      return err;
    }
  }
  std::vector<int64_t> &stamp = _topAmong.stamp;
  stamp.assign((size_t)_T, 0);
  int64_t at = 0;
  for (int64_t l = 0; l < nLists; l++)
    for (int64_t k = 0; k < pListCounts[l]; k++, at++) {
      const int64_t id = pTargets[at];
      if (id >= 0 && id < _T && stamp[(size_t)id] != l + 1) { stamp[(size_t)id] = l + 1; continue; }
      const std::string where = "list=" + std::to_string(l) + " position=" + std::to_string(k) + " targetId=" + std::to_string(id);
      if (id < 0 || id >= _T) return Error::MakeP(ErrCode::IndexOutOfRange, where + " " + RangeParams(id, 0, _T - 1), "A listed target is out of range.");
      return Error::MakeP(ErrCode::IndexOutOfRange, where, "A target appears twice in one list.");
    }
  return Error();
}

Error HipEngine::ListTopTargetsAmongBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pListOf, int64_t nLists, const int64_t *pListCounts,
                                          const int64_t *pTargets, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts, double *pMass) {
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = ValidateTopAmongLocked(n, pQuizzes, pListOf, nLists, pListCounts, pTargets, maxCount, pDest != nullptr, pCounts != nullptr);
  if (!err.ok() || n == 0) return err;
  TopAmongStage &st = _topAmong;
  st.offsets.assign((size_t)nLists + 1, 0);
  for (int64_t l = 0; l < nLists; l++) st.offsets[(size_t)l + 1] = st.offsets[(size_t)l] + pListCounts[l];
  const int64_t total = st.offsets[(size_t)nLists];
  auto listOf = [&](int64_t i) { return pListOf ? pListOf[i] : i; };
  // (a quiz with an empty list takes no part in any launch; maxCount == 0 lists nothing, the mass is computed all the same)
  std::vector<Quiz *> quizzes((size_t)n);
  std::vector<int64_t> small, large;   // positions in the batch
  for (int64_t i = 0; i < n; i++) {
    quizzes[(size_t)i] = UseQuiz(err, pQuizzes[i]);
    if (!quizzes[(size_t)i]) return err;
    pCounts[i] = 0;
    if (pMass) pMass[i] = 0.0;
    const int64_t len = pListCounts[listOf(i)];
    if (len == 0) continue;
    (std::min(maxCount, len) <= 256 ? small : large).push_back(i);
  }
  if (small.empty() && large.empty()) return Error();
  hipSetDevice(_device);
  err = FlushUpdates();
  if (!err.ok()) return err;
  StopServer();   // (thousands of workgroups: they would wait for a resident sweep to idle out)

  // ---- the lists, staged once: offsets | ids
  st.ids.resize((size_t)total);
  for (int64_t k = 0; k < total; k++) st.ids[(size_t)k] = (int32_t)pTargets[k];
  const size_t offBytes = ((size_t)(nLists + 1) * sizeof(int64_t) + 15) / 16 * 16, listBytes = offBytes + (size_t)total * sizeof(int32_t);
  HIP_TRY(GrowDevice(&st.dLists, st.listBytes, listBytes));
  const int64_t *dOffsets = static_cast<const int64_t *>(st.dLists);
  const int32_t *dIds = reinterpret_cast<const int32_t *>(static_cast<const char *>(st.dLists) + offBytes);
  HIP_TRY(hipMemcpyAsync(st.dLists, st.offsets.data(), (size_t)(nLists + 1) * sizeof(int64_t), hipMemcpyHostToDevice, _stream));
  HIP_TRY(hipMemcpyAsync(static_cast<char *>(st.dLists) + offBytes, st.ids.data(), (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, _stream));
  const KbView kb = View();
  TopBatchPriors pr;
  int32_t lists[kTopBatchQuizzes];

  // ---- up to 256 records a quiz: on the device
  for (size_t first = 0; first < small.size(); first += kTopBatchQuizzes) {
    const int64_t m = std::min<int64_t>(kTopBatchQuizzes, (int64_t)(small.size() - first));
    int64_t longest = 0;
    for (int64_t j = 0; j < m; j++) {
      const int64_t i = small[first + (size_t)j];
      pr.prior[j] = quizzes[(size_t)i]->dPrior;
      lists[j] = (int32_t)listOf(i);
      longest = std::max(longest, pListCounts[listOf(i)]);
    }
    const int64_t want = std::max<int64_t>(1, std::min(maxCount, longest));   // (<= 256: every quiz of the group asks for no more)
    err = EnsureTopScratchRecords(m * TopAmongScratchRecords(longest, want));
    if (!err.ok()) return err;
    HIP_TRY(GrowDevice(&st.dPartial, st.partialBytes, (size_t)(m * TopAmongPartials(longest)) * sizeof(double)));
    HIP_TRY(st.lines.Ensure(_stream, m * want, sizeof(double), kTopBatchQuizzes, hipHostMallocDefault));   // records | counts | masses
    RatedTargetDev *const hLines = st.lines.records;
    int64_t *const hCounts = st.lines.Counts();
    double *const hMass = st.lines.Tail<double>();
    HIP_TRY(LaunchTopTargetsAmong(kb, pr, lists, m, dOffsets, dIds, longest, want, _dTopScratch[0], _dTopScratch[1], st.dPartial, hLines, hCounts, hMass, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
    for (int64_t j = 0; j < m; j++) {
      const int64_t i = small[first + (size_t)j], c = std::min<int64_t>(std::min<int64_t>(hCounts[j], want), maxCount);
      pCounts[i] = c;
      std::memcpy(pDest + i * maxCount, hLines + j * want, (size_t)c * sizeof(RatedTargetDev));
      if (pMass) pMass[i] = hMass[j];
    }
  }

  // ---- longer listings: the lists' posteriors gathered, selected here.  A group: up to 256 quizzes and 4M gathered doubles (one quiz at least)
  constexpr int64_t kGatherBudget = 4 << 20;
  std::vector<double> pri;
  std::vector<int64_t> idx;
  for (size_t first = 0; first < large.size();) {
    int64_t m = 0, longest = 0;
    while (m < kTopBatchQuizzes && first + (size_t)m < large.size()) {
      const int64_t len = pListCounts[listOf(large[first + (size_t)m])], pitch = std::max(longest, len);
      if (m > 0 && pitch * (m + 1) > kGatherBudget) break;
      longest = pitch;
      m++;
    }
    for (int64_t j = 0; j < m; j++) {
      const int64_t i = large[first + (size_t)j];
      pr.prior[j] = quizzes[(size_t)i]->dPrior;
      lists[j] = (int32_t)listOf(i);
    }
    const size_t need = (size_t)(m * longest);
    HIP_TRY(GrowDevice(&st.dGather, st.gatherBytes, need * sizeof(double)));
    HIP_TRY(LaunchTopAmongGather(kb, pr, lists, m, dOffsets, dIds, longest, st.dGather, _stream));
    pri.resize(need);
    HIP_TRY(hipMemcpyAsync(pri.data(), st.dGather, need * sizeof(double), hipMemcpyDeviceToHost, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
    for (int64_t j = 0; j < m; j++) {
      const int64_t i = large[first + (size_t)j], len = pListCounts[listOf(i)];
      const int64_t *ids = pTargets + st.offsets[(size_t)listOf(i)];
      const double *p = pri.data() + (size_t)(j * longest);
      double mass = 0.0;
      for (int64_t k = 0; k < len; k++)
        if (p[k] > 0.0) mass += p[k];   // (list order: fixed)
      // ties by the listed id, whatever the list's order
      pCounts[i] = RatedPrefix(p, len, maxCount, [](int64_t) { return true; }, [&](int64_t k) { return ids[k]; }, pDest + i * maxCount, idx);
      if (pMass) pMass[i] = mass;
    }
    first += (size_t)m;
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  _pendingRecordOp = 0;
  return Error();
}

}  // namespace pqa
