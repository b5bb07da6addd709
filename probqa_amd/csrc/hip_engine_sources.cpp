// hip_engine_sources.cpp -- HipEngine: the source queries (hip_engine.h: SourceStage; include/PqaHipExt.h), three families over one skeleton.
// Target similarity -- EvalTargetSimilarity, ListSimilarTargetsBatch, and the pair for shards that processes of their own drive,
// PackTargetSimilaritySums / ListSimilarTargetsFromSums: sim(s, t) = (sum over the questions of the WHOLE knowledge base that are not
// gaps of sum_k sqrt(p_qk(s) p_qk(t))) / nValidQuestions, p_qk(t) = A[q][k][t] / D[q][t]: 1 for targets no quiz can tell apart.
// Question redundancy -- EvalQuestionRedundancy, ListRedundantQuestionsBatch, PackQuestionWeights / EvalQuestionRedundancyFromWeights /
// ListRedundantQuestionsFromWeights: I(s, q), the mutual information in bits between the answers to questions s and q for a target
// drawn from vB, over the K x K table J[k][k'] = sum_t (w[t] p_sk(t)) p_qk'(t).
// Target separation -- EvalTargetSeparation, ListSeparatingQuestionsBatch: sep(G, q), the Jensen-Shannon divergence in bits of the answer
// distributions of a GROUP G of 2 .. 64 listed targets at question q, equal weights.  A value needs the group's columns of q's block and
// nothing else: there is no package, the family's "pack" (StageGroupsLocked) stages a chunk's groups and the sweep's tiles on the device,
// and a shard that a process of its own drives answers for its own questions directly.
// One code path per family: PackSourcesLocked enqueues, per up to 256 sources, this engine's part of a package; SourceRowsLocked turns
// a package -- the engine's own, or the ranks' summed one -- into rows on the device; ListSourcesLocked lists them on the device, or
// copies them and takes the prefix here beyond 256 records.  A whole engine's Eval and List are pack -> rows and pack -> list, in
// chunks of 256 sources.  What a family does its own way is three launches: the pack's, the rows' and the device listing's.
// The calls read only the knowledge base: they work in regular and in maintenance mode and change no quiz.  Everything a call can be
// refused for is decided before anything is launched or written, in one order for both families.
#include "hip_engine_internal.h"

namespace pqa {

namespace {
// What does not need the engine: the counts, the `limit` of sources of the pack / from-package calls (0: none), the buffers, and the
// package's alignment (nullptr where a call has none).
Error SourceArgs(int64_t nSources, int64_t maxCount, int64_t limit, bool haveBuffers, const char *nullText, const void *package, const char *countName = "nSources") {
  if (nSources < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nSources), std::string("|") + countName + "| must be non-negative.");
  if (maxCount < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(maxCount), "|maxCount| must be non-negative.");
  if (limit > 0 && nSources > limit) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(nSources, 0, limit), "Batch size is out of range.");
  if (nSources > 0 && !haveBuffers) return Error::Make(ErrCode::NullArgument, nullText);
  if ((reinterpret_cast<uintptr_t>(package) & 15) != 0)
    return Error::MakeP(ErrCode::IndexOutOfRange, "address mod 16=" + std::to_string(reinterpret_cast<uintptr_t>(package) & 15), "The package must be 16-byte aligned.");
  return Error();
}
constexpr const char *kSimilarityShardAdvice = "Sum the ranks' PqaHip_PackTargetSimilaritySums packages and list with PqaEngine_ListSimilarTargetsFromSums instead.";
constexpr const char *kRedundancyShardAdvice =
    "Sum the ranks' PqaHip_PackQuestionWeights packages and use PqaEngine_EvalQuestionRedundancyFromWeights / "
    "PqaEngine_ListRedundantQuestionsFromWeights instead.";
constexpr const char *kNullBatch = "Nullptr is passed in place of a batch buffer.";
constexpr const char *kNullBatchOrPackage = "Nullptr is passed in place of a batch buffer or the package.";
}  // namespace

// What a call is refused for under the lock: a sharded engine's shard (wholeOnly), the row length (rowLength >= 0), shutdown, a source
// out of range.
Error HipEngine::AdmitSourcesLocked(const SourceStage &st, const char *call, bool wholeOnly, int64_t rowLength, int64_t n, const int64_t *pSources) const {
  if (wholeOnly && IsShard())
    return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + call + " of a sharded engine", st.questions ? kRedundancyShardAdvice : kSimilarityShardAdvice);
  const int64_t results = st.questions ? _Q : _T, limit = st.questions ? _qTotal : _T;
  if (rowLength >= 0 && rowLength != results)
    return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(rowLength, results, results),
                        st.questions ? "Redundancy row length must equal the question count." : "Similarity row length must equal the target count.");
  if (_mode == Mode::Shutdown) return Error::MakeP(ErrCode::ObjectShutDown, std::string("RejectedOperation=") + call, "Engine is shut down.");
  for (int64_t i = 0; i < n; i++)
    if (pSources[i] < 0 || pSources[i] >= limit)
      return Error::MakeP(ErrCode::IndexOutOfRange,
                          "entry=" + std::to_string(i) + (st.questions ? " questionId=" : " targetId=") + std::to_string(pSources[i]) + " " + RangeParams(pSources[i], 0, limit - 1),
                          st.questions ? "A source question is out of range." : "A source target is out of range.");
  return Error();
}

// The groups family's refusals under the lock, in its one order: a group's count, a target, the row length (rowLength >= 0), shutdown.
Error HipEngine::AdmitGroupsLocked(const char *call, int64_t rowLength, int64_t n, const int64_t *pGroupCounts, const int64_t *pTargets) const {
  for (int64_t g = 0; g < n; g++)
    if (pGroupCounts[g] < 2 || pGroupCounts[g] > kSepMaxGroup)
      return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(g) + " count=" + std::to_string(pGroupCounts[g]) + " " + RangeParams(pGroupCounts[g], 2, kSepMaxGroup),
                          "A group's target count is out of range.");
  for (int64_t g = 0, at = 0; g < n; g++)
    for (int64_t j = 0; j < pGroupCounts[g]; j++, at++)
      if (pTargets[at] < 0 || pTargets[at] >= _T)
        return Error::MakeP(ErrCode::IndexOutOfRange,
                            "entry=" + std::to_string(g) + " member=" + std::to_string(j) + " targetId=" + std::to_string(pTargets[at]) + " " + RangeParams(pTargets[at], 0, _T - 1),
                            "A group's target is out of range.");
  if (rowLength >= 0 && rowLength != _Q)
    return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(rowLength, _Q, _Q), "Separation row length must equal the question count.");
  if (_mode == Mode::Shutdown) return Error::MakeP(ErrCode::ObjectShutDown, std::string("RejectedOperation=") + call, "Engine is shut down.");
  return Error();
}

// Groups [first, first + n) of the call (st.offsets: where their entries begin in pTargets) onto the device, through the pack list: the
// groups' starts within the chunk | the first group of every tile of the sweep (kb_plan.h: PlanGroupTiles, whole groups) | per tile the
// power of two that holds its longest group | the entries.
// They stay in _dAqs + 2 for the launches behind this one.
Error HipEngine::StageGroupsLocked(SourceStage &st, int64_t first, int64_t n, const int64_t *pTargets) {
  hipSetDevice(_device);
  if (_serverLaunched) StopServer();   // a launched kernel has no room beside the resident sweep and would wait for it to idle out
  const int64_t *off = st.offsets.data() + first, e0 = off[0], nEntries = off[n] - e0;
  std::vector<int64_t> counts((size_t)n);
  for (int64_t g = 0; g < n; g++) counts[(size_t)g] = off[g + 1] - off[g];
  const std::vector<int64_t> tiles = PlanGroupTiles(n, counts.data(), kSepTileEntries, kSepTileGroups);
  const int64_t nTiles = (int64_t)tiles.size() - 1;
  const int64_t words = 2 + (n + 1) + (nTiles + 1) + nTiles + nEntries;   // {arrival counter, pad}, then the four lists
  const Error err = EnsurePackList(words);
  if (!err.ok()) return err;
  int64_t *w = _hPack + 2;
  for (int64_t g = 0; g <= n; g++) *w++ = off[g] - e0;
  for (int64_t t : tiles) *w++ = t;
  for (int64_t t = 0; t < nTiles; t++) {
    int64_t width = 2;
    for (int64_t g = tiles[(size_t)t]; g < tiles[(size_t)t + 1]; g++)
      while (width < counts[(size_t)g]) width *= 2;
    *w++ = width;
  }
  std::memcpy(w, pTargets + e0, (size_t)nEntries * sizeof(int64_t));
  MarkStreamBusy();
  st.dGroupStart = _dAqs + 2;
  st.dTileGroup = st.dGroupStart + (n + 1);
  st.dTileWidth = st.dTileGroup + (nTiles + 1);
  st.dEntries = st.dTileWidth + nTiles;
  st.nTiles = nTiles;
  st.sources += (uint64_t)n;
  return SubmitPackList(words);
}

// This engine's part of the package of up to kMaxBatch validated sources, into the slots at pDst: enqueued, nothing waited for --
// except where a scratch buffer has to grow, and that the pinned list is not rewritten while an earlier call's copy of it is under
// way.  The sources stay in _dAqs + 2 for the launches behind this one.  Similarity: the sums over THIS engine's questions, slots of
// PackagePitch() doubles (similarity_kernels.hip); redundancy: the weighted rows u_k = w p_sk of those sources (GLOBAL ids) this engine
// holds (redundancy_kernels.hip).
Error HipEngine::PackSourcesLocked(SourceStage &st, int64_t n, const int64_t *pSources, void *pDst, void *pFlag, uint64_t flagValue) {
  if (n == 0 && pFlag == nullptr) return Error();
  hipSetDevice(_device);
  if (_serverLaunched) StopServer();   // a launched kernel has no room beside the resident sweep and would wait for it to idle out
  const Error err = SubmitSources(n, pSources);
  if (!err.ok()) return err;
  const KbView kb = View();
  double *dst = static_cast<double *>(pDst);
  unsigned *counter = reinterpret_cast<unsigned *>(_dAqs);
  if (st.questions) {
    HIP_TRY(LaunchQuestionWeights(kb, _dAqs + 2, n, _qFirst, dst, PackagePitch(), counter, static_cast<uint64_t *>(pFlag), flagValue, _stream));
  } else {
    if (n > 0) {   // the source columns of a tile, the sweep's partial sums per question chunk
      HIP_TRY(GrowDevice(&st.dScratch[0], st.scratchBytes[0], SimSourceScratchBytes(kb)));
      HIP_TRY(GrowDevice(&st.dScratch[1], st.scratchBytes[1], SimPartialBytes(kb)));
    }
    HIP_TRY(LaunchSimilaritySums(kb, _dAqs + 2, n, st.dScratch[0], st.dScratch[1], dst, PackagePitch(), counter, static_cast<uint64_t *>(pFlag), flagValue, _stream));
  }
  st.sources += (uint64_t)n;
  return Error();
}

// rows[i][SourceRowPitch(st)] of the n sources in _dAqs + 2 from the package at dPackage (device-visible), on the engine's stream.
// Similarity: the sums divided by the questions of the WHOLE knowledge base that are not gaps, the gap targets zeroed; redundancy: the
// sweep of this engine's questions against the weighted rows; separation: the gathering sweep of this engine's questions over the staged
// groups (no package).
Error HipEngine::SourceRowsLocked(SourceStage &st, int64_t n, const double *dPackage, bool zeroSelf) {
  const KbView kb = View();
  HIP_TRY(GrowDevice(&st.dRows, st.rowsBytes, (size_t)n * (size_t)SourceRowPitch(st) * sizeof(double)));
  if (st.groups) {
    HIP_TRY(LaunchSeparationSweep(kb, st.dGroupStart, st.dTileGroup, st.dTileWidth, st.dEntries, n, st.nTiles, st.dRows, RedRowPitch(), _stream));
  } else if (st.questions) {
    HIP_TRY(GrowDevice(&st.dScratch[0], st.scratchBytes[0], RedundancyTableBytes(kb)));   // the generic sweep's tables
    HIP_TRY(LaunchRedundancySweep(kb, dPackage, PackagePitch(), _dAqs + 2, n, _qFirst, zeroSelf, st.dRows, RedRowPitch(), st.dScratch[0], _stream));
  } else {
    const int64_t nValid = _qTotal - (int64_t)(IsShard() ? _globalQuestionGaps.size() : _questionGapList.size());
    HIP_TRY(LaunchSimilarityRows(kb, dPackage, PackagePitch(), _dAqs + 2, n, zeroSelf, nValid, st.dRows, _stream));
  }
  return Error();
}

// The sources on the device (_dAqs + 2) and the package where the rows launch may read it (StageHostPackage: into the engine's own
// package)
Error HipEngine::StageSourcesLocked(SourceStage &st, int64_t n, const int64_t *pSources, const void *pPackage, const double **dPackage) {
  hipSetDevice(_device);
  if (_serverLaunched) StopServer();
  Error err;
  *dPackage = static_cast<const double *>(StageHostPackage(pPackage, (size_t)(n * SourceSlotDoubles(st)) * sizeof(double), (void **)&st.dPackage, st.packageBytes, err));
  return *dPackage ? SubmitSources(n, pSources) : err;
}

// the stage's n rows, rowLength doubles of each, to the host; the stream synchronised behind them
Error HipEngine::SourceRowsOutLocked(SourceStage &st, int64_t n, double *pOut, int64_t rowLength) {
  HIP_TRY(hipMemcpy2DAsync(pOut, (size_t)rowLength * sizeof(double), st.dRows, (size_t)SourceRowPitch(st) * sizeof(double), (size_t)rowLength * sizeof(double), (size_t)n,
                           hipMemcpyDeviceToHost, _stream));
  HIP_TRY(hipStreamSynchronize(_stream));
  return Error();
}

// The listing of up to kMaxBatch sources (on the device: _dAqs + 2) from a package (device-visible), maxCount > 0: at most 256 records
// a source on the device -- similarity: the batched target listing over the rows as posteriors (kb_kernels.hip: LaunchTopTargetsBatch);
// redundancy and separation: the question listing over slots that show it the rows (LaunchRedundancySlots, LaunchTopQuestions) --, beyond that the
// rows copied and the prefix taken here in the same order: value descending, id ascending; the source itself, the gaps and what is
// not > 0 are no candidates (zeros in the rows).  GLOBAL ids.
Error HipEngine::ListSourcesLocked(SourceStage &st, int64_t n, const double *dPackage, int64_t maxCount, RatedTargetDev *pDest, int64_t *pCounts) {
  const int64_t results = st.questions ? _Q : _T, want = std::min<int64_t>(maxCount, results), pitch = SourceRowPitch(st), idBase = st.questions ? _qFirst : 0;
  Error err = SourceRowsLocked(st, n, dPackage, true);
  if (!err.ok()) return err;
  if (want > 256) {
    st.rows.resize((size_t)(n * pitch));
    HIP_TRY(hipMemcpyAsync(st.rows.data(), st.dRows, (size_t)(n * pitch) * sizeof(double), hipMemcpyDeviceToHost, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
    std::vector<int64_t> idx;
    for (int64_t i = 0; i < n; i++)
      pCounts[i] = RatedPrefix(st.rows.data() + i * pitch, results, want, [](int64_t) { return true; }, [&](int64_t k) { return idBase + k; }, pDest + i * maxCount, idx);
    return Error();
  }
  err = st.questions ? EnsureTopScratchRecords(n * TopQuestionsScratchRecords(_Q, want)) : EnsureTopScratch(n, want);
  if (!err.ok()) return err;
  HIP_TRY(st.lines.Ensure(_stream, n * want, 0, kMaxBatch, hipHostMallocDefault));
  if (st.questions) {
    if (!st.dSlots) HIP_TRY(hipMalloc((void **)&st.dSlots, (size_t)kMaxBatch * sizeof(QuizSlot)));
    HIP_TRY(LaunchRedundancySlots(st.dSlots, st.dRows, pitch, _dQGap, n, _stream));
    TopQuestions a{};
    a.slots = st.dSlots; a.qgap = _dQGap; a.nQuizzes = (int)n; a.Q = _Q;
    HIP_TRY(LaunchTopQuestions(a, want, _dTopScratch[0], _dTopScratch[1], st.lines.records, st.lines.Counts(), nullptr, 0, _stream));
  } else {
    TopBatchPriors pr;
    for (int64_t i = 0; i < n; i++) pr.prior[i] = st.dRows + i * pitch;
    HIP_TRY(LaunchTopTargetsBatch(View(), pr, n, want, _dTopScratch[0], _dTopScratch[1], st.lines.records, st.lines.Counts(), nullptr, 0, _stream));
  }
  HIP_TRY(hipStreamSynchronize(_stream));
  for (int64_t i = 0; i < n; i++) {
    const int64_t c = std::max<int64_t>(0, std::min<int64_t>(st.lines.Counts()[i], want));
    const RatedTargetDev *rec = st.lines.records + i * want;
    RatedTargetDev *dest = pDest + i * maxCount;
    for (int64_t j = 0; j < c; j++) dest[j] = RatedTargetDev{idBase + rec[j].iTarget, rec[j].prob};
    pCounts[i] = c;
  }
  return Error();
}

// (the groups family: sources [first, first + m) of a chunk are GROUPS, their targets in pSources from st.offsets[first])
void HipEngine::GroupOffsets(SourceStage &st, int64_t nGroups, const int64_t *pGroupCounts) {
  st.offsets.assign((size_t)nGroups + 1, 0);
  for (int64_t g = 0; g < nGroups; g++) st.offsets[(size_t)g + 1] = st.offsets[(size_t)g] + pGroupCounts[g];
}

Error HipEngine::EvalSources(SourceStage &st, const char *call, int64_t nSources, const int64_t *pGroupCounts, const int64_t *pSources, double *pOut, int64_t n) {
  Error err = st.groups ? SourceArgs(nSources, 0, 0, pGroupCounts && pSources && pOut, "Nullptr is passed in place of the groups or the separation buffer.", nullptr, "nGroups")
                        : SourceArgs(nSources, 0, 0, pSources && pOut, st.questions ? "Nullptr is passed in place of the sources or the redundancy buffer."
                                                                                      : "Nullptr is passed in place of the sources or the similarity buffer.", nullptr);
  if (!err.ok()) return err;
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  err = st.groups ? AdmitGroupsLocked(call, n, nSources, pGroupCounts, pSources) : AdmitSourcesLocked(st, call, true, n, nSources, pSources);
  if (!err.ok() || nSources == 0) return err;
  st.calls++;
  if (st.groups) GroupOffsets(st, nSources, pGroupCounts);
  HIP_TRY(GrowDevice(&st.dPackage, st.packageBytes, (size_t)(std::min<int64_t>(nSources, kMaxBatch) * SourceSlotDoubles(st)) * sizeof(double)));
  for (int64_t first = 0; first < nSources; first += kMaxBatch) {
    const int64_t m = std::min<int64_t>(kMaxBatch, nSources - first);
    TimerStart(st.ev);
    err = st.groups ? StageGroupsLocked(st, first, m, pSources) : PackSourcesLocked(st, m, pSources + first, st.dPackage, nullptr, 0);
    if (err.ok()) err = SourceRowsLocked(st, m, st.dPackage, false);
    if (!err.ok()) return err;
    TimerStop(st.ev, st.deviceNs);   // (the copy behind it synchronises the stream)
    err = SourceRowsOutLocked(st, m, pOut + first * n, n);
    if (!err.ok()) return err;
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  return Error();
}

Error HipEngine::ListSources(SourceStage &st, const char *call, int64_t nSources, const int64_t *pGroupCounts, const int64_t *pSources, int64_t maxCount,
                             RatedTargetDev *pDest, int64_t *pCounts) {
  Error err = SourceArgs(nSources, maxCount, 0, (!st.groups || pGroupCounts) && pSources && pCounts && (maxCount == 0 || pDest), kNullBatch, nullptr,
                         st.groups ? "nGroups" : "nSources");
  if (!err.ok()) return err;
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  err = st.groups ? AdmitGroupsLocked(call, -1, nSources, pGroupCounts, pSources) : AdmitSourcesLocked(st, call, true, -1, nSources, pSources);
  if (!err.ok() || nSources == 0) return err;
  st.calls++;
  if (st.groups) GroupOffsets(st, nSources, pGroupCounts);
  for (int64_t i = 0; i < nSources; i++) pCounts[i] = 0;
  if (maxCount == 0) return Error();
  HIP_TRY(GrowDevice(&st.dPackage, st.packageBytes, (size_t)(std::min<int64_t>(nSources, kMaxBatch) * SourceSlotDoubles(st)) * sizeof(double)));
  for (int64_t first = 0; first < nSources; first += kMaxBatch) {
    const int64_t m = std::min<int64_t>(kMaxBatch, nSources - first);
    TimerStart(st.ev);
    err = st.groups ? StageGroupsLocked(st, first, m, pSources) : PackSourcesLocked(st, m, pSources + first, st.dPackage, nullptr, 0);
    if (!err.ok()) return err;
    // "similarity_device_ns" covers the pack; "redundancy_device_ns" and "separation_device_ns" the pack, the sweep and the listing (the stream has been synchronised)
    if (!st.questions) TimerStop(st.ev, st.deviceNs);
    err = ListSourcesLocked(st, m, st.dPackage, maxCount, pDest + first * maxCount, pCounts + first);
    if (!err.ok()) return err;
    if (st.questions) TimerStop(st.ev, st.deviceNs);
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  return Error();
}

Error HipEngine::PackSources(SourceStage &st, const char *call, int64_t nSources, const int64_t *pSources, void *pDst, void *pFlag, uint64_t flagValue) {
  Error err = SourceArgs(nSources, 0, kMaxBatch, pSources && pDst, kNullBatchOrPackage, pDst);
  if (!err.ok()) return err;
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  err = AdmitSourcesLocked(st, call, false, -1, nSources, pSources);
  if (!err.ok()) return err;
  st.calls++;
  return PackSourcesLocked(st, nSources, pSources, pDst, pFlag, flagValue);
}

Error HipEngine::EvalSourcesFromPackage(SourceStage &st, const char *call, int64_t nSources, const int64_t *pSources, const void *pPackage, double *pOut, int64_t n) {
  Error err = SourceArgs(nSources, 0, kMaxBatch, pSources && pPackage && pOut, kNullBatchOrPackage, pPackage);
  if (!err.ok()) return err;
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  err = AdmitSourcesLocked(st, call, false, n, nSources, pSources);
  if (!err.ok() || nSources == 0) return err;
  st.calls++;
  const double *package = nullptr;
  err = StageSourcesLocked(st, nSources, pSources, pPackage, &package);
  if (err.ok()) err = SourceRowsLocked(st, nSources, package, false);
  if (err.ok()) err = SourceRowsOutLocked(st, nSources, pOut, n);
  if (err.ok()) _mu.busy = false;   // (the stream has just been synchronised)
  return err;
}

Error HipEngine::ListSourcesFromPackage(SourceStage &st, const char *call, int64_t nSources, const int64_t *pSources, const void *pPackage, int64_t maxCount,
                                        RatedTargetDev *pDest, int64_t *pCounts) {
  Error err = SourceArgs(nSources, maxCount, kMaxBatch, pSources && pPackage && pCounts && (maxCount == 0 || pDest), kNullBatchOrPackage, pPackage);
  if (!err.ok()) return err;
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  err = AdmitSourcesLocked(st, call, false, -1, nSources, pSources);
  if (!err.ok() || nSources == 0) return err;
  st.calls++;
  for (int64_t i = 0; i < nSources; i++) pCounts[i] = 0;
  if (maxCount == 0) return Error();
  const double *package = nullptr;
  err = StageSourcesLocked(st, nSources, pSources, pPackage, &package);
  if (err.ok()) err = ListSourcesLocked(st, nSources, package, maxCount, pDest, pCounts);
  if (err.ok()) _mu.busy = false;   // (the stream has just been synchronised)
  return err;
}

// ---- the C ABI's entries ----------------------------------------------------------------------------------------------------------------
Error HipEngine::EvalTargetSimilarity(int64_t nSources, const int64_t *pSources, double *pOut, int64_t n) {
  return EvalSources(_sim, "EvalTargetSimilarity", nSources, nullptr, pSources, pOut, n);
}
Error HipEngine::ListSimilarTargetsBatch(int64_t nSources, const int64_t *pSources, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts) {
  return ListSources(_sim, "ListSimilarTargetsBatch", nSources, nullptr, pSources, maxCount, reinterpret_cast<RatedTargetDev *>(pDest), pCounts);
}
Error HipEngine::PackTargetSimilaritySums(int64_t nSources, const int64_t *pSources, void *pDst, void *pFlag, uint64_t flagValue) {
  return PackSources(_sim, "PackTargetSimilaritySums", nSources, pSources, pDst, pFlag, flagValue);
}
Error HipEngine::ListSimilarTargetsFromSums(int64_t nSources, const int64_t *pSources, const void *pSums, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts) {
  return ListSourcesFromPackage(_sim, "ListSimilarTargetsFromSums", nSources, pSources, pSums, maxCount, reinterpret_cast<RatedTargetDev *>(pDest), pCounts);
}
Error HipEngine::EvalQuestionRedundancy(int64_t nSources, const int64_t *pSources, double *pOut, int64_t n) {
  return EvalSources(_red, "EvalQuestionRedundancy", nSources, nullptr, pSources, pOut, n);
}
Error HipEngine::ListRedundantQuestionsBatch(int64_t nSources, const int64_t *pSources, int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) {
  return ListSources(_red, "ListRedundantQuestionsBatch", nSources, nullptr, pSources, maxCount, reinterpret_cast<RatedTargetDev *>(pDest), pCounts);
}
Error HipEngine::PackQuestionWeights(int64_t nSources, const int64_t *pSources, void *pDst, void *pFlag, uint64_t flagValue) {
  return PackSources(_red, "PackQuestionWeights", nSources, pSources, pDst, pFlag, flagValue);
}
Error HipEngine::EvalQuestionRedundancyFromWeights(int64_t nSources, const int64_t *pSources, const void *pWeights, double *pOut, int64_t n) {
  return EvalSourcesFromPackage(_red, "EvalQuestionRedundancyFromWeights", nSources, pSources, pWeights, pOut, n);
}
Error HipEngine::ListRedundantQuestionsFromWeights(int64_t nSources, const int64_t *pSources, const void *pWeights, int64_t maxCount, CiRatedQuestion *pDest,
                                                   int64_t *pCounts) {
  return ListSourcesFromPackage(_red, "ListRedundantQuestionsFromWeights", nSources, pSources, pWeights, maxCount, reinterpret_cast<RatedTargetDev *>(pDest), pCounts);
}
Error HipEngine::EvalTargetSeparation(int64_t nGroups, const int64_t *pGroupCounts, const int64_t *pTargets, double *pOut, int64_t n) {
  return EvalSources(_sep, "EvalTargetSeparation", nGroups, pGroupCounts, pTargets, pOut, n);
}
Error HipEngine::ListSeparatingQuestionsBatch(int64_t nGroups, const int64_t *pGroupCounts, const int64_t *pTargets, int64_t maxCount, CiRatedQuestion *pDest,
                                              int64_t *pCounts) {
  return ListSources(_sep, "ListSeparatingQuestionsBatch", nGroups, pGroupCounts, pTargets, maxCount, reinterpret_cast<RatedTargetDev *>(pDest), pCounts);
}

}  // namespace pqa
