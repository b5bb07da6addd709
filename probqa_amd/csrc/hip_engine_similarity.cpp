// hip_engine_similarity.cpp -- HipEngine: targets that answer like a given one (hip_engine.h, include/PqaHipExt.h):
// EvalTargetSimilarity, ListSimilarTargetsBatch, and the pair for shards that processes of their own drive, PackTargetSimilaritySums /
// ListSimilarTargetsFromSums.  sim(s, t) = (sum over the questions of the WHOLE knowledge base that are not gaps of
// sum_k sqrt(p_qk(s) p_qk(t))) / nValidQuestions, p_qk(t) = A[q][k][t] / D[q][t]: 1 for targets no quiz can tell apart.
// One code path: PackSimilarityLocked enqueues, per up to 256 sources, the sums over THIS engine's questions into a package at the
// posterior packages' pitch (similarity_kernels.hip); ListFromSumsLocked turns a package -- the engine's own, or the ranks' summed
// one -- into rows on the device (divided, the gaps and the source's own entry zeroed) and lists them with the batched target listing
// (kb_kernels.hip: LaunchTopTargetsBatch), or copies them and takes the prefix here beyond 256 records.  A whole engine's Eval and
// List are pack -> rows and pack -> list, in chunks of 256 sources.
// The calls read only the knowledge base: they work in regular and in maintenance mode and change no quiz.  Everything a call can be
// refused for is decided before anything is launched or written.
#include "hip_engine_internal.h"

namespace pqa {

namespace {
Error OnShard(const char *what) {
  return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + what + " of a sharded engine",
                      "Sum the ranks' PqaHip_PackTargetSimilaritySums packages and list with PqaEngine_ListSimilarTargetsFromSums instead.");
}
}  // namespace

int64_t HipEngine::ValidQuestionsOfKb() const {
  return _qTotal - (int64_t)(IsShard() ? _globalQuestionGaps.size() : _questionGapList.size());
}

Error HipEngine::ValidateSimilarityLocked(const char *what, int64_t n, const int64_t *pSources) const {
  if (_mode == Mode::Shutdown) return Error::MakeP(ErrCode::ObjectShutDown, std::string("RejectedOperation=") + what, "Engine is shut down.");
  for (int64_t i = 0; i < n; i++)
    if (pSources[i] < 0 || pSources[i] >= _T)
      return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(i) + " targetId=" + std::to_string(pSources[i]) + " " + RangeParams(pSources[i], 0, _T - 1),
                          "A source target is out of range.");
  return Error();
}

// The sums of up to kMaxBatch validated sources over this engine's questions, into slots of SimPitch() doubles at pDst: enqueued,
// nothing waited for -- except where a scratch buffer has to grow, and that the pinned list is not rewritten while an earlier
// call's copy of it is under way.  The sources stay in _dAqs + 2 for the launches behind this one.
Error HipEngine::PackSimilarityLocked(int64_t n, const int64_t *pSources, void *pDst, void *pFlag, uint64_t flagValue) {
  if (n == 0 && pFlag == nullptr) return Error();
  hipSetDevice(_device);
  if (_serverLaunched) StopServer();   // a launched kernel has no room beside the resident sweep and would wait for it to idle out
  const KbView kb = View();
  SimilarityStage &st = _sim;
  auto grow = [&](double **p, size_t &have, size_t need) -> hipError_t {
    if (need <= have) return hipSuccess;
    hipStreamSynchronize(_stream);   // (nothing in flight reads the buffer about to go)
    hipFree(*p);
    *p = nullptr;
    have = 0;
    const hipError_t e = hipMalloc((void **)p, need);
    if (e == hipSuccess) have = need;
    return e;
  };
  if (n > 0) {
    HIP_TRY(grow(&st.dRS, st.rsBytes, SimSourceScratchBytes(kb)));
    HIP_TRY(grow(&st.dPartial, st.partialBytes, SimPartialBytes(kb)));
  }
  const int64_t words = 2 + n;   // {arrival counter, pad}, then the sources
  Error err = EnsurePackList(words);
  if (!err.ok()) return err;
  for (int64_t i = 0; i < n; i++) _hPack[2 + i] = pSources[i];
  MarkStreamBusy();
  HIP_TRY(hipMemcpyAsync(_dAqs, _hPack, (size_t)words * sizeof(int64_t), hipMemcpyHostToDevice, _stream));
  HIP_TRY(hipEventRecord(_evPack, _stream));
  HIP_TRY(LaunchSimilaritySums(kb, _dAqs + 2, n, st.dRS, st.dPartial, static_cast<double *>(pDst), SimPitch(), reinterpret_cast<unsigned *>(_dAqs),
                               static_cast<uint64_t *>(pFlag), flagValue, _stream));
  _simSources += (uint64_t)n;
  return Error();
}

// rows[i][SimPitch()] of up to kMaxBatch sources from the package at dSums (device-visible), on the engine's stream
Error HipEngine::SimilarityRowsLocked(int64_t n, const int64_t *dSources, const double *dSums, bool zeroSelf) {
  SimilarityStage &st = _sim;
  const size_t need = (size_t)n * (size_t)SimPitch() * sizeof(double);
  if (need > st.rowsBytes) {
    HIP_TRY(hipStreamSynchronize(_stream));
    hipFree(st.dRows);
    st.dRows = nullptr; st.rowsBytes = 0;
    HIP_TRY(hipMalloc((void **)&st.dRows, need));
    st.rowsBytes = need;
  }
  HIP_TRY(LaunchSimilarityRows(View(), dSums, SimPitch(), dSources, n, zeroSelf, ValidQuestionsOfKb(), st.dRows, _stream));
  return Error();
}

// The listing of up to kMaxBatch sources from a package (dSums: device-visible; dSources: the sources on the device): at most 256
// records a source through the batched target listing, beyond that the rows copied and the prefix taken here in the same order --
// similarity descending, target ascending; the source itself, the gaps and what is not > 0 are no candidates.
Error HipEngine::ListFromSumsLocked(int64_t n, const int64_t *dSources, const double *dSums, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts) {
  for (int64_t i = 0; i < n; i++) pCounts[i] = 0;
  const int64_t want = std::min<int64_t>(maxCount, _T);
  if (n == 0 || want <= 0) return Error();
  Error err = SimilarityRowsLocked(n, dSources, dSums, true);
  if (!err.ok()) return err;
  SimilarityStage &st = _sim;
  const int64_t pitch = SimPitch();
  if (want <= 256) {
    err = EnsureTopScratch(n, want);
    if (!err.ok()) return err;
    const int64_t needRecords = n * want;
    if (needRecords > st.hRecords) {   // records | counts
      HIP_TRY(hipStreamSynchronize(_stream));
      if (st.hLines) hipHostFree(st.hLines);
      st.hLines = nullptr; st.hRecords = 0;
      HIP_TRY(hipHostMalloc((void **)&st.hLines, (size_t)needRecords * sizeof(RatedTargetDev) + (size_t)kTopBatchQuizzes * sizeof(int64_t), hipHostMallocDefault));
      st.hRecords = needRecords;
    }
    int64_t *hCounts = reinterpret_cast<int64_t *>(st.hLines + st.hRecords);
    TopBatchPriors pr;
    for (int64_t i = 0; i < n; i++) pr.prior[i] = st.dRows + i * pitch;
    HIP_TRY(LaunchTopTargetsBatch(View(), pr, n, want, _dTopScratch[0], _dTopScratch[1], st.hLines, hCounts, nullptr, 0, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
    for (int64_t i = 0; i < n; i++) {
      const int64_t c = std::max<int64_t>(0, std::min<int64_t>(hCounts[i], want));
      pCounts[i] = c;
      std::memcpy(pDest + i * maxCount, st.hLines + i * want, (size_t)c * sizeof(RatedTargetDev));
    }
    return Error();
  }
  st.rows.resize((size_t)(n * pitch));
  HIP_TRY(hipMemcpyAsync(st.rows.data(), st.dRows, (size_t)(n * pitch) * sizeof(double), hipMemcpyDeviceToHost, _stream));
  HIP_TRY(hipStreamSynchronize(_stream));
  std::vector<int64_t> idx;
  for (int64_t i = 0; i < n; i++) {
    const double *v = st.rows.data() + i * pitch;
    idx.clear();
    for (int64_t t = 0; t < _T; t++)
      if (v[t] > 0.0) idx.push_back(t);   // (the gaps and the source itself are zeros)
    const int64_t c = std::min<int64_t>(want, (int64_t)idx.size());
    std::partial_sort(idx.begin(), idx.begin() + c, idx.end(), [&](int64_t a, int64_t b) { return v[a] > v[b] || (v[a] == v[b] && a < b); });
    CiRatedTarget *dest = pDest + i * maxCount;
    for (int64_t k = 0; k < c; k++) { dest[k]._iTarget = idx[(size_t)k]; dest[k]._prob = v[idx[(size_t)k]]; }
    pCounts[i] = c;
  }
  return Error();
}

void HipEngine::SimilarityTimerStart() {
  if (!_opt.timeSweeps) return;
  if (!_sim.ev[0] && (hipEventCreate(&_sim.ev[0]) != hipSuccess || hipEventCreate(&_sim.ev[1]) != hipSuccess)) { (void)hipGetLastError(); return; }
  if (hipEventRecord(_sim.ev[0], _stream) != hipSuccess) (void)hipGetLastError();
}
void HipEngine::SimilarityTimerStop() {   // (the caller synchronises the stream behind it)
  if (!_opt.timeSweeps || !_sim.ev[1]) return;
  float ms = 0;
  if (hipEventRecord(_sim.ev[1], _stream) == hipSuccess && hipEventSynchronize(_sim.ev[1]) == hipSuccess && hipEventElapsedTime(&ms, _sim.ev[0], _sim.ev[1]) == hipSuccess)
    _simDeviceNs += (uint64_t)(ms * 1e6);
  else (void)hipGetLastError();
}

Error HipEngine::EvalTargetSimilarity(int64_t nSources, const int64_t *pSources, double *pOut, int64_t n) {
  if (nSources < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nSources), "|nSources| must be non-negative.");
  if (nSources > 0 && (!pSources || !pOut)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the sources or the similarity buffer.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  if (IsShard()) return OnShard("EvalTargetSimilarity");
  if (n != _T) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(n, _T, _T), "Similarity row length must equal the target count.");
  Error err = ValidateSimilarityLocked("EvalTargetSimilarity", nSources, pSources);
  if (!err.ok() || nSources == 0) return err;
  _simCalls++;
  const int64_t pitch = SimPitch();
  err = EnsureSimilaritySums(std::min<int64_t>(nSources, kMaxBatch));
  if (!err.ok()) return err;
  for (int64_t first = 0; first < nSources; first += kMaxBatch) {
    const int64_t m = std::min<int64_t>(kMaxBatch, nSources - first);
    SimilarityTimerStart();
    err = PackSimilarityLocked(m, pSources + first, _sim.dSums, nullptr, 0);
    if (err.ok()) err = SimilarityRowsLocked(m, _dAqs + 2, _sim.dSums, false);
    if (!err.ok()) return err;
    SimilarityTimerStop();
    HIP_TRY(hipMemcpy2DAsync(pOut + first * n, (size_t)n * sizeof(double), _sim.dRows, (size_t)pitch * sizeof(double), (size_t)n * sizeof(double), (size_t)m,
                             hipMemcpyDeviceToHost, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  return Error();
}

Error HipEngine::ListSimilarTargetsBatch(int64_t nSources, const int64_t *pSources, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts) {
  if (nSources < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nSources), "|nSources| must be non-negative.");
  if (maxCount < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(maxCount), "|maxCount| must be non-negative.");
  if (nSources > 0 && (!pSources || !pCounts || (maxCount > 0 && !pDest))) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  if (IsShard()) return OnShard("ListSimilarTargetsBatch");
  Error err = ValidateSimilarityLocked("ListSimilarTargetsBatch", nSources, pSources);
  if (!err.ok() || nSources == 0) return err;
  _simCalls++;
  for (int64_t i = 0; i < nSources; i++) pCounts[i] = 0;
  if (maxCount == 0) return Error();
  err = EnsureSimilaritySums(std::min<int64_t>(nSources, kMaxBatch));
  if (!err.ok()) return err;
  for (int64_t first = 0; first < nSources; first += kMaxBatch) {
    const int64_t m = std::min<int64_t>(kMaxBatch, nSources - first);
    SimilarityTimerStart();
    err = PackSimilarityLocked(m, pSources + first, _sim.dSums, nullptr, 0);
    if (!err.ok()) return err;
    SimilarityTimerStop();
    err = ListFromSumsLocked(m, _dAqs + 2, _sim.dSums, maxCount, pDest + first * maxCount, pCounts + first);
    if (!err.ok()) return err;
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  return Error();
}

Error HipEngine::PackTargetSimilaritySums(int64_t nSources, const int64_t *pSources, void *pDst, void *pFlag, uint64_t flagValue) {
  if (nSources < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nSources), "|nSources| must be non-negative.");
  if (nSources > kMaxBatch) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(nSources, 0, kMaxBatch), "Batch size is out of range.");
  if (nSources > 0 && (!pSources || !pDst)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer or the package.");
  if ((reinterpret_cast<uintptr_t>(pDst) & 15) != 0)
    return Error::MakeP(ErrCode::IndexOutOfRange, "address mod 16=" + std::to_string(reinterpret_cast<uintptr_t>(pDst) & 15), "The package must be 16-byte aligned.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = ValidateSimilarityLocked("PackTargetSimilaritySums", nSources, pSources);
  if (!err.ok()) return err;
  _simCalls++;
  return PackSimilarityLocked(nSources, pSources, pDst, pFlag, flagValue);
}

Error HipEngine::ListSimilarTargetsFromSums(int64_t nSources, const int64_t *pSources, const void *pSums, int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts) {
  if (nSources < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nSources), "|nSources| must be non-negative.");
  if (maxCount < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(maxCount), "|maxCount| must be non-negative.");
  if (nSources > kMaxBatch) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(nSources, 0, kMaxBatch), "Batch size is out of range.");
  if (nSources > 0 && (!pSources || !pSums || !pCounts || (maxCount > 0 && !pDest)))
    return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer or the package.");
  if ((reinterpret_cast<uintptr_t>(pSums) & 15) != 0)
    return Error::MakeP(ErrCode::IndexOutOfRange, "address mod 16=" + std::to_string(reinterpret_cast<uintptr_t>(pSums) & 15), "The package must be 16-byte aligned.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = ValidateSimilarityLocked("ListSimilarTargetsFromSums", nSources, pSources);
  if (!err.ok() || nSources == 0) return err;
  _simCalls++;
  for (int64_t i = 0; i < nSources; i++) pCounts[i] = 0;
  if (maxCount == 0) return Error();
  hipSetDevice(_device);
  if (_serverLaunched) StopServer();
  const double *sums = static_cast<const double *>(pSums);
  if (_opt.rowsStage) {   // a package in host memory (registered, as PqaHip_HostRegister leaves it): copied to the device first
    hipPointerAttribute_t at;
    const hipError_t q = hipPointerGetAttributes(&at, pSums);
    if (q != hipSuccess) (void)hipGetLastError();
    if (q == hipSuccess && at.type == hipMemoryTypeHost) {
      err = EnsureSimilaritySums(nSources);
      if (!err.ok()) return err;
      HIP_TRY(hipMemcpyAsync(_sim.dSums, pSums, (size_t)(nSources * SimPitch()) * sizeof(double), hipMemcpyDefault, _stream));
      sums = _sim.dSums;
      _rowsStaged++;
    }
  }
  const int64_t words = 2 + nSources;
  err = EnsurePackList(words);
  if (!err.ok()) return err;
  for (int64_t i = 0; i < nSources; i++) _hPack[2 + i] = pSources[i];
  MarkStreamBusy();
  HIP_TRY(hipMemcpyAsync(_dAqs, _hPack, (size_t)words * sizeof(int64_t), hipMemcpyHostToDevice, _stream));
  HIP_TRY(hipEventRecord(_evPack, _stream));
  err = ListFromSumsLocked(nSources, _dAqs + 2, sums, maxCount, pDest, pCounts);
  if (err.ok()) _mu.busy = false;   // (the stream has just been synchronised)
  return err;
}

Error HipEngine::EnsureSimilaritySums(int64_t n) {
  const size_t need = (size_t)n * (size_t)SimPitch() * sizeof(double);
  if (need <= _sim.sumsBytes) return Error();
  HIP_TRY(hipStreamSynchronize(_stream));
  hipFree(_sim.dSums);
  _sim.dSums = nullptr; _sim.sumsBytes = 0;
  HIP_TRY(hipMalloc((void **)&_sim.dSums, need));
  _sim.sumsBytes = need;
  return Error();
}

}  // namespace pqa
