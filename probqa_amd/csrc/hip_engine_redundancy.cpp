// hip_engine_redundancy.cpp -- HipEngine: questions whose answers a given one predicts (hip_engine.h, include/PqaHipExt.h):
// EvalQuestionRedundancy, ListRedundantQuestionsBatch, and the calls for shards that processes of their own drive, PackQuestionWeights /
// EvalQuestionRedundancyFromWeights / ListRedundantQuestionsFromWeights.  I(s, q) is the mutual information in bits between the
// answers to questions s and q for a target drawn from vB: over the K x K table J[k][k'] = sum_t (w[t] p_sk(t)) p_qk'(t).
// One code path: PackRedundancyLocked enqueues, per up to 256 sources, the weighted rows u_k = w p_sk of the sources THIS engine holds
// into a package (redundancy_kernels.hip); RedundancyRowsLocked sweeps this engine's questions against a package -- the engine's own,
// or the ranks' summed one -- into rows on the device; ListFromWeightsLocked lists them with the question listing (kb_kernels.hip:
// LaunchTopQuestions), or copies them and takes the prefix here beyond 256 records.  A whole engine's Eval and List are pack -> rows
// and pack -> list, in chunks of 256 sources.
// The calls read only the knowledge base: they work in regular and in maintenance mode and change no quiz.  Everything a call can be
// refused for is decided before anything is launched or written.
#include "hip_engine_internal.h"

namespace pqa {

namespace {
Error OnShard(const char *what) {
  return Error::MakeP(ErrCode::NotImplemented, std::string("Feature=") + what + " of a sharded engine",
                      "Sum the ranks' PqaHip_PackQuestionWeights packages and use PqaEngine_EvalQuestionRedundancyFromWeights / "
                      "PqaEngine_ListRedundantQuestionsFromWeights instead.");
}
Error Misaligned(const void *p) {
  return Error::MakeP(ErrCode::IndexOutOfRange, "address mod 16=" + std::to_string(reinterpret_cast<uintptr_t>(p) & 15), "The package must be 16-byte aligned.");
}
}  // namespace

// what does not need the engine: the counts, and with `limited` the 256 sources of the pack / from-weights calls
Error HipEngine::RedundancyArgs(int64_t nSources, int64_t maxCount, bool limited) const {
  if (nSources < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nSources), "|nSources| must be non-negative.");
  if (maxCount < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(maxCount), "|maxCount| must be non-negative.");
  if (limited && nSources > kMaxBatch) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(nSources, 0, kMaxBatch), "Batch size is out of range.");
  return Error();
}

Error HipEngine::ValidateRedundancyLocked(const char *what, int64_t n, const int64_t *pSources) const {
  if (_mode == Mode::Shutdown) return Error::MakeP(ErrCode::ObjectShutDown, std::string("RejectedOperation=") + what, "Engine is shut down.");
  for (int64_t i = 0; i < n; i++)
    if (pSources[i] < 0 || pSources[i] >= _qTotal)
      return Error::MakeP(ErrCode::IndexOutOfRange,
                          "entry=" + std::to_string(i) + " questionId=" + std::to_string(pSources[i]) + " " + RangeParams(pSources[i], 0, _qTotal - 1),
                          "A source question is out of range.");
  return Error();
}

Error HipEngine::EnsureRedundancyWeights(int64_t n) {
  const size_t need = (size_t)n * (size_t)(_K * RedPitch()) * sizeof(double);
  if (need <= _red.weightsBytes) return Error();
  HIP_TRY(hipStreamSynchronize(_stream));
  hipFree(_red.dWeights);
  _red.dWeights = nullptr; _red.weightsBytes = 0;
  HIP_TRY(hipMalloc((void **)&_red.dWeights, need));
  _red.weightsBytes = need;
  return Error();
}

// The weighted rows of up to kMaxBatch validated sources (GLOBAL ids) that this engine holds, into the slots at pDst: enqueued,
// nothing waited for -- except that the pinned list is not rewritten while an earlier call's copy of it is under way.  The sources
// stay in _dAqs + 2 for the launches behind this one.
Error HipEngine::PackRedundancyLocked(int64_t n, const int64_t *pSources, void *pDst, void *pFlag, uint64_t flagValue) {
  if (n == 0 && pFlag == nullptr) return Error();
  hipSetDevice(_device);
  if (_serverLaunched) StopServer();   // a launched kernel has no room beside the resident sweep and would wait for it to idle out
  const int64_t words = 2 + n;   // {arrival counter, pad}, then the sources
  Error err = EnsurePackList(words);
  if (!err.ok()) return err;
  for (int64_t i = 0; i < n; i++) _hPack[2 + i] = pSources[i];
  MarkStreamBusy();
  HIP_TRY(hipMemcpyAsync(_dAqs, _hPack, (size_t)words * sizeof(int64_t), hipMemcpyHostToDevice, _stream));
  HIP_TRY(hipEventRecord(_evPack, _stream));
  HIP_TRY(LaunchQuestionWeights(View(), _dAqs + 2, n, _qFirst, static_cast<double *>(pDst), RedPitch(), reinterpret_cast<unsigned *>(_dAqs),
                                static_cast<uint64_t *>(pFlag), flagValue, _stream));
  _redSources += (uint64_t)n;
  return Error();
}

// rows[i][RedRowPitch()] of up to kMaxBatch sources over this engine's questions from the package at dWeights (device-visible), on
// the engine's stream
Error HipEngine::RedundancyRowsLocked(int64_t n, const int64_t *dSources, const double *dWeights, bool zeroSelf) {
  RedundancyStage &st = _red;
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
  const KbView kb = View();
  HIP_TRY(grow(&st.dRows, st.rowsBytes, (size_t)n * (size_t)RedRowPitch() * sizeof(double)));
  HIP_TRY(grow(&st.dTables, st.tablesBytes, RedundancyTableBytes(kb)));
  HIP_TRY(LaunchRedundancySweep(kb, dWeights, RedPitch(), dSources, n, _qFirst, zeroSelf, st.dRows, RedRowPitch(), st.dTables, _stream));
  return Error();
}

// The listing of up to kMaxBatch sources over this engine's questions from a package: at most 256 records a source through the
// question listing, beyond that the rows copied and the prefix taken here in the same order -- I descending, question ascending; the
// source itself, the gaps and what is not > 0 are no candidates.  GLOBAL ids in the records.
Error HipEngine::ListFromWeightsLocked(int64_t n, const int64_t *dSources, const double *dWeights, int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) {
  for (int64_t i = 0; i < n; i++) pCounts[i] = 0;
  const int64_t want = std::min<int64_t>(maxCount, _Q);
  if (n == 0 || want <= 0) return Error();
  Error err = RedundancyRowsLocked(n, dSources, dWeights, true);
  if (!err.ok()) return err;
  RedundancyStage &st = _red;
  const int64_t rowPitch = RedRowPitch();
  if (want <= 256) {
    err = EnsureTopScratchRecords(n * TopQuestionsScratchRecords(_Q, want));
    if (!err.ok()) return err;
    if (!st.dSlots) HIP_TRY(hipMalloc((void **)&st.dSlots, (size_t)kMaxBatch * sizeof(QuizSlot)));
    const int64_t needRecords = n * want;
    if (needRecords > st.hRecords) {   // records | counts
      HIP_TRY(hipStreamSynchronize(_stream));
      if (st.hLines) hipHostFree(st.hLines);
      st.hLines = nullptr; st.hRecords = 0;
      HIP_TRY(hipHostMalloc((void **)&st.hLines, (size_t)needRecords * sizeof(RatedTargetDev) + (size_t)kMaxBatch * sizeof(int64_t), hipHostMallocDefault));
      st.hRecords = needRecords;
    }
    int64_t *hCounts = reinterpret_cast<int64_t *>(st.hLines + st.hRecords);
    HIP_TRY(LaunchRedundancySlots(st.dSlots, st.dRows, rowPitch, _dQGap, n, _stream));
    TopQuestions a{};
    a.slots = st.dSlots; a.qgap = _dQGap; a.nQuizzes = (int)n; a.Q = _Q;
    HIP_TRY(LaunchTopQuestions(a, want, _dTopScratch[0], _dTopScratch[1], st.hLines, hCounts, nullptr, 0, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
    for (int64_t i = 0; i < n; i++) {
      const int64_t c = std::max<int64_t>(0, std::min<int64_t>(hCounts[i], want));
      const RatedTargetDev *rec = st.hLines + i * want;
      CiRatedQuestion *dest = pDest + i * maxCount;
      for (int64_t j = 0; j < c; j++) { dest[j]._iQuestion = _qFirst + rec[j].iTarget; dest[j]._priority = rec[j].prob; }
      pCounts[i] = c;
    }
    return Error();
  }
  st.rows.resize((size_t)(n * rowPitch));
  HIP_TRY(hipMemcpyAsync(st.rows.data(), st.dRows, (size_t)(n * rowPitch) * sizeof(double), hipMemcpyDeviceToHost, _stream));
  HIP_TRY(hipStreamSynchronize(_stream));
  std::vector<int64_t> idx;
  for (int64_t i = 0; i < n; i++) {
    const double *v = st.rows.data() + i * rowPitch;
    idx.clear();
    for (int64_t q = 0; q < _Q; q++)
      if (v[q] > 0.0) idx.push_back(q);   // (the gaps and the source itself are zeros)
    const int64_t c = std::min<int64_t>(want, (int64_t)idx.size());
    std::partial_sort(idx.begin(), idx.begin() + c, idx.end(), [&](int64_t a, int64_t b) { return v[a] > v[b] || (v[a] == v[b] && a < b); });
    CiRatedQuestion *dest = pDest + i * maxCount;
    for (int64_t k = 0; k < c; k++) { dest[k]._iQuestion = _qFirst + idx[(size_t)k]; dest[k]._priority = v[idx[(size_t)k]]; }
    pCounts[i] = c;
  }
  return Error();
}

void HipEngine::RedundancyTimerStart() {
  if (!_opt.timeSweeps) return;
  if (!_red.ev[0] && (hipEventCreate(&_red.ev[0]) != hipSuccess || hipEventCreate(&_red.ev[1]) != hipSuccess)) { (void)hipGetLastError(); return; }
  if (hipEventRecord(_red.ev[0], _stream) != hipSuccess) (void)hipGetLastError();
}
void HipEngine::RedundancyTimerStop() {   // (the caller synchronises the stream behind it)
  if (!_opt.timeSweeps || !_red.ev[1]) return;
  float ms = 0;
  if (hipEventRecord(_red.ev[1], _stream) == hipSuccess && hipEventSynchronize(_red.ev[1]) == hipSuccess && hipEventElapsedTime(&ms, _red.ev[0], _red.ev[1]) == hipSuccess)
    _redDeviceNs += (uint64_t)(ms * 1e6);
  else (void)hipGetLastError();
}

Error HipEngine::EvalQuestionRedundancy(int64_t nSources, const int64_t *pSources, double *pOut, int64_t n) {
  Error err = RedundancyArgs(nSources, 0, false);
  if (!err.ok()) return err;
  if (nSources > 0 && (!pSources || !pOut)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the sources or the redundancy buffer.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  if (IsShard()) return OnShard("EvalQuestionRedundancy");
  if (n != _Q) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(n, _Q, _Q), "Redundancy row length must equal the question count.");
  err = ValidateRedundancyLocked("EvalQuestionRedundancy", nSources, pSources);
  if (!err.ok() || nSources == 0) return err;
  _redCalls++;
  err = EnsureRedundancyWeights(std::min<int64_t>(nSources, kMaxBatch));
  if (!err.ok()) return err;
  for (int64_t first = 0; first < nSources; first += kMaxBatch) {
    const int64_t m = std::min<int64_t>(kMaxBatch, nSources - first);
    RedundancyTimerStart();
    err = PackRedundancyLocked(m, pSources + first, _red.dWeights, nullptr, 0);
    if (err.ok()) err = RedundancyRowsLocked(m, _dAqs + 2, _red.dWeights, false);
    if (!err.ok()) return err;
    RedundancyTimerStop();
    HIP_TRY(hipMemcpy2DAsync(pOut + first * n, (size_t)n * sizeof(double), _red.dRows, (size_t)RedRowPitch() * sizeof(double), (size_t)n * sizeof(double), (size_t)m,
                             hipMemcpyDeviceToHost, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  return Error();
}

Error HipEngine::ListRedundantQuestionsBatch(int64_t nSources, const int64_t *pSources, int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts) {
  Error err = RedundancyArgs(nSources, maxCount, false);
  if (!err.ok()) return err;
  if (nSources > 0 && (!pSources || !pCounts || (maxCount > 0 && !pDest))) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  if (IsShard()) return OnShard("ListRedundantQuestionsBatch");
  err = ValidateRedundancyLocked("ListRedundantQuestionsBatch", nSources, pSources);
  if (!err.ok() || nSources == 0) return err;
  _redCalls++;
  for (int64_t i = 0; i < nSources; i++) pCounts[i] = 0;
  if (maxCount == 0) return Error();
  err = EnsureRedundancyWeights(std::min<int64_t>(nSources, kMaxBatch));
  if (!err.ok()) return err;
  for (int64_t first = 0; first < nSources; first += kMaxBatch) {
    const int64_t m = std::min<int64_t>(kMaxBatch, nSources - first);
    RedundancyTimerStart();
    err = PackRedundancyLocked(m, pSources + first, _red.dWeights, nullptr, 0);
    if (err.ok()) err = ListFromWeightsLocked(m, _dAqs + 2, _red.dWeights, maxCount, pDest + first * maxCount, pCounts + first);
    if (!err.ok()) return err;
    RedundancyTimerStop();   // (pack, sweep and listing; the stream has been synchronised)
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  return Error();
}

Error HipEngine::PackQuestionWeights(int64_t nSources, const int64_t *pSources, void *pDst, void *pFlag, uint64_t flagValue) {
  Error err = RedundancyArgs(nSources, 0, true);
  if (!err.ok()) return err;
  if (nSources > 0 && (!pSources || !pDst)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer or the package.");
  if ((reinterpret_cast<uintptr_t>(pDst) & 15) != 0) return Misaligned(pDst);
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  err = ValidateRedundancyLocked("PackQuestionWeights", nSources, pSources);
  if (!err.ok()) return err;
  _redCalls++;
  return PackRedundancyLocked(nSources, pSources, pDst, pFlag, flagValue);
}

// The sources on the device (_dAqs + 2) and the package where the sweep may read it: a package in host memory (registered, as
// PqaHip_HostRegister leaves it) is copied to the device first under option "rows_stage".
Error HipEngine::StageRedundancyLocked(int64_t n, const int64_t *pSources, const void *pWeights, const double **dWeights) {
  hipSetDevice(_device);
  if (_serverLaunched) StopServer();
  *dWeights = static_cast<const double *>(pWeights);
  if (_opt.rowsStage) {
    hipPointerAttribute_t at;
    const hipError_t q = hipPointerGetAttributes(&at, pWeights);
    if (q != hipSuccess) (void)hipGetLastError();
    if (q == hipSuccess && at.type == hipMemoryTypeHost) {
      Error err = EnsureRedundancyWeights(n);
      if (!err.ok()) return err;
      HIP_TRY(hipMemcpyAsync(_red.dWeights, pWeights, (size_t)(n * _K * RedPitch()) * sizeof(double), hipMemcpyDefault, _stream));
      *dWeights = _red.dWeights;
      _rowsStaged++;
    }
  }
  const int64_t words = 2 + n;
  Error err = EnsurePackList(words);
  if (!err.ok()) return err;
  for (int64_t i = 0; i < n; i++) _hPack[2 + i] = pSources[i];
  MarkStreamBusy();
  HIP_TRY(hipMemcpyAsync(_dAqs, _hPack, (size_t)words * sizeof(int64_t), hipMemcpyHostToDevice, _stream));
  HIP_TRY(hipEventRecord(_evPack, _stream));
  return Error();
}

Error HipEngine::EvalQuestionRedundancyFromWeights(int64_t nSources, const int64_t *pSources, const void *pWeights, double *pOut, int64_t n) {
  Error err = RedundancyArgs(nSources, 0, true);
  if (!err.ok()) return err;
  if (nSources > 0 && (!pSources || !pWeights || !pOut)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer or the package.");
  if ((reinterpret_cast<uintptr_t>(pWeights) & 15) != 0) return Misaligned(pWeights);
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  if (n != _Q) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(n, _Q, _Q), "Redundancy row length must equal the question count.");
  err = ValidateRedundancyLocked("EvalQuestionRedundancyFromWeights", nSources, pSources);
  if (!err.ok() || nSources == 0) return err;
  _redCalls++;
  const double *weights = nullptr;
  err = StageRedundancyLocked(nSources, pSources, pWeights, &weights);
  if (err.ok()) err = RedundancyRowsLocked(nSources, _dAqs + 2, weights, false);
  if (!err.ok()) return err;
  HIP_TRY(hipMemcpy2DAsync(pOut, (size_t)n * sizeof(double), _red.dRows, (size_t)RedRowPitch() * sizeof(double), (size_t)n * sizeof(double), (size_t)nSources,
                           hipMemcpyDeviceToHost, _stream));
  HIP_TRY(hipStreamSynchronize(_stream));
  _mu.busy = false;   // (the stream has just been synchronised)
  return Error();
}

Error HipEngine::ListRedundantQuestionsFromWeights(int64_t nSources, const int64_t *pSources, const void *pWeights, int64_t maxCount, CiRatedQuestion *pDest,
                                                   int64_t *pCounts) {
  Error err = RedundancyArgs(nSources, maxCount, true);
  if (!err.ok()) return err;
  if (nSources > 0 && (!pSources || !pWeights || !pCounts || (maxCount > 0 && !pDest)))
    return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer or the package.");
  if ((reinterpret_cast<uintptr_t>(pWeights) & 15) != 0) return Misaligned(pWeights);
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  err = ValidateRedundancyLocked("ListRedundantQuestionsFromWeights", nSources, pSources);
  if (!err.ok() || nSources == 0) return err;
  _redCalls++;
  for (int64_t i = 0; i < nSources; i++) pCounts[i] = 0;
  if (maxCount == 0) return Error();
  const double *weights = nullptr;
  err = StageRedundancyLocked(nSources, pSources, pWeights, &weights);
  if (err.ok()) err = ListFromWeightsLocked(nSources, _dAqs + 2, weights, maxCount, pDest, pCounts);
  if (err.ok()) _mu.busy = false;   // (the stream has just been synchronised)
  return err;
}

}  // namespace pqa
