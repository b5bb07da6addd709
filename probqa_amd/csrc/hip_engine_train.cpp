// hip_engine_train.cpp -- HipEngine: many trainings in one call -- TrainBatch (logged quizzes, a KB built from records) and
// RecordQuizTargetBatch (many finished quizzes) -- as chunks of one launch each (kb_kernels.hip: train_chains_kernel).
//
// Why the KB ends bit-identical to consecutive Train / RecordQuizTarget calls in record order.  A record with target t touches
// only column t: A[q][*][t], D[q][t] and vB[t].  A cell ends with the same bits if the floating-point operations on it are the
// same and run in the same order.  Every step's operations depend only on the cells it touches and its record's amount, so:
//   * steps of different targets touch disjoint cells and commute exactly;
//   * steps of one target on different questions touch disjoint cells and commute exactly;
//   * only the steps on one (t, q) must keep their order.
// A chain is the steps on one (t, q): in record order and, within a record, in BuildTrainSteps' execution order.  One lane runs
// a chain from first to last; another lane adds target t's amounts to vB[t] in record order.  The batch is cut into chunks
// anywhere in the sequence of steps taken in record order (a record may straddle two chunks): the chunks run one after the
// other on the engine's stream, so every cell still sees its steps in that sequence's order.
#include "hip_engine_internal.h"

namespace pqa {

struct HipEngine::TrainBulk {
  // host scratch (grown, never shrunk): one record's steps, the chunk's steps in record order with their chain links, the chunk's
  // records, per-target and per-question list heads (-1 between calls; reset only where touched)
  std::vector<TrainStep> recSteps;
  std::vector<int64_t> bucketScratch;
  std::vector<TrainChainStep> seq;      // kindRec = local record << 2 | kind, until the chain pass rewrites it
  std::vector<int32_t> next;            // per step of seq: the next step of its chain
  std::vector<int32_t> recFirst;        // per local record: its first step in seq (+ an end marker)
  std::vector<int64_t> recOf;           // per local record: the batch record
  std::vector<int32_t> recNext, amountAt;
  std::vector<int32_t> tHead, tTail, qHead, qTail;
  std::vector<int64_t> touchedT;
  std::vector<int32_t> touchedQ;
  std::vector<TrainChain> targetSlots;
  // staging: two pinned host buffers and their device twins, so that chunk k+1 is prepared while chunk k runs
  char *h[2] = {nullptr, nullptr}, *d[2] = {nullptr, nullptr};
  size_t hBytes[2] = {0, 0}, dBytes[2] = {0, 0};
  hipEvent_t ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [slot][start, end] around the slot's launch
  bool inFlight[2] = {false, false};
};

void HipEngine::FreeTrainBulk() {
  if (!_tb) return;
  for (int s = 0; s < 2; s++) {
    if (_tb->inFlight[s]) hipEventSynchronize(_tb->ev[s][1]);
    hipHostFree(_tb->h[s]);
    hipFree(_tb->d[s]);
    for (hipEvent_t e : _tb->ev[s]) if (e) hipEventDestroy(e);
  }
  delete _tb;
  _tb = nullptr;
}

namespace {
Error EntryError(int64_t i, Error e) {
  e.message = "Batch entry " + std::to_string(i) + ": " + e.message;
  return e;
}
constexpr int64_t kChunkRecords = int64_t(1) << 20;   // (a chunk's records: amounts indexed by 30 bits of kindRec)
}  // namespace

// ---- arguments and validation ---------------------------------------------------------------------------------------------------
// Train's checks (hip_engine_update.cpp: Train) entry by entry, before the lock.
Error HipEngine::CheckTrainBatchArgs(int64_t n, const int64_t *pCounts, const AQ *pAQs, const int64_t *pTargets, const double *pAmounts) {
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "|nRecords| must be non-negative.");
  if (n > 0 && (!pCounts || !pTargets || !pAmounts)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  for (int64_t i = 0; i < n; i++) {
    if (pCounts[i] < 0)
      return EntryError(i, Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(pCounts[i]), "|nQuestions| must be non-negative."));
    if (!(pAmounts[i] > 0))
      return EntryError(i, Error::MakeP(ErrCode::NonPositiveAmount, "amount=" + std::to_string(pAmounts[i]), "|amount| must be positive."));
    if (pCounts[i] > 0 && pAQs == nullptr)
      return EntryError(i, Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of answered questions."));
  }
  return Error();
}

// RecordQuizTarget's check before the lock (hip_engine_update.cpp: RecordQuizTarget).
Error HipEngine::CheckQuizTargetBatchArgs(int64_t n, const int64_t *pQuizzes, const int64_t *pTargets, const double *pAmounts) {
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "|nQuizzes| must be non-negative.");
  if (n > 0 && (!pQuizzes || !pTargets || !pAmounts)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  for (int64_t i = 0; i < n; i++)
    if (!(pAmounts[i] > 0))
      return EntryError(i, Error::MakeP(ErrCode::NonPositiveAmount, "amount=" + std::to_string(pAmounts[i]), "|amount| must be positive."));
  return Error();
}

// Everything the single calls check under the lock, for every entry before any cell changes.
Error HipEngine::ValidateTrainBatchLocked(int64_t n, const int64_t *pCounts, const AQ *pAQs, const int64_t *pTargets, const int64_t *pQuizzes) {
  if (pQuizzes == nullptr) {
    if (_mode == Mode::Shutdown) return Error::MakeP(ErrCode::ObjectShutDown, "RejectedOperation=Train", "Engine is shut down.");
    for (int64_t i = 0, at = 0; i < n; at += pCounts[i], i++) {
      Error e = ValidateTrainLocked(pCounts[i], pAQs + at, pTargets[i]);
      if (!e.ok()) return EntryError(i, e);
    }
    return Error();
  }
  Error err = CheckRegular("record quiz target");
  if (!err.ok()) return err;
  for (int64_t i = 0; i < n; i++) {   // RecordQuizTargetLocked's order: target range, target gap, the quiz, then its answers
    const int64_t iTarget = pTargets[i];
    if (iTarget < 0 || iTarget >= _T)
      return EntryError(i, Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(iTarget, 0, _T - 1), "Target index is not in KB range."));
    if (BitTest(_hTGap, iTarget))
      return EntryError(i, Error::MakeP(ErrCode::AbsentId, "id=" + std::to_string(iTarget), "Target index is not in KB (but rather at a gap)."));
    Quiz *q = UseQuiz(err, pQuizzes[i]);
    if (!q) return EntryError(i, err);
    err = ValidateTrainLocked((int64_t)q->answers.size(), q->answers.data(), iTarget);
    if (!err.ok()) return EntryError(i, err);
  }
  return Error();
}

Error HipEngine::ValidateTrainBatch(int64_t n, const int64_t *pCounts, const AQ *pAQs, const int64_t *pTargets, const int64_t *pQuizzes) {
  std::lock_guard<EngineMutex> lk(_mu);
  return ValidateTrainBatchLocked(n, pCounts, pAQs, pTargets, pQuizzes);
}

// ---- the two calls --------------------------------------------------------------------------------------------------------------
Error HipEngine::TrainBatch(int64_t n, const int64_t *pCounts, const AQ *pAQs, const int64_t *pTargets, const double *pAmounts) {
  Error err = CheckTrainBatchArgs(n, pCounts, pAQs, pTargets, pAmounts);
  if (!err.ok() || n == 0) return err;
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  err = ValidateTrainBatchLocked(n, pCounts, pAQs, pTargets, nullptr);
  if (!err.ok()) return err;
  std::vector<TrainRecord> recs((size_t)n);
  int64_t total = 0;
  for (int64_t i = 0; i < n; total += pCounts[i], i++) recs[(size_t)i] = TrainRecord{pAQs + total, pCounts[i], pTargets[i], pAmounts[i]};
  err = TrainRecordsLocked(recs, false);
  if (err.ok()) _nQuestionsAsked.fetch_add((uint64_t)total, std::memory_order_relaxed);   // reference CpuEngine.cpp:176, per record
  return err;
}

Error HipEngine::RecordQuizTargetBatch(int64_t n, const int64_t *pQuizzes, const int64_t *pTargets, const double *pAmounts) {
  Error err = CheckQuizTargetBatchArgs(n, pQuizzes, pTargets, pAmounts);
  if (!err.ok() || n == 0) return err;
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  err = ValidateTrainBatchLocked(n, nullptr, nullptr, pTargets, pQuizzes);
  if (!err.ok()) return err;
  std::vector<TrainRecord> recs((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    const Quiz *q = _quizzes[(size_t)pQuizzes[i]];   // (validated: present; the lock keeps its answers as they are)
    recs[(size_t)i] = TrainRecord{q->answers.data(), (int64_t)q->answers.size(), pTargets[i], pAmounts[i]};
  }
  return TrainRecordsLocked(recs, true);   // (the asked-questions counter is not touched: CpuEngine.cpp:442-466)
}

// ---- host preparation and launches ----------------------------------------------------------------------------------------------
// The records are valid.  Linear in records + steps; no allocation once the scratch and staging have grown to the batch's size.
Error HipEngine::TrainRecordsLocked(const std::vector<TrainRecord> &recs, bool fromQuiz) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  clock::duration waited{};
  StopServer();   // the cube changes (as in TrainLocked): deferred updates run first, a speculative sweep is dropped
  hipSetDevice(_device);
  if (!_tb) _tb = new TrainBulk();
  TrainBulk &b = *_tb;
  if ((int64_t)b.tHead.size() < _T) { b.tHead.resize((size_t)_T, -1); b.tTail.resize((size_t)_T, -1); }
  if ((int64_t)b.qHead.size() < _Q) { b.qHead.resize((size_t)_Q, -1); b.qTail.resize((size_t)_Q, -1); }
  for (int s = 0; s < 2; s++)
    for (hipEvent_t &e : b.ev[s])
      if (!e) HIP_TRY(hipEventCreate(&e));
  const int64_t cap = _opt.trainChunkSteps;
  int slot = 0;
  uint64_t launches = 0;

  // wait until slot s's previous launch has run (its staging is free again) and count its device time
  auto settle = [&](int s) -> hipError_t {
    if (!b.inFlight[s]) return hipSuccess;
    const auto w0 = clock::now();
    hipError_t he = hipEventSynchronize(b.ev[s][1]);
    waited += clock::now() - w0;
    b.inFlight[s] = false;
    float ms = 0;
    if (he == hipSuccess && hipEventElapsedTime(&ms, b.ev[s][0], b.ev[s][1]) == hipSuccess) _trainBulkDeviceNs += (uint64_t)(ms * 1e6);
    return he;
  };

  // One chunk: the steps in seq, the records in recOf (the last one continues into the next chunk if `continues`: its vB
  // amount is added there).  Groups the records by target, the steps of each target by question, stages, launches.
  auto flush = [&](bool continues) -> hipError_t {
    const int64_t nLocal = (int64_t)b.recOf.size(), nSteps = (int64_t)b.seq.size();
    if (nLocal == 0) return hipSuccess;
    b.recFirst.push_back((int32_t)nSteps);
    // records by target, each target's in record order
    b.recNext.resize((size_t)nLocal);
    b.amountAt.resize((size_t)nLocal);
    for (int64_t i = 0; i < nLocal; i++) {
      const int64_t t = recs[(size_t)b.recOf[(size_t)i]].iTarget;
      if (b.tHead[(size_t)t] < 0) { b.tHead[(size_t)t] = (int32_t)i; b.touchedT.push_back(t); }
      else b.recNext[(size_t)b.tTail[(size_t)t]] = (int32_t)i;
      b.tTail[(size_t)t] = (int32_t)i;
      b.recNext[(size_t)i] = -1;
    }
    const int64_t nT = (int64_t)b.touchedT.size();
    // staging layout: [amounts: nLocal doubles | chains and target slots: <= nSteps + nT | steps: nSteps]
    const size_t offChains = (size_t)nLocal * sizeof(double);
    const size_t offSteps = offChains + (size_t)(nSteps + nT) * sizeof(TrainChain);
    const size_t need = offSteps + (size_t)nSteps * sizeof(TrainChainStep);
    hipError_t he = settle(slot);
    if (he != hipSuccess) return he;
    if (need > b.hBytes[slot]) {
      hipHostFree(b.h[slot]);
      b.h[slot] = nullptr;
      b.hBytes[slot] = 0;
      he = hipHostMalloc((void **)&b.h[slot], need + need / 2, hipHostMallocDefault);
      if (he != hipSuccess) return he;
      b.hBytes[slot] = need + need / 2;
    }
    if (need > b.dBytes[slot]) {
      hipFree(b.d[slot]);
      b.d[slot] = nullptr;
      b.dBytes[slot] = 0;
      he = hipMalloc((void **)&b.d[slot], need + need / 2);
      if (he != hipSuccess) return he;
      b.dBytes[slot] = need + need / 2;
    }
    double *amounts = reinterpret_cast<double *>(b.h[slot]);
    TrainChain *chains = reinterpret_cast<TrainChain *>(b.h[slot] + offChains);
    TrainChainStep *steps = reinterpret_cast<TrainChainStep *>(b.h[slot] + offSteps);
    // amounts grouped by target, in record order within a target: the vB lanes' ranges; each record's position is its index
    b.targetSlots.clear();
    int32_t at = 0;
    for (int64_t t : b.touchedT) {
      const int32_t first = at;
      for (int32_t i = b.tHead[(size_t)t]; i >= 0; i = b.recNext[(size_t)i]) {
        amounts[at] = recs[(size_t)b.recOf[(size_t)i]].amount;
        b.amountAt[(size_t)i] = at++;
      }
      const bool last = continues && b.tTail[(size_t)t] == nLocal - 1;   // (its amount belongs to the next chunk's vB lane)
      b.targetSlots.push_back(TrainChain{t, first, at - (last ? 1 : 0)});
    }
    // chains: per target, its steps linked per question in record order, then written out chain by chain
    b.next.resize((size_t)nSteps);
    int32_t nChains = 0, out = 0;
    for (int64_t t : b.touchedT) {
      for (int32_t i = b.tHead[(size_t)t]; i >= 0; i = b.recNext[(size_t)i])
        for (int32_t j = b.recFirst[(size_t)i]; j < b.recFirst[(size_t)i + 1]; j++) {
          const int32_t q = b.seq[(size_t)j].q;
          if (b.qHead[(size_t)q] < 0) { b.qHead[(size_t)q] = j; b.touchedQ.push_back(q); }
          else b.next[(size_t)b.qTail[(size_t)q]] = j;
          b.qTail[(size_t)q] = j;
          b.next[(size_t)j] = -1;
        }
      for (int32_t q : b.touchedQ) {
        const int32_t first = out;
        for (int32_t j = b.qHead[(size_t)q]; j >= 0; j = b.next[(size_t)j]) {
          TrainChainStep st = b.seq[(size_t)j];
          st.kindRec = (uint32_t)b.amountAt[(size_t)(st.kindRec >> 2)] << 2 | (st.kindRec & 3u);
          steps[out++] = st;
        }
        chains[nChains++] = TrainChain{t, first, out};
        b.qHead[(size_t)q] = -1;
        b.qTail[(size_t)q] = -1;
      }
      b.touchedQ.clear();
    }
    for (int64_t j = 0; j < nT; j++) chains[nChains + j] = b.targetSlots[(size_t)j];
    for (int64_t t : b.touchedT) { b.tHead[(size_t)t] = -1; b.tTail[(size_t)t] = -1; }
    b.touchedT.clear();
    he = hipMemcpyAsync(b.d[slot], b.h[slot], need, hipMemcpyHostToDevice, _stream);
    if (he == hipSuccess) he = hipEventRecord(b.ev[slot][0], _stream);
    if (he == hipSuccess)
      he = LaunchTrainChains(_dCube, _elem, _dVB, _K, _ldT, reinterpret_cast<const TrainChain *>(b.d[slot] + offChains), nChains, nT,
                             reinterpret_cast<const TrainChainStep *>(b.d[slot] + offSteps), reinterpret_cast<const double *>(b.d[slot]), _stream);
    if (he == hipSuccess) he = hipEventRecord(b.ev[slot][1], _stream);
    if (he != hipSuccess) return he;
    b.inFlight[slot] = true;
    slot ^= 1;
    launches++;
    b.seq.clear();
    b.recOf.clear();
    b.recFirst.clear();
    return hipSuccess;
  };

  hipError_t he = hipSuccess;
  b.seq.clear();
  b.recOf.clear();
  b.recFirst.clear();
  for (size_t r = 0; r < recs.size() && he == hipSuccess; r++) {
    b.recSteps.clear();
    AppendTrainSteps(recs[r].n, recs[r].pAQs, fromQuiz, b.recSteps, b.bucketScratch);
    const int64_t nRec = (int64_t)b.recSteps.size();
    if ((nRec > 0 && (int64_t)b.seq.size() == cap) || (int64_t)b.recOf.size() == kChunkRecords) he = flush(false);
    if (he != hipSuccess) break;
    b.recOf.push_back((int64_t)r);
    b.recFirst.push_back((int32_t)b.seq.size());
    for (int64_t k = 0; k < nRec;) {
      if ((int64_t)b.seq.size() == cap) {   // full in the middle of record r: the rest of it opens the next chunk
        he = flush(true);
        if (he != hipSuccess) break;
        b.recOf.push_back((int64_t)r);
        b.recFirst.push_back(0);
      }
      const uint32_t local = (uint32_t)(b.recOf.size() - 1);
      const int64_t take = std::min<int64_t>(nRec - k, cap - (int64_t)b.seq.size());
      for (int64_t i = 0; i < take; i++, k++) {
        const TrainStep &st = b.recSteps[(size_t)k];
        b.seq.push_back(TrainChainStep{(int32_t)st.q, local << 2 | (uint32_t)st.kind, (int32_t)st.a1, (int32_t)st.a2});
      }
    }
  }
  if (he == hipSuccess) he = flush(false);
  const hipError_t h0 = settle(0), h1 = settle(1);
  if (he == hipSuccess) he = h0 != hipSuccess ? h0 : h1;
  _trainBulkHostNs += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(clock::now() - t0 - waited).count();
  _trainBulkLaunches += launches;
  if (he != hipSuccess) return HipErr(he, "TrainBatch / RecordQuizTargetBatch");
  _trainBulkCalls++;
  _trainBulkRecords += (uint64_t)recs.size();
  return Error();
}

}  // namespace pqa
