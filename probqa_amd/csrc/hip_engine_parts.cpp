// hip_engine_parts.cpp -- HipEngine: the reference's sampled selector (PqaCore/CpuEngine.cpp:362-400) on a shard that a process of its
// own drives (probqa_amd/dist.py: next_question_sampled_batch).  The selector splits the GLOBAL question axis into subtasks and runs
// one Kahan chain per subtask; a shard holds a stretch of that axis, so it packs a SELECTION PART per quiz (sampled_part.h: the
// totals of the subtasks that lie whole inside it, the raw priorities of the at most two its bounds cut), the ranks all-gather the
// parts, every rank picks from all of them (select_kernels.hip), the ranks agree on the one pick that is not -1, and every rank
// takes it.  Nothing of the size of the question axis crosses between ranks.  A whole engine is a world of one.
#include "hip_engine_internal.h"
#include "sampled_part.h"

namespace pqa {

namespace {
Error PartsModeErr(const std::string &why) {
  return Error::Make(ErrCode::WrongMode, "Can't pick from these selection parts - " + why);
}
}  // namespace

int64_t HipEngine::SampledPartBytes() const {
  std::lock_guard<EngineMutex> lk(_mu);
  return sampled_part_bytes(sampled_split(_qTotal, SampledSubtasks()));
}

// The batched sweep PqaEngine_EvalPrioritiesBatch would run for this batch (the pole fix behind it), then ONE launch that writes
// the parts; nothing here waits for the device.
Error HipEngine::PackSampledParts(int64_t n, const int64_t *pQuizzes, void *pDst, void *pFlag, uint64_t flagValue) {
  std::lock_guard<std::mutex> selLk(_ctx[0].mu);   // (this context's staging buffers: not while a leader's combined sweep uses them)
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = ValidateBatchLocked(n, pQuizzes);
  if (!err.ok()) return err;
  if (n > 0 && !pDst) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the parts' buffer.");
  if ((reinterpret_cast<uintptr_t>(pDst) & 15) != 0)
    return Error::MakeP(ErrCode::IndexOutOfRange, "address mod 16=" + std::to_string(reinterpret_cast<uintptr_t>(pDst) & 15), "The parts' buffer must be 16-byte aligned.");
  if (n == 0 && pFlag == nullptr) return Error();
  hipSetDevice(_device);
  err = FlushUpdates();
  if (!err.ok()) return err;
  BatchCtx &c = _ctx[0];
  const int64_t nSub = SampledSubtasks();
  const SampledSplit sp = sampled_split(_qTotal, nSub);
  _parts.seq = 0;   // (whatever fails from here on: the previous pack's run lengths are no longer to be picked from)
  if (n > 0) {
    err = BatchSweep(c, n, pQuizzes, _batchQuizzes, true, NextLaunchTag());
    if (!err.ok()) return err;
  } else if (_serverLaunched) {
    StopServer();   // a launched kernel has no room beside the resident sweep and would wait for it to idle out
  }
  if (_dPartsWords == nullptr) HIP_TRY(hipMalloc((void **)&_dPartsWords, (2 + (size_t)kMaxBatch) * sizeof(uint64_t)));
  const bool matrix = c.lastBp > 0;
  const int Bq = matrix ? c.lastBp : (int)((n + 63) / 64 * 64);
  HIP_TRY(GrowDevice(&_dPartsRun, _partsRunBytes, (size_t)_Q * (size_t)std::max(Bq, 64) * sizeof(double)));
  HIP_TRY(hipMemsetAsync(_dPartsWords, 0, 2 * sizeof(uint64_t), _stream));   // the arrival counter
  const uint64_t seq = ++_opSeq;
  SampledPartsPack a{};
  a.slots = c.dSlots; a.nSlots = (int)n; a.Bq = Bq;
  a.priorityT = matrix ? c.dPriT : nullptr;
  a.qgap = _dQGap;
  a.qFirst = _qFirst; a.nLocal = _Q; a.qTotal = _qTotal; a.nWorkers = nSub;
  a.dst = static_cast<char *>(pDst); a.partBytes = sampled_part_bytes(sp);
  a.run = _dPartsRun; a.stamp = _dPartsWords + 2; a.seq = seq;
  a.counter = reinterpret_cast<unsigned *>(_dPartsWords); a.flag = static_cast<uint64_t *>(pFlag); a.flagValue = flagValue;
  MarkStreamBusy();
  HIP_TRY(LaunchSampledPackParts(a, _stream));
  if (n == 0) return Error();
  _parts.seq = seq;
  _parts.quizzes.assign(pQuizzes, pQuizzes + n);
  _parts.serials.resize((size_t)n);
  _parts.versions.resize((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    _parts.serials[(size_t)i] = _batchQuizzes[(size_t)i]->serial;
    _parts.versions[(size_t)i] = _batchQuizzes[(size_t)i]->priorVersion;
  }
  _parts.nSub = nSub; _parts.qFirst = _qFirst; _parts.nLocal = _Q; _parts.qTotal = _qTotal; _parts.kbVersion = _kbVersion;
  _parts.runQuiz = matrix ? 1 : _Q;
  _parts.runStride = matrix ? Bq : 1;
  return Error();
}

// One launch over the gathered parts; no bookkeeping, no change of quiz state.
Error HipEngine::SampledPickFromParts(int64_t n, const int64_t *pQuizzes, const uint64_t *pRnd, const void *pParts, int64_t rank, int64_t world,
                                      CiHipSelection *pOut) {
  std::lock_guard<std::mutex> selLk(_ctx[0].mu);
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = ValidateBatchLocked(n, pQuizzes);
  if (!err.ok() || n == 0) return err;
  if (!pRnd || !pParts || !pOut) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  if (world < 1 || world > kSampledMaxWorld) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(world, 1, kSampledMaxWorld), "The number of ranks is out of range.");
  if (rank < 0 || rank >= world) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(rank, 0, world - 1), "The rank is out of range.");
  // the engine's latest pack must be of this very batch, and nothing it depends on may have changed since
  BatchCtx &c = _ctx[0];
  if (_parts.seq == 0 || c.h == nullptr) return PartsModeErr("this engine has packed no parts since it last failed to.");
  bool same = (int64_t)_parts.quizzes.size() == n && _parts.nSub == SampledSubtasks() && _parts.qFirst == _qFirst && _parts.nLocal == _Q &&
              _parts.qTotal == _qTotal && _parts.kbVersion == _kbVersion;
  for (int64_t i = 0; same && i < n; i++) {
    const Quiz *q = _quizzes[(size_t)pQuizzes[i]];
    same = _parts.quizzes[(size_t)i] == pQuizzes[i] && q->serial == _parts.serials[(size_t)i] && q->priorVersion == _parts.versions[(size_t)i];
  }
  if (!same) return PartsModeErr("the engine's latest pack was made for another batch, or a quiz, the gaps or the split have changed since.");
  hipSetDevice(_device);
  const SampledSplit sp = sampled_split(_qTotal, _parts.nSub);
  HIP_TRY(GrowDevice(&_dPartsGrand, _partsGrandBytes, (size_t)n * (size_t)sp.nS * sizeof(double)));
  HIP_TRY(GrowDevice(&_dPartsPickRun, _partsPickRunBytes, (size_t)n * (size_t)sp.L * sizeof(double)));
  std::memcpy(c.h->rnd, pRnd, (size_t)n * sizeof(uint64_t));   // (host-coherent: the kernel reads them there)
  const uint64_t tag = NextLaunchTag();
  SampledPartsPick a{};
  a.nSlots = (int)n; a.world = (int)world; a.rank = (int)rank;
  a.parts = static_cast<const char *>(pParts); a.partBytes = sampled_part_bytes(sp);
  a.qTotal = _qTotal; a.nWorkers = _parts.nSub;
  a.rnd = c.h->rnd;
  a.packRun = _dPartsRun; a.packRunQuiz = _parts.runQuiz; a.packRunStride = _parts.runStride;
  a.stamp = _dPartsWords + 2; a.seq = _parts.seq;
  a.grand = _dPartsGrand; a.run = _dPartsPickRun;
  a.out = c.h->out; a.flags = c.h->seq; a.flagValue = tag;
  if (_serverLaunched) StopServer();   // a launched kernel has no room beside the resident sweep and would wait for it to idle out
  HIP_TRY(LaunchSampledPickParts(a, _stream));
  err = WaitBatchFlags(c, n, tag);
  if (!err.ok()) return err;
  for (int64_t i = 0; i < n; i++) {
    if (c.h->out[i].index == -2) return PartsModeErr("the part of this rank is not of the engine's latest pack (a stale sequence number).");
    if (c.h->out[i].index == kSelIncomplete) return PartsModeErr("the parts' question ranges do not tile the question axis, or they were packed under another subtask count.");
  }
  for (int64_t i = 0; i < n; i++) {
    pOut[i]._priority = c.h->out[i].priority;
    pOut[i]._iQuestion = c.h->out[i].index;
  }
  return Error();
}

// Host only: the agreed picks become the quizzes' active questions -- through the reference's fallback (PqaCore/CpuEngine.cpp:403-407,
// BaseEngine::FindNearestQuestion) over the WHOLE question axis, which every rank can run alike: the axis' gaps are replicated, and
// a quiz keeps its answered questions, other ranks' among them.
Error HipEngine::TakeSampledPicks(int64_t n, const int64_t *pQuizzes, const int64_t *pPicks, int64_t *pQuestions) {
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = ValidateBatchLocked(n, pQuizzes);
  if (!err.ok() || n == 0) return err;
  if (!pPicks || !pQuestions) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  for (int64_t i = 0; i < n; i++)
    if (pPicks[i] < 0 || pPicks[i] >= _qTotal)
      return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(pPicks[i], 0, _qTotal - 1), "Batch entry " + std::to_string(i) + ": the pick is not a question of the KB.");
  const int64_t packs = (_qTotal + 63) >> 6;
  std::vector<uint64_t> gaps((size_t)packs, 0), taken;
  auto mark = [](std::vector<uint64_t> &w, int64_t q) { w[(size_t)(q >> 6)] |= 1ULL << (q & 63); };
  if (IsShard()) for (int64_t g : _globalQuestionGaps) mark(gaps, g);
  else for (int64_t g : _questionGapList) mark(gaps, g);
  if (_qTotal & 63) gaps[(size_t)packs - 1] |= ~0ULL << (_qTotal & 63);   // (questions past the count are never available)
  for (int64_t i = 0; i < n; i++) {
    Quiz *q = _quizzes[(size_t)pQuizzes[i]];
    taken = gaps;
    for (const AQ &aq : q->answers) mark(taken, aq.iQuestion);
    int64_t sel = pPicks[i];
    if ((taken[(size_t)(sel >> 6)] >> (sel & 63)) & 1) sel = FindNearestInPacks(sel, _qTotal, [&](int64_t p) { return ~taken[(size_t)p]; });
    if (sel >= 0) {
      q->activeQuestion = sel;
      _nQuestionsAsked.fetch_add(1, std::memory_order_relaxed);
    }
    pQuestions[i] = sel;   // (-1: no question left, as the batch calls report it)
  }
  return Error();
}

}  // namespace pqa
