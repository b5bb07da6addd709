// hip_engine_resume.cpp -- HipEngine: ResumeQuiz for many quizzes at once -- ResumeQuizBatch, the ResumeQuiz calls a drain gathers
// (option "combine"), and a single ResumeQuiz on long rows -- with one launch sequence and one synchronisation per chunk
// (prior_kernels.hip: resume_quiz_batch_kernel, the long-row resume).  Every posterior is the one CreateQuiz's resume_quiz_kernel
// gives, bit for bit, and every quiz is built as CreateQuiz builds it (asked bits, answers, lastUsage).
#include "hip_engine_internal.h"

namespace pqa {

namespace {
// Exponent scratch (ldT int64 per quiz of a chunk) a chunk may take: 256 quizzes up to 32768-target rows, fewer beyond (83 at
// 100000 targets).  The tables grow to the largest chunk so far and stay.
constexpr size_t kResumeExpsBudget = (size_t)64 << 20;
inline size_t Align256(size_t x) { return (x + 255) & ~(size_t)255; }
}  // namespace

Error HipEngine::ResumeEntriesLocked(std::vector<ResumeEntry> &e, bool allOrNone) {
  Error err = CheckRegular("Start/Resume quiz");
  if (!err.ok()) {
    for (ResumeEntry &x : e) x.err = err;
    return err;
  }
  hipSetDevice(_device);
  const int64_t n = (int64_t)e.size();
  const size_t askedWords = BitWords(_Q);
  auto drop = [&](ResumeEntry &x) {
    if (x.quiz != nullptr) DestroyQuiz(x.quiz);
    x.quiz = nullptr;
    x.id = -1;
  };
  auto failAll = [&](const Error &er) {
    for (ResumeEntry &x : e) drop(x);
    return er;
  };
  // ---- validate (reference PqaCore/CpuEngine.cpp:216-233) and take every quiz's buffers
  for (int64_t i = 0; i < n; i++) {
    ResumeEntry &x = e[(size_t)i];
    std::unique_ptr<Quiz> quiz(new Quiz());
    quiz->hAsked.assign(askedWords, 0);
    bool allLocal = true;
    for (int64_t j = 0; j < x.nAnswered && x.err.ok(); j++) {
      const int64_t iq = x.pAQs[j].iQuestion, ia = x.pAQs[j].iAnswer;
      if (iq < 0 || iq >= _qTotal)
        x.err = Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(iq, 0, _qTotal - 1), "Question index is not in KB range.");
      else if (ia < 0 || ia >= _K)
        x.err = Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(ia, 0, _K - 1), "Answer index is not in KB range.");
      else if (iq >= _qFirst && iq < _qFirst + _Q) BitSet(quiz->hAsked, iq - _qFirst, true);
      else allLocal = false;
    }
    if (x.err.ok() && !allLocal && x.rows == nullptr)
      x.err = Error::MakeP(ErrCode::NotImplemented, "Feature=ResumeQuiz across separately driven shards",
                           "An answered question belongs to another shard: its rows are not reachable from this engine alone "
                           "(PQA_DEVICES / the sharded engine of one process resolves them).");
    if (x.err.ok()) {
      quiz->serial = ++_quizSerial;
      quiz->pin = TakePin();
      if (quiz->pin == nullptr) x.err = HipErr(hipErrorOutOfMemory, "quiz result lines");
      else {
        const hipError_t he = TakeQuizBuffers(quiz.get());
        if (he != hipSuccess) x.err = HipErr(he, "quiz allocation");
      }
      if (!x.err.ok()) DestroyQuiz(quiz.release());   // (its pin and whatever buffers it got go back)
    }
    if (!x.err.ok()) {
      if (allOrNone) return failAll(x.err);
      continue;
    }
    x.quiz = quiz.release();
  }
  // ---- the entries without answers are StartQuiz (BaseEngine.cpp:393-395): one start_quiz_batch_kernel per kStartInline of them
  const KbView kb = View();
  std::unique_ptr<StartBatchInline> starts(new StartBatchInline());
  starts->n = 0;
  starts->askedWords = (int64_t)askedWords;
  std::vector<ResumeEntry *> startChunk;
  auto launchStarts = [&]() -> hipError_t {
    hipError_t he = hipSuccess;
    if (starts->n > 0) {
      MarkStreamBusy();
      he = LaunchStartQuizBatch(kb, *starts, _opt.workers, _stream);
      if (he != hipSuccess)
        for (ResumeEntry *x : startChunk) { drop(*x); x->err = HipErr(he, "StartQuiz"); }
    }
    starts->n = 0;
    startChunk.clear();
    return he;
  };
  for (ResumeEntry &x : e) {
    if (x.quiz == nullptr || x.nAnswered != 0) continue;
    starts->prior[starts->n] = x.quiz->dPrior;
    starts->asked[starts->n] = x.quiz->dAsked;
    starts->n++;
    startChunk.push_back(&x);
    if (starts->n == kStartInline && launchStarts() != hipSuccess && allOrNone) return failAll(x.err);
  }
  if (launchStarts() != hipSuccess && allOrNone) {
    for (ResumeEntry &x : e) if (!x.err.ok()) return failAll(x.err);
  }
  // ---- the resumes, in chunks: one copy of the chunk's tables, the launch sequence, one copy of the statuses back, one synchronisation
  const bool longRow = ResumeTakesLongRow(kb);
  const int64_t chunkCap = std::max<int64_t>(1, std::min<int64_t>(kResumeChunk, (int64_t)(kResumeExpsBudget / ((size_t)_ldT * sizeof(int64_t)))));
  const int64_t stride = ResumeLongStride(_opt.workers);
  std::vector<ResumeEntry *> chunk;
  size_t next = 0;
  for (;;) {
    chunk.clear();
    size_t nRows = 0;
    for (; next < e.size() && (int64_t)chunk.size() < chunkCap; next++)
      if (e[next].quiz != nullptr && e[next].nAnswered > 0) { chunk.push_back(&e[next]); nRows += 2 * (size_t)e[next].nAnswered; }
    if (chunk.empty()) break;
    const size_t m = chunk.size();
    const size_t offStatus = Align256(m * sizeof(ResumeSlot));
    const size_t offAsked = offStatus + Align256(m * 2 * sizeof(int64_t));
    const size_t offRows = offAsked + Align256(m * askedWords * sizeof(uint32_t));
    const size_t hostBytes = offRows + Align256(nRows * sizeof(void *));
    const size_t offLong = hostBytes;
    const size_t offExps = offLong + (longRow ? Align256(m * (size_t)stride * sizeof(uint64_t)) : 0);
    const size_t devBytes = offExps + m * (size_t)_ldT * sizeof(int64_t);
    hipError_t he = hipSuccess;
    if (devBytes > _dResumeBytes) {   // (nothing in flight uses the tables: every chunk before was synchronised)
      hipFree(_dResume);
      _dResume = nullptr;
      _dResumeBytes = 0;
      he = hipMalloc((void **)&_dResume, devBytes);
      if (he == hipSuccess) _dResumeBytes = devBytes;
    }
    if (he == hipSuccess && hostBytes > _hResumeBytes) {
      hipHostFree(_hResume);
      _hResume = nullptr;
      _hResumeBytes = 0;
      he = hipHostMalloc((void **)&_hResume, hostBytes, hipHostMallocDefault);
      if (he == hipSuccess) _hResumeBytes = hostBytes;
    }
    if (he == hipSuccess) {
      ResumeSlot *slots = reinterpret_cast<ResumeSlot *>(_hResume);
      const void **rows = reinterpret_cast<const void **>(_hResume + offRows);
      size_t at = 0;
      for (size_t k = 0; k < m; k++) {
        const ResumeEntry &x = *chunk[k];
        std::memcpy(_hResume + offAsked + k * askedWords * sizeof(uint32_t), x.quiz->hAsked.data(), askedWords * sizeof(uint32_t));
        slots[k] = ResumeSlot{x.quiz->dPrior, x.quiz->dAsked, reinterpret_cast<const uint32_t *>(_dResume + offAsked + k * askedWords * sizeof(uint32_t)),
                              reinterpret_cast<const void *const *>(_dResume + offRows + at * sizeof(void *)),
                              reinterpret_cast<int64_t *>(_dResume + offExps + k * (size_t)_ldT * sizeof(int64_t)),
                              reinterpret_cast<int64_t *>(_dResume + offStatus + k * 2 * sizeof(int64_t)), x.nAnswered, 0};
        for (int64_t j = 0; j < x.nAnswered; j++, at += 2) {
          if (x.rows != nullptr) { rows[at] = x.rows[2 * j]; rows[at + 1] = x.rows[2 * j + 1]; continue; }
          rows[at] = CubeAt(x.pAQs[j].iQuestion - _qFirst, x.pAQs[j].iAnswer);
          rows[at + 1] = CubeAt(x.pAQs[j].iQuestion - _qFirst, _K);
        }
      }
      he = hipMemcpyAsync(_dResume, _hResume, hostBytes, hipMemcpyHostToDevice, _stream);
    }
    if (he == hipSuccess && longRow) he = hipMemsetAsync(_dResume + offLong, 0, m * (size_t)stride * sizeof(uint64_t), _stream);
    if (he == hipSuccess)
      he = LaunchResumeQuizBatch(kb, reinterpret_cast<const ResumeSlot *>(_dResume), (int64_t)m, (int64_t)askedWords, _opt.workers, (int)_opt.bugCompat,
                                 longRow ? reinterpret_cast<uint64_t *>(_dResume + offLong) : nullptr, _stream);
    if (he == hipSuccess)
      he = hipMemcpyAsync(_hResume + offStatus, _dResume + offStatus, m * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, _stream);
    if (he == hipSuccess) he = hipStreamSynchronize(_stream);
    if (he != hipSuccess) {
      (void)hipGetLastError();
      const Error he2 = HipErr(he, "ResumeQuiz");
      if (allOrNone) { chunk[0]->err = he2; return failAll(he2); }
      for (ResumeEntry *x : chunk) { drop(*x); x->err = he2; }
      continue;
    }
    const int64_t *status = reinterpret_cast<const int64_t *>(_hResume + offStatus);
    for (size_t k = 0; k < m; k++) {
      if (status[2 * k] == 0) continue;
      // reference PqaCore/CpuEngine.cpp:317-321
      const int64_t highBound = 1023 + 1023 - (int64_t)std::ceil(std::log2((double)_T)) - 2;
      const int64_t minAllowed = INT64_MIN + highBound + 1;
      chunk[k]->err = Error::MakeP(ErrCode::I64Underflow,
                                   "actual=" + std::to_string(status[2 * k + 1]) + ", minAllowed=" + std::to_string(minAllowed),
                                   "Max exponent over the priors is too low. Are all the targets in gaps?");
      if (allOrNone) return failAll(chunk[k]->err);
      drop(*chunk[k]);
    }
  }
  // ---- the ids, in entry order: what consecutive ResumeQuiz calls would assign
  const time_t now = time(nullptr);
  for (ResumeEntry &x : e) {
    if (x.quiz == nullptr) continue;
    x.quiz->answers.assign(x.pAQs, x.pAQs + x.nAnswered);
    x.quiz->lastUsage = now;
    x.id = AssignQuiz(x.quiz);
    x.quiz = nullptr;
  }
  return Error();
}

Error HipEngine::ResumeQuizBatch(int64_t n, const int64_t *pCounts, const AQ *pAQs, int64_t *pQuizzes) {
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "|nQuizzes| must be non-negative.");
  if (n > 0 && (!pCounts || !pQuizzes)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  int64_t total = 0;
  for (int64_t i = 0; i < n; i++) {
    if (pCounts[i] < 0)   // reference PqaCore/BaseEngine.cpp:388-392
      return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(pCounts[i]),
                          "Batch entry " + std::to_string(i) + ": |nAnswered| must be non-negative.");
    total += pCounts[i];
  }
  if (total > 0 && pAQs == nullptr) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of answered questions.");
  for (int64_t i = 0; i < n; i++) pQuizzes[i] = -1;
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  std::vector<ResumeEntry> e((size_t)n);
  for (int64_t i = 0, at = 0; i < n; at += pCounts[i], i++) { e[(size_t)i].nAnswered = pCounts[i]; e[(size_t)i].pAQs = pAQs + at; }
  const Error err = ResumeEntriesLocked(e, true);
  for (int64_t i = 0; i < n; i++)
    if (!e[(size_t)i].err.ok()) {
      Error r = e[(size_t)i].err;
      r.message = "Batch entry " + std::to_string(i) + ": " + r.message;
      return r;
    }
  if (!err.ok()) return err;
  for (int64_t i = 0; i < n; i++) pQuizzes[i] = e[(size_t)i].id;
  return Error();
}

// (hip_engine_shard.cpp: ResumeQuizRows, for a batch)
Error HipEngine::ResumeQuizBatchRows(int64_t n, const int64_t *pCounts, const AQ *pAQs, const void *const *rows, const int *rowDevices,
                                     const char *stageRow, int64_t *pQuizzes) {
  std::lock_guard<EngineMutex> lk(_mu);
  hipSetDevice(_device);
  int64_t total = 0;
  for (int64_t i = 0; i < n; i++) total += pCounts[i];
  std::vector<const void *> local(rows, rows + 2 * total);
  char *stage = nullptr;
  if (rowDevices != nullptr && stageRow != nullptr) {
    const size_t rowBytes = (size_t)_ldT * (size_t)_elem;
    size_t nStage = 0;
    for (int64_t i = 0; i < 2 * total; i++) nStage += stageRow[i] ? 1 : 0;
    if (nStage > 0) {
      hipError_t he = hipMalloc((void **)&stage, nStage * rowBytes);
      size_t at = 0;
      for (int64_t i = 0; he == hipSuccess && i < 2 * total; i++) {
        if (!stageRow[i]) continue;
        he = hipMemcpyPeerAsync(stage + at * rowBytes, _device, rows[i], rowDevices[i], rowBytes, _stream);
        local[(size_t)i] = stage + at * rowBytes;
        at++;
      }
      if (he != hipSuccess) { hipStreamSynchronize(_stream); hipFree(stage); return HipErr(he, "staging another device's rows for ResumeQuizBatch"); }
    }
  }
  const Error err = ResumeBatchEntriesLocked(n, pCounts, pAQs, local.data(), pQuizzes);
  if (stage) { hipStreamSynchronize(_stream); hipFree(stage); }
  return err;
}

// A batch whose row pointers are resolved (2 sum(pCounts) of them, in entry order): all or none, the error names its entry
Error HipEngine::ResumeBatchEntriesLocked(int64_t n, const int64_t *pCounts, const AQ *pAQs, const void *const *rows, int64_t *pQuizzes) {
  std::vector<ResumeEntry> e((size_t)n);
  for (int64_t i = 0, at = 0; i < n; at += pCounts[i], i++) {
    e[(size_t)i].nAnswered = pCounts[i];
    e[(size_t)i].pAQs = pAQs + at;
    e[(size_t)i].rows = rows + 2 * at;
  }
  Error err = ResumeEntriesLocked(e, true);
  for (int64_t i = 0; i < n; i++)
    if (!e[(size_t)i].err.ok()) {
      err = e[(size_t)i].err;
      err.message = "Batch entry " + std::to_string(i) + ": " + err.message;
      return err;
    }
  if (!err.ok()) return err;
  for (int64_t i = 0; i < n; i++) pQuizzes[i] = e[(size_t)i].id;
  return Error();
}

// ---- ResumeQuiz on a shard that is driven by a process of its own (probqa_amd/dist.py): the rows of answered questions other
// ranks hold arrive as a package -- slot i = the two rows of answered question i as they lie in the owner's cube -- that the
// owners fill with PackAnswerRows and the ranks exchange.  Resuming from it is the row-pointer path of the sharded engine
// (CreateQuiz / ResumeEntriesLocked with `rows`), its pointers aimed at the package's slots.

// One launch (kb_kernels.hip: pack_answer_rows_kernel) behind one copy of the pointer list; nothing here waits for the device,
// except that the pinned list is not rewritten while an earlier call's copy of it is still under way.
Error HipEngine::PackAnswerRows(int64_t n, const AQ *pAQs, void *pDst, void *pFlag, uint64_t flagValue) {
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "|nAnswered| must be non-negative.");
  if (n > 0 && (!pAQs || !pDst)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of answered questions or the package.");
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = CheckRegular("pack answer rows");
  if (!err.ok()) return err;
  for (int64_t i = 0; i < n; i++) {   // (everything is checked before anything is launched)
    const int64_t iq = pAQs[i].iQuestion, ia = pAQs[i].iAnswer;
    if (iq < 0 || iq >= _qTotal) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(iq, 0, _qTotal - 1), "Question index is not in KB range.");
    if (ia < 0 || ia >= _K) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(ia, 0, _K - 1), "Answer index is not in KB range.");
  }
  int64_t m = 0;
  for (int64_t i = 0; i < n; i++) m += OwnsQuestion(pAQs[i].iQuestion) ? 1 : 0;
  if (m == 0 && pFlag == nullptr) return Error();
  hipSetDevice(_device);
  if (_serverLaunched) StopServer();   // a launched kernel has no room beside the resident sweep and would wait for it to idle out
  // the list: {arrival counter, pad} and then a PackPair per row pair of this engine's questions
  static_assert(sizeof(PackPair) == 3 * sizeof(int64_t), "the pairs travel in the answered-question buffer");
  const int64_t words = 2 + 3 * m;
  err = EnsurePackList(words);
  if (!err.ok()) return err;
  PackPair *pairs = reinterpret_cast<PackPair *>(_hPack + 2);
  const size_t slotBytes = (size_t)AnswerRowSlotBytes();
  for (int64_t i = 0, at = 0; i < n; i++) {
    if (!OwnsQuestion(pAQs[i].iQuestion)) continue;
    pairs[at++] = PackPair{CubeAt(pAQs[i].iQuestion - _qFirst, pAQs[i].iAnswer), CubeAt(pAQs[i].iQuestion - _qFirst, _K),
                           static_cast<char *>(pDst) + (size_t)i * slotBytes};
  }
  MarkStreamBusy();
  err = SubmitPackList(words);
  if (!err.ok()) return err;
  HIP_TRY(LaunchPackAnswerRows(reinterpret_cast<const PackPair *>(_dAqs + 2), m, (int64_t)(slotBytes / 2), reinterpret_cast<unsigned *>(_dAqs),
                               static_cast<uint64_t *>(pFlag), flagValue, _stream));
  _packCalls++;
  _packBytes += (uint64_t)m * slotBytes;
  return Error();
}

// The pointer list of a pack call (PackAnswerRows, PackQuestionBlocks, the posterior packages' two calls): `words` 8-byte words fit the device buffer and its pinned
// source, the copy of the previous call's list has left the pinned one, and the header -- the arrival counter -- is zero.
Error HipEngine::EnsurePackList(int64_t words) {
  if (words > 2 * _aqCapacity) {
    hipFree(_dAqs);   // (waits for whatever still reads it)
    _dAqs = nullptr;
    _aqCapacity = 0;
    const int64_t cap = std::max<int64_t>((words + 1) / 2, 64);
    HIP_TRY(hipMalloc(&_dAqs, (size_t)cap * 2 * sizeof(int64_t)));
    _aqCapacity = cap;
  }
  if (_evPack == nullptr) HIP_TRY(hipEventCreateWithFlags(&_evPack, hipEventDisableTiming));
  else HIP_TRY(hipEventSynchronize(_evPack));
  if (words > _hPackWords) {
    hipHostFree(_hPack);
    _hPack = nullptr;
    _hPackWords = 0;
    const int64_t cap = std::max<int64_t>(words, 128);
    HIP_TRY(hipHostMalloc((void **)&_hPack, (size_t)cap * sizeof(int64_t), hipHostMallocDefault));
    _hPackWords = cap;
  }
  _hPack[0] = _hPack[1] = 0;
  return Error();
}

Error HipEngine::SubmitPackList(int64_t words) {
  HIP_TRY(hipMemcpyAsync(_dAqs, _hPack, (size_t)words * sizeof(int64_t), hipMemcpyHostToDevice, _stream));
  HIP_TRY(hipEventRecord(_evPack, _stream));
  return Error();
}

Error HipEngine::SubmitSources(int64_t n, const int64_t *pSources) {
  const int64_t words = 2 + n;   // {arrival counter, pad}, then the sources
  Error err = EnsurePackList(words);
  if (!err.ok()) return err;
  for (int64_t i = 0; i < n; i++) _hPack[2 + i] = pSources[i];
  MarkStreamBusy();
  return SubmitPackList(words);
}

bool HipEngine::IsStagedHostMemory(const void *p) const {
  if (!_opt.rowsStage) return false;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeHost;
}

const void *HipEngine::StageHostPackage(const void *p, size_t bytes, void **buf, size_t &have, Error &err) {
  if (!IsStagedHostMemory(p)) return p;
  hipError_t e = GrowDeviceBytes(buf, have, bytes);
  if (e == hipSuccess) e = hipMemcpyAsync(*buf, p, bytes, hipMemcpyDefault, _stream);
  if (e != hipSuccess) { err = HipErr(e, "StageHostPackage"); return nullptr; }
  _rowsStaged++;
  return *buf;
}

// The 2 `total` row pointers of a package's slots; a package in host memory is first copied into the engine's own device scratch when
// option "rows_stage" says so (IsStagedHostMemory): `base` then points there.
Error HipEngine::PackageRowsLocked(int64_t total, const AQ *pAQs, const void *pRows, std::vector<const void *> &rows) {
  rows.assign(2 * (size_t)total, nullptr);
  bool anyForeign = false;
  for (int64_t i = 0; i < total; i++) anyForeign = anyForeign || !OwnsQuestion(pAQs[i].iQuestion);
  if (anyForeign && pRows == nullptr) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the row package.");
  const size_t slotBytes = (size_t)AnswerRowSlotBytes();
  const char *base = static_cast<const char *>(pRows);
  if (anyForeign && _opt.rowsStage) {
    hipSetDevice(_device);
    if (IsStagedHostMemory(pRows)) {
      HIP_TRY(GrowDeviceBytes(&_dRowStage, _rowStageBytes, (size_t)total * slotBytes));
      char *stage = static_cast<char *>(_dRowStage);
      // one copy per run of slots of other engines' questions: this engine's own slots may be unfilled and are not read
      for (int64_t i = 0; i < total;) {
        if (OwnsQuestion(pAQs[i].iQuestion)) { i++; continue; }
        int64_t j = i + 1;
        while (j < total && !OwnsQuestion(pAQs[j].iQuestion)) j++;
        HIP_TRY(hipMemcpyAsync(stage + (size_t)i * slotBytes, base + (size_t)i * slotBytes, (size_t)(j - i) * slotBytes, hipMemcpyDefault, _stream));
        i = j;
      }
      base = stage;
      _rowsStaged++;
    }
  }
  for (int64_t i = 0; i < total; i++) {
    if (OwnsQuestion(pAQs[i].iQuestion)) {
      const bool valid = pAQs[i].iAnswer >= 0 && pAQs[i].iAnswer < _K;   // (an answer out of range is refused further down, before any row is read)
      rows[2 * (size_t)i] = CubeAt(pAQs[i].iQuestion - _qFirst, valid ? pAQs[i].iAnswer : 0);
      rows[2 * (size_t)i + 1] = CubeAt(pAQs[i].iQuestion - _qFirst, _K);
    } else {
      rows[2 * (size_t)i] = base + (size_t)i * slotBytes;
      rows[2 * (size_t)i + 1] = base + (size_t)i * slotBytes + slotBytes / 2;
    }
  }
  return Error();
}

int64_t HipEngine::ResumeQuizFromRows(Error &err, int64_t nAnswered, const AQ *pAQs, const void *pRows) {
  if (nAnswered < 0) {  // reference PqaCore/BaseEngine.cpp:388-392
    err = Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nAnswered), "|nAnswered| must be non-negative.");
    return -1;
  }
  if (nAnswered > 0 && pAQs == nullptr) {
    err = Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of answered questions.");
    return -1;
  }
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);   // (not a posted operation: concurrent calls take the engine one after the other)
  std::vector<const void *> rows;
  err = PackageRowsLocked(nAnswered, pAQs, pRows, rows);
  if (!err.ok()) return -1;
  if (nAnswered > 0 && ResumeTakesLongRow(View())) {   // long rows: the multi-workgroup form, as a batch of one
    std::vector<ResumeEntry> e(1);
    e[0].nAnswered = nAnswered;
    e[0].pAQs = pAQs;
    e[0].rows = rows.data();
    err = ResumeEntriesLocked(e, true);
    if (!e[0].err.ok()) err = e[0].err;
    return SpeculateFor(err.ok() ? e[0].id : -1);
  }
  return SpeculateFor(CreateQuiz(err, nAnswered, pAQs, nAnswered > 0 ? rows.data() : nullptr, nullptr, 0, nullptr));
}

Error HipEngine::ResumeQuizBatchFromRows(int64_t n, const int64_t *pCounts, const AQ *pAQs, const void *pRows, int64_t *pQuizzes) {
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "|nQuizzes| must be non-negative.");
  if (n > 0 && (!pCounts || !pQuizzes)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  int64_t total = 0;
  for (int64_t i = 0; i < n; i++) {
    if (pCounts[i] < 0)   // reference PqaCore/BaseEngine.cpp:388-392
      return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(pCounts[i]),
                          "Batch entry " + std::to_string(i) + ": |nAnswered| must be non-negative.");
    total += pCounts[i];
  }
  if (total > 0 && pAQs == nullptr) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of answered questions.");
  for (int64_t i = 0; i < n; i++) pQuizzes[i] = -1;
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  std::vector<const void *> rows;
  const Error err = PackageRowsLocked(total, pAQs, pRows, rows);
  if (!err.ok()) return err;
  if (total == 0) rows.assign(1, nullptr);   // (a batch of StartQuiz entries: the pointer list is never read)
  return ResumeBatchEntriesLocked(n, pCounts, pAQs, rows.data(), pQuizzes);
}

}  // namespace pqa
