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
      he = LaunchStartQuizBatch(kb, *starts, _optWorkers, _stream);
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
  const int64_t stride = ResumeLongStride(_optWorkers);
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
      he = LaunchResumeQuizBatch(kb, reinterpret_cast<const ResumeSlot *>(_dResume), (int64_t)m, (int64_t)askedWords, _optWorkers, (int)_optBugCompat,
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
  std::vector<ResumeEntry> e((size_t)n);
  for (int64_t i = 0, at = 0; i < n; at += pCounts[i], i++) {
    e[(size_t)i].nAnswered = pCounts[i];
    e[(size_t)i].pAQs = pAQs + at;
    e[(size_t)i].rows = local.data() + 2 * at;
  }
  Error err = ResumeEntriesLocked(e, true);
  if (stage) { hipStreamSynchronize(_stream); hipFree(stage); }
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

}  // namespace pqa
