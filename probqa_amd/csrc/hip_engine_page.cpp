// hip_engine_page.cpp -- HipEngine::EvalConditionalGainsBatch and HipEngine::ListQuestionPageBatch (hip_engine.h, include/PqaHipExt.h):
// what every question would tell a quiz once the answers to a given set of questions are known, and a page of questions filled greedily
// by that number (page_kernels.hip has the definition).
//   * validation: everything a call can be refused for, in the header's order, before anything is launched or written;
//   * a call runs in chunks of whole quizzes (page_plan.h) whose branch rows at their largest step stay within one chunk of the gain
//     sweep and within the scratch limit.  The rows live in two halves of one scratch area: an expansion reads a quiz's rows in one
//     half and writes their children into the other, so each quiz changes sides when IT is expanded;
//   * per chunk one list of PageQuiz records, a run per launch, travels in the pack list; then the launches back to back: the roots,
//     one expansion per level of the given sets, and per step the gain sweep over every branch row of the chunk (LaunchQuestionGains,
//     unchanged), the combine, and for a page the listing of ONE record (LaunchTopQuestions over slots that carry the quiz's exclusion
//     bitmap) followed by the expansion that reads that record on the device.  Every grid size is known ahead, so the host waits once
//     per chunk.
// Nothing of a quiz changes: the posteriors and asked bits are only read.
#include "hip_engine_internal.h"
#include "page_plan.h"

namespace pqa {

static_assert(sizeof(PageQuiz) == 8 * sizeof(int64_t), "the records travel in the pack list");
static_assert(kPageMaxBranches == kTopBatchQuizzes, "a step's rows are one chunk of the gain sweep");

namespace {
constexpr int64_t kPageSetCap = 16;   // a set is at most 8 questions deep at 2 answers (2^8 rows), and a page's last pick is noted too
constexpr int64_t kPageMaxSteps = 9;
}  // namespace

// Everything both calls can be refused for under the lock, in the header's order from the row length on.  Fills st.given (LOCAL ids,
// one set after another), st.givenFirst (nQuizzes + 1) and st.largest (the quizzes' branch rows at their largest step).
// pkg (the FromBlocks forms): a given question another engine holds gets given -1 and givenSlot its slot of the package; the package's
// own refusals come last.
Error HipEngine::AdmitPageLocked(const char *call, int64_t rowLength, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven,
                                 int64_t pageSize, bool page, const PageBlocks *pkg) {
  if (!pkg && IsShard()) return NoPages(call);
  Error err = AdmitGainsLocked(rowLength, nQuizzes, pQuizzes);
  if (!err.ok()) return err;
  PageStage &st = _page;
  st.given.clear();
  st.givenSlot.clear();
  st.givenFirst.assign(1, 0);
  st.largest.clear();
  st.blocks = nullptr;
  for (int64_t i = 0, at = 0; i < nQuizzes; i++) {
    const int64_t c = pGivenCounts ? pGivenCounts[i] : 0;
    for (int64_t j = 0; j < c; j++) {
      const int64_t id = pGiven[at + j];
      const std::string where = "entry=" + std::to_string(i) + " questionId=" + std::to_string(id);
      if (id < 0 || id >= _qTotal) return Error::MakeP(ErrCode::IndexOutOfRange, where + " " + RangeParams(id, 0, _qTotal - 1), "A given question is out of range.");
      const bool own = OwnsQuestion(id);   // (a shard knows the whole axis' gaps)
      if (own ? BitTest(_hQGap, id - _qFirst) : std::find(_globalQuestionGaps.begin(), _globalQuestionGaps.end(), id) != _globalQuestionGaps.end())
        return Error::MakeP(ErrCode::IndexOutOfRange, where, "A given question is a gap.");
      st.given.push_back(own ? (int32_t)(id - _qFirst) : -1);
      st.givenSlot.push_back(-1);
    }
    at += c;
    st.givenFirst.push_back(at);
  }
  for (int64_t i = 0; i < nQuizzes; i++) {
    const int64_t branches = PageLargestBranches(_K, st.givenFirst[(size_t)i + 1] - st.givenFirst[(size_t)i], pageSize, page);
    if (!PageFits(branches, _ldT))
      return Error::MakeP(ErrCode::IndexOutOfRange,
                          "entry=" + std::to_string(i) + " branches=" + (branches > kPageMaxBranches ? ">" + std::to_string(kPageMaxBranches) : std::to_string(branches)),
                          "A quiz's answer combinations must be at most 256 and their rows fit 64 MiB of scratch.");
    st.largest.push_back(branches);
  }
  if (!pkg) return Error();
  // ---- the package: its slot size, a slot for every given question this engine does not hold, and the package itself
  if ((pkg->n > 0 || pkg->blocks) && pkg->slotBytes != QuestionBlockSlotBytes())
    return Error::MakeP(ErrCode::IndexOutOfRange, "[slotBytes=" + std::to_string(pkg->slotBytes) + " of " + std::to_string(QuestionBlockSlotBytes()) + "]",
                        "The block package's slot size is not this engine's (PqaHip_QuestionBlockSlotBytes).");
  std::unordered_map<int64_t, int64_t> slotOf;
  for (int64_t s = 0; s < pkg->n; s++) slotOf.emplace(pkg->questions[s], s);
  bool foreign = false;
  for (int64_t i = 0; i < nQuizzes; i++)
    for (int64_t g = st.givenFirst[(size_t)i]; g < st.givenFirst[(size_t)i + 1]; g++) {
      if (st.given[(size_t)g] >= 0) continue;
      const auto it = slotOf.find(pGiven[g]);
      if (it == slotOf.end())
        return Error::MakeP(ErrCode::IndexOutOfRange, "entry=" + std::to_string(i) + " questionId=" + std::to_string(pGiven[g]),
                            "A given question that this engine does not hold is not in the block package.");
      st.givenSlot[(size_t)g] = it->second;
      foreign = true;
    }
  if (foreign && !pkg->blocks) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the block package.");
  if (foreign && (reinterpret_cast<uintptr_t>(pkg->blocks) & 15) != 0)
    return Error::MakeP(ErrCode::IndexOutOfRange, "address mod 16=" + std::to_string(reinterpret_cast<uintptr_t>(pkg->blocks) & 15), "The package must be 16-byte aligned.");
  return Error();
}

// The slots the call reads, where the kernels read them: a package in registered host memory is copied to the device first under option
// "rows_stage" -- one copy per run of needed slots; this engine's own questions' slots may be unfilled and are not read.
Error HipEngine::StagePageBlocksLocked(const PageBlocks &pkg) {
  PageStage &st = _page;
  st.blocks = static_cast<const char *>(pkg.blocks);
  std::vector<char> needed((size_t)pkg.n, 0);
  bool any = false;
  for (int64_t s : st.givenSlot)
    if (s >= 0) needed[(size_t)s] = 1, any = true;
  if (!any || !IsStagedHostMemory(pkg.blocks)) return Error();
  const size_t slotBytes = (size_t)pkg.slotBytes;
  HIP_TRY(GrowDeviceBytes(&_dRowStage, _rowStageBytes, (size_t)pkg.n * slotBytes));
  char *stage = static_cast<char *>(_dRowStage);
  for (int64_t i = 0; i < pkg.n;) {
    if (!needed[(size_t)i]) { i++; continue; }
    int64_t j = i + 1;
    while (j < pkg.n && needed[(size_t)j]) j++;
    HIP_TRY(hipMemcpyAsync(stage + (size_t)i * slotBytes, st.blocks + (size_t)i * slotBytes, (size_t)(j - i) * slotBytes, hipMemcpyDefault, _stream));
    i = j;
  }
  st.blocks = stage;
  _rowsStaged++;
  return Error();
}

// One chunk, quizzes [first, first + m) of the call: everything enqueued, the stream not yet waited for.  steps == 0: Eval -- the
// combined rows of the given sets stay in st.dCombined; otherwise step s's record of quiz j arrives at st.lines record s * 256 + j.
Error HipEngine::PageChunkLocked(int64_t first, int64_t m, const int64_t *pQuizzes, int64_t steps) {
  PageStage &st = _page;
  if (steps > kPageMaxSteps) return Error::Make(ErrCode::Internal, "Internal error at hip_engine_page.cpp: a page outgrew its result lines.");   // (2^8 rows: 9 steps)
  const KbView kb = View();
  const int64_t pitch = _ldT, gainPitch = RedRowPitch(), exclWords = (_Q + 31) / 32;
  const int64_t slotBytes = QuestionBlockSlotBytes(), blockLdT = st.blocks ? slotBytes / (_K + 1) / _elem : 0;   // (a slot's pitch: RoundLdT(T), not the allocation's)
  Error err;
  // ---- where the quizzes' rows lie: quiz j's at off[j] of either half of R rows
  std::vector<int64_t> off((size_t)m), branches((size_t)m, 1), side((size_t)m, 0), nGiven((size_t)m);
  std::vector<const Quiz *> quiz((size_t)m);
  int64_t R = 0, deepest = 0;
  for (int64_t j = 0; j < m; j++) {
    quiz[(size_t)j] = UseQuiz(err, pQuizzes[first + j]);
    if (!quiz[(size_t)j]) return err;
    off[(size_t)j] = R;
    R += st.largest[(size_t)(first + j)];
    nGiven[(size_t)j] = st.givenFirst[(size_t)(first + j) + 1] - st.givenFirst[(size_t)(first + j)];
    deepest = std::max(deepest, nGiven[(size_t)j]);
  }
  HIP_TRY(GrowDevice(&st.dRows, st.rowsBytes, (size_t)(2 * R * pitch) * sizeof(double)));
  HIP_TRY(GrowDevice(&st.dMasses, st.massesBytes, (size_t)(2 * kPageMaxBranches) * sizeof(double)));
  HIP_TRY(GrowDevice(&st.dGains, st.gainsBytes, (size_t)(kPageMaxBranches * gainPitch) * sizeof(double)));
  HIP_TRY(GrowDevice(&st.dCombined, st.combinedBytes, (size_t)(kTopBatchQuizzes * gainPitch) * sizeof(double)));
  HIP_TRY(GrowDevice(&st.dExcl, st.exclBytes, (size_t)(kTopBatchQuizzes * exclWords) * sizeof(uint32_t)));
  if (!st.dSet) HIP_TRY(hipMalloc((void **)&st.dSet, (size_t)(kTopBatchQuizzes * kPageSetCap) * sizeof(int32_t)));
  if (!st.dSlots) HIP_TRY(hipMalloc((void **)&st.dSlots, (size_t)kTopBatchQuizzes * sizeof(QuizSlot)));
  HIP_TRY(st.lines.Ensure(_stream, kPageMaxSteps * kTopBatchQuizzes, 0, kPageMaxSteps * kTopBatchQuizzes, hipHostMallocDefault));
  if (steps > 0) {
    err = EnsureTopScratchRecords(m * TopQuestionsScratchRecords(_Q, 1));
    if (!err.ok()) return err;
  }
  // ---- the launches and their records
  enum Kind { kRoot, kExpand, kSweep };
  struct Launch { Kind kind; int64_t at, maxParents, step; std::vector<int32_t> rows; };
  std::vector<Launch> launches;
  const int64_t nLaunches = 1 + deepest + (steps > 0 ? 2 * steps - 1 : 1), words = 2 + 8 * m * nLaunches;
  err = EnsurePackList(words);
  if (!err.ok()) return err;
  PageQuiz *const hList = reinterpret_cast<PageQuiz *>(_hPack + 2);
  const PageQuiz *const dList = reinterpret_cast<const PageQuiz *>(_dAqs + 2);
  int64_t at = 0;
  TopBatchPriors priors;
  GainAsked excl;
  const auto rowOf = [&](int64_t j) { return (int32_t)(side[(size_t)j] * R + off[(size_t)j]); };
  const auto base = [&](int64_t j) {
    PageQuiz z{};
    z.asked = quiz[(size_t)j]->dAsked;
    z.set = st.dSet + j * kPageSetCap;
    return z;
  };
  const auto expand = [&](int64_t level, int64_t step) {   // level >= 0: of the given sets; otherwise the pick of `step`
    Launch l{kExpand, at, 0, step, {}};
    for (int64_t j = 0; j < m; j++) {
      PageQuiz z = base(j);
      const bool takes = level < 0 || level < nGiven[(size_t)j];
      if (takes) {
        z.parent0 = rowOf(j);
        z.nParents = (int32_t)branches[(size_t)j];
        side[(size_t)j] ^= 1;
        branches[(size_t)j] *= _K;
        z.row0 = rowOf(j);
        z.nRows = (int32_t)branches[(size_t)j];
        if (level >= 0) {
          const size_t g = (size_t)(st.givenFirst[(size_t)(first + j)] + level);
          z.question = st.given[g];
          if (st.givenSlot[g] >= 0) {   // another engine's question: its block in the package
            z.question = kPageBlockGiven;
            z.block = st.blocks + (size_t)st.givenSlot[g] * (size_t)slotBytes;
          }
          z.nSet = (int32_t)level;
        } else {
          z.question = kPagePickListed;
          z.pick = st.lines.records + step * kTopBatchQuizzes + j;
          z.nPick = st.lines.Counts() + step * kTopBatchQuizzes + j;
          z.nSet = (int32_t)(nGiven[(size_t)j] + step);
        }
        l.maxParents = std::max<int64_t>(l.maxParents, z.nParents);
      }
      hList[at++] = z;
    }
    launches.push_back(std::move(l));
  };
  const auto sweep = [&](int64_t step) {
    Launch l{kSweep, at, 0, step, {}};
    for (int64_t j = 0; j < m; j++) {
      PageQuiz z = base(j);
      z.row0 = rowOf(j);
      z.nRows = (int32_t)branches[(size_t)j];
      z.gain0 = (int32_t)l.rows.size();
      z.nSet = (int32_t)(nGiven[(size_t)j] + step);
      for (int64_t b = 0; b < branches[(size_t)j]; b++) l.rows.push_back(z.row0 + (int32_t)b);
      hList[at++] = z;
    }
    launches.push_back(std::move(l));
  };
  {
    Launch l{kRoot, at, 0, 0, {}};
    for (int64_t j = 0; j < m; j++) {
      priors.prior[j] = quiz[(size_t)j]->dPrior;
      excl.asked[j] = st.dExcl + j * exclWords;
      PageQuiz z = base(j);
      z.row0 = rowOf(j);
      z.nRows = 1;
      hList[at++] = z;
    }
    launches.push_back(std::move(l));
  }
  for (int64_t level = 0; level < deepest; level++) expand(level, 0);
  sweep(0);
  for (int64_t s = 1; s < steps; s++) {
    expand(-1, s - 1);
    sweep(s);
  }
  if (at * 8 + 2 > words) return Error::Make(ErrCode::Internal, "Internal error at hip_engine_page.cpp: the launch list outgrew its room.");
  MarkStreamBusy();
  err = SubmitPackList(2 + 8 * at);
  if (!err.ok()) return err;
  TimerStart(st.ev);
  if (steps > 0) HIP_TRY(LaunchGainSlots(st.dSlots, st.dCombined, gainPitch, excl, m, _stream));
  bool headTimed = false;
  for (const Launch &l : launches) {
    if (l.kind == kSweep && !headTimed && _opt.timeSweeps) {   // what came before the first sweep: the roots and the given sets' expansions
      headTimed = true;
      if (!st.evHead && hipEventCreate(&st.evHead) != hipSuccess) { (void)hipGetLastError(); st.evHead = nullptr; }
      if (st.evHead && hipEventRecord(st.evHead, _stream) != hipSuccess) (void)hipGetLastError();
    }
    switch (l.kind) {
      case kRoot:
        HIP_TRY(LaunchPageRoots(kb, priors, dList + l.at, m, st.dRows, pitch, st.dMasses, _stream));
        break;
      case kExpand:
        if (l.maxParents > 0) HIP_TRY(LaunchPageExpand(kb, dList + l.at, m, l.maxParents, st.dRows, pitch, st.dMasses, blockLdT, _stream));
        break;
      case kSweep: {
        TopBatchPriors rows;
        const int64_t n = (int64_t)l.rows.size();
        if (n > kTopBatchQuizzes) return Error::Make(ErrCode::Internal, "Internal error at hip_engine_page.cpp: a step's rows outgrew a sweep.");
        for (int64_t r = 0; r < n; r++) rows.prior[r] = st.dRows + (int64_t)l.rows[(size_t)r] * pitch;
        HIP_TRY(LaunchQuestionGains(kb, rows, n, st.dGains, gainPitch, _stream));
        HIP_TRY(LaunchPageCombine(kb, dList + l.at, m, st.dGains, gainPitch, st.dMasses, st.dCombined, gainPitch, steps > 0 ? st.dExcl : nullptr, exclWords, _stream));
        if (steps > 0) {
          TopQuestions a{};
          a.slots = st.dSlots; a.qgap = _dQGap; a.nQuizzes = (int)m; a.Q = _Q;
          HIP_TRY(LaunchTopQuestions(a, 1, _dTopScratch[0], _dTopScratch[1], st.lines.records + l.step * kTopBatchQuizzes, st.lines.Counts() + l.step * kTopBatchQuizzes,
                                     nullptr, 0, _stream));
        }
        break;
      }
    }
  }
  TimerStop(st.ev, _pageDeviceNs);   // (waits for its event, which lies behind evHead)
  float headMs = 0;
  if (headTimed && st.evHead && st.ev[0]) {
    if (hipEventElapsedTime(&headMs, st.ev[0], st.evHead) == hipSuccess) _pageHeadNs += (uint64_t)(headMs * 1e6);
    else (void)hipGetLastError();
  }
  return Error();
}

namespace {
Error PageArguments(int64_t nQuizzes, int64_t pageSize, const int64_t *pGivenCounts, const int64_t *pGiven, bool buffersThere) {
  if (nQuizzes < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nQuizzes), "|nQuizzes| must be non-negative.");
  if (pageSize < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(pageSize), "|pageSize| must be non-negative.");
  bool any = false;
  for (int64_t i = 0; pGivenCounts && i < nQuizzes; i++) {
    if (pGivenCounts[i] < 0)
      return Error::MakeP(ErrCode::NegativeCount, "entry=" + std::to_string(i) + " count=" + std::to_string(pGivenCounts[i]), "A given set's length must be non-negative.");
    any = any || pGivenCounts[i] > 0;
  }
  if (nQuizzes > 0 && (!buffersThere || (any && !pGiven))) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of a batch buffer.");
  return Error();
}
// ... and of the FromBlocks forms, behind the plain call's own
Error BlockArguments(int64_t nQuizzes, int64_t nBlocks, const int64_t *pBlockQuestions) {
  if (nBlocks < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nBlocks), "|nBlocks| must be non-negative.");
  if (nQuizzes > 0 && nBlocks > 0 && !pBlockQuestions) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the package's questions.");
  return Error();
}
}  // namespace

Error HipEngine::EvalConditionalGainsBatch(int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven, double *pOut, int64_t n) {
  return EvalPageRows("EvalConditionalGainsBatch", nQuizzes, pQuizzes, pGivenCounts, pGiven, nullptr, pOut, n);
}

Error HipEngine::EvalConditionalGainsBatchFromBlocks(int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven, int64_t nBlocks,
                                                     const int64_t *pBlockQuestions, const void *pBlocks, int64_t slotBytes, double *pOut, int64_t n) {
  const PageBlocks pkg{nBlocks, pBlockQuestions, pBlocks, slotBytes};
  return EvalPageRows("EvalConditionalGainsBatchFromBlocks", nQuizzes, pQuizzes, pGivenCounts, pGiven, &pkg, pOut, n);
}

Error HipEngine::EvalPageRows(const char *call, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven, const PageBlocks *pkg,
                              double *pOut, int64_t n) {
  Error err = PageArguments(nQuizzes, 0, pGivenCounts, pGiven, pQuizzes && pOut);
  if (err.ok() && pkg) err = BlockArguments(nQuizzes, pkg->n, pkg->questions);
  if (!err.ok()) return err;
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  err = AdmitPageLocked(call, n, nQuizzes, pQuizzes, pGivenCounts, pGiven, 0, false, pkg);
  if (!err.ok() || nQuizzes == 0) return err;
  _pageCalls++;
  _pageQuizzes += (uint64_t)nQuizzes;
  hipSetDevice(_device);
  err = FlushUpdates();   // (the quizzes' deferred answers: their posteriors are read below)
  if (!err.ok()) return err;
  if (_serverLaunched) StopServer();   // a launched kernel has no room beside the resident sweep and would wait for it to idle out
  if (pkg) {
    err = StagePageBlocksLocked(*pkg);
    if (!err.ok()) return err;
  }
  const PageChunks plan = PlanPageChunks(nQuizzes, _page.largest.data(), _ldT);
  for (int64_t c = 0; c < plan.Chunks(); c++) {
    const int64_t first = plan.start[(size_t)c], m = plan.start[(size_t)c + 1] - first;
    err = PageChunkLocked(first, m, pQuizzes, 0);
    if (!err.ok()) return err;
    HIP_TRY(hipMemcpy2DAsync(pOut + first * n, (size_t)n * sizeof(double), _page.dCombined, (size_t)RedRowPitch() * sizeof(double), (size_t)n * sizeof(double), (size_t)m,
                             hipMemcpyDeviceToHost, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  _pendingRecordOp = 0;
  return Error();
}

Error HipEngine::ListQuestionPageBatch(int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven, int64_t pageSize,
                                       CiRatedQuestion *pDest, int64_t *pCounts) {
  Error err = PageArguments(nQuizzes, pageSize, pGivenCounts, pGiven, pQuizzes && pCounts && (pageSize == 0 || pDest));
  if (!err.ok()) return err;
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  err = AdmitPageLocked("ListQuestionPageBatch", -1, nQuizzes, pQuizzes, pGivenCounts, pGiven, pageSize, true);
  if (!err.ok() || nQuizzes == 0) return err;
  _pageCalls++;
  _pageQuizzes += (uint64_t)nQuizzes;
  for (int64_t i = 0; i < nQuizzes; i++) pCounts[i] = 0;
  if (pageSize == 0) return Error();
  hipSetDevice(_device);
  err = FlushUpdates();
  if (!err.ok()) return err;
  if (_serverLaunched) StopServer();
  const PageChunks plan = PlanPageChunks(nQuizzes, _page.largest.data(), _ldT);
  for (int64_t c = 0; c < plan.Chunks(); c++) {
    const int64_t first = plan.start[(size_t)c], m = plan.start[(size_t)c + 1] - first;
    err = PageChunkLocked(first, m, pQuizzes, pageSize);
    if (!err.ok()) return err;
    HIP_TRY(hipStreamSynchronize(_stream));
    for (int64_t j = 0; j < m; j++) {
      CiRatedQuestion *dest = pDest + (first + j) * pageSize;
      int64_t taken = 0;
      for (int64_t s = 0; s < pageSize; s++) {   // (a step without a pick ends the page: the later steps found zero rows)
        const RatedTargetDev &rec = _page.lines.records[s * kTopBatchQuizzes + j];
        if (_page.lines.Counts()[s * kTopBatchQuizzes + j] <= 0 || rec.iTarget < 0) break;
        dest[taken]._iQuestion = _qFirst + rec.iTarget;
        dest[taken]._priority = rec.prob;
        taken++;
      }
      pCounts[first + j] = taken;
    }
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  _pendingRecordOp = 0;
  return Error();
}

// One step of a page for this engine's questions: PageChunkLocked with one step, the record of quiz j at st.lines record j.
Error HipEngine::SelectPageStepFromBlocks(int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts, const int64_t *pGiven, int64_t nBlocks,
                                          const int64_t *pBlockQuestions, const void *pBlocks, int64_t slotBytes, CiHipSelection *pOut) {
  Error err = PageArguments(nQuizzes, 1, pGivenCounts, pGiven, pQuizzes && pOut);
  if (err.ok()) err = BlockArguments(nQuizzes, nBlocks, pBlockQuestions);
  if (!err.ok()) return err;
  const PageBlocks pkg{nBlocks, pBlockQuestions, pBlocks, slotBytes};
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  err = AdmitPageLocked("SelectPageStepFromBlocks", -1, nQuizzes, pQuizzes, pGivenCounts, pGiven, 1, true, &pkg);
  if (!err.ok() || nQuizzes == 0) return err;
  _pageCalls++;
  _pageQuizzes += (uint64_t)nQuizzes;
  hipSetDevice(_device);
  err = FlushUpdates();
  if (!err.ok()) return err;
  if (_serverLaunched) StopServer();
  err = StagePageBlocksLocked(pkg);
  if (!err.ok()) return err;
  const PageChunks plan = PlanPageChunks(nQuizzes, _page.largest.data(), _ldT);
  for (int64_t c = 0; c < plan.Chunks(); c++) {
    const int64_t first = plan.start[(size_t)c], m = plan.start[(size_t)c + 1] - first;
    err = PageChunkLocked(first, m, pQuizzes, 1);
    if (!err.ok()) return err;
    HIP_TRY(hipStreamSynchronize(_stream));
    for (int64_t j = 0; j < m; j++) {
      const RatedTargetDev &rec = _page.lines.records[j];
      const bool picked = _page.lines.Counts()[j] > 0 && rec.iTarget >= 0;
      pOut[first + j]._priority = picked ? rec.prob : 0.0;
      pOut[first + j]._iQuestion = picked ? _qFirst + rec.iTarget : -1;
    }
  }
  _mu.busy = false;   // (the stream has just been synchronised)
  _pendingRecordOp = 0;
  return Error();
}

// PackQuestionBlocks in regular mode, for the given questions of the FromBlocks forms: the same launch, the same slots; a gap is refused.
Error HipEngine::PackGivenBlocks(int64_t n, const int64_t *pQuestions, void *pDst, void *pFlag, uint64_t flagValue) {
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "The number of question blocks must be non-negative.");
  if (n > 0 && (!pQuestions || !pDst)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the questions or the package.");
  CallScope scope(_activeCallers);
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = CheckRegular("pack given blocks");
  if (!err.ok()) return err;
  int64_t m = 0;
  for (int64_t i = 0; i < n; i++) {   // (everything is checked before anything is launched)
    const int64_t id = pQuestions[i];
    if (id < 0 || id >= _qTotal)
      return Error::MakeP(ErrCode::IndexOutOfRange, "questionId=" + std::to_string(id) + " " + RangeParams(id, 0, _qTotal - 1), "Question index is not in KB range.");
    const bool own = OwnsQuestion(id);
    if (own ? BitTest(_hQGap, id - _qFirst) : std::find(_globalQuestionGaps.begin(), _globalQuestionGaps.end(), id) != _globalQuestionGaps.end())
      return Error::MakeP(ErrCode::IndexOutOfRange, "questionId=" + std::to_string(id), "A given question is a gap.");
    m += own ? 1 : 0;
  }
  if (m == 0 && pFlag == nullptr) return Error();
  hipSetDevice(_device);
  err = FlushUpdates();   // (the stream's order: nothing of a cube changes, but the deferred launches keep their place)
  if (!err.ok()) return err;
  if (_serverLaunched) StopServer();
  const int64_t words = 2 + 2 * m;   // {arrival counter, pad}, then a BlockCopy per block of this engine's
  err = EnsurePackList(words);
  if (!err.ok()) return err;
  BlockCopy *blocks = reinterpret_cast<BlockCopy *>(_hPack + 2);
  const size_t slotBytes = (size_t)QuestionBlockSlotBytes();
  for (int64_t i = 0, at = 0; i < n; i++)
    if (OwnsQuestion(pQuestions[i])) blocks[at++] = BlockCopy{CubeAt(pQuestions[i] - _qFirst), static_cast<char *>(pDst) + (size_t)i * slotBytes};
  MarkStreamBusy();
  err = SubmitPackList(words);
  if (!err.ok()) return err;
  HIP_TRY(LaunchCopyQuestionBlocks(reinterpret_cast<const BlockCopy *>(_dAqs + 2), m, _K + 1, _T * _elem / 4, _ldT * _elem, (int64_t)slotBytes / (_K + 1), true,
                                   reinterpret_cast<unsigned *>(_dAqs), static_cast<uint64_t *>(pFlag), flagValue, _stream));
  _packCalls++;
  _packBytes += (uint64_t)m * slotBytes;
  return Error();
}

}  // namespace pqa
