// hip_engine_combine.cpp -- HipEngine under concurrent callers: operations posted to the holder of the engine lock, and the
// flat combining of concurrent NextQuestion calls into one sweep (hip_engine.h: Combine).
#include "hip_engine_internal.h"

namespace pqa {
// ------------------------------------------------------------------------------------------------------------------
// concurrent NextQuestion calls (see SelRequest in hip_engine.h)
// ------------------------------------------------------------------------------------------------------------------
// How many CPUs the process may keep busy: a container's CPU quota (cgroup v2 cpu.max / v1 cfs quota) or else the affinity mask.
// The GPU boxes of this project allow a container 16 of the host's 256 hardware threads: waiting policies that spin are right for
// up to that many client threads and wrong beyond (measured: 64 spinning clients 40 k questions/s against 54 k sleeping).
int HipEngine::AllowedCpus() {
  static const int n = [] {
    int cpus = (int)std::thread::hardware_concurrency();
    if (cpus <= 0) cpus = 1;
    if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char quota[32] = {0};
      long long period = 0;
      if (std::fscanf(f, "%31s %lld", quota, &period) == 2 && period > 0 && quota[0] != 'm') {
        const long long q = std::atoll(quota);
        if (q > 0) cpus = std::min<int>(cpus, (int)std::max<long long>(1, q / period));
      }
      std::fclose(f);
    } else if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
      long long q = -1, period = 100000;
      if (std::fscanf(g, "%lld", &q) != 1) q = -1;
      std::fclose(g);
      if (FILE *h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (std::fscanf(h, "%lld", &period) != 1) period = 100000; std::fclose(h); }
      if (q > 0 && period > 0) cpus = std::min<int>(cpus, (int)std::max<long long>(1, q / period));
    }
    return cpus;
  }();
  return n;
}

// Everything posted so far, in the order it was posted.  The order of the stages is the contract: the RecordAnswers first go where
// RecordAnswer puts them (the list of deferred updates) and ReleaseQuiz runs as it comes; then ONE launch runs every deferred update if a
// ListTopTargets of this drain needs its quiz's posterior; then the RecordQuizTarget calls (the updates read the cube as it was), the StartQuiz
// calls in one launch and the ResumeQuiz calls in theirs; then the combined sweeps leaders have posted; then the listings not made already.
void HipEngine::DrainPosted(PostedOp *ordered) {
  _postedDrains++;
  const PostedCounts n = RunPostedInPlace(ordered);
  Error flushErr;
  if (n.needFlush) flushErr = FlushUpdates();
  if (n.trains > 0) { TrainPosted(ordered); MarkStreamBusy(); }
  if (n.starts > 0) StartPosted(ordered);
  if (n.resumes > 0) ResumePosted(ordered, n.resumes);
  for (PostedOp *op = ordered; op != nullptr; op = op->next)   // (behind the updates, ahead of the listings: the sweep is what the most clients wait for)
    if (op->kind == OpKind::LaunchBatch) LaunchBatchLocked(*op->ctx, *op->batch, *op->flight);
  ListPosted(ordered, flushErr);
  // The drain runs on the holder's way out -- possibly after a selection path declared the stream idle -- and may have launched
  // updates, trainings, quiz starts and listings: whoever takes the lock next finds the stream marked busy.
  MarkStreamBusy();
}

HipEngine::PostedCounts HipEngine::RunPostedInPlace(PostedOp *ordered) {
  PostedCounts n;
  for (PostedOp *op = ordered; op != nullptr; op = op->next) {
    _postedOps++;
    switch (op->kind) {
      case OpKind::RecordAnswer: op->err = RecordAnswerLocked(op->iQuiz, op->iAnswer, op->remote, false); break;
      case OpKind::ReleaseQuiz: op->err = ReleaseQuizLocked(op->iQuiz, false); break;
      case OpKind::RecordQuizTarget: n.trains++; break;
      case OpKind::StartQuiz: n.starts++; break;
      case OpKind::ResumeQuiz: n.resumes++; break;
      case OpKind::LaunchBatch: break;
      case OpKind::ListTopTargets:
        op->result = -1;
        op->err = CheckRegular("list top targets");
        if (!op->err.ok()) break;
        op->quiz = UseQuiz(op->err, op->iQuiz);
        if (op->quiz != nullptr) { op->serial = op->quiz->serial; n.needFlush = n.needFlush || op->quiz->updatePending; }
        break;
    }
  }
  return n;
}

// The StartQuiz calls of a drain: ONE launch sets all their priors (as StartQuizBatch; chunks of kStartInline)
void HipEngine::StartPosted(PostedOp *ordered) {
  MarkStreamBusy();
  hipSetDevice(_device);
  static thread_local StartBatchInline batch;   // (4 KB of pointers: not on a client thread's stack)
  batch.n = 0;
  batch.askedWords = (int64_t)BitWords(_Q);
  std::vector<PostedOp *> chunk;
  auto launch = [&]() {
    if (batch.n > 0) {
      const hipError_t he = LaunchStartQuizBatch(View(), batch, _opt.workers, _stream);
      if (he != hipSuccess)
        for (PostedOp *o : chunk)
          if (o->result >= 0) {
            Quiz *q = _quizzes[(size_t)o->result];
            UnassignQuiz(o->result);
            DestroyQuiz(q);
            o->result = -1;
            o->err = HipErr(he, "StartQuiz");
          }
    }
    batch.n = 0;
    chunk.clear();
  };
  for (PostedOp *op = ordered; op != nullptr; op = op->next) {
    if (op->kind != OpKind::StartQuiz) continue;
    _startBatch = &batch;
    op->result = CreateQuiz(op->err, 0, nullptr, nullptr, nullptr, 0, nullptr);
    _startBatch = nullptr;
    chunk.push_back(op);
    if (batch.n == kStartInline) launch();
  }
  launch();
}

// The ResumeQuiz calls of a drain: one launch sequence and one synchronisation per chunk for all (as ResumeQuizBatch), each call failing or succeeding on its own
void HipEngine::ResumePosted(PostedOp *ordered, int64_t nResumes) {
  MarkStreamBusy();
  std::vector<ResumeEntry> es;
  es.reserve((size_t)nResumes);
  for (PostedOp *op = ordered; op != nullptr; op = op->next)
    if (op->kind == OpKind::ResumeQuiz) { es.emplace_back(); es.back().nAnswered = op->nAnswered; es.back().pAQs = op->aqs; }
  (void)ResumeEntriesLocked(es, false);
  size_t i = 0;
  for (PostedOp *op = ordered; op != nullptr; op = op->next)
    if (op->kind == OpKind::ResumeQuiz) { op->err = es[i].err; op->result = es[i].err.ok() ? es[i].id : -1; i++; }
  _resumeBatches++;
  _resumesBatched += (uint64_t)nResumes;
}

// The listings that the update kernel has not made already (flushErr: the deferred updates' launch).  The last stage: every record is handed back here.
void HipEngine::ListPosted(PostedOp *ordered, const Error &flushErr) {
  for (PostedOp *op = ordered; op != nullptr;) {
    PostedOp *const next = op->next;   // (the operation is its thread's again the moment it is done)
    if (op->kind == OpKind::ListTopTargets && op->quiz != nullptr) {
      Quiz *q = op->quiz;
      const int64_t want = std::min<int64_t>(op->maxCount, _T);
      // (a ReleaseQuiz of the same quiz later in this drain -- a client's error, IPqaEngine.h:44 -- has taken it away since)
      const bool gone = (size_t)op->iQuiz >= _quizzes.size() || _quizzes[(size_t)op->iQuiz] != q || q->serial != op->serial;
      if (gone) { op->result = -1; op->err = Error::MakeP(ErrCode::AbsentId, "id=" + std::to_string(op->iQuiz), "Quiz index is not in the registry (but rather at a gap)."); }
      else if (!flushErr.ok()) op->err = flushErr;
      else if (want > kQuizTop || _T > 16384) op->result = PostedOp::kTakeLockYourself;
      else {
        _topWantRecent = want >= _topWantRecent ? want : want + (_topWantRecent - want) * 7 / 8;
        const bool cached = q->topOp != 0 && q->topVersion == q->priorVersion && want <= q->topCount;
        hipError_t he = hipSuccess;
        if (!cached) {
          hipSetDevice(_device);
          const uint64_t opNo = ++_opSeq;
          he = LaunchTopTargets(View(), q->dPrior, want, q->pin->top, &q->pin->nOut, &q->pin->topFlag, opNo, _stream);
          if (he == hipSuccess) { q->topOp = opNo; q->topVersion = q->priorVersion; q->topCount = want; }
        }
        if (he != hipSuccess) op->err = HipErr(he, "ListTopTargets");
        else { op->pin = q->pin; op->flagOp = q->topOp; op->result = want; }
      }
    }
    _mu.Done(op);
    op = next;
  }
}

// The RecordQuizTarget calls of a drain, in the order they were posted: calls with different targets touch disjoint cells
// and go out in ONE launch (train_batch_inline_kernel: a workgroup per call); a call whose target is already in the batch, or that
// does not fit the kernel's arguments, closes the batch first (or runs alone, the usual way).
void HipEngine::TrainPosted(PostedOp *ordered) {
  static thread_local TrainBatchInline tb;   // (2.5 KB)
  tb.nCalls = 0; tb.nChainsTotal = 0; tb.nSteps = 0;
  std::vector<PostedOp *> inBatch;
  hipSetDevice(_device);
  auto launch = [&]() {
    if (tb.nCalls > 0) {
      const hipError_t he = LaunchTrainBatchInline(_dCube, _elem, _dVB, _K, _ldT, tb, _stream);
      if (he != hipSuccess) for (PostedOp *o : inBatch) o->err = HipErr(he, "RecordQuizTarget");
      _trainBatches++;
      _trainBatchCalls += (uint64_t)tb.nCalls;
    }
    tb.nCalls = 0; tb.nChainsTotal = 0; tb.nSteps = 0;
    inBatch.clear();
  };
  bool stopped = false;
  for (PostedOp *op = ordered; op != nullptr; op = op->next) {
    if (op->kind != OpKind::RecordQuizTarget) continue;
    op->err = CheckRegular("record quiz target");
    if (!op->err.ok()) continue;
    const int64_t iTarget = op->iTarget;
    Quiz *q = UseQuiz(op->err, op->iQuiz);
    if (q == nullptr) continue;
    op->err = ValidateTrainLocked((int64_t)q->answers.size(), q->answers.data(), iTarget);
    if (!op->err.ok()) continue;
    if (!stopped) { StopServer(); stopped = true; }   // the cube changes (and the deferred updates read it as it was: they run first)
    std::vector<TrainStep> steps;
    std::vector<int64_t> chainStart;
    BuildTrainSteps((int64_t)q->answers.size(), q->answers.data(), true, steps, chainStart);
    const int64_t nChains = (int64_t)chainStart.size() - 1;
    bool fits = (int64_t)steps.size() <= kTrainBatchSteps && nChains + 1 <= (int64_t)(sizeof(tb.chainStart) / sizeof(tb.chainStart[0]));
    for (const TrainStep &st : steps) fits = fits && st.q <= INT32_MAX && st.a1 < 256 && st.a2 < 256;
    if (!fits) {   // a long quiz: the usual way, in its place in the order
      launch();
      op->err = TrainLocked((int64_t)q->answers.size(), q->answers.data(), iTarget, op->amount, true);
      continue;
    }
    bool clash = tb.nCalls == kTrainBatchCalls || tb.nSteps + (int64_t)steps.size() > kTrainBatchSteps ||
                 tb.nChainsTotal + tb.nCalls + nChains + 1 > (int64_t)(sizeof(tb.chainStart) / sizeof(tb.chainStart[0]));
    for (int c = 0; c < tb.nCalls && !clash; c++) clash = tb.calls[c].iTarget == iTarget;
    if (clash) launch();
    TrainBatchCall &call = tb.calls[tb.nCalls];
    call.iTarget = iTarget; call.amount = op->amount; call.firstChain = tb.nChainsTotal; call.nChains = (int32_t)nChains;
    uint16_t *cs = tb.chainStart + tb.nChainsTotal + tb.nCalls;   // (every call's chain starts are followed by one end marker)
    for (int64_t c = 0; c <= nChains; c++) cs[c] = (uint16_t)(tb.nSteps + chainStart[(size_t)c]);
    for (size_t i = 0; i < steps.size(); i++)
      tb.steps[tb.nSteps + (int64_t)i] = TrainBatchStep{(int32_t)steps[i].q, (uint8_t)steps[i].kind, (uint8_t)steps[i].a1, (uint8_t)steps[i].a2, 0};
    tb.nSteps += (int32_t)steps.size();
    tb.nChainsTotal += (int32_t)nChains;
    tb.nCalls++;
    inBatch.push_back(op);
  }
  launch();
}

int64_t HipEngine::Combine(Error &err, int64_t iQuiz, SelKind kind, uint64_t rnd) {
  CallScope scope(_activeCallers);
  _mu.spinFirst.store(ClientsFitCpus() && _activeCallers.load(std::memory_order_relaxed) > 1, std::memory_order_relaxed);
  if (!_opt.combine) {
    std::lock_guard<EngineMutex> lk(_mu);
    return SelectLocked(err, iQuiz, kind, rnd);
  }
  // Nobody else is inside a quiz-level call (the usual case of the reference's wrappers: one quiz loop on one thread): straight to
  // the single-quiz path -- no request to queue, no batch context, no flight.  Racing with a client that arrives just now is
  // harmless: each is served by itself, under the engine's lock, as with combining switched off.
  if (_activeCallers.load(std::memory_order_relaxed) == 1 && _extCallers == nullptr && _mu.try_lock()) {
    std::lock_guard<EngineMutex> lk(_mu, std::adopt_lock);
    _flushedSinceSweep.store(0, std::memory_order_relaxed);
    return SelectLocked(err, iQuiz, kind, rnd);
  }
  SelRequest r;
  r.iQuiz = iQuiz; r.kind = kind; r.rnd = rnd;
  int st = _comb.Wait(r, &_sweepNsEwma, ClientsFitCpus());
  if (st == kReqLead) {   // (the lead: nobody else led, or the leader before served its own batch and handed the lead to this, the oldest request)
    if (_opt.lingerUs > 0 && Concurrent())   // (alone in the engine: nobody to wait for)
      _comb.Linger(_opt.lingerUs, _flushedSinceSweep.load(std::memory_order_relaxed), _activeCallers);
    Flight f;
    st = _comb.Lead(
        r, kMaxBatch, [this](int64_t m) { return PreferredCombinedBatch(m); },
        [&](BatchCtx &c, std::vector<SelRequest *> &batch, std::chrono::steady_clock::time_point tA) {
          f.tA = tA;
          LaunchBatch(c, batch, f);   // (under the engine's lock; what could not be launched has its error -- or its result, for a batch of one)
        },
        [&](BatchCtx &c, std::vector<SelRequest *> &batch) { return !f.live.empty() && CollectBatch(c, batch, f, &r); });
  }
  if (st == kReqSelect) {   // the sweep has run: this quiz's priorities are on the host, the selection is this thread's own work
    SelectFromPriorities(&r);
    r.ctx->readers.fetch_sub(1, std::memory_order_release);
  }
  err = r.err;
  return r.result;
}

// One request of a combined sweep, after the sweep: this quiz's priority vector out of the batch's matrix, then the selector (as
// the single-quiz path's host_sampled form: SelectSampledHost; the argmax by the device's rule), then NextQuestion's bookkeeping.
int64_t HipEngine::SelectFromPriorities(SelRequest *r) {
  // No engine lock: the priorities are the sweep's, the asked / gap bits the leader's snapshot of the moment it launched the
  // sweep (what the kernel saw), the quiz object is held by inSelection, and the two things written -- the quiz's active
  // question, the asked-questions counter -- are this quiz's own or atomic.
  Quiz *q = r->quiz;
  const int64_t nQ = r->nQ;
  auto skip = [&](int64_t k) { return BitTest(r->unavailable, k); };
  std::vector<double> run((size_t)nQ);
  if (!TakePriorities(r->view, nQ, skip, run.data(), std::chrono::seconds(30))) {
    r->err = HipErr(hipErrorNotReady, "priority vector hand-over (combined sweep)");
    q->inSelection.store(false, std::memory_order_release);
    return r->result = -1;
  }
  BestPick best;   // (kb_plan.h: the device's rule -- maximum priority, lowest index on ties, NaN never wins)
  if (r->kind == SelKind::Argmax) for (int64_t k = 0; k < nQ; k++) if (!skip(k)) best.Offer(run[(size_t)k], k);
  const int64_t pick = r->kind == SelKind::Sampled ? SelectSampledHostBits(run.data(), nQ, r->nSub, r->rnd, r->unavailable.data(), nullptr) : best.index;
  r->result = FinishSelection(r->err, q, pick, nQ, r->unavailable.data());
  q->inSelection.store(false, std::memory_order_release);
  return r->result;
}

// How many of `m` waiting requests a combined sweep should take.  The (quiz, chunk) sweep costs by its quiz slots -- 8, 16, 32 or
// groups of 64 (tools/midbatch_bench.py at 1000 x 5 x 1000: 60 / 107 / 192 / 362 us of kernel) -- so 20 requests cost what 32 do; with
// the device as the bottleneck of a busy server, a sweep of 16 now and the other 4 with the next one serve more clients per second.
int64_t HipEngine::PreferredCombinedBatch(int64_t m) const {
  if (_opt.batchForm != 0 || _elem != 8 || !EvalMidBatchSupported(View())) return m;
  if (m <= 8) return m;
  if (m <= 10) return 8;
  if (m <= 16) return m;
  if (m <= 25) return 16;
  if (m <= 32) return m;
  if (m <= 51) return 32;
  const int64_t full = m / 64 * 64, rem = m % 64;
  return rem == 0 || rem >= 52 ? m : std::max<int64_t>(full, 32);
}

// Validate and launch (the caller holds the context; the engine's lock is taken and released here).  f.live: the requests whose
// sweep is in flight; every other request of `batch` has its result or error.
void HipEngine::LaunchBatch(BatchCtx &c, std::vector<SelRequest *> &batch, Flight &f) {
  std::unique_lock<EngineMutex> lk(_mu, std::defer_lock);
  if (batch.size() > 1) {
    // (taken: its holder launches this sweep on its way out.  Not TakeOrPost: "post_always" forces the clients' calls only)
    LaunchBatchOp op(c, batch, f);
    if (TryLockOrPost(_mu, lk, op)) return;
  } else lk.lock();   // (a batch of one is the single-quiz path: nothing for a holder to share, so it waits for the lock)
  LaunchBatchLocked(c, batch, f);
}

void HipEngine::LaunchBatchLocked(BatchCtx &c, std::vector<SelRequest *> &batch, Flight &f) {
  auto single = [&](SelRequest *r) { r->result = SelectLocked(r->err, r->iQuiz, r->kind, r->rnd); };
  f.tB = std::chrono::steady_clock::now();
  if (batch.size() == 1) { _flushedSinceSweep.store(0, std::memory_order_relaxed); single(batch[0]); return; }
  auto failAll = [&](const Error &e) { for (SelRequest *r : batch) { r->err = e; r->result = -1; } };
  Error err = CheckRegular("compute next question");
  if (!err.ok()) { failAll(err); return; }
  hipSetDevice(_device);
  err = FlushUpdates();
  if (!err.ok()) { failAll(err); return; }
  std::vector<SelRequest *> live;
  std::vector<int64_t> ids;
  for (SelRequest *r : batch) {
    Error qe;
    if (UseQuiz(qe, r->iQuiz) == nullptr) { r->err = qe; r->result = -1; continue; }
    live.push_back(r);
    ids.push_back(r->iQuiz);
    f.anySampled = f.anySampled || r->kind == SelKind::Sampled;
  }
  if (live.empty()) return;
  if (live.size() == 1 || (_opt.server && ServerUsable()) || _opt.useGraph) {   // (the resident sweep and graph replay serve one quiz at a time)
    for (SelRequest *r : live) single(r);
    return;
  }
  const int64_t n = (int64_t)live.size();
  std::vector<Quiz *> quizzes;
  err = EnqueueCombinedLocked(c, n, ids.data(), f.anySampled, &f.cf, quizzes);
  if (!err.ok()) { for (SelRequest *r : live) { r->err = err; r->result = -1; } return; }
  const int64_t nSubtasks = SampledSubtasks();
  for (int64_t i = 0; i < n; i++) {
    SelRequest *r = live[(size_t)i];
    Quiz *q = quizzes[(size_t)i];
    r->serial = q->serial;
    // what finishes the selection once the sweep has run (the client itself, from the priorities, if any request of the batch is
    // sampled; else the leader, from the kernel's choices) without the engine's lock: the quiz (held), the asked questions and
    // gaps as the sweep sees them
    r->quiz = q;
    q->inSelection.store(true, std::memory_order_relaxed);
    r->nQ = _Q;
    r->nSub = nSubtasks;
    r->unavailable.resize(_hQGap.size());
    for (size_t w = 0; w < r->unavailable.size(); w++) r->unavailable[w] = _hQGap[w] | q->hAsked[w];
  }
  _combBatches++;
  _combRequests += (uint64_t)n;
  if ((uint64_t)n > _combMaxBatch) _combMaxBatch = (uint64_t)n;
  f.live.swap(live);
  c.inFlight.store(true, std::memory_order_relaxed);
  f.tC = std::chrono::steady_clock::now();
}

// Wait for the sweep and hand the results out -- the engine open to the other clients' calls meanwhile (RecordAnswer,
// ListTopTargets, StartQuiz ... and the next leader's launch).  Returns true if `own` is to select for itself.
bool HipEngine::CollectBatch(BatchCtx &c, std::vector<SelRequest *> &batch, Flight &f, SelRequest *own) {
  const int64_t n = (int64_t)f.live.size();
  CiHipSelection winners[kMaxBatch];   // (argmax batches: the kernel's choices)
  const Error err = CollectCombined(c, f.cf, f.anySampled ? nullptr : winners, nullptr);
  c.inFlight.store(false, std::memory_order_relaxed);
  const auto tD = std::chrono::steady_clock::now();
  auto ns = [](auto a, auto b) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count(); };
  if (!err.ok()) {
    for (SelRequest *r : f.live) {
      r->err = err;
      r->result = -1;
      if (r->quiz) r->quiz->inSelection.store(false, std::memory_order_release);
    }
    return false;
  }
  _combNs[0] += ns(f.tA, f.tB); _combNs[1] += ns(f.tB, f.tC); _combNs[2] += ns(f.tC, tD);
  if (f.anySampled) {
    // The priority vectors are on the host: every client selects for ITSELF (the O(Q) scalar Kahan steps of the reference's
    // selector, CpuEngine.cpp:362-400, run on as many cores as there are clients), the leader only for its own request.
    c.readers.fetch_add((int)n, std::memory_order_acq_rel);
    bool ownLive = false;
    for (int64_t i = 0; i < n; i++) {
      SelRequest *r = f.live[(size_t)i];
      r->view = ViewOf(c, f.cf, i);
      r->ctx = &c;
      if (r == own) { ownLive = true; continue; }
      Combiner<SelRequest, BatchCtx>::LetSelect(batch, r);
    }
    _combNs[3] += ns(tD, std::chrono::steady_clock::now());
    return ownLive;
  }
  // The kernel's choices: finished here for every request, and without the engine's lock -- the quizzes are held (inSelection:
  // a ReleaseQuiz of one waits), what is written is each quiz's own or atomic.
  const auto tE = std::chrono::steady_clock::now();
  for (int64_t i = 0; i < n; i++) {
    SelRequest *r = f.live[(size_t)i];
    const int64_t pick = winners[i]._iQuestion < 0 ? kSelNone : winners[i]._iQuestion - _qFirst;
    r->result = FinishSelection(r->err, r->quiz, pick, r->nQ, r->unavailable.data());
    r->quiz->inSelection.store(false, std::memory_order_release);
  }
  _combNs[3] += ns(tD, tE);
  _combNs[4] += ns(tE, std::chrono::steady_clock::now());
  return false;
}

Error HipEngine::EvalPriorities(int64_t iQuiz, double *pOut, int64_t n) {
  std::lock_guard<EngineMutex> lk(_mu);
  Error err = CheckRegular("compute next question");
  if (!err.ok()) return err;
  Quiz *q = UseQuiz(err, iQuiz);
  if (!q) return err;
  if (!pOut) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the priority buffer.");
  if (n != _Q) return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(n, _Q, _Q), "Priority buffer length must equal the local question count.");
  hipSetDevice(_device);
  StopServer();   // a launched sweep has no room beside the resident one and would wait for it to idle out
  err = LaunchSingleSweep(q, nullptr);
  if (!err.ok()) return err;
  HIP_TRY(hipMemcpyAsync(pOut, _dPriority, (size_t)_Q * sizeof(double), hipMemcpyDeviceToHost, _stream));
  HIP_TRY(hipStreamSynchronize(_stream));
  return Error();
}

}  // namespace pqa
