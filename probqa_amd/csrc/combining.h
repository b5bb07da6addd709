// combining.h -- how many client threads share one engine, for HipEngine (hip_engine_combine.cpp) and ShardedEngine
// (sharded_engine.cpp) alike: a lock whose holder runs the operations posted meanwhile on its way out (PostingLock), and the flat
// combining of concurrent selection requests into one sweep (Combiner).  Host C++17 only -- no HIP -- so that a plain g++ build
// stress-tests it (tests/combining_check.cpp).
#pragma once

#include <immintrin.h>
#include <linux/futex.h>
#include <sys/prctl.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

namespace pqa {

// A waiting client sleeps on ITS OWN record's state word and is woken alone (futex): with one condition variable for all
// requests every published batch woke every sleeper, most of them only to find their own request unserved and sleep again.
inline void FutexWait(std::atomic<int> *word, int expected) {
  syscall(SYS_futex, reinterpret_cast<int *>(word), FUTEX_WAIT_PRIVATE, expected, nullptr, nullptr, 0);
}
inline void FutexWakeOne(std::atomic<int> *word) { syscall(SYS_futex, reinterpret_cast<int *>(word), FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0); }
// The new state, then the wake -- always: whether the owner sleeps cannot be asked once the state is stored (it may have seen it,
// returned and gone with its request), and a wake on a word nobody sleeps on only costs the call.
inline void PublishState(std::atomic<int> *word, int state) {
  word->store(state, std::memory_order_release);
  FutexWakeOne(word);
}
static_assert(sizeof(std::atomic<int>) == sizeof(int), "the state word is slept on as a futex");
// What the state words hold (plain ints: the word is slept on as a futex).
// A posted operation's (PostingLock): posted; posted and its thread asleep on this word; done -- the record is its thread's again.
constexpr int kOpPosted = 0, kOpDone = 1, kOpAsleep = 2;
// A selection request's (Combiner): waiting; served; the lead handed over -- serve the queue yourself; the sweep is done -- select
// for yourself, then release one reader of the request's context.
constexpr int kReqWaiting = 0, kReqServed = 1, kReqLead = 2, kReqSelect = 3;
enum class SelKind { Argmax, Sampled };   // what a selection request asks for (Sampled: with its random number)

struct CallScope {   // a client thread inside the engine's quiz-level calls
  std::atomic<int> &n;
  explicit CallScope(std::atomic<int> &c) : n(c) { n.fetch_add(1, std::memory_order_relaxed); }
  ~CallScope() { n.fetch_sub(1, std::memory_order_relaxed); }
};

// ---- the posting lock ------------------------------------------------------------------------------------------------------------
// With dozens of client threads an engine's lock is not held long but changes hands through the kernel every time, one wake-up
// latency per call, serially.  So a call that finds the lock taken may POST its operation instead (PostAndWait) and sleep on the
// record's own word; whoever holds the lock runs everything posted so far, in post order, right before it lets go (the owner's
// `run` over the ordered list) and wakes the posters after releasing.
// Op: a record with `std::atomic<int> state` (kOpPosted, kOpAsleep, kOpDone) and `Op *next`.
template <typename Op, typename Owner>
class PostingLock {
 public:
  using Run = void (Owner::*)(Op *ordered);
  PostingLock(Owner *owner, Run run) : _owner(owner), _run(run) {}
  bool try_lock() { return _m.try_lock(); }
  void lock() { _m.lock(); }
  void unlock() {
    for (;;) {
      std::atomic<int> *wake[64];   // (no allocation for up to 64 sleepers)
      size_t nWake = 0;
      std::vector<std::atomic<int> *> more;
      if (_posted.load(std::memory_order_acquire) != nullptr) {
        Drain();
        nWake = _nWake;
        std::copy(_wake, _wake + nWake, wake);
        more.swap(_more);
        _nWake = 0;
      }
      _m.unlock();
      for (size_t i = 0; i < nWake; i++) FutexWakeOne(wake[i]);
      for (std::atomic<int> *word : more) FutexWakeOne(word);
      // Posted between the drain and the release: its thread saw the lock taken and sleeps.  (Both sides are a locked
      // read-modify-write followed by a load -- the post then try_lock there, the release then this load here: one of the two sees
      // the other.)  If somebody else has the lock by now, the operation is theirs to run.
      if (_posted.load(std::memory_order_seq_cst) == nullptr || !_m.try_lock()) return;
    }
  }
  void Push(Op &op) {   // (PostAndWait's first step)
    Op *head = _posted.load(std::memory_order_relaxed);
    do op.next = head; while (!_posted.compare_exchange_weak(head, &op, std::memory_order_seq_cst, std::memory_order_relaxed));
  }
  // (the owner's run, optionally) `op` -- the first record of the ordered list not handed back yet -- is done: it is its thread's
  // again from here on, and the ones after it are published as they are done too, not all at the end
  void Done(Op *op) {
    _rest = op->next;
    Publish(op);
  }
  // `op` run under the lock: here if the lock is free (with whatever else has been posted, on the way out), else by its holder.
  // Returns true if it had to be posted.
  bool RunOrPost(Op &op);

 private:
  // Everything posted so far, in the order it was posted, to the owner; then every record it has not handed back (Done) is its
  // thread's again
  void Drain() {
    Op *list = _posted.exchange(nullptr, std::memory_order_acq_rel);
    Op *ordered = nullptr;
    while (list != nullptr) { Op *n = list->next; list->next = ordered; ordered = list; list = n; }
    _rest = ordered;
    (_owner->*_run)(ordered);
    while (_rest != nullptr) Done(_rest);
  }
  void Publish(Op *op) {   // (the record is its thread's again the moment its state says so: nothing of it is read after)
    std::atomic<int> *word = &op->state;
    if (word->exchange(kOpDone, std::memory_order_acq_rel) == kOpAsleep) {
      if (_nWake < 64) _wake[_nWake++] = word;
      else _more.push_back(word);
    }
  }
  std::mutex _m;
  std::atomic<Op *> _posted{nullptr};
  // (the holder's) the drain's records not handed back yet, and its sleepers, woken once the lock is released
  Op *_rest = nullptr;
  std::atomic<int> *_wake[64];
  size_t _nWake = 0;
  std::vector<std::atomic<int> *> _more;
  Owner *const _owner;
  const Run _run;
};

// Post `op` to `lock` and return once its holder has run it.  `lock` is taken through its own try_lock (a lock derived from
// PostingLock may do more there).
template <typename Lock, typename Op>
void PostAndWait(Lock &lock, Op &op) {
  lock.Push(op);
  for (;;) {
    if (lock.try_lock()) lock.unlock();   // (free after all: the release runs it -- and the others')
    for (int spins = 0; spins < 300; spins++) {
      if (op.state.load(std::memory_order_acquire) == kOpDone) return;
      _mm_pause();
    }
    int expected = kOpPosted;
    if (op.state.compare_exchange_strong(expected, kOpAsleep, std::memory_order_seq_cst) || expected == kOpAsleep) {
      // (the timeout is a belt to the braces of unlock(): a millisecond, then the lock is tried again)
      struct timespec ts{0, 1000000};
      syscall(SYS_futex, reinterpret_cast<int *>(&op.state), FUTEX_WAIT_PRIVATE, kOpAsleep, &ts, nullptr, 0);
    }
    if (op.state.load(std::memory_order_acquire) == kOpDone) return;
  }
}

// `op` posted to `lock`'s holder if the lock is taken -- or in any case with `force` -- and run by the time this returns: true.
// Otherwise false: `lk` holds the lock, and `op` is the caller's to run in whatever form it likes (nothing has seen it).
template <typename Lock, typename Op>
bool TryLockOrPost(Lock &lock, std::unique_lock<Lock> &lk, Op &op, bool force = false) {
  if (!force && lock.try_lock()) {
    lk = std::unique_lock<Lock>(lock, std::adopt_lock);
    return false;
  }
  PostAndWait(lock, op);
  return true;
}

template <typename Op, typename Owner>
bool PostingLock<Op, Owner>::RunOrPost(Op &op) {
  if (try_lock()) {
    op.next = nullptr;
    (_owner->*_run)(&op);
    unlock();
    return false;
  }
  PostAndWait(*this, op);
  return true;
}

// ---- the combiner ----------------------------------------------------------------------------------------------------------------
// Concurrent selection calls (the reference serves them under a SHARED lock).  A caller queues its request; if a leader is at work
// it waits for its result, otherwise it becomes the leader: it takes everything queued so far -- distinct quizzes -- launches ONE
// sweep for it, hands the lead to the oldest request still waiting as soon as the sweep is LAUNCHED, and then collects.  Two
// batch contexts alternate, so that the next leader launches the next sweep while this one's runs and the device finds it queued.
struct CombineCtx {
  std::mutex mu;                       // one batch at a time in this context
  std::atomic<int> readers{0};         // clients still selecting out of the context's host buffers
  std::atomic<bool> inFlight{false};   // a leader's sweep launched and not yet collected
};

// Req: `int64_t iQuiz` and `std::atomic<int> state` (kReqWaiting, kReqServed, kReqLead, kReqSelect).  Ctx: derived from CombineCtx.
template <typename Req, typename Ctx>
class Combiner {
 public:
  using Clock = std::chrono::steady_clock;
  explicit Combiner(Ctx *ctx) : _ctx(ctx) {}

  // Queue `r` and wait for its state: kReqLead at once if nobody leads.  sweepNs: the followers' wait is averaged into it, and with `nap`
  // (fewer clients than CPUs) a follower sleeps most of that expected wait in short naps, then spins; without, a short spin, then
  // the futex (spinning waiters would take the CPUs from the threads that have work).
  int Wait(Req &r, std::atomic<int64_t> *sweepNs = nullptr, bool nap = false) {
    {
      std::lock_guard<std::mutex> lk(_mu);
      _queue.push_back(&r);
      if (!_leaderActive) { _leaderActive = true; return kReqLead; }
    }
    int st = kReqWaiting;
    const auto tw0 = Clock::now();
    for (int spins = 0; spins < 1500 && (st = r.state.load(std::memory_order_acquire)) == kReqWaiting; spins++) _mm_pause();
    if (st == kReqWaiting && nap && sweepNs != nullptr) {
      // (woken through the kernel the clients of one sweep arrive tens of microseconds apart)
      const int64_t expect = sweepNs->load(std::memory_order_relaxed);
      if (expect > 90000) {
        static thread_local bool slackSet = false;
        if (!slackSet) { prctl(PR_SET_TIMERSLACK, 2000UL, 0, 0, 0); slackSet = true; }
        const auto until = tw0 + std::chrono::nanoseconds(std::min<int64_t>(expect - 50000, 2000000));
        // (in naps of 40 us: the lead may be handed to this request meanwhile, and the next sweep waits for its leader)
        while ((st = r.state.load(std::memory_order_acquire)) == kReqWaiting && Clock::now() < until) {
          struct timespec ts{0, 40000};
          nanosleep(&ts, nullptr);
        }
      }
      for (int spins = 0; spins < 12000 && (st = r.state.load(std::memory_order_acquire)) == kReqWaiting; spins++) _mm_pause();
    }
    while (st == kReqWaiting) {
      FutexWait(&r.state, kReqWaiting);   // (returns at once if the state is no longer that)
      st = r.state.load(std::memory_order_acquire);
    }
    if (sweepNs != nullptr) {
      const int64_t waited = std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - tw0).count();
      const int64_t old = sweepNs->load(std::memory_order_relaxed);
      sweepNs->store(old == 0 ? waited : old + (waited - old) / 8, std::memory_order_relaxed);
    }
    return st;
  }

  // The leader, before it takes its batch.  The clients whose answers were recorded since the last sweep (`sinceSweep`) are on their
  // way here: a leader that starts at once sweeps for the two or three that were quickest and makes the rest wait for a second
  // sweep.  So it waits -- microseconds -- until most of them have queued, or nobody new comes.  While the previous leader's sweep
  // still runs there is no hurry at all: a sweep launched now only queues behind it, so the requests that arrive until it is
  // (nearly) done ride along for free.
  void Linger(int64_t lingerUs, int64_t sinceSweep, const std::atomic<int> &callers) {
    const int64_t expect = std::min<int64_t>(sinceSweep, callers.load(std::memory_order_relaxed) - 1);
    const Ctx &other = _ctx[_next ^ 1];
    const auto t0 = Clock::now();
    const auto limit = std::chrono::microseconds(lingerUs), limitBusy = std::chrono::microseconds(8 * lingerUs);
    for (;;) {
      size_t have;
      { std::lock_guard<std::mutex> lk(_mu); have = _queue.size(); }
      const bool busy = other.inFlight.load(std::memory_order_relaxed);
      if (!busy && (expect <= 1 || (int64_t)have * 5 >= expect * 4)) break;
      if (busy && (int64_t)have >= callers.load(std::memory_order_relaxed) - 1) break;   // (everybody is here)
      for (int i = 0; i < 32; i++) _mm_pause();
      if (Clock::now() - t0 > (busy ? limitBusy : limit)) break;
    }
  }

  // The leader's turn: ONE batch -- at most maxBatch distinct quizzes, `own` among them (it is the oldest request), cut to
  // trim(size) -- in the next context, once its previous sweep has been collected and the clients selecting out of it are done.
  // launch(ctx, batch, tPicked) launches it (what could not be launched has its error, or its result); the lead goes on at once;
  // collect(ctx, batch) waits for the sweep and hands the results out (a request told to select for itself through LetSelect
  // leaves the batch) and returns true if `own` is to select for itself.  Returns `own`'s state: kReqServed or kReqSelect.
  template <typename Trim, typename Launch, typename Collect>
  int Lead(Req &own, int64_t maxBatch, Trim &&trim, Launch &&launch, Collect &&collect) {
    Ctx &c = _ctx[_next];
    _next ^= 1;
    const auto tPicked = Clock::now();
    std::unique_lock<std::mutex> ctxLock(c.mu);
    while (c.readers.load(std::memory_order_acquire) != 0) _mm_pause();
    std::vector<Req *> batch;
    {
      std::lock_guard<std::mutex> lk(_mu);
      std::vector<Req *> rest;
      for (Req *r : _queue) {
        bool take = (int64_t)batch.size() < maxBatch;
        for (size_t i = 0; take && i < batch.size(); i++) take = batch[i]->iQuiz != r->iQuiz;   // a quiz once per sweep
        (take ? batch : rest).push_back(r);
      }
      // (the sweep's lanes come in groups: the newest requests beyond the last well-filled group wait for the next sweep -- it is
      //  launched right behind this one)
      const size_t keep = (size_t)trim((int64_t)batch.size());
      if (keep < batch.size()) {
        rest.insert(rest.begin(), batch.begin() + (std::ptrdiff_t)keep, batch.end());
        batch.resize(keep);
      }
      _queue.swap(rest);
    }
    launch(c, batch, tPicked);
    {
      std::lock_guard<std::mutex> lk(_mu);
      if (_queue.empty()) _leaderActive = false;
      else PublishState(&_queue.front()->state, kReqLead);
    }
    const bool ownSelects = collect(c, batch);
    ctxLock.unlock();
    for (Req *r : batch)
      if (r != nullptr && r != &own) PublishState(&r->state, kReqServed);   // (r is its caller's again from here on)
    return ownSelects ? kReqSelect : kReqServed;
  }

  // (collect's) `r` is to select for itself out of its context: it is told so now, and leaves the batch -- not the leader's to
  // publish again
  static void LetSelect(std::vector<Req *> &batch, Req *r) {
    for (Req *&slot : batch) if (slot == r) slot = nullptr;
    PublishState(&r->state, kReqSelect);
  }

 private:
  Ctx *const _ctx;                     // [2]
  int _next = 0;                       // (the leader's)
  std::mutex _mu;
  std::vector<Req *> _queue;
  bool _leaderActive = false;
};

}  // namespace pqa
