// Stress check of probqa_amd/csrc/combining.h with fake operations and fake sweeps, no GPU (tests/test_combining.py builds it
// with g++, plain and with -fsanitize=thread).  Prints one "ok" line per part and exits 0, or names the broken property and exits 1.
//   combining_check lock <posters> <ops each>      the posting lock
//   combining_check combine <clients> <calls each>  the combiner
//   combining_check take <threads> <ops each>       TryLockOrPost: one way in for posted and direct calls
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "../probqa_amd/csrc/combining.h"

using namespace pqa;
using Clock = std::chrono::steady_clock;

#define CHECK(cond, ...)                                              \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "FAILED: %s: ", #cond);                    \
      std::fprintf(stderr, __VA_ARGS__);                              \
      std::fprintf(stderr, "\n");                                     \
      std::_Exit(1);                                                  \
    }                                                                 \
  } while (0)

static void SpinFor(int us) {
  const auto until = Clock::now() + std::chrono::microseconds(us);
  while (Clock::now() < until) _mm_pause();
}

// Join `threads`; a thread still running after `seconds` is stranded (its record never ran, or its request was never served).
static void JoinWithin(std::vector<std::thread> &threads, std::atomic<int> &finished, int seconds) {
  const auto deadline = Clock::now() + std::chrono::seconds(seconds);
  while (finished.load() < (int)threads.size()) {
    CHECK(Clock::now() < deadline, "%d of %zu threads still waiting after %d s", (int)threads.size() - finished.load(), threads.size(), seconds);
    std::this_thread::sleep_for(std::chrono::milliseconds(1));
  }
  for (std::thread &t : threads) t.join();
}

// ---- the posting lock -------------------------------------------------------------------------------------------------------------
struct Op {
  int tid = 0, idx = 0;
  std::atomic<int> runs{0};
  std::atomic<int> state{kOpPosted};
  Op *next = nullptr;
};

struct LockOwner {
  explicit LockOwner(int nThreads) : last(nThreads, -1) {}
  PostingLock<Op, LockOwner> lock{this, &LockOwner::Run};
  std::vector<int> last;               // per thread: the index of its newest record run (the lock held)
  int64_t ran = 0, drains = 0, inside = 0;
  void Run(Op *ordered) {
    CHECK(++inside == 1, "two drains at once");
    drains++;
    const bool handBack = drains % 2 == 1;   // (every other drain hands its records back one by one as they are done)
    for (Op *op = ordered; op != nullptr;) {
      Op *const next = op->next;
      CHECK(op->state.load() != kOpDone, "record of thread %d published before it ran", op->tid);
      CHECK(op->runs.fetch_add(1) == 0, "record %d of thread %d ran twice", op->idx, op->tid);
      CHECK(op->idx > last[(size_t)op->tid], "thread %d: record %d ran after %d (not in post order)", op->tid, op->idx, last[(size_t)op->tid]);
      last[(size_t)op->tid] = op->idx;
      ran++;
      if (handBack) lock.Done(op);
      op = next;
    }
    inside--;
  }
};

static void CheckLock(int posters, int opsEach) {
  // posters: PostAndWait, one record at a time; burst threads: several records pushed at once, the last one posted and waited for;
  // takers: the lock taken and released around a little work, and records run through RunOrPost
  const int bursts = 8, takers = 4, burst = 8;
  const int nThreads = posters + bursts + takers;
  LockOwner owner(nThreads);
  std::vector<std::vector<Op>> ops((size_t)nThreads);
  std::atomic<int> finished{0};
  std::vector<std::thread> threads;
  for (int t = 0; t < nThreads; t++) {
    ops[(size_t)t] = std::vector<Op>((size_t)opsEach);
    for (int i = 0; i < opsEach; i++) { ops[(size_t)t][(size_t)i].tid = t; ops[(size_t)t][(size_t)i].idx = i; }
  }
  for (int t = 0; t < nThreads; t++)
    threads.emplace_back([&, t] {
      std::vector<Op> &mine = ops[(size_t)t];
      if (t < posters) {
        for (Op &op : mine) { PostAndWait(owner.lock, op); CHECK(op.runs.load() == 1, "a record returned to its poster unrun"); }
      } else if (t < posters + bursts) {
        for (int i = 0; i < opsEach; i += burst) {
          const int end = std::min(opsEach, i + burst);
          for (int k = i; k < end - 1; k++) owner.lock.Push(mine[(size_t)k]);
          PostAndWait(owner.lock, mine[(size_t)end - 1]);
          for (int k = i; k < end; k++) CHECK(mine[(size_t)k].state.load(std::memory_order_acquire) == kOpDone, "an earlier record of a burst is not done");
        }
      } else {
        for (Op &op : mine) {
          { std::lock_guard<PostingLock<Op, LockOwner>> lk(owner.lock); SpinFor(2); }
          owner.lock.RunOrPost(op);
          CHECK(op.runs.load() == 1, "RunOrPost returned before its record ran");
        }
      }
      finished.fetch_add(1);
    });
  JoinWithin(threads, finished, 20);
  for (auto &v : ops) for (Op &op : v) CHECK(op.runs.load() == 1, "record %d of thread %d ran %d times", op.idx, op.tid, op.runs.load());
  CHECK(owner.ran == (int64_t)nThreads * opsEach, "%lld records run", (long long)owner.ran);
  std::printf("ok lock: %d threads, %lld records in %lld drains\n", nThreads, (long long)owner.ran, (long long)owner.drains);
}

// ---- one way in: TryLockOrPost ---------------------------------------------------------------------------------------------------------
struct TakeOp {
  bool forced = false;                 // posted whether the lock is free or not: must never run on the direct path
  std::atomic<int> runs{0};
  bool direct = false;                 // run by its own thread, holding the lock
  std::atomic<int> state{kOpPosted};
  TakeOp *next = nullptr;
};

struct TakeOwner {
  PostingLock<TakeOp, TakeOwner> lock{this, &TakeOwner::Drain};
  std::atomic<int> holders{0};         // threads inside the lock: 1 wherever a record runs
  int64_t drained = 0, direct = 0;     // (the lock held)
  void RunOne(TakeOp &op) {
    CHECK(holders.fetch_add(1) == 0, "a record ran while another thread held the lock");
    CHECK(op.runs.fetch_add(1) == 0, "a record ran twice");
    SpinFor(1);
    CHECK(holders.fetch_sub(1) == 1, "the lock was shared while a record ran");
  }
  void Drain(TakeOp *ordered) {
    for (TakeOp *op = ordered; op != nullptr; op = op->next) { RunOne(*op); drained++; }
  }
};

static void CheckTake(int nThreads, int opsEach) {
  TakeOwner owner;
  std::vector<std::vector<TakeOp>> ops((size_t)nThreads);
  for (auto &v : ops) v = std::vector<TakeOp>((size_t)opsEach);
  std::atomic<int> finished{0};
  std::vector<std::thread> threads;
  for (int t = 0; t < nThreads; t++)
    threads.emplace_back([&, t] {
      for (int i = 0; i < opsEach; i++) {
        TakeOp &op = ops[(size_t)t][(size_t)i];
        op.forced = (t + i) % 3 == 0;
        std::unique_lock<PostingLock<TakeOp, TakeOwner>> lk;
        if (TryLockOrPost(owner.lock, lk, op, op.forced)) {
          CHECK(!lk.owns_lock(), "a posted call came back holding the lock");
          CHECK(op.runs.load() == 1, "TryLockOrPost returned before its posted record ran");
        } else {
          CHECK(lk.owns_lock(), "a direct call came back without the lock");
          CHECK(!op.forced, "a forced record came back for the direct path");
          op.direct = true;
          owner.RunOne(op);
          owner.direct++;
        }
        if (t % 2 == 0) SpinFor(i % 3);   // (half the threads come back at once: the lock is mostly taken)
      }
      finished.fetch_add(1);
    });
  JoinWithin(threads, finished, 20);
  int64_t direct = 0;
  for (auto &v : ops)
    for (TakeOp &op : v) {
      CHECK(op.runs.load() == 1, "a record ran %d times", op.runs.load());
      CHECK(!(op.forced && op.direct), "a forced record ran on the direct path");
      direct += op.direct;
    }
  CHECK(direct == owner.direct && owner.drained + owner.direct == (int64_t)nThreads * opsEach, "%lld drained + %lld direct records",
        (long long)owner.drained, (long long)owner.direct);
  CHECK(owner.drained > 0 && owner.direct > 0, "one of the two outcomes never happened (%lld drained, %lld direct)", (long long)owner.drained, (long long)owner.direct);
  std::printf("ok take: %d threads, %lld records posted and drained, %lld run by their own threads\n", nThreads, (long long)owner.drained, (long long)owner.direct);
}

// ---- the combiner -----------------------------------------------------------------------------------------------------------------
struct Req {
  int64_t iQuiz = -1;
  std::atomic<int> state{kReqWaiting};
  int64_t result = -1;
  int served = 0;                      // times a result was given (by the leader, or by the client from its context)
  struct Ctx *ctx = nullptr;
  int slot = -1;
};

struct Ctx : CombineCtx {
  int64_t value[64] = {0};             // the fake sweep's results, read by the clients that select for themselves
  int batches = 0;
};

constexpr int64_t kMaxBatch = 12;
static int64_t Trim(int64_t m) { return m <= 4 ? m : m / 4 * 4; }   // lane groups of 4

struct Combine {
  Ctx ctx[2];
  Combiner<Req, Ctx> comb{ctx};
  std::atomic<int> callers{0};
  std::atomic<int64_t> sinceSweep{0}, sweepNs{0};
  std::atomic<int64_t> batches{0}, requests{0}, selfSelected{0}, leads{0};
  int64_t trimIn = -1, trimOut = -1;   // (the leader's)
};

static int64_t Expected(int64_t iQuiz, int batchNo) { return iQuiz * 1000003 + batchNo; }

static void ClientCall(Combine &S, int64_t iQuiz, bool nap) {
  CallScope scope(S.callers);
  Req r;
  r.iQuiz = iQuiz;
  int st = S.comb.Wait(r, nap ? &S.sweepNs : nullptr, nap);
  if (st == kReqLead) {
    S.leads.fetch_add(1);
    S.comb.Linger(20, S.sinceSweep.load(), S.callers);
    int batchNo = 0;
    bool selfSelect = false;
    st = S.comb.Lead(
        r, kMaxBatch,
        [&](int64_t m) { S.trimIn = m; return S.trimOut = Trim(m); },
        [&](Ctx &c, std::vector<Req *> &batch, Clock::time_point) {
          CHECK(c.readers.load() == 0, "a context reused while %d clients select out of it", c.readers.load());
          CHECK(!batch.empty() && batch[0] == &r, "the leader is not the oldest waiting request");
          CHECK(S.trimIn <= kMaxBatch, "batch of %lld beyond the limit", (long long)S.trimIn);
          CHECK((int64_t)batch.size() == S.trimOut, "batch of %zu, trimmed to %lld", batch.size(), (long long)S.trimOut);
          for (size_t i = 0; i < batch.size(); i++)
            for (size_t j = 0; j < i; j++) CHECK(batch[i]->iQuiz != batch[j]->iQuiz, "quiz %lld twice in a batch", (long long)batch[i]->iQuiz);
          batchNo = ++c.batches;
          selfSelect = batchNo % 2 == 0;
          for (size_t i = 0; i < batch.size(); i++) { c.value[i] = Expected(batch[i]->iQuiz, batchNo); batch[i]->slot = (int)i; }
          S.sinceSweep.store(0);
          c.inFlight.store(true, std::memory_order_relaxed);
        },
        [&](Ctx &c, std::vector<Req *> &batch) {
          SpinFor(batch.size() > 1 ? 30 : 5);   // the sweep
          c.inFlight.store(false, std::memory_order_relaxed);
          S.batches.fetch_add(1);
          S.requests.fetch_add((int64_t)batch.size());
          if (!selfSelect) {
            for (Req *q : batch) { q->result = c.value[q->slot]; q->served++; }
            return false;
          }
          c.readers.fetch_add((int)batch.size(), std::memory_order_acq_rel);
          bool own = false;
          std::vector<Req *> live(batch);
          for (Req *q : live) {
            q->ctx = &c;
            if (q == &r) { own = true; continue; }
            Combiner<Req, Ctx>::LetSelect(batch, q);
          }
          return own;
        });
    (void)batchNo;
  }
  if (st == kReqSelect) {   // select for yourself out of the context, then let it go
    SpinFor(3);
    r.result = r.ctx->value[r.slot];
    r.served++;
    r.ctx->readers.fetch_sub(1, std::memory_order_release);
    S.selfSelected.fetch_add(1);
  }
  CHECK(st == kReqServed || st == kReqSelect, "final state %d", st);
  CHECK(r.served == 1, "request of quiz %lld served %d times", (long long)iQuiz, r.served);
  CHECK(r.result % 1000003 != 0 && (r.result - r.result % 1000003) / 1000003 == iQuiz, "request of quiz %lld got the result %lld", (long long)iQuiz, (long long)r.result);
}

static void CheckCombine(int clients, int callsEach) {
  Combine S;
  std::atomic<int> finished{0};
  std::vector<std::thread> threads;
  for (int t = 0; t < clients; t++)
    threads.emplace_back([&, t] {
      for (int i = 0; i < callsEach; i++) {
        // (two clients per quiz: a quiz may be asked for twice at once, and is then swept once per batch)
        ClientCall(S, (t / 2) + 1, t % 4 == 1);
        S.sinceSweep.fetch_add(1);
        SpinFor(t % 7);
      }
      finished.fetch_add(1);
    });
  JoinWithin(threads, finished, 20);
  CHECK(S.requests.load() == (int64_t)clients * callsEach, "%lld requests swept for %lld calls", (long long)S.requests.load(), (long long)clients * callsEach);
  for (Ctx &c : S.ctx) CHECK(c.readers.load() == 0, "a context left with %d readers", c.readers.load());
  CHECK(S.selfSelected.load() > 0, "no request selected for itself");
  std::printf("ok combine: %d clients, %lld requests in %lld batches (%lld leads, %lld selected by their clients)\n", clients,
              (long long)S.requests.load(), (long long)S.batches.load(), (long long)S.leads.load(), (long long)S.selfSelected.load());
}

int main(int argc, char **argv) {
  if (argc == 4 && std::strcmp(argv[1], "lock") == 0) CheckLock(std::atoi(argv[2]), std::atoi(argv[3]));
  else if (argc == 4 && std::strcmp(argv[1], "combine") == 0) CheckCombine(std::atoi(argv[2]), std::atoi(argv[3]));
  else if (argc == 4 && std::strcmp(argv[1], "take") == 0) CheckTake(std::atoi(argv[2]), std::atoi(argv[3]));
  else { std::fprintf(stderr, "usage: %s lock|combine|take <threads> <per thread>\n", argv[0]); return 2; }
  return 0;
}
