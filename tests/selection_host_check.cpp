// Stand-alone check of probqa_amd/csrc/selection_host.h -- what a selection does on the host after the sweep -- without a GPU.
// Parts (argv[1]); every part ends with a line "ok <part>", a failed check prints to stderr and exits 1:
//   nearest   FindNearestInPacks for every middle over random, all-set and all-clear masks.  Lines "N Q maskhex pick_0 .. pick_Q-1"
//             (maskhex: the unavailable questions, question 0 = lowest bit) for tests/test_selection_host.py to compare.
//   selector  SelectSampledHost by closure, by one word array and by two: they must agree.  Lines "V Q set skiphex pri_0 .." (the
//             priorities as hex floats) and "S Q set nSub rnd pick".
//   handover  TakePriorities against a writer thread, the three layouts, skipped entries, the timeout.
//   finish    FinishOverSnapshot.
#include <atomic>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

#include "../probqa_amd/csrc/selection_host.h"

namespace pqa {
static int gAnomalies = 0;
void LogAnomaly(bool, const char *, double) { gAnomalies++; }   // (the engine writes its log; here they are counted)
}  // namespace pqa
using namespace pqa;

#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

static const int64_t kQs[] = {1, 2, 63, 64, 65, 130, 200};
static const uint64_t kRnds[] = {0, 1, 0x123456789ABCDEFull, 0x7FFFFFFFFFFFFFFFull, 0x8000000000000000ull, 0xC0FFEE0DDBA11ull,
                                 0xFEDCBA9876543210ull, 0xFFFFFFFFFFFFFFFFull};   // tests/test_gpu_publish.py: SAMPLED_RNDS

struct Rng {   // splitmix64
  uint64_t s;
  uint64_t Next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double Unit() { return (double)(Next() >> 11) / 9007199254740992.0; }
};

// unavailable questions as 32-bit words in whole 64-bit packs (+ slack), the bits past Q set -- as the engines keep them
struct Mask {
  int64_t Q;
  std::vector<uint32_t> w;
  explicit Mask(int64_t q) : Q(q), w((size_t)((q + 63) / 64) * 2 + 2, 0) { for (int64_t i = q; i < (int64_t)w.size() * 32; i++) Set(i); }
  void Set(int64_t i) { w[(size_t)(i >> 5)] |= 1u << (i & 31); }
  bool Test(int64_t i) const { return (w[(size_t)(i >> 5)] >> (i & 31)) & 1u; }
  uint64_t Pack(int64_t p) const { return (uint64_t)w[(size_t)(2 * p)] | ((uint64_t)w[(size_t)(2 * p + 1)] << 32); }
  std::string Hex() const {   // the first Q bits, most significant digit first
    std::string s;
    for (int64_t d = (Q + 3) / 4 - 1; d >= 0; d--) {
      int v = 0;
      for (int b = 0; b < 4; b++) if (4 * d + b < Q && Test(4 * d + b)) v |= 1 << b;
      s += "0123456789abcdef"[v];
    }
    return s;
  }
  static Mask Random(int64_t q, Rng &r, double density) {
    Mask m(q);
    for (int64_t i = 0; i < q; i++) if (r.Unit() < density) m.Set(i);
    return m;
  }
};

static void Nearest() {
  Rng r{1};
  const double densities[] = {0.3, 0.6, 0.9, 0.97, 0.995};
  for (int64_t Q : kQs) {
    std::vector<Mask> masks;
    masks.push_back(Mask(Q));                        // nothing asked
    masks.push_back(Mask::Random(Q, r, 2.0));        // nothing left
    for (int i = 0; i < 200; i++) masks.push_back(Mask::Random(Q, r, densities[i % 5]));
    for (const Mask &m : masks) {
      std::printf("N %" PRId64 " %s", Q, m.Hex().c_str());
      for (int64_t middle = 0; middle < Q; middle++) {
        const int64_t pick = FindNearestInPacks(middle, Q, [&](int64_t p) { return ~m.Pack(p); });
        CHECK(pick >= -1 && pick < Q && (pick < 0 || !m.Test(pick)));
        std::printf(" %" PRId64, pick);
      }
      std::printf("\n");
    }
  }
}

static void Selector() {
  Rng r{2};
  const double densities[] = {0.0, 0.3, 0.9, 2.0};
  for (int64_t Q : kQs)
    for (int set = 0; set < 4; set++) {
      const Mask skip = Mask::Random(Q, r, densities[set]);
      Mask a(Q), b(Q);                               // a | b == skip
      for (int64_t i = 0; i < Q; i++)
        if (skip.Test(i)) { const uint64_t w = r.Next() % 3; if (w != 1) a.Set(i); if (w != 0) b.Set(i); }
      std::vector<double> pri((size_t)Q);
      std::printf("V %" PRId64 " %d %s", Q, set, skip.Hex().c_str());
      for (double &p : pri) { p = std::ldexp(0.5 + r.Unit(), (int)(r.Next() % 40) - 20); std::printf(" %a", p); }
      std::printf("\n");
      const int64_t subs[] = {1, 3, 8, Q, Q + 5};
      for (int64_t nSub : subs)
        for (uint64_t rnd : kRnds) {
          std::vector<double> r1 = pri, r2 = pri, r3 = pri;
          const int64_t byClosure = SelectSampledHost(r1.data(), Q, nSub, rnd, [&](int64_t i) { return skip.Test(i); });
          const int64_t byWord = SelectSampledHostBits(r2.data(), Q, nSub, rnd, skip.w.data(), nullptr);
          const int64_t byWords = SelectSampledHostBits(r3.data(), Q, nSub, rnd, a.w.data(), b.w.data());
          CHECK(byClosure == byWord && byClosure == byWords && byClosure >= 0 && byClosure < Q);
          CHECK(std::memcmp(r1.data(), r2.data(), (size_t)Q * 8) == 0 && std::memcmp(r1.data(), r3.data(), (size_t)Q * 8) == 0);   // the run lengths too
          std::printf("S %" PRId64 " %d %" PRId64 " %" PRIu64 " %" PRId64 "\n", Q, set, nSub, rnd, byClosure);
        }
    }
  CHECK(gAnomalies > 0);   // (the sets with nothing left: "Grand-grand total is 0")
}

// One hand-over: n questions, entry k at buf[k * stride] (tagged: its tag in the word behind it).  The writer stores the entries of
// the questions that are not skipped in a scrambled order with small delays -- value first, tag behind it with release order, as
// the sweep's one 16-byte store makes them visible together; untagged layouts are read once the writer is done, as behind an event.
static void HandOver(int64_t n, int64_t stride, uint64_t tag, uint64_t seed) {
  Rng r{seed};
  const Mask skip = Mask::Random(n, r, 0.25);
  const double stale = -1234.5;
  std::vector<double> buf((size_t)(n * stride + 2), stale), want((size_t)n), run((size_t)n, -1.0);
  uint64_t *words = reinterpret_cast<uint64_t *>(buf.data());
  if (tag != 0) for (int64_t k = 0; k < n; k++) words[k * stride + 1] = tag - 1;   // the previous launch's
  std::vector<int64_t> order;
  for (int64_t k = 0; k < n; k++) { want[(size_t)k] = skip.Test(k) ? 0.0 : 1.0 + (double)k + r.Unit(); if (!skip.Test(k)) order.push_back(k); }
  for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[(size_t)(r.Next() % i)]);
  std::atomic<bool> done{false};
  std::thread writer([&] {
    for (size_t i = 0; i < order.size(); i++) {
      const int64_t k = order[i];
      __atomic_store(&buf[(size_t)(k * stride)], &want[(size_t)k], __ATOMIC_RELAXED);
      if (tag != 0) __atomic_store_n(&words[k * stride + 1], tag, __ATOMIC_RELEASE);
      if (i % 7 == 0) std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    done.store(true, std::memory_order_release);
  });
  if (tag == 0) while (!done.load(std::memory_order_acquire)) std::this_thread::yield();
  const bool ok = TakePriorities(PriorityView{buf.data(), stride, tag}, n, [&](int64_t k) { return skip.Test(k); }, run.data(), std::chrono::seconds(30));
  writer.join();
  CHECK(ok);
  for (int64_t k = 0; k < n; k++) CHECK(run[(size_t)k] == want[(size_t)k]);   // (skipped: 0, their entries were never written)
}

static void HandOverParts() {
  for (uint64_t seed = 1; seed <= 10; seed++)
    for (int64_t n : {1, 65, 200, 1000}) {
      HandOver(n, 1, 0, seed);                    // a quiz's own plain vector
      HandOver(n, 64, 0, seed);                   // a column of the quiz-minor matrix, Bp = 64
      HandOver(n, 2, 0x100000000ull + seed, seed);   // tagged records
    }
  // the last entry keeps the previous launch's tag: false, and not before the timeout
  const int64_t n = 100;
  const uint64_t tag = 77;
  std::vector<double> buf((size_t)(2 * n), 1.0), run((size_t)n);
  uint64_t *words = reinterpret_cast<uint64_t *>(buf.data());
  for (int64_t k = 0; k < n; k++) words[2 * k + 1] = k == n - 1 ? tag - 1 : tag;
  const auto timeout = std::chrono::milliseconds(300);
  const auto t0 = std::chrono::steady_clock::now();
  const bool ok = TakePriorities(PriorityView{buf.data(), 2, tag}, n, [](int64_t) { return false; }, run.data(), timeout);
  const auto took = std::chrono::steady_clock::now() - t0;
  CHECK(!ok && took >= timeout && took < std::chrono::seconds(5));
  // ... and the same vector with that question skipped is complete at once
  CHECK(TakePriorities(PriorityView{buf.data(), 2, tag}, n, [&](int64_t k) { return k == n - 1; }, run.data(), timeout) && run[(size_t)n - 1] == 0.0 && run[0] == 1.0);
}

static void Finish() {
  Rng r{3};
  for (int64_t Q : kQs) {
    const Mask none(Q), all = Mask::Random(Q, r, 2.0);
    for (int64_t pick = 0; pick < Q; pick++) {
      CHECK(FinishOverSnapshot(pick, Q, none.w.data()) == pick);         // available: as it is
      CHECK(FinishOverSnapshot(pick, Q, all.w.data()) == -1);            // nothing left
      CHECK(FinishOverSnapshot(pick, Q, none.w.data(), all.w.data()) == -1);
    }
    CHECK(FinishOverSnapshot(-1, Q, none.w.data()) == -1);               // the sweep itself found nothing
    for (int i = 0; i < 50; i++) {
      const Mask a = Mask::Random(Q, r, 0.5), b = Mask::Random(Q, r, i % 2 ? 0.9 : 0.2);
      Mask both(Q);
      for (int64_t k = 0; k < Q; k++) if (a.Test(k) || b.Test(k)) both.Set(k);
      for (int64_t pick = 0; pick < Q; pick++) {
        const int64_t want = both.Test(pick) ? FindNearestInPacks(pick, Q, [&](int64_t p) { return ~both.Pack(p); }) : pick;
        CHECK(FinishOverSnapshot(pick, Q, both.w.data()) == want && FinishOverSnapshot(pick, Q, a.w.data(), b.w.data()) == want);
        CHECK(want == -1 || !both.Test(want));
      }
    }
  }
  // by hand: questions 0..69, all but 3 and 68 unavailable; from 40 the reference looks in pack 0 only (40's own), from 66 in pack 1
  Mask m(70);
  for (int64_t k = 0; k < 70; k++) if (k != 3 && k != 68) m.Set(k);
  CHECK(FinishOverSnapshot(40, 70, m.w.data()) == 3 && FinishOverSnapshot(66, 70, m.w.data()) == 68 && FinishOverSnapshot(68, 70, m.w.data()) == 68);
}

int main(int argc, char **argv) {
  const std::string part = argc > 1 ? argv[1] : "";
  if (part == "nearest") Nearest();
  else if (part == "selector") Selector();
  else if (part == "handover") HandOverParts();
  else if (part == "finish") Finish();
  else { std::fprintf(stderr, "usage: %s nearest|selector|handover|finish\n", argv[0]); return 2; }
  std::printf("ok %s\n", part.c_str());
  return 0;
}
