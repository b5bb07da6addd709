// selection_host.h -- what a selection does on the host once the sweep has answered, in ONE place for every path: the codes of an
// answer, the wait for a priority vector the sweep hands over (TakePriorities), the reference's sampled selector, the nearest free
// question and the finish over a snapshot of the unavailable questions.
// Plain C++ without HIP: included by both engines and checked without a GPU (tests/selection_host_check.cpp).
#pragma once
#include <immintrin.h>
#include <sched.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

namespace pqa {

// What a sweep answers instead of a question (select_record.h packs them): nothing left, an incomplete sweep, redo with the fix of
// pole_kernels.hip.
constexpr int64_t kSelNone = -1, kSelIncomplete = -3, kSelRedo = -4;

// A wait for a word the GPU writes: a pure spin while the answer is a kernel's time away (the first ~50 us), then the core is
// offered to whoever else wants it between looks (sched_yield) -- a process whose clients outnumber its CPUs otherwise burns its
// allowance on waiting -- and the clock is read only every so often.  Tick() returns false once `limit` has passed.
struct SpinWait {
  uint64_t spins = 0;
  bool yielding = false;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  // (by TIME, not by count: a pause is 15 - 40 ns on the hosts met so far, and a count that ran out just before a 20 us step's answer
  //  put a system call -- a microsecond -- into every selection)
  bool Tick(std::chrono::nanoseconds limit) {
    ++spins;
    if (!yielding) {
      _mm_pause();
      if ((spins & 63) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) yielding = true;
      return true;
    }
    if ((spins & 0xFF) == 0 && std::chrono::steady_clock::now() - t0 > limit) return false;
    sched_yield();
    return true;
  }
  bool Due() const { return (spins & 0xFFF) == 0; }   // (for the occasional look at something else while waiting)
};

// A quiz's priority vector where a sweep delivered it: local question k at pri[k * stride].  tag != 0: the entries are {priority,
// launch tag} records (TaggedPriority, stride 2) and one is taken once the word behind it carries the tag.
struct PriorityView { const double *pri = nullptr; int64_t stride = 0; uint64_t tag = 0; };

// run[k] = 0 for skipped(k), else entry k of the view.  A flag or an event has said that every workgroup has reported, not that
// every one of its stores has landed: a tagged entry is waited for until it carries the tag (it almost always does by then) and
// read behind that load-acquire.  False: `timeout` has passed -- the error's code and text are the caller's.
template <class Skip>
bool TakePriorities(const PriorityView &v, int64_t n, const Skip &skipped, double *run, std::chrono::nanoseconds timeout) {
  SpinWait w;
  for (int64_t k = 0; k < n; k++) {
    if (skipped(k)) { run[k] = 0.0; continue; }
    const double *rec = v.pri + k * v.stride;
    if (v.tag != 0) {
      const uint64_t *tagWord = reinterpret_cast<const uint64_t *>(rec + 1);
      while (__atomic_load_n(tagWord, __ATOMIC_ACQUIRE) != v.tag)
        if (!w.Tick(timeout)) return false;
    }
    run[k] = *rec;   // (a plain read: behind the tag's load-acquire, or behind the caller's event / flag)
  }
  return true;
}

// BaseEngine::FindNearestQuestion, reference PqaCore/BaseEngine.cpp:60-124: the available question "nearest" to iMiddle as the
// reference finds it -- exact within iMiddle's own 64-bit pack, then pack by pack outwards, comparing only the two packs at the
// same pack distance.  avail(p): bit i set = question 64 p + i is neither asked nor a gap (bits past nQuestions clear).
template <class Avail>
int64_t FindNearestInPacks(int64_t iMiddle, int64_t nQuestions, const Avail &avail) {
  const uint32_t dInf = 200;
  const int64_t iPack64 = iMiddle >> 6;
  const uint32_t iWithin = (uint32_t)(iMiddle & 63);
  const uint64_t available = avail(iPack64);
  if (available != 0) {
    const uint64_t baseMask = (1ULL << iWithin) - 1;
    const uint64_t higher = available & ~baseMask, lower = baseMask & available;
    const uint32_t dHigher = higher ? ((uint32_t)__builtin_ctzll(higher) - iWithin) : dInf;
    const uint32_t dLower = lower ? (iWithin - (uint32_t)(63 - __builtin_clzll(lower))) : dInf;
    return (dHigher < dLower) ? iMiddle + dHigher : iMiddle - dLower;
  }
  const int64_t limPack64 = (nQuestions + 63) >> 6;
  int64_t i = 1;
  while ((iPack64 >= i) && (iPack64 + i < limPack64)) {
    const uint64_t availLeft = avail(iPack64 - i), availRight = avail(iPack64 + i);
    if ((availLeft | availRight) == 0) { i++; continue; }
    const uint32_t dHigher = availRight ? ((uint32_t)__builtin_ctzll(availRight) + 64 - iWithin) : dInf;
    const uint32_t dLower = availLeft ? (iWithin + 64 - (uint32_t)(63 - __builtin_clzll(availLeft))) : dInf;
    if (dHigher < dLower) return iMiddle + dHigher + ((i - 1) << 6);
    return iMiddle - dLower - ((i - 1) << 6);
  }
  while (iPack64 >= i) {
    const uint64_t availLeft = avail(iPack64 - i);
    if (!availLeft) { i++; continue; }
    return iMiddle - (iWithin + 64 - (uint32_t)(63 - __builtin_clzll(availLeft))) - ((i - 1) << 6);
  }
  while (iPack64 + i < limPack64) {
    const uint64_t availRight = avail(iPack64 + i);
    if (!availRight) { i++; continue; }
    return iMiddle + ((uint32_t)__builtin_ctzll(availRight) + 64 - iWithin) + ((i - 1) << 6);
  }
  return -1;
}

// The finish of a selection over 32-bit words (reference PqaCore/CpuEngine.cpp:403-407): a question is unavailable -- asked or a
// gap -- if its bit is set in `a` or in `b` (`b` may be null); whole 64-bit packs of words, the bits past nQuestions set.  A pick
// that is available stays, one that is not falls to the nearest free question; -1: nothing left.
inline int64_t FinishOverSnapshot(int64_t pick, int64_t nQuestions, const uint32_t *a, const uint32_t *b = nullptr) {
  auto word = [a, b](int64_t w) { return b ? a[w] | b[w] : a[w]; };
  if (pick < 0 || ((word(pick >> 5) >> (pick & 31)) & 1u) == 0) return pick < 0 ? -1 : pick;
  return FindNearestInPacks(pick, nQuestions, [&](int64_t p) { return ~((uint64_t)word(2 * p) | ((uint64_t)word(2 * p + 1) << 32)); });
}

// The reference reports numeric anomalies of a sweep in its log -- non-finite grand totals of the priorities (CpuEngine.cpp:370-373),
// a non-positive grand total (:375-377), a priority that is not a positive finite number (CEEvalQsSubtaskConsider.cpp:209-211) --
// and goes on.  So does this engine, for what reaches the host: the selected question's priority, the totals of the sampled
// selector.  (NaN never wins an argmax here, so a NaN winner means that every available question's priority is NaN.)
// LogAnomaly is whoever includes this header's: the engine writes its log, rate-limited (hip_engine_select.cpp).
void LogAnomaly(bool isError, const char *what, double value);
inline void CheckPriority(double priority, int64_t index) {   // CEEvalQsSubtaskConsider.cpp:209-211, for the question that was selected
  if (index >= 0 && !(priority > 0 && std::isfinite(priority))) LogAnomaly(false, "Got priority=", priority);
}

// The reference's selector (PqaCore/CpuEngine.cpp:362-400) on the host, over a priority vector the sweep has delivered: the same
// per-subtask Kahan run lengths (CEEvalQsSubtaskConsider.cpp:52-58, :212-214), Kahan grand totals and two upper_bounds as
// select_sampled_wg_impl (pqa_device.h) -- operation for operation, so with the same priorities, subtask count and random number it
// picks the same question.  run: priorities in, run lengths out.  Returns the pick before the gap / asked fallback (:403-407).
// (a template: the test of a question is inlined instead of a call through std::function per question, 1000 of them per selection)
template <class Skip>
int64_t SelectSampledHost(double *run, int64_t n, int64_t nWorkers, uint64_t rnd, const Skip &skipped) {
  struct Kahan {                 // SRAccumulator<SRDoubleNumber> (SRPlatform/Interface/SRAccumulator.h:15-39)
    double sum = 0, corr = 0;
    void add(double v) { const double y = v - corr; const double t = sum + y; corr = (t - sum) - y; sum = t; }
    double get() const { return sum - corr; }
  };
  const int64_t quot = n / nWorkers, rem = n % nWorkers, nSubtasks = quot == 0 ? rem : nWorkers;   // SRPoolRunner::CalcSplit
  auto bound = [&](int64_t i) { return (i + 1) * quot + std::min<int64_t>(i + 1, rem); };           // end of subtask i
  std::vector<double> grand((size_t)nSubtasks);
  for (int64_t s = 0; s < nSubtasks; s++) {
    Kahan acc;
    for (int64_t i = s == 0 ? 0 : bound(s - 1); i < bound(s); i++) {
      if (!skipped(i)) acc.add(run[i]);   // gap / asked questions only copy the running sum
      run[i] = acc.get();
    }
    grand[(size_t)s] = acc.get();
  }
  Kahan tot;                                                     // CpuEngine.cpp:362-368
  for (int64_t s = 0; s < nSubtasks; s++) {
    tot.add(grand[(size_t)s]);
    grand[(size_t)s] = tot.get();
    if (!std::isfinite(grand[(size_t)s]))                          // :370-373
      LogAnomaly(true, "Overflow or underflow has happened in the question evaluation subtasks: ", grand[(size_t)s]);
  }
  const double totG = grand[(size_t)nSubtasks - 1];
  if (totG <= 0) LogAnomaly(false, "Grand-grand total is ", totG);   // :375-377
  const double selRunLen = totG * (double)rnd / 18446744073709551615.0;   // :379, SRDoubleNumber::MakeRandom
  const int64_t iWorker = std::upper_bound(grand.begin(), grand.end(), selRunLen) - grand.begin();   // :380-381
  if (iWorker >= nSubtasks) return n - 1;                         // :384
  const double inWorker = selRunLen - (iWorker == 0 ? 0.0 : grand[(size_t)iWorker - 1]);   // :388
  const int64_t first = iWorker == 0 ? 0 : bound(iWorker - 1), limit = bound(iWorker);
  int64_t sel = std::upper_bound(run + first, run + limit, inWorker) - run;   // :391
  if (sel >= limit) sel = limit - 1;                              // :392-400
  return sel;
}
// (the same over bit words -- a question is skipped if its bit is set in either array; `b` may be null)
inline int64_t SelectSampledHostBits(double *run, int64_t n, int64_t nWorkers, uint64_t rnd, const uint32_t *a, const uint32_t *b) {
  if (b == nullptr) return SelectSampledHost(run, n, nWorkers, rnd, [a](int64_t i) { return ((a[i >> 5] >> (i & 31)) & 1u) != 0; });
  return SelectSampledHost(run, n, nWorkers, rnd, [a, b](int64_t i) { return (((a[i >> 5] | b[i >> 5]) >> (i & 31)) & 1u) != 0; });
}

}  // namespace pqa
