// hip_engine_internal.h -- small helpers shared by the files that implement HipEngine (hip_engine.cpp: construction, options,
// registry; hip_engine_select.cpp: the selection paths; hip_engine_combine.cpp: concurrent clients; hip_engine_update.cpp:
// posterior updates, listings, training; hip_engine_shard.cpp: what a sharded engine asks of its shards; hip_engine_kb.cpp: id maps, .kb files, maintenance).
#pragma once

#include <sched.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <sstream>

#include "combining.h"   // FutexWait, PublishState, PostingLock, Combiner
#include "hip_engine.h"

namespace pqa {
namespace {

inline Error HipErr(hipError_t e, const char *what) {
  std::string msg = std::string("HIP failure in ") + what + ": " + hipGetErrorString(e);
  DefaultLogger::Log(DefaultLogger::Severity::Error, msg);
  return Error::MakeP(ErrCode::Internal, std::string("Internal error at hip_engine.cpp(") + what + ")", msg);
}
#define HIP_TRY(expr)                                   \
  do {                                                  \
    const hipError_t e_ = (expr);                       \
    if (e_ != hipSuccess) return HipErr(e_, #expr);     \
  } while (0)

inline std::string RangeParams(int64_t subj, int64_t lo, int64_t hi) {  // IndexOutOfRangeErrorParams::ToString
  return "subjIndex=" + std::to_string(subj) + " not in " + std::to_string(lo) + "..." + std::to_string(hi);
}

inline bool BitTest(const std::vector<uint32_t> &bits, int64_t i) { return (bits[i >> 5] >> (i & 31)) & 1u; }
inline void BitSet(std::vector<uint32_t> &bits, int64_t i, bool v) {
  if (v) bits[i >> 5] |= 1u << (i & 31); else bits[i >> 5] &= ~(1u << (i & 31));
}
inline size_t BitWords(int64_t nBits) { return (size_t)((nBits + 63) / 64) * 2 + 2; }  // whole 64-bit packs + slack
inline uint64_t Pack64(const std::vector<uint32_t> &bits, int64_t iPack) {
  return (uint64_t)bits[2 * iPack] | ((uint64_t)bits[2 * iPack + 1] << 32);
}

// An id table of Compact as the C ABI hands it out: the caller frees it (never of size zero)
inline int64_t *MallocCopy(const std::vector<int64_t> &v) {
  int64_t *p = (int64_t *)std::malloc(sizeof(int64_t) * std::max<size_t>(v.size(), 1));
  std::copy(v.begin(), v.end(), p);
  return p;
}

// A wait for a word the GPU writes: a pure spin while the answer is a kernel's time away (the first ~50 us), then the core is
// offered to whoever else wants it between looks (sched_yield) -- a process whose clients outnumber its CPUs otherwise burns its
// allowance on waiting -- and the clock is read only every so often.  Tick() returns false once `limit` has passed.
struct SpinWait {
  uint64_t spins = 0;
  bool yielding = false;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  // (by TIME, not by count: a pause is 15 - 40 ns on the hosts met so far, and a count that ran out just before a 20 us step's answer
  //  put a system call -- a microsecond -- into every selection)
  bool Tick(std::chrono::seconds limit) {
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


}  // namespace
}  // namespace pqa
