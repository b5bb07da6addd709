// hip_engine_internal.h -- small helpers shared by the files that implement HipEngine (hip_engine.cpp: construction, options,
// registry; hip_engine_select.cpp: the selection paths; hip_engine_combine.cpp: concurrent clients; hip_engine_update.cpp:
// posterior updates, listings, training; hip_engine_shard.cpp: what a sharded engine asks of its shards; hip_engine_kb.cpp: id maps, .kb files, maintenance;
// hip_engine_resume.cpp, hip_engine_parts.cpp, hip_engine_record_parts.cpp: row packages, selection parts and posterior packages of
// shards that separate processes drive; hip_engine_train.cpp: many trainings in one call; hip_engine_server.cpp: the resident sweep;
// hip_engine_list.cpp: ListTopQuestions; hip_engine_among.cpp, hip_engine_top_among.cpp: the Among calls and the listing within listed
// sets; hip_engine_sources.cpp: the source queries, target similarity, question redundancy and target separation; hip_engine_gain.cpp:
// the information gain of every question of a quiz; hip_engine_page.cpp: conditional gains and question pages).
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

// An id table of Compact as the C ABI hands it out: the caller frees it (never of size zero)
inline int64_t *MallocCopy(const std::vector<int64_t> &v) {
  int64_t *p = (int64_t *)std::malloc(sizeof(int64_t) * std::max<size_t>(v.size(), 1));
  std::copy(v.begin(), v.end(), p);
  return p;
}

}  // namespace
}  // namespace pqa
