// kb_plan.h -- the decisions both engines must take alike, over plain vectors and no engine state: which ids an AddQsTs call
// hands out, what a Compact moves where, whether a removal is valid, and which of several shards' winners is the selection.
// HipEngine (hip_engine_kb.cpp) then moves the data on its device, ShardedEngine (sharded_engine.cpp) rebuilds its shards; the
// C ABI's multi-process exchanges (c_abi.cpp) use the pick.  Host C++17 only -- no HIP -- like combining.h, so that the CPU
// suite drives it (tests/test_host_logic.py through PqaHip_HostLogicProbe).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/PqaCInterop.h"

namespace pqa {

// CpuEngine::AddQsTsSpec, reference PqaCore/CpuEngine.cpp:468-575: gaps are reused LIFO (:476-482 questions, :488-493 targets),
// the rest is appended (:500, :531); entry i of the caller's parameters belongs to id i of the plan.
// NOTE reference :516,:523,:529 index the target parameters with nQReuse + j; the evident intent nTReuse + j is used.
struct AddPlan {
  std::vector<int64_t> qIds, tIds;     // in the caller's order: the reused gaps first, then the appended ids
  std::vector<double> qInit, tInit;    // their init amounts
  int64_t nQReuse = 0, nTReuse = 0;    // how many leading ids are reused gaps (the last entries of the gap lists)
  int64_t newQ = 0, newT = 0;          // the dimensions afterwards
};
inline AddPlan PlanAdd(const std::vector<int64_t> &qGapList, const std::vector<int64_t> &tGapList, int64_t Q, int64_t T,
                       int64_t nQuestions, const CiAddQorTParam *pAqps, int64_t nTargets, const CiAddQorTParam *pAtps) {
  AddPlan p;
  auto axis = [](const std::vector<int64_t> &gaps, int64_t size, int64_t n, const CiAddQorTParam *params, std::vector<int64_t> &ids,
                 std::vector<double> &init, int64_t &nReuse, int64_t &newSize) {
    nReuse = std::min<int64_t>(n, (int64_t)gaps.size());
    newSize = size + (n - nReuse);
    for (int64_t i = 0; i < nReuse; i++) ids.push_back(gaps[gaps.size() - 1 - (size_t)i]);
    for (int64_t i = nReuse; i < n; i++) ids.push_back(size + (i - nReuse));
    for (int64_t i = 0; i < n; i++) init.push_back(params[i]._initAmount);
  };
  axis(qGapList, Q, nQuestions, pAqps, p.qIds, p.qInit, p.nQReuse, p.newQ);
  axis(tGapList, T, nTargets, pAtps, p.tIds, p.tInit, p.nTReuse, p.newT);
  return p;
}

// CpuEngine::CompactSpec, reference PqaCore/CpuEngine.cpp:577-658.  Questions: a gap in the kept prefix takes the LAST surviving
// question (:586-601).  Targets: gaps of the kept prefix (ascending) take the survivors of the dropped tail (ascending) -- the
// pairing the reference produces when no gap lies in the tail (:604-618); with tail gaps the reference's move table is
// under-filled, here the pairing simply continues.
struct CompactPlan {
  std::vector<int64_t> oldQ, oldT;                    // new id -> the old id whose data it keeps
  std::vector<std::pair<int64_t, int64_t>> qMoves;    // (dst, src) whole-question moves, in the order they must be made
};
inline CompactPlan PlanCompact(const std::vector<int64_t> &qGapList, const std::vector<int64_t> &tGapList, int64_t Q, int64_t T) {
  std::vector<char> qGap((size_t)Q, 0), tGap((size_t)T, 0);
  for (int64_t g : qGapList) qGap[(size_t)g] = 1;
  for (int64_t g : tGapList) tGap[(size_t)g] = 1;
  const int64_t nQ = Q - (int64_t)qGapList.size(), nT = T - (int64_t)tGapList.size();
  CompactPlan p;
  p.oldQ.resize((size_t)nQ);
  p.oldT.resize((size_t)nT);
  int64_t iFirst = 0, iLast = Q - 1;
  for (; iFirst <= iLast; iFirst++) {
    if (!qGap[(size_t)iFirst]) { p.oldQ[(size_t)iFirst] = iFirst; continue; }
    while (qGap[(size_t)iLast] && iLast > iFirst) iLast--;
    if (iFirst == iLast) break;
    p.oldQ[(size_t)iFirst] = iLast;
    p.qMoves.emplace_back(iFirst, iLast);
    iLast--;
  }
  int64_t src = nT;
  for (int64_t t = 0; t < nT; t++) {
    if (!tGap[(size_t)t]) { p.oldT[(size_t)t] = t; continue; }
    while (tGap[(size_t)src]) src++;
    p.oldT[(size_t)t] = src++;
  }
  return p;
}

// Compact on shards that separate processes drive (hip_engine_kb.cpp: CompactFromBlocks): the plan is PlanCompact over the GLOBAL
// axis; no question changes its shard's range by being kept, so a shard that held [qFirst, qFirst + nLocal) keeps the part of it below
// the new question count nQ -- possibly nothing, which refuses the compaction.  bounds: the shards' upper bounds, ascending.
inline int64_t ClippedQuestions(int64_t qFirst, int64_t nLocal, int64_t nQ) { return std::max<int64_t>(0, std::min(qFirst + nLocal, nQ) - qFirst); }
inline int64_t OwnerIn(const std::vector<int64_t> &bounds, int64_t q) {   // the shard whose range holds q; bounds.size() if none does
  return (int64_t)(std::upper_bound(bounds.begin(), bounds.end(), q) - bounds.begin());
}
struct ShardCompactPlan {
  bool refused = false;                    // a shard would be left without a question
  std::vector<int64_t> newBounds;          // every bound clipped to the new question count (also when refused)
  std::vector<int64_t> moves;              // per question move of the plan: dst, src, the shard that holds dst, the shard that holds src
};
inline ShardCompactPlan PlanShardCompact(const std::vector<int64_t> &bounds, const CompactPlan &plan) {
  ShardCompactPlan s;
  const int64_t nQ = (int64_t)plan.oldQ.size();
  for (size_t r = 0; r < bounds.size(); r++) {
    const int64_t first = r == 0 ? 0 : bounds[r - 1];
    const int64_t kept = ClippedQuestions(first, bounds[r] - first, nQ);
    s.refused = s.refused || kept == 0;
    s.newBounds.push_back(std::min(bounds[r], nQ));
  }
  for (const auto &mv : plan.qMoves) {
    s.moves.push_back(mv.first); s.moves.push_back(mv.second);
    s.moves.push_back(OwnerIn(bounds, mv.first)); s.moves.push_back(OwnerIn(bounds, mv.second));
  }
  return s;
}

// RemoveQuestions / RemoveTargets: every id is validated -- range, gaps, repeats within the call -- before the first one is
// removed.  The position of the first id that cannot be removed, -1 if the call is valid.
template <typename IsGap>
inline int64_t FirstBadRemoval(int64_t n, const int64_t *ids, int64_t limit, IsGap isGap) {
  std::vector<bool> seen((size_t)std::max<int64_t>(limit, 0), false);
  for (int64_t i = 0; i < n; i++) {
    const int64_t id = ids[i];
    if (id < 0 || id >= limit || isGap(id) || seen[(size_t)id]) return i;
    seen[(size_t)id] = true;
  }
  return -1;
}

// The winner among several shards' winners: maximum priority, lowest index on ties, a NaN counts as -infinity (it never beats
// a number), a negative index is no candidate.  True if {p, i} is to replace {bestP, bestI}.
inline bool BetterPick(double bestP, int64_t bestI, double p, int64_t i) {
  if (i < 0) return false;
  if (bestI < 0) return true;
  if (p != p) p = -HUGE_VAL;
  if (bestP != bestP) bestP = -HUGE_VAL;
  return p > bestP || (p == bestP && i < bestI);
}
struct BestPick {   // {0, -1} while nothing was offered that is a candidate
  double priority = 0;
  int64_t index = -1;
  void Offer(double p, int64_t i) {
    if (BetterPick(priority, index, p, i)) { priority = p != p ? -HUGE_VAL : p; index = i; }
  }
};

// The best maxCount of several shards' listings (ListTopQuestions) under the listings' own order: descending priority, ascending
// index among equal priorities.  A record whose priority is not > 0 (a NaN among them) or whose index is negative is no candidate.
// Every list is in that order already and the shards' indices are distinct; neither is relied upon.
struct RatedIndex { int64_t index; double priority; };   // == CiRatedQuestion
inline bool RatedBefore(const RatedIndex &a, const RatedIndex &b) { return a.priority > b.priority || (a.priority == b.priority && a.index < b.index); }
inline std::vector<RatedIndex> MergeTop(const std::vector<std::pair<const RatedIndex *, int64_t>> &lists, int64_t maxCount) {
  std::vector<RatedIndex> all;
  for (const auto &l : lists)
    for (int64_t i = 0; i < l.second; i++)
      if (l.first[i].priority > 0 && l.first[i].index >= 0) all.push_back(l.first[i]);
  const size_t n = (size_t)std::max<int64_t>(0, std::min<int64_t>(maxCount, (int64_t)all.size()));
  std::partial_sort(all.begin(), all.begin() + n, all.end(), RatedBefore);
  all.resize(n);
  return all;
}

// The host's prefix of a rated vector -- every listing of more than 256 records, in the device listings' order: of the n entries that
// are eligible(i) and whose value is > 0 (a NaN is not), the first `want` by value descending, idOf(i) ascending, as {id, value} records
// (Rec: CiRatedTarget, CiRatedQuestion or RatedIndex).  idx: the caller's scratch, reused from vector to vector.  Returns the count.
template <typename Rec, typename Eligible, typename IdOf>
inline int64_t RatedPrefix(const double *v, int64_t n, int64_t want, Eligible eligible, IdOf idOf, Rec *dest, std::vector<int64_t> &idx) {
  static_assert(sizeof(Rec) == sizeof(RatedIndex), "a record is {int64 id, double value}");
  idx.clear();
  for (int64_t i = 0; i < n; i++)
    if (eligible(i) && v[i] > 0.0) idx.push_back(i);
  const int64_t c = std::max<int64_t>(0, std::min<int64_t>(want, (int64_t)idx.size()));
  std::partial_sort(idx.begin(), idx.begin() + c, idx.end(), [&](int64_t a, int64_t b) { return v[a] > v[b] || (v[a] == v[b] && idOf(a) < idOf(b)); });
  for (int64_t k = 0; k < c; k++) {
    const RatedIndex r{idOf(idx[(size_t)k]), v[idx[(size_t)k]]};
    std::memcpy(dest + k, &r, sizeof(r));
  }
  return c;
}

// The tiles of the separation sweep (separation_kernels.hip) over the groups of a launch, counts[g] entries each: a tile is a run of
// whole groups -- a group is never split -- with at most maxEntries entries and at most maxGroups groups, filled in order; a group
// longer than maxEntries (the callers admit none) gets a tile of its own.  -> the first group of every tile and nGroups behind them:
// nTiles + 1 words, {0} for no groups.
inline std::vector<int64_t> PlanGroupTiles(int64_t nGroups, const int64_t *counts, int64_t maxEntries, int64_t maxGroups) {
  std::vector<int64_t> tileGroup{0};
  int64_t entries = 0;
  for (int64_t g = 0; g < nGroups; g++) {
    const int64_t first = tileGroup.back();
    if (g > first && (entries + counts[g] > maxEntries || g - first >= maxGroups)) {
      tileGroup.push_back(g);
      entries = 0;
    }
    entries += counts[g];
  }
  if (nGroups > 0) tileGroup.push_back(nGroups);
  return tileGroup;
}

// Where the arrays of a .kb file lie (layout: hip_engine_kb.cpp), in bytes from the file's start, and where the rows of a window of
// questions [qFirst, qFirst + nLocal) lie within them: a shard seeks to its two blocks instead of reading through the others'.
//   header 40 | sA [Q][K][T] | mD [Q][T] | vB [T] | trailer
// `elem`: bytes of the file's number type (4 or 8).  Every product is checked: dimensions a damaged header may claim do not wrap.
struct KbLayout {
  static constexpr int64_t kHeaderBytes = 40;
  int64_t K = 0, Q = 0, T = 0, elem = 0;
  int64_t rowBytes = 0, saBytes = 0, mdBytes = 0, vbOff = 0, trailerOff = 0;   // (the sizes of the whole blocks)
  bool valid = false;
  static bool Mul(int64_t a, int64_t b, int64_t &out) { return !__builtin_mul_overflow(a, b, &out); }
  static bool Add(int64_t a, int64_t b, int64_t &out) { return !__builtin_add_overflow(a, b, &out); }
  KbLayout() {}
  KbLayout(int64_t nAnswers, int64_t nQuestions, int64_t nTargets, int64_t elemBytes) : K(nAnswers), Q(nQuestions), T(nTargets), elem(elemBytes) {
    if (K < 1 || Q < 1 || T < 1 || (elem != 4 && elem != 8)) return;
    int64_t qk = 0, end = 0;
    valid = Mul(T, elem, rowBytes) && Mul(Q, K, qk) && Mul(qk, rowBytes, saBytes) && Mul(Q, rowBytes, mdBytes) &&
            Add(kHeaderBytes, saBytes, end) && Add(end, mdBytes, vbOff) && Add(vbOff, rowBytes, trailerOff);
  }
  bool HasWindow(int64_t qFirst, int64_t nLocal) const { return valid && qFirst >= 0 && nLocal >= 1 && qFirst <= Q && nLocal <= Q - qFirst; }
  int64_t SaOffset(int64_t qFirst) const { return kHeaderBytes + qFirst * K * rowBytes; }          // the K rows of question qFirst, then the next question's
  int64_t MdOffset(int64_t qFirst) const { return kHeaderBytes + saBytes + qFirst * rowBytes; }    // one row per question
  int64_t ArraysEnd() const { return trailerOff; }                                                 // a file shorter than this is cut inside its arrays
};

}  // namespace pqa
