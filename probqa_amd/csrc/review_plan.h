// review_plan.h -- how ReviewAnswersBatch (hip_engine_review.cpp) cuts a call's (quiz, position) pairs into chunks: plain host logic
// without a device, so the suite drives it (PqaHip_HostLogicProbe "review_plan").
#pragma once
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace pqa {

// The scratch a chunk takes: 16 bytes per element of a row (mantissas and exponent sums), and per distinct quiz whose ratios do not stay
// in LDS (more than ldsAnswers answers) nAnswers x ldT doubles.
inline int64_t ReviewRowBytes(int64_t ldT) { return 16 * ldT; }
inline int64_t ReviewSpillBytes(int64_t nAnswers, int64_t ldT, int64_t ldsAnswers) { return nAnswers > ldsAnswers ? 8 * nAnswers * ldT : 0; }

// Chunks of pair indices.  The pairs of one quiz form a group, in call order; the groups follow each other in the order their quizzes
// first appear, so every pair is placed exactly once.  A group goes into the open chunk whole where it fits under the row cap and the
// byte budget; where it does not, the chunk is closed, and a group that an empty chunk cannot hold is split -- a chunk takes at least
// one row, whatever the budget says.
inline std::vector<std::vector<int64_t>> PlanReviewChunks(int64_t nPairs, const int64_t *quizOf, const int64_t *answersOf, int64_t ldT, int64_t rowCap,
                                                          int64_t budgetBytes, int64_t ldsAnswers) {
  std::vector<std::vector<int64_t>> groups;
  std::unordered_map<int64_t, size_t> groupOf;
  for (int64_t i = 0; i < nPairs; i++) {
    const auto it = groupOf.emplace(quizOf[i], groups.size());
    if (it.second) groups.emplace_back();
    groups[it.first->second].push_back(i);
  }
  std::vector<std::vector<int64_t>> chunks;
  std::vector<int64_t> open;
  int64_t openBytes = 0;
  const int64_t rowBytes = ReviewRowBytes(ldT);
  auto close = [&]() {
    if (!open.empty()) chunks.push_back(std::move(open));
    open.clear();
    openBytes = 0;
  };
  for (const std::vector<int64_t> &g : groups) {
    const int64_t spill = ReviewSpillBytes(answersOf[g[0]], ldT, ldsAnswers);
    size_t at = 0;
    while (at < g.size()) {
      const int64_t left = (int64_t)(g.size() - at);
      const int64_t byRows = rowCap - (int64_t)open.size();
      const int64_t byBytes = budgetBytes - openBytes - spill >= rowBytes ? (budgetBytes - openBytes - spill) / rowBytes : 0;
      int64_t fit = std::min(byRows, byBytes);
      if (fit < left && !open.empty()) { close(); continue; }   // (kept together: the group starts a chunk of its own)
      fit = std::max<int64_t>(1, std::min(fit, left));
      open.insert(open.end(), g.begin() + (std::ptrdiff_t)at, g.begin() + (std::ptrdiff_t)(at + (size_t)fit));
      openBytes += spill + fit * rowBytes;
      at += (size_t)fit;
      if (at < g.size()) close();   // (split: the rest of the group opens the next chunk)
    }
  }
  close();
  return chunks;
}

}  // namespace pqa
