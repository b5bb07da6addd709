// page_plan.h -- how the question page calls (hip_engine_page.cpp) count a quiz's branch rows, hold them to their limits and group a
// call's quizzes into chunks: plain host logic without a device, so the suite drives it (tests/page_plan_check.cpp).
#pragma once
#include <cstdint>
#include <vector>

namespace pqa {

// A quiz whose set holds j questions has K^j branch rows: one per combination of their answers.  The rows of ONE step of a chunk go
// through one chunk of the gain sweep (LaunchQuestionGains: kTopBatchQuizzes rows), and they live in engine scratch.
constexpr int64_t kPageMaxBranches = 256;
constexpr int64_t kPageScratchBytes = (int64_t)64 << 20;

// K^exponent, or kPageMaxBranches + 1 for everything above kPageMaxBranches (K >= 2, exponent >= 0: no overflow at any exponent)
inline int64_t PageBranches(int64_t K, int64_t exponent) {
  int64_t b = 1;
  for (int64_t i = 0; i < exponent; i++) {
    b *= K;
    if (b > kPageMaxBranches) return kPageMaxBranches + 1;
  }
  return b;
}

// The set's length at the largest step of a call: Eval sweeps the given set's branches; a page's last step sweeps the branches of the
// given set and the pageSize - 1 questions taken before it (a page of 0 launches nothing and is held to the given set alone).
inline int64_t PageDeepestSet(int64_t nGiven, int64_t pageSize, bool page) { return page && pageSize > 1 ? nGiven + (pageSize - 1) : nGiven; }
inline int64_t PageLargestBranches(int64_t K, int64_t nGiven, int64_t pageSize, bool page) {
  if (nGiven > 64 || (page && pageSize > 64)) return kPageMaxBranches + 1;   // (2^9 is too many already; and the sum below cannot wrap)
  return PageBranches(K, PageDeepestSet(nGiven, pageSize, page));
}

// rowDoubles: the doubles of a branch row
inline bool PageFits(int64_t branches, int64_t rowDoubles) {
  return branches >= 1 && branches <= kPageMaxBranches && branches * rowDoubles * (int64_t)sizeof(double) <= kPageScratchBytes;
}

// Chunks of whole quizzes in call order: quizzes [start[c], start[c + 1]).  largest[i]: quiz i's branch rows at its largest step (it
// fits by itself).  A chunk takes the next quiz as long as the chunk's rows stay within both limits, so a quiz is never split and
// every chunk holds at least one.
struct PageChunks {
  std::vector<int64_t> start;   // nChunks + 1
  int64_t Chunks() const { return (int64_t)start.size() - 1; }
};
inline PageChunks PlanPageChunks(int64_t nQuizzes, const int64_t *largest, int64_t rowDoubles) {
  PageChunks plan;
  plan.start.push_back(0);
  int64_t rows = 0;
  for (int64_t i = 0; i < nQuizzes; i++) {
    if (rows > 0 && !PageFits(rows + largest[i], rowDoubles)) {
      plan.start.push_back(i);
      rows = 0;
    }
    rows += largest[i];
  }
  if (nQuizzes > 0) plan.start.push_back(nQuizzes);
  return plan;
}

}  // namespace pqa
