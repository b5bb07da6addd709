// The tile grouping of RankTargetsBatch (probqa_amd/csrc/status_plan.h: PlanRankTiles) as a program of its own, for a build under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_host_status_plan.py): seeded calls, every plan checked against the rule --
// one quiz per tile, call order, the cap, every pair exactly once, a quiz's tiles full but its last -- and the results scattered back the
// way the engine scatters them.
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "../probqa_amd/csrc/status_plan.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
  state ^= state << 13; state ^= state >> 7; state ^= state << 17;
  return state;
}

static bool check(const std::vector<int64_t> &quizzes, int64_t cap) {
  const int64_t n = (int64_t)quizzes.size();
  const pqa::RankTiles plan = pqa::PlanRankTiles(n, quizzes.data(), cap);
  if (plan.start.empty() || plan.start.front() != 0 || plan.start.back() != n || (int64_t)plan.order.size() != n) return false;
  std::vector<int> seen((size_t)n, 0);
  std::map<int64_t, int64_t> lastOf, openSize;   // per quiz: its last pair placed so far, the size of its newest tile
  for (int64_t i = 0; i < plan.Tiles(); i++) {
    const int64_t a = plan.start[(size_t)i], b = plan.start[(size_t)i + 1];
    if (a >= b || b - a > cap) return false;
    const int64_t quiz = quizzes[(size_t)plan.order[(size_t)a]];
    if (openSize.count(quiz) && openSize[quiz] != cap) return false;   // an earlier tile of the quiz was left short
    for (int64_t k = a; k < b; k++) {
      const int64_t pair = plan.order[(size_t)k];
      if (pair < 0 || pair >= n || seen[(size_t)pair]++ || quizzes[(size_t)pair] != quiz) return false;
      if (lastOf.count(quiz) && lastOf[quiz] >= pair) return false;    // call order within the quiz
      lastOf[quiz] = pair;
    }
    openSize[quiz] = b - a;
  }
  // the engine's scatter: a result per position of `order` goes back to its pair
  std::vector<int64_t> out((size_t)n, -1);
  for (int64_t k = 0; k < n; k++) out[(size_t)plan.order[(size_t)k]] = quizzes[(size_t)plan.order[(size_t)k]];
  for (int64_t i = 0; i < n; i++)
    if (out[(size_t)i] != quizzes[(size_t)i]) return false;
  return true;
}

int main() {
  int64_t calls = 0;
  const std::vector<std::vector<int64_t>> named = {{}, {5}, std::vector<int64_t>(32, 5), std::vector<int64_t>(33, 5), std::vector<int64_t>(70, 5),
                                                   {1, 2, 1, 2, 1}, {3, 1, 3, 3}, {INT64_MAX, INT64_MIN, INT64_MAX}};
  for (const auto &q : named) {
    if (!check(q, 32) || !check(q, 1) || !check(q, 2)) { std::printf("named case %lld failed\n", (long long)calls); return 1; }
    calls++;
  }
  for (int round = 0; round < 2000; round++) {
    std::vector<int64_t> quizzes((size_t)(next() % 400));
    const int64_t nQuizzes = 1 + (int64_t)(next() % 12);
    for (auto &q : quizzes) q = (int64_t)(next() % (uint64_t)nQuizzes);
    const int64_t cap = round % 2 ? 32 : 1 + (int64_t)(next() % 40);
    if (!check(quizzes, cap)) { std::printf("round %d failed\n", round); return 1; }
    calls++;
  }
  std::printf("ok %lld\n", (long long)calls);
  return 0;
}
