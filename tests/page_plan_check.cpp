// The branch counts, limits and chunking of the question page calls (probqa_amd/csrc/page_plan.h) as a program of its own, for a build
// under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_host_page_plan.py).  Without arguments: named edges and seeded calls,
// every plan checked against the rule -- whole quizzes in call order, every chunk within both limits, no chunk that could have taken its
// successor's first quiz.  With arguments it answers one question on stdout, for the test to hold against its own restatement:
//   branches K nGiven pageSize page      -> the largest branch count (257: too many)
//   fits branches rowDoubles             -> 0 | 1
//   chunks rowDoubles n_1 n_2 ...        -> the chunks' first quizzes and the end
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../probqa_amd/csrc/page_plan.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
  state ^= state << 13; state ^= state >> 7; state ^= state << 17;
  return state;
}

static bool check(const std::vector<int64_t> &largest, int64_t rowDoubles) {
  const int64_t n = (int64_t)largest.size();
  const pqa::PageChunks plan = pqa::PlanPageChunks(n, largest.data(), rowDoubles);
  if (plan.start.empty() || plan.start.front() != 0) return false;
  if (n == 0) return plan.Chunks() == 0;
  if (plan.start.back() != n) return false;
  for (int64_t c = 0; c < plan.Chunks(); c++) {
    const int64_t a = plan.start[(size_t)c], b = plan.start[(size_t)c + 1];
    if (a >= b) return false;
    int64_t rows = 0;
    for (int64_t i = a; i < b; i++) rows += largest[(size_t)i];
    if (!pqa::PageFits(rows, rowDoubles)) return false;                                       // within both limits
    if (b < n && pqa::PageFits(rows + largest[(size_t)b], rowDoubles)) return false;         // and closed only because the next quiz did not fit
  }
  return true;
}

static int64_t power(int64_t K, int64_t e) {
  int64_t b = 1;
  for (int64_t i = 0; i < e && b <= 256; i++) b *= K;
  return b > 256 ? 257 : b;
}

int main(int argc, char **argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "branches") && argc == 6) {
    std::printf("%lld\n", (long long)pqa::PageLargestBranches(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), std::atoll(argv[5]) != 0));
    return 0;
  }
  if (argc >= 2 && !std::strcmp(argv[1], "fits") && argc == 4) {
    std::printf("%d\n", pqa::PageFits(std::atoll(argv[2]), std::atoll(argv[3])) ? 1 : 0);
    return 0;
  }
  if (argc >= 3 && !std::strcmp(argv[1], "chunks")) {
    std::vector<int64_t> largest;
    for (int i = 3; i < argc; i++) largest.push_back(std::atoll(argv[i]));
    const pqa::PageChunks plan = pqa::PlanPageChunks((int64_t)largest.size(), largest.data(), std::atoll(argv[2]));
    for (int64_t s : plan.start) std::printf("%lld ", (long long)s);
    std::printf("\n");
    return 0;
  }
  if (argc != 1) return 2;
  int64_t calls = 0;
  // branch counts: K^|S| for Eval, K^(|S| + pageSize - 1) for a page, a page of 0 held to the set alone, 257 for everything beyond 256
  for (int64_t K = 2; K <= 7; K++)
    for (int64_t given = 0; given <= 10; given++) {
      if (pqa::PageLargestBranches(K, given, 0, false) != power(K, given)) { std::printf("eval K=%lld given=%lld\n", (long long)K, (long long)given); return 1; }
      for (int64_t page = 0; page <= 10; page++) {
        const int64_t want = power(K, given + (page > 1 ? page - 1 : 0));
        if (pqa::PageLargestBranches(K, given, page, true) != want) { std::printf("page K=%lld given=%lld page=%lld\n", (long long)K, (long long)given, (long long)page); return 1; }
        calls++;
      }
    }
  if (pqa::PageLargestBranches(2, 8, 1, true) != 256 || pqa::PageLargestBranches(2, 8, 2, true) != 257 || pqa::PageLargestBranches(2, 0, 9, true) != 256 ||
      pqa::PageLargestBranches(2, 0, 10, true) != 257 || pqa::PageLargestBranches(4, 4, 0, false) != 256 || pqa::PageLargestBranches(16, 2, 1, true) != 256 ||
      pqa::PageLargestBranches(2, INT64_MAX, INT64_MAX, true) != 257 || pqa::PageLargestBranches(2, 0, INT64_MAX, true) != 257 ||
      pqa::PageLargestBranches(300, 1, 0, false) != 257 || pqa::PageLargestBranches(300, 0, 1, true) != 1) {
    std::printf("a branch count at an edge\n");
    return 1;
  }
  // the limits at their edges: 256 rows, 64 MiB
  if (!pqa::PageFits(256, 16) || pqa::PageFits(257, 16) || pqa::PageFits(0, 16) || !pqa::PageFits(256, 32768) || pqa::PageFits(256, 32769) ||
      !pqa::PageFits(1, 8388608) || pqa::PageFits(1, 8388609) || !pqa::PageFits(125, 67108) || pqa::PageFits(125, 67109)) {
    std::printf("a limit at its edge\n");
    return 1;
  }
  const std::vector<std::vector<int64_t>> named = {{}, {1}, {256}, {256, 256}, {125, 125, 125}, {128, 128, 1}, std::vector<int64_t>(600, 1), {1, 256, 1}, {255, 1, 1}};
  for (const auto &q : named) {
    if (!check(q, 16) || !check(q, 32768))   // (256 rows of 32768 doubles: the scratch limit exactly)
      { std::printf("named case %lld failed\n", (long long)calls); return 1; }
    calls++;
  }
  for (int round = 0; round < 2000; round++) {
    const int64_t rowDoubles = round % 3 == 0 ? 16 : (int64_t)16 << (next() % 18);
    int64_t cap = 256;
    while (!pqa::PageFits(cap, rowDoubles)) cap /= 2;
    std::vector<int64_t> largest((size_t)(next() % 300));
    for (auto &b : largest) b = 1 + (int64_t)(next() % (uint64_t)cap);   // (every quiz fits by itself: the engine has refused the others)
    if (!check(largest, rowDoubles)) { std::printf("round %d failed\n", round); return 1; }
    calls++;
  }
  std::printf("ok %lld\n", (long long)calls);
  return 0;
}
