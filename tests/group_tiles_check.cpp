// The tile planner of the separation sweep (probqa_amd/csrc/kb_plan.h: PlanGroupTiles) as a program of its own, for a build under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_host_separation.py): seeded calls, every plan checked against the rules --
// whole groups, the caps, every group once and in order -- and the tiles walked the way the engine's staging walks them.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../probqa_amd/csrc/kb_plan.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
  state ^= state << 13; state ^= state >> 7; state ^= state << 17;
  return state;
}

static bool check(const std::vector<int64_t> &counts, int64_t maxEntries, int64_t maxGroups) {
  const int64_t n = (int64_t)counts.size();
  const std::vector<int64_t> tiles = pqa::PlanGroupTiles(n, counts.data(), maxEntries, maxGroups);
  if (n == 0) return tiles.size() == 1 && tiles[0] == 0;
  if (tiles.size() < 2 || tiles.front() != 0 || tiles.back() != n) return false;
  for (size_t i = 0; i + 1 < tiles.size(); i++) {
    const int64_t a = tiles[i], b = tiles[i + 1];
    if (a >= b || b - a > maxGroups) return false;
    int64_t entries = 0;
    for (int64_t g = a; g < b; g++) entries += counts[(size_t)g];
    if (entries > maxEntries && b - a != 1) return false;
    if (b < n && entries + counts[(size_t)b] <= maxEntries && b - a < maxGroups) return false;   // the next group would have fitted
  }
  return true;
}

int main() {
  int64_t calls = 0;
  const std::vector<std::vector<int64_t>> named = {{}, {2}, {64}, std::vector<int64_t>(128, 2), std::vector<int64_t>(129, 2), std::vector<int64_t>(5, 64),
                                                   {64, 2, 2, 64, 64, 2, 64, 2}, std::vector<int64_t>(256, 64), {300, 2, 2}};
  for (const auto &c : named) {
    if (!check(c, 256, 128)) { std::printf("named case %lld failed\n", (long long)calls); return 1; }
    calls++;
  }
  for (int round = 0; round < 2000; round++) {
    std::vector<int64_t> counts((size_t)(next() % 300));
    const int kind = (int)(next() % 3);
    for (auto &c : counts) c = kind == 0 ? 2 + (int64_t)(next() % 63) : kind == 1 ? (next() % 2 ? 64 : 2) : 2 + (int64_t)(next() % 3);
    const int64_t maxEntries = round % 2 ? 256 : 64 + (int64_t)(next() % 236), maxGroups = round % 2 ? 128 : 1 + (int64_t)(next() % 140);
    if (!check(counts, maxEntries, maxGroups)) { std::printf("round %d failed\n", round); return 1; }
    calls++;
  }
  std::printf("ok %lld\n", (long long)calls);
  return 0;
}
