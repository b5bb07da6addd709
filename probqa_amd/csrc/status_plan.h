// status_plan.h -- how RankTargetsBatch (hip_engine_status.cpp) groups a call's (quiz, target) pairs into tiles: plain host logic
// without a device, so the suite drives it (PqaHip_HostLogicProbe "status_plan"; tests/status_plan_check.cpp).
#pragma once
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace pqa {

// A tile is up to tileCap pairs of ONE quiz: the pairs' positions in the call are order[start[i] .. start[i + 1]), and the tile's quiz is
// that of any of them.  The pairs of one quiz stay in call order and fill that quiz's open tile until it is full; the tiles stand in the
// order they were opened.  Every pair is in exactly one tile, so a result per position of `order` scatters back to the call by
// out[order[k]] = result[k].  A pair that repeats is a pair like any other.
struct RankTiles {
  std::vector<int64_t> start;   // nTiles + 1
  std::vector<int64_t> order;   // nPairs
  int64_t Tiles() const { return (int64_t)start.size() - 1; }
};
inline RankTiles PlanRankTiles(int64_t nPairs, const int64_t *quizOf, int64_t tileCap) {
  std::vector<std::vector<int64_t>> tiles;
  std::unordered_map<int64_t, size_t> openOf;   // quiz -> its newest tile
  for (int64_t i = 0; i < nPairs; i++) {
    const auto it = openOf.emplace(quizOf[i], tiles.size());
    if (!it.second && (int64_t)tiles[it.first->second].size() >= tileCap) {
      it.first->second = tiles.size();
      tiles.emplace_back();
    } else if (it.second) {
      tiles.emplace_back();
    }
    tiles[it.first->second].push_back(i);
  }
  RankTiles plan;
  plan.start.reserve(tiles.size() + 1);
  plan.order.reserve((size_t)(nPairs > 0 ? nPairs : 0));
  plan.start.push_back(0);
  for (const std::vector<int64_t> &t : tiles) {
    plan.order.insert(plan.order.end(), t.begin(), t.end());
    plan.start.push_back((int64_t)plan.order.size());
  }
  return plan;
}

}  // namespace pqa
