// Stand-alone check of the .kb window arithmetic (probqa_amd/csrc/kb_plan.h: KbLayout) for sanitizer builds:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I. tools/kb_layout_check.cpp -o /tmp/kb_layout_check && /tmp/kb_layout_check
// Walks every shard window of a set of shapes against a byte map of the file (every array byte belongs to exactly one shard's block),
// then the truncated-file and out-of-range cases: dimensions a damaged header may claim, windows past the end, sizes cut inside a block.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "probqa_amd/csrc/kb_plan.h"

using pqa::KbLayout;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static void ShardRange(int64_t Q, int64_t world, int64_t rank, int64_t &first, int64_t &limit) {   // SRPoolRunner::CalcSplit
  const int64_t quot = Q / world, rem = Q % world;
  first = rank * quot + (rank < rem ? rank : rem);
  limit = first + quot + (rank < rem ? 1 : 0);
}

int main() {
  const int64_t shapes[][3] = {{2, 3, 1}, {3, 5, 3}, {4, 50, 67}, {5, 37, 101}, {5, 8, 1025}, {2, 3, 16387}};
  for (const auto &s : shapes)
    for (int64_t elem : {4, 8})
      for (int64_t world : {1, 2, 3, 8}) {
        const int64_t K = s[0], Q = s[1], T = s[2];
        if (Q < world) continue;
        const KbLayout lay(K, Q, T, elem);
        CHECK(lay.valid);
        std::vector<unsigned char> owner((size_t)lay.trailerOff, 0);
        for (int64_t r = 0; r < world; r++) {
          int64_t first, limit;
          ShardRange(Q, world, r, first, limit);
          CHECK(lay.HasWindow(first, limit - first));
          for (int64_t b = lay.SaOffset(first); b < lay.SaOffset(first) + (limit - first) * K * lay.rowBytes; b++) owner[(size_t)b]++;
          for (int64_t b = lay.MdOffset(first); b < lay.MdOffset(first) + (limit - first) * lay.rowBytes; b++) owner[(size_t)b]++;
        }
        for (int64_t b = 0; b < lay.trailerOff; b++) CHECK(owner[(size_t)b] == ((b >= KbLayout::kHeaderBytes && b < lay.vbOff) ? 1 : 0));
        // a file cut anywhere inside its arrays is shorter than ArraysEnd()
        CHECK(lay.ArraysEnd() == lay.vbOff + T * elem);
        CHECK(lay.MdOffset(Q) == lay.vbOff && lay.SaOffset(Q) == lay.MdOffset(0));
      }
  const KbLayout lay(5, 10, 7, 8);
  const int64_t bad[][2] = {{4, 7}, {10, 1}, {-1, 2}, {0, 0}, {0, -3}, {11, 1}, {INT64_MAX, 1}, {1, INT64_MAX}, {INT64_MIN, INT64_MAX}, {INT64_MAX, INT64_MAX}};
  for (const auto &w : bad) CHECK(!lay.HasWindow(w[0], w[1]));
  CHECK(lay.HasWindow(0, 10) && lay.HasWindow(9, 1) && lay.HasWindow(4, 6));
  const int64_t absurd[][4] = {{5, 10, 7, 2}, {0, 10, 7, 8}, {5, 0, 7, 8}, {5, 10, -7, 8}, {5, (int64_t)1 << 40, (int64_t)1 << 40, 8}, {(int64_t)1 << 31, (int64_t)1 << 31, 2, 8},
                               {INT64_MAX, INT64_MAX, INT64_MAX, 8}, {INT64_MIN, 1, 1, 4}, {1, 1, INT64_MAX / 8 + 1, 8}, {2, INT64_MAX / 16, 1, 8}};
  for (const auto &a : absurd) CHECK(!KbLayout(a[0], a[1], a[2], a[3]).valid);
  CHECK(KbLayout(5, 10000000, 1000000, 8).valid);   // 400 TB: large, not absurd
  std::printf(failures ? "kb_layout_check: %d failures\n" : "kb_layout_check: ok\n", failures);
  return failures ? 1 : 0;
}
