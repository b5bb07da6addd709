// select_record_check.cpp -- the packed selection record of probqa_amd/csrc/select_record.h without a GPU: what the finisher packs
// is what the host unpacks, and a record is accepted only by the wait for the tag it carries.  Driven by tests/test_select_record.py.
//   select_record_check roundtrip | tags
#include <cstdio>
#include <cstring>
#include <string>

#include "../probqa_amd/csrc/select_record.h"

using namespace pqa;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static void Roundtrip() {
  static_assert(sizeof(PackedSelection) == 16 && alignof(PackedSelection) == 16, "one 16-byte granule");
  const uint64_t tags[] = {1, 2, 0xFFFFFFFFull, 0x100000001ull, (1ull << 40) + 7, 0x123456789ABCDEFull};
  const int64_t indices[] = {0, 1, kPackedMaxIndex};
  const int64_t codes[] = {-1, -3, -4};
  static_assert(kPackedMaxIndex == (1ll << 31) - 4, "the largest index below the three codes");
  for (uint64_t tag : tags) {
    for (int64_t i : indices) {
      const uint64_t w = PackSelection(tag, i);
      CHECK(PackedTag(w) == (uint32_t)tag);
      CHECK(PackedCarries(w, tag));
      CHECK(UnpackSelection(w, 0) == i);
      CHECK(UnpackSelection(w, 5000) == i + 5000);      // outBase: added by the host
    }
    for (int64_t c : codes) {
      const uint64_t w = PackSelection(tag, c);
      CHECK(PackedCarries(w, tag));
      CHECK(UnpackSelection(w, 0) == c);
      CHECK(UnpackSelection(w, 5000) == c);              // ... to questions only
    }
  }
  // the codes and the indices do not meet
  CHECK(UnpackSelection(PackSelection(1, kPackedMaxIndex), 0) != -4);
  CHECK((uint32_t)PackSelection(1, -4) == (uint32_t)kPackedMaxIndex + 1);
}

static void Tags() {
  // no launch has tag 0 (a cleared record), consecutive tags differ in the low word -- also across the wrap past 2^32
  const uint64_t starts[] = {0, 1, 0xFFFFFFFDull, 0xFFFFFFFEull, 0xFFFFFFFFull, 0x1FFFFFFFEull, (1ull << 40), (1ull << 40) + 0xFFFFFFFEull};
  for (uint64_t t : starts) {
    uint64_t prev = t;
    for (int k = 0; k < 6; k++) {
      const uint64_t next = NextSelectionTag(prev);
      CHECK(next > prev);
      CHECK((uint32_t)next != 0);
      CHECK((uint32_t)next != (uint32_t)prev);
      // a record left by the previous launch is not this launch's, nor is a cleared one
      CHECK(!PackedCarries(PackSelection(prev, 3), next) || (uint32_t)prev == 0);
      CHECK(!PackedCarries(0, next));
      CHECK(PackedCarries(PackSelection(next, 3), next));
      prev = next;
    }
  }
  CHECK(NextSelectionTag(0xFFFFFFFFull) == 0x100000001ull);     // the wrap skips the tag whose low word is 0
  CHECK(!PackedCarries(PackSelection(0xFFFFFFFFull, 0), 0x100000001ull));
}

int main(int argc, char **argv) {
  const std::string part = argc > 1 ? argv[1] : "";
  if (part == "roundtrip") Roundtrip();
  else if (part == "tags") Tags();
  else { std::printf("usage: select_record_check roundtrip | tags\n"); return 2; }
  if (failures) return 1;
  std::printf("ok %s\n", part.c_str());
  return 0;
}
