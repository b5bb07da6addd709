// select_record.h -- the packed, self-tagged record of a selection the engine's own host thread waits for.
//
// 16 bytes, 16-byte aligned, written by the finisher with ONE write-through store and nothing behind it (no fence, no flag):
//   word 0: the priority (bits of a double)
//   word 1: launch tag (low 32 bits) << 32 | answer
// answer: a local question index of up to 31 bits, or one of three codes -- nothing left (-1 to the callers), an incomplete sweep
// (-3), redo with the fix of pole_kernels.hip (-4).  The host polls the tag half and takes the record once it carries the tag of
// the launch it waits for (as CollectHostPriority takes a TaggedPriority).  No launch has tag 0 -- the state of a cleared record --
// and consecutive launches on one record differ in the low 32 bits of their tags.
// Plain C++: included by the kernels and by the host, and checked without a GPU (tests/select_record_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PQA_HD __host__ __device__
#else
#define PQA_HD
#endif

namespace pqa {

struct alignas(16) PackedSelection { uint64_t priorityBits, tagAnswer; };

constexpr uint32_t kPackedNone = 0x7FFFFFFFu, kPackedIncomplete = 0x7FFFFFFEu, kPackedRedo = 0x7FFFFFFDu;
constexpr int64_t kPackedMaxIndex = 0x7FFFFFFC;   // 2^31 - 4

// index: a local question index in [0, kPackedMaxIndex], or -1 / -3 / -4
PQA_HD inline uint64_t PackSelection(uint64_t tag, int64_t index) {
  const uint32_t answer = index == -1 ? kPackedNone : index == -3 ? kPackedIncomplete : index == -4 ? kPackedRedo : (uint32_t)index;
  return ((uint64_t)(uint32_t)tag << 32) | answer;
}
PQA_HD inline uint32_t PackedTag(uint64_t tagAnswer) { return (uint32_t)(tagAnswer >> 32); }
PQA_HD inline bool PackedCarries(uint64_t tagAnswer, uint64_t tag) { return PackedTag(tagAnswer) == (uint32_t)tag; }
// what the callers handle: index + outBase, or -1 / -3 / -4 as they are
PQA_HD inline int64_t UnpackSelection(uint64_t tagAnswer, int64_t outBase) {
  const uint32_t answer = (uint32_t)tagAnswer;
  return answer == kPackedNone ? -1 : answer == kPackedIncomplete ? -3 : answer == kPackedRedo ? -4 : (int64_t)answer + outBase;
}
// the tag behind `tag`: never one whose low 32 bits are 0
PQA_HD inline uint64_t NextSelectionTag(uint64_t tag) {
  if ((uint32_t)++tag == 0) ++tag;
  return tag;
}

}  // namespace pqa
