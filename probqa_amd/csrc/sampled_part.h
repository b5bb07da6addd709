// sampled_part.h -- the SELECTION PART of the reference's sampled selector across shards that separate processes drive
// (PqaHip_PackSampledParts / PqaHip_SampledPickFromParts): one layout for the host code, the kernels of select_kernels.hip and the
// "sampled_part" script of PqaHip_HostLogicProbe.
//
// The selector (PqaCore/CpuEngine.cpp:362-400) splits the GLOBAL question axis into subtasks (SRPoolRunner::CalcSplit) and runs one
// Kahan chain per subtask in question order.  A shard's range does not end on subtask bounds, and a Kahan chain cannot be cut and
// re-joined bit for bit from two totals -- but it can be CONTINUED by whoever sees the earlier questions' priorities and skip bits.
// So a part -- one quiz on one shard -- carries the totals of the subtasks that lie whole inside the shard, and the raw priorities
// and skip bits of the at most two subtasks its bounds cut:
//   SampledPartHeader                       {qFirst, nLocal, nS, seq}
//   double total[nS]                        Kahan total of subtask s where it lies whole in the shard, 0 elsewhere
//   piece 0, piece 1                        each L doubles, then W = ceil(L / 64) 64-bit skip words (bit j: question j of the piece is
//                                           a gap or was asked); L = the longest subtask.  A piece holds the shard's questions of ONE
//                                           cut subtask in question order: the one cut at the shard's lower bound first, then the one
//                                           cut at its upper bound; both bounds inside one subtask make one piece.  What lies behind a
//                                           piece's questions, and an unused piece, is not written.
// The size, rounded up to 16 bytes, depends on the question count and the subtask count alone: every rank computes the same value.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pqa {

struct SampledSplit {      // CalcSplit of Q questions over nSub subtasks
  int64_t Q, quot, rem, nS, L, W;
};
__host__ __device__ inline SampledSplit sampled_split(int64_t Q, int64_t nSub) {
  SampledSplit sp;
  sp.Q = Q;
  sp.quot = Q / nSub;
  sp.rem = Q % nSub;
  sp.nS = sp.quot == 0 ? sp.rem : nSub;   // CalcSplit stops once the items run out
  sp.L = sp.quot + (sp.rem > 0 ? 1 : 0);
  sp.W = (sp.L + 63) / 64;
  return sp;
}
__host__ __device__ inline int64_t sampled_limit(const SampledSplit &sp, int64_t s) {   // end of subtask s (calc_split_bound, for the host too)
  return (s + 1) * sp.quot + (s + 1 < sp.rem ? s + 1 : sp.rem);
}
__host__ __device__ inline int64_t sampled_first(const SampledSplit &sp, int64_t s) { return s == 0 ? 0 : sampled_limit(sp, s - 1); }
__host__ __device__ inline int64_t sampled_subtask_of(const SampledSplit &sp, int64_t q) {   // the first `rem` subtasks hold quot + 1 questions
  const int64_t head = sp.rem * (sp.quot + 1);
  return q < head ? q / (sp.quot + 1) : sp.rem + (q - head) / sp.quot;
}

struct SampledPartHeader {
  int64_t qFirst, nLocal, nS;
  uint64_t seq;            // the pack's sequence number on the engine that packed
};
__host__ __device__ inline int64_t sampled_totals_offset() { return (int64_t)sizeof(SampledPartHeader); }
__host__ __device__ inline int64_t sampled_piece_offset(const SampledSplit &sp, int piece) {
  return sampled_totals_offset() + 8 * sp.nS + piece * 8 * (sp.L + sp.W);
}
__host__ __device__ inline int64_t sampled_part_bytes(const SampledSplit &sp) { return (sampled_piece_offset(sp, 2) + 15) / 16 * 16; }

// What a shard [qFirst, qFirst + nLocal) contributes: whole subtasks [firstWhole, firstWhole + nWhole) and pieces (subtask -1: none).
// A piece covers questions [pXFirst, pXFirst + pXLen) of subtask pXSub.
struct SampledPartShape {
  int64_t firstWhole, nWhole;
  int64_t p0Sub, p0First, p0Len, p1Sub, p1First, p1Len;
};
__host__ __device__ inline SampledPartShape sampled_part_shape(const SampledSplit &sp, int64_t qFirst, int64_t nLocal) {
  SampledPartShape sh{0, 0, -1, 0, 0, -1, 0, 0};
  if (nLocal <= 0) return sh;
  const int64_t lo = qFirst, hi = qFirst + nLocal;
  const int64_t sLo = sampled_subtask_of(sp, lo), sHi = sampled_subtask_of(sp, hi - 1);
  const int64_t firstLo = sampled_first(sp, sLo), limitLo = sampled_limit(sp, sLo);
  const bool loCut = firstLo < lo || limitLo > hi;
  const bool hiCut = sHi != sLo && sampled_limit(sp, sHi) > hi;
  if (loCut) {
    sh.p0Sub = sLo;
    sh.p0First = firstLo < lo ? lo : firstLo;
    sh.p0Len = (limitLo < hi ? limitLo : hi) - sh.p0First;
  }
  if (hiCut) {
    const int64_t f = sampled_first(sp, sHi);
    if (loCut) { sh.p1Sub = sHi; sh.p1First = f; sh.p1Len = hi - f; }
    else { sh.p0Sub = sHi; sh.p0First = f; sh.p0Len = hi - f; }
  }
  sh.firstWhole = sLo + (loCut ? 1 : 0);
  sh.nWhole = sHi + 1 - (hiCut ? 1 : 0) - sh.firstWhole;
  if (sh.nWhole < 0) sh.nWhole = 0;
  return sh;
}

}  // namespace pqa
