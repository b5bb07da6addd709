// separation_kernels.hip -- questions that tell listed targets apart (include/PqaHipExt.h: PqaEngine_EvalTargetSeparation,
// PqaEngine_ListSeparatingQuestionsBatch; host side: hip_engine_sources.cpp).
//
// A group G is a list of n targets t_0 .. t_{n-1}, 2 <= n <= kSepMaxGroup (a repeated id counts twice).  With
// p_k(j) = A[q][k][t_j] * div_nr(1, D[q][t_j]) and f(x) = x log2 x (f(0) = 0), for a question q that is no gap
//     sep(G, q) = max(0, (1 / n) sum_j sum_k f(p_k(j))  -  sum_k f(m_k)),   m_k = (sum_j p_k(j)) * (1 / n)     bits:
// the Jensen-Shannon divergence of the members' answer distributions under equal weights.  It reads the members' columns of q's block
// and nothing else: a GATHER, whose cost follows the groups and not T.  Everything is fp64 whatever the cube's element type (a Float
// engine's elements are converted exactly).
//
//   sep_sweep_kernel          a workgroup per (question, TILE): a tile is a run of whole groups with at most kSepTileEntries entries and
//                             kSepTileGroups groups, planned on the host (kb_plan.h: PlanGroupTiles); the workgroups of a question lie
//                             next to each other in the grid.  Phase 1: a lane per entry gathers D[q][t] once and A[q][k][t] for every
//                             k -- K + 1 independent 8- or 4-byte loads in flight a lane, offsets in 64 bits --, forms p in fp64 and
//                             leaves it in LDS as p[k][entry], with the entry's gap bit beside it.  Phase 2: the tile's groups are
//                             dealt over the waves, 64 / W groups a pass, each in an aligned SEGMENT of W lanes -- W the power of two
//                             that holds the tile's longest group (tileWidth, from the host) --, lane j of a segment takes member j:
//                             h_j = sum_k f(p_k(j)) with k ascending, then seg_sum -- the first log2 W steps of wave_sum
//                             (pqa_device.h), a fixed tree over the segment's lanes, the idle lanes adding zeros -- of h and of every
//                             p_k, and the segment's lane 0 finishes: sum_k f(m_k) with k ascending, the difference, the clamp, ONE
//                             store.  (The logarithms are the sweep's arithmetic; with a whole wave per group a pair would use 2 lanes
//                             of 64 for them: 256 pairs took 4.3 ms that way and take 0.64 ms in segments)
//   sep_sweep_generic_kernel  answer counts without an instantiation: the same grid, segments and order of summation without LDS -- the
//                             segment that owns a group gathers its members' columns itself, an answer at a time.
//
// No atomics.  A value is a function of the members' columns of q's block, n, K and the listed order of the members alone: a member's
// place in the sums is its lane WITHIN THE SEGMENT, which is its place in the group, not its place in the tile; the tree's step s adds
// the sums of two runs of 2^s members, and a run of idle lanes adds +0.0, so the segment's width -- which follows the other groups of
// the tile -- does not change a bit.  Nothing depends on the other groups of the call, on the tiling or the host's chunks, or on where q
// falls in the grid or in a shard, and a block that is a bitwise copy of another gives the other's bits.  A gap question's workgroups
// store zeros; a group with a gap member stores zeros.
//
// Entries of one load instruction that fall into the same line are merged by the memory pipeline, and the K + 1 rows of a tile are read
// by one workgroup within one phase, so a line that entries of different waves share is in the CU's L1 when the second asks: the tile's
// entries are NOT sorted.
#include "pqa_device.h"
#include "pqa_kernels.h"

namespace pqa {

namespace {

constexpr int kSepThreads = 256, kSepWaves = kSepThreads / kWave;
static_assert(kSepTileEntries == kSepThreads, "phase 1 gives every lane one entry");
static_assert(kSepMaxGroup <= kWave, "phase 2 gives every member a lane");

struct SepSweep {
  const void *cube;
  const uint32_t *tgap, *qgap;
  const int64_t *groupStart;   // [groups of the launch + 1]: where a group's entries begin in `entries`
  const int64_t *tileGroup;    // [nTiles + 1]: a tile's first group
  const int64_t *tileWidth;    // [nTiles]: the power of two (2 .. 64) that holds the tile's longest group
  const int64_t *entries;      // the groups' targets one after another, ids in [0, T)
  double *rows;                // [group of the launch][rowPitch]
  int64_t Q, K, ldT, rowPitch;
  int64_t qBase, qCount;       // this launch's questions
  int nTiles;
};

__device__ __forceinline__ double sep_f(double x) { return x > 0.0 ? x * log2(x) : 0.0; }

// All-reduce (sum) over every aligned segment of W lanes, W a wave-uniform power of two in 2 .. 64: wave_sum's first log2 W steps.
__device__ __forceinline__ double seg_sum(double v, int W) {
  v += mov_dpp<kDppXor1>(v);
  if (W >= 4) v += mov_dpp<kDppXor2>(v);
  if (W >= 8) v += mov_dpp<kDppHalfMirror>(v);
  if (W >= 16) v += mov_dpp<kDppMirror>(v);
  if (W >= 32) { const Pair p = swap16(v); v = p.a + p.b; }
  if (W >= 64) { const Pair p = swap32(v); v = p.a + p.b; }
  return v;
}
__device__ __forceinline__ int sep_width(int64_t w) { return w >= 64 ? 64 : w >= 32 ? 32 : w >= 16 ? 16 : w >= 8 ? 8 : w >= 4 ? 4 : 2; }
// the bit of every lane of the caller's segment
__device__ __forceinline__ uint64_t seg_mask(int lane, int W) { return (W >= 64 ? ~0ull : (1ull << W) - 1ull) << (lane & ~(W - 1)); }

// lane 0 of the segment that owns a group: S1 = sum_j h_j, s[k] = sum_j p_k(j)
template <typename GetSum>
__device__ __forceinline__ double sep_finish(double S1, int n, int K, GetSum s) {
  const double invN = 1.0 / (double)n;
  double F2 = 0.0;
  for (int k = 0; k < K; k++) F2 += sep_f(s(k) * invN);
  const double v = invN * S1 - F2;
  return v > 0.0 ? v : 0.0;   // (a NaN is no value either)
}

template <typename E, int K>
__global__ __launch_bounds__(kSepThreads) void sep_sweep_kernel(SepSweep a) {
  __shared__ double p[K][kSepTileEntries];
  __shared__ uint32_t gapAt[kSepTileEntries];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int64_t q = a.qBase + blockIdx.x / a.nTiles;
  const int tile = (int)(blockIdx.x % a.nTiles);
  const int64_t g0 = a.tileGroup[tile], g1 = a.tileGroup[tile + 1];
  if (bit_test(a.qgap, q)) {
    for (int64_t g = g0 + tid; g < g1; g += kSepThreads) a.rows[g * a.rowPitch + q] = 0.0;
    return;
  }
  const int64_t e0 = a.groupStart[g0];
  const int64_t e1 = min(a.groupStart[g1], e0 + (int64_t)kSepTileEntries);   // (the plan keeps to the cap; the LDS is never overrun)
  const int64_t ldT = a.ldT;
  const E *block = static_cast<const E *>(a.cube) + q * (int64_t)(K + 1) * ldT;
  if (e0 + tid < e1) {
    const int64_t t = a.entries[e0 + tid];
    const E d = block[(int64_t)K * ldT + t];
    E v[K];
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = block[(int64_t)k * ldT + t];
    const double inv = div_nr(1.0, (double)d);
#pragma unroll
    for (int k = 0; k < K; k++) p[k][tid] = (double)v[k] * inv;
    gapAt[tid] = bit_test(a.tgap, t) ? 1u : 0u;
  }
  __syncthreads();
  const int W = sep_width(a.tileWidth[tile]), perPass = kWave / W, j = lane & (W - 1);
  for (int64_t first = g0 + (int64_t)wave * perPass; first < g1; first += (int64_t)kSepWaves * perPass) {
    const int64_t g = first + lane / W;
    const bool have = g < g1;
    const int64_t s = have ? a.groupStart[g] - e0 : 0;
    const int n = have ? (int)min(a.groupStart[g + 1] - a.groupStart[g], (int64_t)W) : 0;
    const bool active = j < n && s + j < e1 - e0;
    double pk[K], h = 0.0;
    bool gap = false;
#pragma unroll
    for (int k = 0; k < K; k++) {
      pk[k] = active ? p[k][s + j] : 0.0;
      h += sep_f(pk[k]);
    }
    if (active) gap = gapAt[s + j] != 0u;
    const bool anyGap = (__ballot(gap) & seg_mask(lane, W)) != 0ull;
    const double S1 = seg_sum(h, W);
#pragma unroll
    for (int k = 0; k < K; k++) pk[k] = seg_sum(pk[k], W);
    if (have && j == 0) a.rows[g * a.rowPitch + q] = anyGap ? 0.0 : sep_finish(S1, n, K, [&](int k) { return pk[k]; });
  }
}

// Any answer count: a running sum over k takes the place of the finish, in the same order.
template <typename E>
__global__ __launch_bounds__(kSepThreads) void sep_sweep_generic_kernel(SepSweep a) {
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int64_t q = a.qBase + blockIdx.x / a.nTiles;
  const int tile = (int)(blockIdx.x % a.nTiles);
  const int64_t g0 = a.tileGroup[tile], g1 = a.tileGroup[tile + 1];
  if (bit_test(a.qgap, q)) {
    for (int64_t g = g0 + tid; g < g1; g += kSepThreads) a.rows[g * a.rowPitch + q] = 0.0;
    return;
  }
  const int64_t ldT = a.ldT, K = a.K;
  const E *block = static_cast<const E *>(a.cube) + q * (K + 1) * ldT;
  const int W = sep_width(a.tileWidth[tile]), perPass = kWave / W, j = lane & (W - 1);
  for (int64_t first = g0 + (int64_t)wave * perPass; first < g1; first += (int64_t)kSepWaves * perPass) {
    const int64_t g = first + lane / W;
    const bool have = g < g1;
    const int64_t s = have ? a.groupStart[g] : 0;
    const int n = have ? (int)min(a.groupStart[g + 1] - s, (int64_t)W) : 0;
    const bool active = j < n;
    const int64_t t = active ? a.entries[s + j] : 0;
    const bool anyGap = (__ballot(active && bit_test(a.tgap, t)) & seg_mask(lane, W)) != 0ull;
    const double inv = active ? div_nr(1.0, (double)block[K * ldT + t]) : 0.0;
    const double invN = have ? 1.0 / (double)n : 0.0;
    double h = 0.0, F2 = 0.0;
    for (int64_t k = 0; k < K; k++) {
      const double pk = active ? (double)block[k * ldT + t] * inv : 0.0;
      h += sep_f(pk);
      F2 += sep_f(seg_sum(pk, W) * invN);   // (used on the segment's lane 0)
    }
    const double S1 = seg_sum(h, W);
    if (have && j == 0) {
      const double v = invN * S1 - F2;
      a.rows[g * a.rowPitch + q] = anyGap ? 0.0 : (v > 0.0 ? v : 0.0);
    }
  }
}

constexpr int64_t kSepMaxWorkgroups = 1 << 22;   // of a launch

template <typename Kernel>
hipError_t launch_questions(Kernel kernel, SepSweep a, hipStream_t stream) {
  const int64_t qPer = std::max<int64_t>(1, std::min<int64_t>(a.Q, kSepMaxWorkgroups / a.nTiles));
  for (int64_t q = 0; q < a.Q; q += qPer) {
    a.qBase = q;
    a.qCount = std::min<int64_t>(qPer, a.Q - q);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(a.qCount * a.nTiles)), dim3(kSepThreads), 0, stream, a);
  }
  return hipGetLastError();
}

template <typename E>
hipError_t launch_sweep_any(const SepSweep &a, hipStream_t stream) {
  switch (a.K) {
    case 2: return launch_questions(sep_sweep_kernel<E, 2>, a, stream);
    case 3: return launch_questions(sep_sweep_kernel<E, 3>, a, stream);
    case 4: return launch_questions(sep_sweep_kernel<E, 4>, a, stream);
    case 5: return launch_questions(sep_sweep_kernel<E, 5>, a, stream);
    default: return launch_questions(sep_sweep_generic_kernel<E>, a, stream);
  }
}

}  // namespace

hipError_t LaunchSeparationSweep(const KbView &kb, const int64_t *groupStart, const int64_t *tileGroup, const int64_t *tileWidth, const int64_t *entries,
                                 int64_t nGroups, int64_t nTiles, double *rows, int64_t rowPitch, hipStream_t stream) {
  if (nGroups <= 0) return hipSuccess;
  if (nGroups > kTopBatchQuizzes || nTiles < 1 || nTiles > nGroups || groupStart == nullptr || tileGroup == nullptr || tileWidth == nullptr || entries == nullptr || rows == nullptr ||
      rowPitch < kb.Q || (kb.elem != 8 && kb.elem != 4) || kb.K < 2 || kb.K > 32767 || kb.Q < 1)
    return hipErrorInvalidValue;
  SepSweep a{kb.cube, kb.tgap, kb.qgap, groupStart, tileGroup, tileWidth, entries, rows, kb.Q, kb.K, kb.ldT, rowPitch, 0, kb.Q, (int)nTiles};
  return kb.elem == 8 ? launch_sweep_any<double>(a, stream) : launch_sweep_any<float>(a, stream);
}

}  // namespace pqa
