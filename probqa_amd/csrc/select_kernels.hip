// select_kernels.hip -- picking the next question from the priority vector (gfx950).
//   * argmax (the north-star selector): lowest index among the maximal priorities of eligible questions;
//   * sampled (the reference's selector, PqaCore/CpuEngine.cpp:362-400): per-subtask Kahan run lengths,
//     Kahan grand totals, one uniform number, two upper_bounds -- reproduced step for step, so with the same
//     priorities, subtask count and random number it returns the reference's question.
// Both are single-workgroup kernels over Q doubles: latency-bound, nothing to tile.
#include "pqa_device.h"
#include "pqa_kernels.h"
#include "sampled_part.h"

namespace pqa {

namespace {

struct Best {
  double p;
  int64_t i;
};

__device__ __forceinline__ bool better(const Best &a, const Best &b) {  // is a better than b
  if (b.i < 0) return a.i >= 0;
  if (a.i < 0) return false;
  return (a.p > b.p) || (a.p == b.p && a.i < b.i);
}

__global__ __launch_bounds__(1024) void select_argmax_kernel(const double *__restrict__ priority,
                                                             const uint32_t *__restrict__ qgap,
                                                             const uint32_t *__restrict__ asked, int64_t qFirst,
                                                             int64_t n, int64_t outBase, SelectResult *out, uint64_t *flag,
                                                             uint64_t flagValue, int packed) {
  __shared__ double sp[16];
  __shared__ int64_t si[16];
  Best b = {0.0, -1};
  for (int64_t j = threadIdx.x; j < n; j += blockDim.x) {
    const int64_t q = qFirst + j;
    if (bit_test(qgap, q) || bit_test(asked, q)) continue;
    double p = priority[j];
    if (p != p) p = -__builtin_huge_val();  // NaN never wins over a number
    const Best c = {p, q};
    if (better(c, b)) b = c;
  }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    Best o;
    o.p = __shfl_xor(b.p, m, kWave);
    o.i = __shfl_xor(b.i, m, kWave);
    if (better(o, b)) b = o;
  }
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) {
    sp[wave] = b.p;
    si[wave] = b.i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Best r = {sp[0], si[0]};
    const int nw = (blockDim.x + kWave - 1) / kWave;
    for (int w = 1; w < nw; w++) {
      const Best c = {sp[w], si[w]};
      if (better(c, r)) r = c;
    }
    // `out` and `flag` (where given) in host-coherent memory: the host polls instead of copying + synchronising
    // (packed: the engine's own cell -- one tagged granule, the host adds outBase: select_record.h)
    if (packed) host_publish_packed(out, r.p, flagValue, r.i < 0 ? -1 : r.i - qFirst);
    else host_publish(out, r.p, r.i < 0 ? -1 : r.i - qFirst + outBase, flag, flagValue);
  }
}

__global__ __launch_bounds__(1024) void select_sampled_kernel(const double *__restrict__ priority,
                                                              const uint32_t *__restrict__ qgap,
                                                              const uint32_t *__restrict__ asked, int64_t qFirst,
                                                              int64_t n, int64_t nWorkers, uint64_t rnd,
                                                              double *__restrict__ runLength, SelectResult *out, uint64_t *flag, uint64_t flagValue) {
  extern __shared__ double grand[];  // nSubtasks doubles
  const SampledPick r = select_sampled_wg_impl<false>(priority, qgap, asked, qFirst, n, nWorkers, rnd, runLength, grand);
  if (threadIdx.x == 0) {
    // `out` and `flag` (where given) in host-coherent memory: the host polls instead of copying + synchronising
    host_publish(out, r.priority, r.index, flag, flagValue);
  }
}

// The same selection with priorities, run lengths and totals staged in LDS (select_sampled_wg_lds): every global load of the
// kernel is issued in one parallel round instead of one per item of a subtask's dependent chain.  For question counts whose
// staging fits 64 KiB.
__global__ __launch_bounds__(256) void select_sampled_lds_kernel(const double *__restrict__ priority,
                                                                 const uint32_t *__restrict__ qgap,
                                                                 const uint32_t *__restrict__ asked, int64_t qFirst, int64_t n,
                                                                 int64_t nWorkers, uint64_t rnd, SelectResult *out, uint64_t *flag,
                                                                 uint64_t flagValue) {
  extern __shared__ double lds[];
  const SampledPick r = select_sampled_wg_lds<false>(priority, qgap, asked, qFirst, n, nWorkers, rnd, lds);
  if (threadIdx.x == 0) {
    host_publish(out, r.priority, r.index, flag, flagValue);
  }
}

// ---- the reference's selector for every quiz of a batched sweep (NextQuestionSampledBatch) --------------------------------------
// The priorities are read where the batched sweep (and the pole fix behind it) left them.  Per-quiz vectors (grid.y = quiz): one
// workgroup per quiz runs the single-quiz selector's own workgroup code, staged in LDS while it fits, with run lengths in global
// scratch beyond that.
template <bool LDS>
__global__ __launch_bounds__(256) void select_sampled_batch_vec_kernel(SampledBatch a) {
  extern __shared__ double lds[];   // LDS: the whole staging; else the subtasks' totals
  const int b = blockIdx.x;
  const QuizSlot s = a.slots[b];
  const uint64_t rnd = a.rnd[b];
  SampledPick r;
  if constexpr (LDS) r = select_sampled_wg_lds<false>(s.priority, a.qgap, s.asked, 0, a.n, a.nWorkers, rnd, lds);
  else r = select_sampled_wg_impl<false>(s.priority, a.qgap, s.asked, 0, a.n, a.nWorkers, rnd, a.run + (size_t)b * (size_t)a.n, lds);
  if (threadIdx.x == 0) {
    host_publish(a.out + b, r.priority, r.index + a.outBase, a.seq + b, a.flagValue);
  }
}

// The quiz-minor matrix priorityT[q * Bp + b] (row-sharing and mid-batch sweeps): the lane is the quiz.  A thread runs ONE subtask's
// Kahan chain (PqaCore/CEEvalQsSubtaskConsider.cpp:52-58, :212-214) of ONE quiz over consecutive questions; the 64 lanes of a wave
// are 64 adjacent quizzes on the same subtask, so every load instruction covers 64 adjacent doubles of a matrix row.  The eight
// loads of a round are issued before the chain consumes them.  STORE: the running sums go to run[(i - first) * stride + b].
template <bool STORE>
__device__ __forceinline__ double sampled_lane_chain(const double *__restrict__ col, int64_t stride, const uint32_t *__restrict__ qgap,
                                                     const uint32_t *__restrict__ asked, int64_t first, int64_t limit, double *run) {
  Kahan1 acc;
  acc.init(0.0);
  int64_t word = -1;
  uint32_t bits = 0;
  for (int64_t i0 = first; i0 < limit; i0 += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = i0 + u < limit ? col[(i0 + u) * stride] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int64_t i = i0 + u;
      if (i < limit) {
        if ((i >> 5) != word) { word = i >> 5; bits = qgap[word] | asked[word]; }
        if (!((bits >> (i & 31)) & 1u)) acc.add(v[u]);   // gap / asked questions only copy the running sum (:54-58)
        if constexpr (STORE) run[(i - first) * stride] = acc.get();
      }
    }
  }
  return acc.get();
}

// grand[s * Bp + b] = total of subtask s for quiz b
__global__ __launch_bounds__(256) void select_sampled_lanes_kernel(SampledBatch a) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = (int)(g % a.Bp);
  const int64_t s = g / a.Bp;
  const int64_t quot = a.n / a.nWorkers, rem = a.n % a.nWorkers;
  const int64_t nSubtasks = (quot == 0) ? rem : a.nWorkers;  // CalcSplit stops once the items run out
  if (s >= nSubtasks || b >= a.nSlots) return;
  const int64_t first = (s == 0) ? 0 : calc_split_bound(s - 1, quot, rem), limit = calc_split_bound(s, quot, rem);
  a.grand[s * a.Bp + b] = sampled_lane_chain<false>(a.priorityT + b, a.Bp, a.qgap, a.slots[b].asked, first, limit, nullptr);
}

// ... and the finish, a lane per quiz: Kahan grand totals in subtask order (PqaCore/CpuEngine.cpp:362-368), the uniform number, the
// upper_bound over the totals, then the chosen subtask's chain once more -- the same operations on the same values, so the same
// bits -- with its running sums STORED (run[j * Bp + b]) and the second upper_bound over them as stored values.
__global__ __launch_bounds__(64) void select_sampled_lanes_finish_kernel(SampledBatch a) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= a.nSlots) return;
  const int64_t Bp = a.Bp, n = a.n;
  const int64_t quot = n / a.nWorkers, rem = n % a.nWorkers;
  const int64_t nSubtasks = (quot == 0) ? rem : a.nWorkers;
  double *grand = a.grand + b;
  Kahan1 accTotG;
  accTotG.init(0.0);                                           // :362
  for (int64_t s0 = 0; s0 < nSubtasks; s0 += 16) {             // (16 loads together, as select_sampled_wg_impl)
    double g[16];
#pragma unroll
    for (int u = 0; u < 16; u++) g[u] = s0 + u < nSubtasks ? grand[(s0 + u) * Bp] : 0.0;
#pragma unroll
    for (int u = 0; u < 16; u++) {
      if (s0 + u < nSubtasks) {
        accTotG.add(g[u]);                                     // :366-367
        g[u] = accTotG.get();                                  // :368
      }
    }
#pragma unroll
    for (int u = 0; u < 16; u++)
      if (s0 + u < nSubtasks) grand[(s0 + u) * Bp] = g[u];
  }
  const double totG = grand[(nSubtasks - 1) * Bp];             // :375
  const double selRunLen = totG * (double)a.rnd[b] / 18446744073709551615.0;  // :379, SRDoubleNumber::MakeRandom
  int64_t sel;
  const int64_t iWorker = upper_bound_strided(grand, nSubtasks, Bp, selRunLen);   // :380-381
  if (iWorker >= nSubtasks) {
    sel = n - 1;                                               // :384
  } else {
    const double inWorkerRunLen = selRunLen - ((iWorker == 0) ? 0.0 : grand[(iWorker - 1) * Bp]);  // :388
    const int64_t first = (iWorker == 0) ? 0 : calc_split_bound(iWorker - 1, quot, rem);           // :389
    const int64_t limit = calc_split_bound(iWorker, quot, rem);                                     // :390
    double *run = a.run + b;
    sampled_lane_chain<true>(a.priorityT + b, Bp, a.qgap, a.slots[b].asked, first, limit, run);
    sel = first + upper_bound_strided(run, limit - first, Bp, inWorkerRunLen);                      // :391
    if (sel >= limit) sel = limit - 1;                         // :392-400
  }
  host_publish(a.out + b, totG, sel + a.outBase, a.seq + b, a.flagValue);
}

// ---- the same selector over shards that separate processes drive: selection parts (sampled_part.h) ---------------------------------
// Pack, behind this shard's batched sweep: a thread is ONE (quiz, global subtask), the lanes of a wave adjacent quizzes as in
// select_sampled_lanes_kernel.  A subtask that lies whole in the shard is chained here -- sampled_lane_chain over the shard's local
// questions, its running sums kept in `run` for the pick -- and its total goes into the part; of a subtask that the shard's bounds
// cut, the same thread copies the shard's priorities and skip bits into a piece instead, for the ranks to chain; every other total
// is 0.  The flag protocol is pack_answer_rows_kernel's (kb_kernels.hip).
__global__ __launch_bounds__(256) void sampled_pack_parts_kernel(SampledPartsPack a) {
  const SampledSplit sp = sampled_split(a.qTotal, a.nWorkers);
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = (int)(g % a.Bq);
  const int64_t s = g / a.Bq;
  if (s < sp.nS && b < a.nSlots) {
    char *part = a.dst + (int64_t)b * a.partBytes;
    const SampledPartShape sh = sampled_part_shape(sp, a.qFirst, a.nLocal);
    if (s == 0) {
      SampledPartHeader *h = reinterpret_cast<SampledPartHeader *>(part);
      h->qFirst = a.qFirst;
      h->nLocal = a.nLocal;
      h->nS = sp.nS;
      h->seq = a.seq;
      a.stamp[b] = a.seq;
    }
    const bool matrix = a.priorityT != nullptr;
    const double *col = matrix ? a.priorityT + b : a.slots[b].priority;
    const int64_t stride = matrix ? a.Bq : 1;
    const uint32_t *asked = a.slots[b].asked;
    double total = 0.0;
    if (s >= sh.firstWhole && s < sh.firstWhole + sh.nWhole) {
      const int64_t first = sampled_first(sp, s) - a.qFirst, limit = sampled_limit(sp, s) - a.qFirst;   // local questions
      double *run = matrix ? a.run + first * a.Bq + b : a.run + (int64_t)b * a.nLocal + first;
      total = sampled_lane_chain<true>(col, stride, a.qgap, asked, first, limit, run);
    } else if (s == sh.p0Sub || s == sh.p1Sub) {
      const int piece = s == sh.p0Sub ? 0 : 1;
      const int64_t first = (piece == 0 ? sh.p0First : sh.p1First) - a.qFirst, len = piece == 0 ? sh.p0Len : sh.p1Len;
      double *pri = reinterpret_cast<double *>(part + sampled_piece_offset(sp, piece));
      uint64_t *skip = reinterpret_cast<uint64_t *>(pri + sp.L);
      uint64_t word = 0;
#pragma unroll 4
      for (int64_t j = 0; j < len; j++) {
        const int64_t i = first + j;
        pri[j] = col[i * stride];
        word |= (uint64_t)(((a.qgap[i >> 5] | asked[i >> 5]) >> (i & 31)) & 1u) << (j & 63);
        if ((j & 63) == 63 || j == len - 1) { skip[j >> 6] = word; word = 0; }
      }
    }
    reinterpret_cast<double *>(part + sampled_totals_offset())[s] = total;
  }
  if (a.flag == nullptr) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope: this thread's part of the parts before the count
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (__hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != gridDim.x - 1) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  __hip_atomic_store(a.flag, a.flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// A piece's questions added to a chain that an earlier rank's piece may have begun: sampled_lane_chain's round of eight loads and
// its operations, on the Kahan state handed in, with the skip bits as the piece carries them.  STORE: run[j] = the running sum.
template <bool STORE>
__device__ __forceinline__ void sampled_piece_chain(Kahan1 &acc, const double *__restrict__ pri, const uint64_t *__restrict__ skip, int64_t n,
                                                    double *run) {
  for (int64_t i0 = 0; i0 < n; i0 += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = i0 + u < n ? pri[i0 + u] : 0.0;
    const uint64_t bits = skip[i0 >> 6];   // (eight questions from a multiple of eight: one word)
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int64_t i = i0 + u;
      if (i < n) {
        if (!((bits >> (i & 63)) & 1u)) acc.add(v[u]);   // gap / asked questions only copy the running sum
        if constexpr (STORE) run[i] = acc.get();
      }
    }
  }
}

__device__ __forceinline__ int sampled_rank_of(const int64_t *firsts, int world, int64_t q) {   // firsts[r]: rank r's first question, ascending
  int r = 0;
  while (r + 1 < world && firsts[r + 1] <= q) r++;
  return r;
}

// Subtask s, cut by rank bounds: ONE Kahan chain continued through the ranks' pieces in rank order.  Returns its total.
template <bool STORE>
__device__ __forceinline__ double sampled_cut_chain(const SampledPartsPick &a, const SampledSplit &sp, const int64_t *firsts, int b, int64_t s,
                                                    double *run) {
  Kahan1 acc;
  acc.init(0.0);
  const int64_t limit = sampled_limit(sp, s);
  int64_t done = 0;
  for (int r = sampled_rank_of(firsts, a.world, sampled_first(sp, s)); r < a.world && firsts[r] < limit; r++) {
    const SampledPartShape sh = sampled_part_shape(sp, firsts[r], firsts[r + 1] - firsts[r]);
    if (sh.p0Sub != s && sh.p1Sub != s) break;
    const int piece = sh.p0Sub == s ? 0 : 1;
    const int64_t len = piece == 0 ? sh.p0Len : sh.p1Len;
    const char *part = a.parts + ((int64_t)r * a.nSlots + b) * a.partBytes;
    const double *pri = reinterpret_cast<const double *>(part + sampled_piece_offset(sp, piece));
    sampled_piece_chain<STORE>(acc, pri, reinterpret_cast<const uint64_t *>(pri + sp.L), len, STORE ? run + done : nullptr);
    done += len;
  }
  return acc.get();
}

// Pick, over the gathered parts of every rank: a workgroup of one wave per quiz.  The headers are checked first (the ranges tile the
// question axis, so every index below is within the parts).  Then the subtasks' totals are collected -- a whole subtask's from the
// rank whose range contains it, a cut subtask's by the lane of the first rank bound inside it, which continues one chain through
// the pieces -- and lane 0 runs select_sampled_lanes_finish_kernel's finish over them: the same operations on the same values, so
// the same bits as the whole engine's selector.  The second upper_bound runs over the chain's stored running sums for a cut
// subtask (every rank gets the pick), over the run lengths the pack kernel saved for a subtask whole on this rank, and is left to
// its rank (index -1) otherwise.
__global__ __launch_bounds__(64) void sampled_pick_parts_kernel(SampledPartsPick a) {
  __shared__ int64_t firsts[kSampledMaxWorld + 1];
  __shared__ int64_t counts[kSampledMaxWorld];
  __shared__ int bad;   // bit 0: the part of this rank or the saved run lengths are not of the engine's latest pack; bit 1: the headers
  const int b = blockIdx.x, t = threadIdx.x;
  const SampledSplit sp = sampled_split(a.qTotal, a.nWorkers);
  if (t == 0) bad = 0;
  __syncthreads();
  for (int r = t; r < a.world; r += blockDim.x) {
    const SampledPartHeader *h = reinterpret_cast<const SampledPartHeader *>(a.parts + ((int64_t)r * a.nSlots + b) * a.partBytes);
    firsts[r] = h->qFirst;
    counts[r] = h->nLocal;
    if (h->nS != sp.nS) atomicOr(&bad, 2);
    if (r == a.rank && (h->seq != a.seq || a.stamp[b] != a.seq)) atomicOr(&bad, 1);
  }
  __syncthreads();
  if (t == 0) {
    int64_t at = 0;
    bool tiles = true;
    for (int r = 0; r < a.world; r++) {
      tiles = tiles && firsts[r] == at && counts[r] >= 1 && counts[r] <= a.qTotal - at;
      if (!tiles) break;
      at += counts[r];
    }
    firsts[a.world] = at;
    if (!tiles || at != a.qTotal) bad |= 2;
  }
  __syncthreads();
  if (bad != 0) {
    if (t == 0) {
      host_publish(a.out + b, 0.0, (bad & 1) ? -2 : -3, a.flags + b, a.flagValue);   // a stale part first: its header is not to be believed
    }
    return;
  }
  double *grand = a.grand + (int64_t)b * sp.nS;
  for (int64_t s = t; s < sp.nS; s += blockDim.x) {   // whole subtasks: the total of the rank that holds them
    const int r = sampled_rank_of(firsts, a.world, sampled_first(sp, s));
    if (sampled_limit(sp, s) <= firsts[r + 1])
      grand[s] = reinterpret_cast<const double *>(a.parts + ((int64_t)r * a.nSlots + b) * a.partBytes + sampled_totals_offset())[s];
  }
  for (int r = t + 1; r < a.world; r += blockDim.x) {   // cut subtasks: the first bound inside one chains it
    const int64_t s = sampled_subtask_of(sp, firsts[r]), first = sampled_first(sp, s);
    if (first == firsts[r] || (r > 1 && first < firsts[r - 1])) continue;   // not cut here, or an earlier bound's
    grand[s] = sampled_cut_chain<false>(a, sp, firsts, b, s, nullptr);
  }
  __syncthreads();
  if (t != 0) return;
  const int64_t nSubtasks = sp.nS;
  Kahan1 accTotG;
  accTotG.init(0.0);                                           // PqaCore/CpuEngine.cpp:362
  for (int64_t s0 = 0; s0 < nSubtasks; s0 += 16) {             // (16 loads together, as select_sampled_lanes_finish_kernel)
    double g[16];
#pragma unroll
    for (int u = 0; u < 16; u++) g[u] = s0 + u < nSubtasks ? grand[s0 + u] : 0.0;
#pragma unroll
    for (int u = 0; u < 16; u++) {
      if (s0 + u < nSubtasks) {
        accTotG.add(g[u]);                                     // :366-367
        g[u] = accTotG.get();                                  // :368
      }
    }
#pragma unroll
    for (int u = 0; u < 16; u++)
      if (s0 + u < nSubtasks) grand[s0 + u] = g[u];
  }
  const double totG = grand[nSubtasks - 1];                    // :375
  const double selRunLen = totG * (double)a.rnd[b] / 18446744073709551615.0;  // :379, SRDoubleNumber::MakeRandom
  int64_t sel;
  const int64_t iWorker = upper_bound_strided(grand, nSubtasks, 1, selRunLen);   // :380-381
  if (iWorker >= nSubtasks) {
    sel = a.qTotal - 1;                                        // :384
  } else {
    const double inWorkerRunLen = selRunLen - ((iWorker == 0) ? 0.0 : grand[iWorker - 1]);  // :388
    const int64_t first = sampled_first(sp, iWorker), limit = sampled_limit(sp, iWorker);   // :389-390
    const int r = sampled_rank_of(firsts, a.world, first);
    if (limit > firsts[r + 1]) {                               // cut: the chain once more, its running sums stored
      double *run = a.run + (int64_t)b * sp.L;
      sampled_cut_chain<true>(a, sp, firsts, b, iWorker, run);
      sel = first + upper_bound_strided(run, limit - first, 1, inWorkerRunLen);             // :391
      if (sel >= limit) sel = limit - 1;                       // :392-400
    } else if (r == a.rank) {                                  // whole on this rank: the pack kernel's run lengths
      const double *run = a.packRun + (int64_t)b * a.packRunQuiz + (first - firsts[r]) * a.packRunStride;
      sel = first + upper_bound_strided(run, limit - first, a.packRunStride, inWorkerRunLen);
      if (sel >= limit) sel = limit - 1;
    } else {
      sel = -1;                                                // whole on another rank: that rank reports it
    }
  }
  host_publish(a.out + b, totG, sel, a.flags + b, a.flagValue);
}

}  // namespace

hipError_t LaunchSelectArgmax(const double *priority, const uint32_t *qgap, const uint32_t *asked, int64_t qFirst,
                              int64_t n, int64_t outBase, SelectResult *out, uint64_t *flag, uint64_t flagValue,
                              hipStream_t stream, bool packed) {
  const unsigned threads = n >= 1024 ? 1024 : (unsigned)(((n + 63) / 64) * 64 ? ((n + 63) / 64) * 64 : 64);
  hipLaunchKernelGGL(select_argmax_kernel, dim3(1), dim3(threads), 0, stream, priority, qgap, asked, qFirst, n,
                     outBase, out, flag, flagValue, packed ? 1 : 0);
  return hipGetLastError();
}

hipError_t LaunchSelectSampled(const double *priority, const uint32_t *qgap, const uint32_t *asked, int64_t qFirst,
                               int64_t n, int64_t nSubtasks, uint64_t rnd, double *runLength, SelectResult *out,
                               uint64_t *flag, uint64_t flagValue, hipStream_t stream) {
  if (n <= 0 || nSubtasks <= 0) return hipErrorInvalidValue;
  const size_t staged = (size_t)select_sampled_lds_doubles(n, nSubtasks) * sizeof(double);
  if (staged <= kLdsNoOptIn) {
    hipLaunchKernelGGL(select_sampled_lds_kernel, dim3(1), dim3(256), staged, stream, priority, qgap, asked, qFirst, n, nSubtasks,
                       rnd, out, flag, flagValue);
    return hipGetLastError();
  }
  const size_t shmem = (size_t)nSubtasks * sizeof(double);
  if (shmem > kLdsNoOptIn) return hipErrorInvalidValue;
  hipLaunchKernelGGL(select_sampled_kernel, dim3(1), dim3(1024), shmem, stream, priority, qgap, asked, qFirst, n, nSubtasks,
                     rnd, runLength, out, flag, flagValue);
  return hipGetLastError();
}

void SelectSampledBatchScratch(int64_t n, int64_t nSubtasks, int nSlots, int Bp, size_t *grandDoubles, size_t *runDoubles) {
  const int64_t quot = n / nSubtasks, rem = n % nSubtasks, subtasks = quot == 0 ? rem : nSubtasks;
  if (Bp > 0) {   // the matrix: the subtasks' totals and one subtask's running sums, quiz-minor both
    *grandDoubles = (size_t)subtasks * (size_t)Bp;
    *runDoubles = (size_t)(quot + 1) * (size_t)Bp;
    return;
  }
  *grandDoubles = 0;   // (LDS)
  *runDoubles = (size_t)select_sampled_lds_doubles(n, nSubtasks) * sizeof(double) <= kSampledBatchLdsBytes ? 0 : (size_t)nSlots * (size_t)n;
}

hipError_t LaunchSelectSampledBatch(const SampledBatch &a, hipStream_t stream) {
  if (a.n <= 0 || a.nWorkers <= 0 || a.nSlots <= 0 || a.nSlots > 256 || !a.slots || !a.rnd || !a.out || !a.seq) return hipErrorInvalidValue;
  if (a.priorityT != nullptr) {
    if (a.Bp < a.nSlots || a.Bp % kWave != 0 || !a.grand || !a.run) return hipErrorInvalidValue;
    const int64_t quot = a.n / a.nWorkers, rem = a.n % a.nWorkers, nSubtasks = quot == 0 ? rem : a.nWorkers;
    const int64_t threads = nSubtasks * a.Bp;
    hipLaunchKernelGGL(select_sampled_lanes_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(select_sampled_lanes_finish_kernel, dim3((unsigned)((a.nSlots + kWave - 1) / kWave)), dim3(kWave), 0, stream, a);
    return hipGetLastError();
  }
  const size_t staged = (size_t)select_sampled_lds_doubles(a.n, a.nWorkers) * sizeof(double);
  if (staged <= kSampledBatchLdsBytes) {
    if (staged > kLdsNoOptIn) {
      static LaunchCache cache;   // (per device)
      const hipError_t e = cache.OptIn(DeviceSlot(), select_sampled_batch_vec_kernel<true>, kSampledBatchLdsBytes);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(select_sampled_batch_vec_kernel<true>, dim3((unsigned)a.nSlots), dim3(256), staged, stream, a);
    return hipGetLastError();
  }
  const size_t shmem = (size_t)a.nWorkers * sizeof(double);
  if (shmem > kLdsNoOptIn || !a.run) return hipErrorInvalidValue;
  hipLaunchKernelGGL(select_sampled_batch_vec_kernel<false>, dim3((unsigned)a.nSlots), dim3(256), shmem, stream, a);
  return hipGetLastError();
}

hipError_t LaunchSampledPackParts(const SampledPartsPack &a, hipStream_t stream) {
  if (a.nSlots < 0 || a.nSlots > 256 || a.qTotal <= 0 || a.nWorkers <= 0 || a.nLocal <= 0 || a.qFirst < 0 || a.qFirst + a.nLocal > a.qTotal)
    return hipErrorInvalidValue;
  if (a.nSlots > 0 && (!a.slots || !a.qgap || !a.dst || !a.run || !a.stamp || a.Bq < a.nSlots || a.Bq % kWave != 0)) return hipErrorInvalidValue;
  if (a.flag != nullptr && a.counter == nullptr) return hipErrorInvalidValue;
  const SampledSplit sp = sampled_split(a.qTotal, a.nWorkers);
  if (a.nSlots > 0 && a.partBytes != sampled_part_bytes(sp)) return hipErrorInvalidValue;
  const int64_t threads = a.nSlots > 0 ? sp.nS * a.Bq : 1;   // (no quiz: the flag alone)
  hipLaunchKernelGGL(sampled_pack_parts_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t LaunchSampledPickParts(const SampledPartsPick &a, hipStream_t stream) {
  if (a.nSlots <= 0 || a.nSlots > 256 || a.world <= 0 || a.world > kSampledMaxWorld || a.rank < 0 || a.rank >= a.world || a.qTotal <= 0 ||
      a.nWorkers <= 0 || !a.parts || !a.rnd || !a.packRun || !a.stamp || !a.grand || !a.run || !a.out || !a.flags)
    return hipErrorInvalidValue;
  if (a.partBytes != sampled_part_bytes(sampled_split(a.qTotal, a.nWorkers))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sampled_pick_parts_kernel, dim3((unsigned)a.nSlots), dim3(kWave), 0, stream, a);
  return hipGetLastError();
}

}  // namespace pqa
