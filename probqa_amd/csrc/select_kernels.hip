// select_kernels.hip -- picking the next question from the priority vector (gfx950).
//   * argmax (the north-star selector): lowest index among the maximal priorities of eligible questions;
//   * sampled (the reference's selector, PqaCore/CpuEngine.cpp:362-400): per-subtask Kahan run lengths,
//     Kahan grand totals, one uniform number, two upper_bounds -- reproduced step for step, so with the same
//     priorities, subtask count and random number it returns the reference's question.
// Both are single-workgroup kernels over Q doubles: latency-bound, nothing to tile.
#include "pqa_device.h"
#include "pqa_kernels.h"

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
                                                             uint64_t flagValue) {
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
    out->priority = r.p;
    out->index = r.i < 0 ? -1 : r.i - qFirst + outBase;
    if (flag != nullptr) {  // `out` and `flag` in host-coherent memory: the host polls instead of copying + synchronising
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      __hip_atomic_store(flag, flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
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
    out->priority = r.priority;
    out->index = r.index;
    if (flag != nullptr) {  // `out` and `flag` in host-coherent memory: the host polls instead of copying + synchronising
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      __hip_atomic_store(flag, flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
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
    out->priority = r.priority;
    out->index = r.index;
    if (flag != nullptr) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      __hip_atomic_store(flag, flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
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
    a.out[b].priority = r.priority;
    a.out[b].index = r.index + a.outBase;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __hip_atomic_store(a.seq + b, a.flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
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
  a.out[b].priority = totG;
  a.out[b].index = sel + a.outBase;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  __hip_atomic_store(a.seq + b, a.flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

hipError_t LaunchSelectArgmax(const double *priority, const uint32_t *qgap, const uint32_t *asked, int64_t qFirst,
                              int64_t n, int64_t outBase, SelectResult *out, uint64_t *flag, uint64_t flagValue,
                              hipStream_t stream) {
  const unsigned threads = n >= 1024 ? 1024 : (unsigned)(((n + 63) / 64) * 64 ? ((n + 63) / 64) * 64 : 64);
  hipLaunchKernelGGL(select_argmax_kernel, dim3(1), dim3(threads), 0, stream, priority, qgap, asked, qFirst, n,
                     outBase, out, flag, flagValue);
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

}  // namespace pqa
