// status_kernels.hip -- QuizStatusBatch and RankTargetsBatch (include/PqaHipExt.h): where a quiz stands, read off its posterior.
//
// quiz_status_kernel: one workgroup per quiz, one pass over the posterior's [0, T) and the target-gap bitmap.  A CANDIDATE is a target
// that is no gap and holds p > 0 (ListTopTargets' rule; a NaN is never one).  Over the candidates: the entropy -sum p log2 p in bits,
// the mass sum p, their number, the largest p with the lowest target among equals, and per level (at most kStatusLevels, in LDS) the
// number and the sum of the candidates with p >= level.
//   The entropy is PreviewAnswersBatch's promise kept: preview_rows_kernel's workgroup shape (256 threads up to 1024 targets, else
//   1024), its element order per thread (t = threadIdx.x, + blockDim.x, ...: so a lane's loads are 8 bytes, a wave's 512 consecutive
//   bytes -- the order fixes which thread owns which element) and its reduction (prior_device.h: ordered_sum_share / _collect).  What
//   is not a candidate adds nothing there either, so gaps and padding cannot disturb the order.  The mass and the level masses take
//   the same partition and order.  Counts and the argmax reduce as integers; no atomics anywhere.
// rank_targets_kernel: one workgroup per TILE of up to kRankTile named targets of one quiz (status_plan.h).  The tile's p_x go to LDS,
// the posterior is streamed once, every thread counts per named target the candidates that come before it -- probability descending,
// target ascending among equals: the batched listing's order -- and the counts reduce as integers.  A named target that is no
// candidate gets rank -1; its probability is the stored value either way.  No summation order to keep: 256 threads up to 1024 targets,
// else 512, so that the 32 counters have registers.
// Results go to host-coherent lines by host_store, as the listing kernels' do; the stream's order publishes them.
#include "pqa_device.h"
#include "pqa_kernels.h"
#include "prior_device.h"

namespace pqa {

namespace {

constexpr int kThreads = 1024, kSmallThreads = 256;   // (preview_rows_kernel's two shapes)
constexpr int kRankThreads = 512;                     // the ranks' long-row shape: no order to keep, and 32 counters beside the tile want more than 128 registers

template <int CTRL>
__device__ __forceinline__ int add_dpp(int v) { return v + __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ int wave_sum_i32(int v) {   // (wave_min's moves, pqa_device.h)
  v = add_dpp<kDppXor1>(v);
  v = add_dpp<kDppXor2>(v);
  v = add_dpp<kDppHalfMirror>(v);
  v = add_dpp<kDppMirror>(v);
  auto t = __builtin_amdgcn_permlane16_swap((uint32_t)v, (uint32_t)v, false, false);
  v = (int)t[0] + (int)t[1];
  t = __builtin_amdgcn_permlane32_swap((uint32_t)v, (uint32_t)v, false, false);
  return (int)t[0] + (int)t[1];
}

struct StatusAcc {
  double h, mass, best, levelMass[kStatusLevels];
  int n, bestT, levelCount[kStatusLevels];
};
// one element in the thread's order (t ascends from call to call: the first maximum is the lowest target)
// (levels: read from LDS at every use -- sixteen doubles kept in registers beside the accumulators do not fit the 128 of a 1024-thread workgroup)
__device__ __forceinline__ void status_step(StatusAcc &s, double p, bool gap, int t, const volatile double *levels, int nLevels) {
  if (gap || !(p > 0.0)) return;
  s.h += p * log2(p);
  s.mass += p;
  s.n++;
  if (p > s.best) {
    s.best = p;
    s.bestT = t;
  }
#pragma unroll
  for (int j = 0; j < kStatusLevels; j++) {
    if (j < nLevels && p >= levels[j]) {   // (j < nLevels: uniform)
      s.levelMass[j] += p;
      s.levelCount[j]++;
    }
  }
}

template <bool SMALL>
__global__ __launch_bounds__(SMALL ? kSmallThreads : kThreads) void quiz_status_kernel(TopBatchPriors priors, const uint32_t *__restrict__ tgap, int64_t T,
                                                                                       StatusLevels lv, int64_t *__restrict__ lines) {
  constexpr int kWaves = (SMALL ? kSmallThreads : kThreads) / kWave;
  __shared__ double sLevels[kStatusLevels];
  __shared__ double sSum[2 + kStatusLevels][kWaves];   // entropy, mass, the levels' masses: a row of wave sums each
  __shared__ int sCount[1 + kStatusLevels][kWaves];
  __shared__ double sBest[kWaves];
  __shared__ int sBestT[kWaves];
  const double *__restrict__ prior = priors.prior[blockIdx.x];
  const int nLevels = lv.n;
  if (threadIdx.x < kStatusLevels) sLevels[threadIdx.x] = lv.level[threadIdx.x];
  __syncthreads();
  StatusAcc s;
  s.h = 0.0;
  s.mass = 0.0;
  s.best = -1.0;
  s.n = 0;
  s.bestT = kTopNone;
#pragma unroll
  for (int j = 0; j < kStatusLevels; j++) {
    s.levelMass[j] = 0.0;
    s.levelCount[j] = 0;
  }
  const int64_t step = blockDim.x;
  int64_t t = threadIdx.x;
  if constexpr (!SMALL)
  for (; t + step < T; t += 2 * step) {   // (two loads requested together; the elements are taken in order)
    double p[2];
    bool gap[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
      p[e] = prior[t + e * step];
      gap[e] = bit_test(tgap, t + e * step);
    }
#pragma unroll
    for (int e = 0; e < 2; e++) status_step(s, p[e], gap[e], (int)(t + e * step), sLevels, nLevels);
  }
  for (; t < T; t += step) status_step(s, prior[t], bit_test(tgap, t), (int)t, sLevels, nLevels);

  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  ordered_sum_share(s.h, sSum[0]);
  ordered_sum_share(s.mass, sSum[1]);
  const int n = wave_sum_i32(s.n);
  const double wm = wave_max(s.best);
  const int wt = wave_min(s.best == wm ? s.bestT : kTopNone);
  if (lane == 0) {
    sCount[0][wave] = n;
    sBest[wave] = wm;
    sBestT[wave] = wt;
  }
#pragma unroll
  for (int j = 0; j < kStatusLevels; j++) {
    if (j < nLevels) {
      ordered_sum_share(s.levelMass[j], sSum[2 + j]);
      const int c = wave_sum_i32(s.levelCount[j]);
      if (lane == 0) sCount[1 + j][wave] = c;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int64_t *line = lines + (int64_t)blockIdx.x * kStatusLineWords;
  double best = sBest[0];
  int bestT = sBestT[0];
  int64_t count = sCount[0][0];
  for (int w = 1; w < kWaves; w++) {
    count += sCount[0][w];
    if (sBest[w] > best || (sBest[w] == best && sBestT[w] < bestT)) {
      best = sBest[w];
      bestT = sBestT[w];
    }
  }
  const bool any = best > 0.0;
  host_store(reinterpret_cast<double *>(line) + 0, 0.0 - ordered_sum_collect(sSum[0]));
  host_store(reinterpret_cast<double *>(line) + 1, ordered_sum_collect(sSum[1]));
  host_store(reinterpret_cast<double *>(line) + 2, any ? best : 0.0);
  host_store(line + 3, any ? (int64_t)bestT : (int64_t)-1);
  host_store(line + 4, count);
  for (int j = 0; j < nLevels; j++) {
    int64_t c = sCount[1 + j][0];
    for (int w = 1; w < kWaves; w++) c += sCount[1 + j][w];
    host_store(line + kStatusLineCounts + j, c);
    host_store(reinterpret_cast<double *>(line) + kStatusLineMasses + j, ordered_sum_collect(sSum[2 + j]));
  }
}

template <bool SMALL>
__global__ __launch_bounds__(SMALL ? kSmallThreads : kRankThreads) void rank_targets_kernel(const RankTile *__restrict__ tiles, const int32_t *__restrict__ ids,
                                                                                        const uint32_t *__restrict__ tgap, int64_t T,
                                                                                        RatedTargetDev *__restrict__ out) {
  constexpr int kWaves = (SMALL ? kSmallThreads : kRankThreads) / kWave;
  __shared__ double sP[kRankTile];
  __shared__ int sT[kRankTile];
  __shared__ int sBefore[kWaves][kRankTile];
  const RankTile tile = tiles[blockIdx.x];
  const double *__restrict__ prior = tile.prior;
  const int count = tile.count < kRankTile ? tile.count : kRankTile;   // (wave-uniform; the host makes no longer tile)
  if ((int)threadIdx.x < kRankTile) {
    const int x = (int)threadIdx.x < count ? ids[tile.first + threadIdx.x] : 0;   // (validated by the host: in [0, T))
    sT[threadIdx.x] = x;
    sP[threadIdx.x] = (int)threadIdx.x < count ? prior[x] : 0.0;
  }
  __syncthreads();
  int before[kRankTile];
#pragma unroll
  for (int x = 0; x < kRankTile; x++) before[x] = 0;
  auto take = [&](double p, bool gap, int t) {
    if (gap || !(p > 0.0)) return;
#pragma unroll
    for (int x = 0; x < kRankTile; x++) {
      if (x < count) {   // (uniform)
        const double px = sP[x];
        before[x] += (p > px || (p == px && t < sT[x])) ? 1 : 0;
      }
    }
  };
  const int64_t step = blockDim.x;
  int64_t t = threadIdx.x;
  if constexpr (!SMALL)
  for (; t + 3 * step < T; t += 4 * step) {
    double p[4];
    bool gap[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      p[e] = prior[t + e * step];
      gap[e] = bit_test(tgap, t + e * step);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) take(p[e], gap[e], (int)(t + e * step));
  }
  for (; t < T; t += step) take(prior[t], bit_test(tgap, t), (int)t);

  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
  for (int x = 0; x < kRankTile; x++) {
    if (x < count) {
      const int c = wave_sum_i32(before[x]);
      if (lane == 0) sBefore[wave][x] = c;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < count) {
    const int x = threadIdx.x;
    int64_t rank = 0;
    for (int w = 0; w < kWaves; w++) rank += sBefore[w][x];
    const double px = sP[x];
    const bool candidate = px > 0.0 && !bit_test(tgap, sT[x]);
    host_store(&out[tile.first + x].iTarget, candidate ? rank : (int64_t)-1);
    host_store(&out[tile.first + x].prob, px);
  }
}

}  // namespace

hipError_t LaunchQuizStatus(const KbView &kb, const TopBatchPriors &priors, int64_t nQuizzes, const StatusLevels &levels, int64_t *lines, hipStream_t stream) {
  if (nQuizzes < 1 || nQuizzes > kTopBatchQuizzes || levels.n < 0 || levels.n > kStatusLevels || lines == nullptr || kb.tgap == nullptr || kb.T < 1 ||
      kb.T > 0x7FFFFFFF)
    return hipErrorInvalidValue;
  if (kb.T <= 4 * kSmallThreads)
    hipLaunchKernelGGL(quiz_status_kernel<true>, dim3((unsigned)nQuizzes), dim3(kSmallThreads), 0, stream, priors, kb.tgap, kb.T, levels, lines);
  else
    hipLaunchKernelGGL(quiz_status_kernel<false>, dim3((unsigned)nQuizzes), dim3(kThreads), 0, stream, priors, kb.tgap, kb.T, levels, lines);
  return hipGetLastError();
}

hipError_t LaunchRankTargets(const KbView &kb, const RankTile *tiles, int64_t nTiles, const int32_t *ids, RatedTargetDev *out, hipStream_t stream) {
  if (nTiles < 1 || nTiles > kTopBatchQuizzes || tiles == nullptr || ids == nullptr || out == nullptr || kb.tgap == nullptr || kb.T < 1 || kb.T > 0x7FFFFFFF)
    return hipErrorInvalidValue;
  if (kb.T <= 4 * kSmallThreads)
    hipLaunchKernelGGL(rank_targets_kernel<true>, dim3((unsigned)nTiles), dim3(kSmallThreads), 0, stream, tiles, ids, kb.tgap, kb.T, out);
  else
    hipLaunchKernelGGL(rank_targets_kernel<false>, dim3((unsigned)nTiles), dim3(kRankThreads), 0, stream, tiles, ids, kb.tgap, kb.T, out);
  return hipGetLastError();
}

}  // namespace pqa
