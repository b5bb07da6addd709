// review_kernels.hip -- ReviewAnswersBatch (include/PqaHipExt.h): a quiz with each of its answers left out, without resuming a quiz per answer.
//
// A ROW stands for one (quiz, position i): the posterior ResumeQuiz would leave over the quiz's answers without answer i, in their
// order -- the product chain, the exponent maximum and correction, the reference-order sum and the division of resume_quiz_body
// (prior_kernels.hip), through the same device functions (prior_device.h: chain_step, exponent_correction, replace_exponent,
// reference_order_sum), so the same bits.  Two launches per chunk:
//
//   review_chains_kernel   grid (tiles of 256 targets, distinct quizzes of the chunk), a lane per target.  The n leave-one-out chains
//     of a quiz share (1) the RATIOS A[q_j][a_j][t] / D[q_j][t] -- one IEEE division per (answer, target), computed once and kept in
//     LDS while n <= kReviewLdsAnswers (n x 256 doubles), else in engine scratch laid out [answer][target] (a lane re-reads its own
//     column: coalesced, from L2) -- and (2) the PREFIX: the chain that skips position i is the full chain through 0 .. i-1, the same
//     operands in the same order.  So the lane walks i upward with a running prefix (mantissa, exponent sum); for every requested
//     position it continues a copy of the prefix over j > i and writes mantissa and exponent sum into the row's scratch, then folds
//     answer i into the prefix.  Per target and quiz with all n positions requested: n divisions and n (n - 1) / 2 + n - 1
//     multiplications, where n resumes take n (n - 1) of each.  (The rows kernel divides once more per row, for the left-out answer's
//     likelihood: answer_products, RecordAnswer's own element step.)
//   review_rows_kernel     a workgroup per row, at every row length (ResumeQuiz's long-row launches promise the one-workgroup kernel's
//     bits): the exponent maximum over the targets that are no gaps, status and correction, the exponent replacement, the
//     reference-order sum over `workers` subtasks and the division; the entropy of the divided values in preview_rows_kernel's fixed
//     order (no atomics); the likelihood of the left-out answer under that posterior -- answer_products and the reference-order sum
//     over max(1, workers - 1) subtasks, what PreviewAnswersBatch returns for a twin quiz.  A row without remaining answers is
//     StartQuiz's posterior.  The divided row stays in the row's scratch, where the batched listing (kb_kernels.hip:
//     LaunchTopTargetsBatch) takes it for a posterior.  A dead row -- I64Underflow, or a total that is 0 or not finite -- leaves
//     zeros and two quiet NaNs.
#include "pqa_device.h"
#include "pqa_kernels.h"
#include "prior_device.h"

namespace pqa {

namespace {

constexpr int kThreads = 1024, kSmallThreads = 256;   // (the update kernels' two shapes: rows of up to 1024 targets take the small one)
constexpr int kTile = 256;                            // targets per workgroup of the chains kernel

__global__ __launch_bounds__(kTile) void review_chains_kernel(PriorArgs a, const ReviewQuiz *__restrict__ quizzes, int bugCompat, double *__restrict__ mants,
                                                              int64_t *__restrict__ exps, int64_t pitch) {
  extern __shared__ double ldsRatios[];   // [answer][lane] for the quizzes whose ratios stay here
  const ReviewQuiz q = quizzes[blockIdx.y];
  const int64_t t = (int64_t)blockIdx.x * kTile + threadIdx.x;
  if (t >= a.ldT || q.nRequests == 0) return;   // (no barrier below: a lane reads only what it wrote itself)
  const int64_t n = q.nAnswered;
  // the ratios, once: a lane's column in LDS (stride kTile) or in the quiz's scratch (stride ldT)
  double *ratios = q.ratios != nullptr ? q.ratios + t : ldsRatios + threadIdx.x;
  const int64_t stride = q.ratios != nullptr ? a.ldT : kTile;
  const int64_t last = q.requests[q.nRequests - 1].position;   // (sorted: nothing past the last requested position is folded)
  int64_t j = 0;
  for (; j + 4 <= n; j += 4) {   // (the eight loads of four answers are requested together)
    double av[4], dv[4];
#pragma unroll
    for (int e = 0; e < 4; e++) { av[e] = cube_ld(q.rows[2 * (j + e)], a.elem, t); dv[e] = cube_ld(q.rows[2 * (j + e) + 1], a.elem, t); }
#pragma unroll
    for (int e = 0; e < 4; e++) ratios[(j + e) * stride] = av[e] / dv[e];
  }
  for (; j < n; j++) ratios[j * stride] = cube_ld(q.rows[2 * j], a.elem, t) / cube_ld(q.rows[2 * j + 1], a.elem, t);
  // the prefix: vB[t] as it is, then one chain_step per answer (resume_quiz_body's first factor has no exponent reset in front)
  double mant = bugCompat ? a.vB[t & 3] : a.vB[t];   // CEUpdatePriorsSubtaskMul.cpp:53 loads pvB, not pvB+j
  int64_t ex = 0;
  int64_t k = 0;
  for (int64_t i = 0; i <= last; i++) {
    if (k < q.nRequests && q.requests[k].position == i) {
      double m = mant;
      int64_t e = ex;
      for (int64_t s = i + 1; s < n; s++) chain_step(m, e, ratios[s * stride]);
      for (; k < q.nRequests && q.requests[k].position == i; k++) {   // (a position asked for twice: two rows of the same bits)
        const int64_t at = (int64_t)q.requests[k].row * pitch + t;
        mants[at] = m;
        exps[at] = e;
      }
    }
    chain_step(mant, ex, ratios[i * stride]);
  }
}

template <bool SMALL>
__global__ __launch_bounds__(SMALL ? kSmallThreads : kThreads) void review_rows_kernel(PriorArgs a, const ReviewRow *__restrict__ rows, double *__restrict__ mants,
                                                                                       int64_t *__restrict__ exps, int64_t pitch, int64_t nLoose,
                                                                                       double *__restrict__ likelihood, double *__restrict__ entropy) {
  extern __shared__ double lds[];   // the sums' 8 * nWorkers + 1 doubles, then (a.stage) the row's ldT values
  constexpr int kWaves = (SMALL ? kSmallThreads : kThreads) / kWave;
  __shared__ long long sMax[kWaves];
  __shared__ long long sCorr;
  __shared__ double sWave[kWaves];
  const ReviewRow r = rows[blockIdx.x];
  double *slot = mants + (int64_t)blockIdx.x * pitch;
  int64_t *ex = exps + (int64_t)blockIdx.x * pitch;
  a.prior = slot;
  double *stage = prior_stage(a, lds);
  const int64_t nVects = (a.T + 3) >> 2;
  const int64_t step = blockDim.x;
  const double nan = u2d(0x7FF8000000000000ULL);
  bool dead = false;   // (block-uniform throughout)
  if (r.nRemaining == 0) {
    for (int64_t t = threadIdx.x; t < a.ldT; t += step) stage[t] = bit_test(a.tgap, t) ? 0.0 : a.vB[t];   // StartQuiz: CESetPriorsSubtaskSum.cpp:28-31
  } else {
    // CENormPriorsSubtaskMax (gap lanes retain the running maximum)
    long long myMax = INT64_MIN;
    for (int64_t t = threadIdx.x; t < 4 * nVects && t < a.ldT; t += step) {
      const long long totExp = chain_total_exp(slot[t], ex[t]);
      if (!bit_test(a.tgap, t) && totExp > myMax) myMax = totExp;
    }
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {
      const long long o = __shfl_xor(myMax, m, kWave);
      myMax = o > myMax ? o : myMax;
    }
    if (threadIdx.x % kWave == 0) sMax[threadIdx.x / kWave] = myMax;
    __syncthreads();
    if (threadIdx.x == 0) {
      long long fullMax = sMax[0];
      for (int w = 1; w < kWaves; w++) fullMax = sMax[w] > fullMax ? sMax[w] : fullMax;
      sCorr = exponent_correction(fullMax, a.T);
    }
    __syncthreads();
    const long long corrExp = sCorr;
    dead = corrExp == INT64_MIN;   // I64Underflow
    if (!dead)
      for (int64_t t = threadIdx.x; t < a.ldT; t += step) stage[t] = replace_exponent(slot[t], ex[t], corrExp, bit_test(a.tgap, t));
  }
  double total = 0.0;
  if (!dead) {
    total = reference_order_sum<!SMALL>(stage, nVects, a.nWorkers, lds);
    dead = total == 0.0 || !(fabs(total) <= 1.7976931348623157e308);
  }
  // the division (CEDivTargPriors :19) and, over the divided values, this thread's share of sum p log2 p
  double h = 0.0;
  for (int64_t t = threadIdx.x; t < a.ldT; t += step) {
    double p = 0.0;
    if (!dead) {
      const double x = stage[t];
      p = t < 4 * nVects ? x / total : x;
    }
    slot[t] = p;
    if (p > 0.0) h += p * log2(p);
  }
  h = wave_sum(h);
  if (threadIdx.x % kWave == 0) sWave[threadIdx.x / kWave] = h;
  // the likelihood of the left-out answer under the divided row: RecordAnswer's element step and its sum (block-uniform branch)
  double like = nan;
  if (!dead && likelihood != nullptr) {
    __syncthreads();   // (stage and the sums' LDS are reused)
    PriorArgs b = a;
    b.cube = r.rowA;
    b.nWorkers = nLoose;
    const int64_t rowD = (int64_t)((static_cast<const char *>(r.rowD) - static_cast<const char *>(r.rowA)) / a.elem);
    double *products = a.stage ? stage : reinterpret_cast<double *>(ex);   // (the exponent sums have been consumed)
    answer_products<SMALL, false>(b, 0, rowD, slot, products);
    like = reference_order_sum<!SMALL>(products, nVects, nLoose, lds);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = sWave[0];
    for (int w = 1; w < kWaves; w++) sum += sWave[w];
    if (likelihood != nullptr) likelihood[blockIdx.x] = like;
    if (entropy != nullptr) entropy[blockIdx.x] = dead ? nan : 0.0 - sum;
  }
}

size_t sum_lds_bytes(int64_t nWorkers) { return (size_t)(8 * nWorkers + 1) * sizeof(double); }
// (1 KiB of the 64 is left to the kernel's static arrays)
bool rows_stage_in_lds(const KbView &kb, int64_t nWorkers) { return sum_lds_bytes(nWorkers) + (size_t)kb.ldT * sizeof(double) <= 65536 - 1024; }

}  // namespace

hipError_t LaunchReviewChains(const KbView &kb, const ReviewQuiz *quizzes, int64_t nQuizzes, int64_t maxLdsAnswers, bool bugCompat, double *mants, int64_t *exps,
                              int64_t pitch, hipStream_t stream) {
  if (nQuizzes < 1 || nQuizzes > kTopBatchQuizzes || quizzes == nullptr || mants == nullptr || exps == nullptr || pitch < kb.ldT || (kb.elem != 8 && kb.elem != 4) ||
      maxLdsAnswers < 0 || maxLdsAnswers > kReviewLdsAnswers)
    return hipErrorInvalidValue;
  PriorArgs a;
  a.cube = nullptr;
  a.elem = kb.elem;
  a.vB = kb.vB;
  a.tgap = kb.tgap;
  a.prior = nullptr;
  a.K = kb.K;
  a.T = kb.T;
  a.ldT = kb.ldT;
  a.nWorkers = 1;
  a.stage = 0;
  const unsigned tiles = (unsigned)((kb.ldT + kTile - 1) / kTile);
  hipLaunchKernelGGL(review_chains_kernel, dim3(tiles, (unsigned)nQuizzes), dim3(kTile), (size_t)maxLdsAnswers * kTile * sizeof(double), stream, a, quizzes,
                     bugCompat ? 1 : 0, mants, exps, pitch);
  return hipGetLastError();
}

hipError_t LaunchReviewRows(const KbView &kb, const ReviewRow *rows, int64_t nRows, int64_t nWorkers, double *mants, int64_t *exps, int64_t pitch,
                            double *likelihood, double *entropy, hipStream_t stream) {
  if (nWorkers < 1 || nWorkers > kMaxWorkers || nRows < 1 || nRows > kTopBatchQuizzes || rows == nullptr || mants == nullptr || exps == nullptr || pitch < kb.ldT ||
      (kb.elem != 8 && kb.elem != 4))
    return hipErrorInvalidValue;
  const bool staged = rows_stage_in_lds(kb, nWorkers);
  PriorArgs a;
  a.cube = nullptr;
  a.elem = kb.elem;
  a.vB = kb.vB;
  a.tgap = kb.tgap;
  a.prior = nullptr;
  a.K = kb.K;
  a.T = kb.T;
  a.ldT = kb.ldT;
  a.nWorkers = nWorkers;
  a.stage = staged ? 1 : 0;
  const int64_t nLoose = nWorkers > 1 ? nWorkers - 1 : 1;   // RecordAnswer's split: reference PqaCore/CEQuiz.h:98
  const size_t ldsBytes = sum_lds_bytes(nWorkers) + (staged ? (size_t)kb.ldT * sizeof(double) : 0);
  if (kb.T <= 4 * kSmallThreads)
    hipLaunchKernelGGL(review_rows_kernel<true>, dim3((unsigned)nRows), dim3(kSmallThreads), ldsBytes, stream, a, rows, mants, exps, pitch, nLoose, likelihood, entropy);
  else
    hipLaunchKernelGGL(review_rows_kernel<false>, dim3((unsigned)nRows), dim3(kThreads), ldsBytes, stream, a, rows, mants, exps, pitch, nLoose, likelihood, entropy);
  return hipGetLastError();
}

}  // namespace pqa
