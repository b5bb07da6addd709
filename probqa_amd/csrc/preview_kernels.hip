// preview_kernels.hip -- PreviewAnswersBatch (include/PqaHipExt.h): what every answer to a question would do to a quiz, without doing it.
//
// A ROW stands for one (quiz, question, answer): the posterior RecordAnswer would leave there, p = x / total with
// x[t] = prior[t] * (A[q][k][t] / D[q][t]) (0 at target gaps) and total the reference-order sum of x -- the element step, the sum and
// the division of record_answer_body (prior_device.h) on the same values in the same order, so the same bits.  The quiz's posterior
// is only read; the row lands in engine scratch, where the batched listing (kb_kernels.hip: LaunchTopTargetsBatch) takes it for a
// posterior.  RecordAnswer's long-row launches promise the bits of its one-workgroup kernel, so one workgroup per row serves every
// row length here: a call has K rows per pair and they run side by side.
//
// Per row, beside the posterior: the likelihood of the answer (total) and the entropy of the posterior in bits, -sum p log2 p over the
// p > 0, from the DIVIDED values (log2(total) - sum x log2 x / total cancels where total is small) in a fixed order: every thread adds
// its elements in ascending order, the wave's lanes are added by wave_sum, thread 0 adds the waves in order.  No atomics.
// A dead answer -- total 0 or not finite -- leaves a row of zeros (the listing then finds no candidate) and a quiet NaN for an entropy.
#include "pqa_device.h"
#include "pqa_kernels.h"
#include "prior_device.h"

namespace pqa {

namespace {

constexpr int kThreads = 1024, kSmallThreads = 256;   // (the update kernels' two shapes, prior_kernels.hip: rows of up to 1024 targets take the small one)

template <bool SMALL>
__global__ __launch_bounds__(SMALL ? kSmallThreads : kThreads) void preview_rows_kernel(PriorArgs a, const PreviewRow *__restrict__ rows, double *__restrict__ scratch,
                                                                                        int64_t pitch, int writeRows, double *__restrict__ likelihood,
                                                                                        double *__restrict__ entropy) {
  extern __shared__ double lds[];   // the sum's 8 * nWorkers + 1 doubles, then (a.stage) the row's ldT values
  __shared__ double sWave[(SMALL ? kSmallThreads : kThreads) / kWave];
  const PreviewRow r = rows[blockIdx.x];
  double *slot = scratch + (int64_t)blockIdx.x * pitch;   // (only touched where the host has provided it: !a.stage or writeRows)
  // the question's block stands in for a one-question cube, as for RecordAnswer's rows by pointer: offsets from the A row
  a.cube = r.rowA;
  a.prior = slot;
  const int64_t rowD = (int64_t)((static_cast<const char *>(r.rowD) - static_cast<const char *>(r.rowA)) / a.elem);
  const int64_t nVects = (a.T + 3) >> 2;
  double *stage = prior_stage(a, lds);
  answer_products<SMALL, false>(a, 0, rowD, r.prior, stage);
  const double total = reference_order_sum<!SMALL>(stage, nVects, a.nWorkers, lds);
  const bool dead = total == 0.0 || !(fabs(total) <= 1.7976931348623157e308);   // (wave-uniform)
  // the division (CEDivTargPriors :19) and, over the divided values, this thread's share of sum p log2 p
  double h = 0.0;
  const int64_t step = blockDim.x;
  int64_t t = threadIdx.x;
  if constexpr (!SMALL)
  for (; t + 3 * step < a.ldT; t += 4 * step) {
    double x[4];
#pragma unroll
    for (int e = 0; e < 4; e++) x[e] = stage[t + e * step];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const double p = dead ? 0.0 : (t + e * step < 4 * nVects ? x[e] / total : x[e]);
      if (writeRows) slot[t + e * step] = p;
      if (p > 0.0) h += p * log2(p);
    }
  }
  for (; t < a.ldT; t += step) {
    const double x = stage[t];
    const double p = dead ? 0.0 : (t < 4 * nVects ? x / total : x);
    if (writeRows) slot[t] = p;
    if (p > 0.0) h += p * log2(p);
  }
  ordered_sum_share(h, sWave);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sum = ordered_sum_collect(sWave);
    if (likelihood != nullptr) likelihood[blockIdx.x] = total;
    if (entropy != nullptr) entropy[blockIdx.x] = dead ? u2d(0x7FF8000000000000ULL) : 0.0 - sum;
  }
}

size_t sum_lds_bytes(int64_t nWorkers) { return (size_t)(8 * nWorkers + 1) * sizeof(double); }

}  // namespace

bool PreviewStagesInLds(const KbView &kb, int64_t nWorkers) { return sum_lds_bytes(nWorkers) + (size_t)kb.ldT * sizeof(double) <= 65536; }

hipError_t LaunchPreviewRows(const KbView &kb, const PreviewRow *rows, int64_t nRows, int64_t nWorkers, double *scratch, int64_t pitch, bool writeRows,
                             double *likelihood, double *entropy, hipStream_t stream) {
  const bool staged = PreviewStagesInLds(kb, nWorkers);
  if (nWorkers < 1 || nWorkers > kMaxWorkers || nRows < 1 || nRows > kTopBatchQuizzes || rows == nullptr || (kb.elem != 8 && kb.elem != 4) ||
      ((writeRows || !staged) && (scratch == nullptr || pitch < kb.ldT)))
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
  a.nWorkers = nWorkers;
  a.stage = staged ? 1 : 0;
  const size_t ldsBytes = sum_lds_bytes(nWorkers) + (staged ? (size_t)kb.ldT * sizeof(double) : 0);
  if (kb.T <= 4 * kSmallThreads)
    hipLaunchKernelGGL(preview_rows_kernel<true>, dim3((unsigned)nRows), dim3(kSmallThreads), ldsBytes, stream, a, rows, scratch, pitch, writeRows ? 1 : 0,
                       likelihood, entropy);
  else
    hipLaunchKernelGGL(preview_rows_kernel<false>, dim3((unsigned)nRows), dim3(kThreads), ldsBytes, stream, a, rows, scratch, pitch, writeRows ? 1 : 0,
                       likelihood, entropy);
  return hipGetLastError();
}

}  // namespace pqa
