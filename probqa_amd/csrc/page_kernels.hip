// page_kernels.hip -- conditional information gains and a greedy page of questions (include/PqaHipExt.h:
// PqaEngine_EvalConditionalGainsBatch and its neighbour; host side: hip_engine_page.cpp).
//
// CG(q | S) = I(A_q ; T | A_S): what question q tells about the target once the answers to the set S = (q_1 .. q_j) are known.  With
// the quiz's posterior p (0 at a gap target and where it is not > 0) and r_k^q(t) = A[q][k][t] * (1 / D[q][t]) (0 at gap targets),
// BRANCH b = ((k_1 K + k_2) K + ...) + k_j of the set is the row
//     w_b(t) = (((p_t r_k1^q1(t)) r_k2^q2(t)) ...)          each product rounded and stored as a double
// -- the posterior after those answers, not normalised --, its mass m_b the sum of the stored values, M = sum_b m_b, and
//     CG(q | S) = sum_b (m_b / M) gain(w_b, q)               b ascending, one fma chain
// with gain(w_b, q) the value gain_kernels.hip computes for the row w_b: that value is normalised by its own table's total, so the
// rows need no division.  A branch whose mass is not > 0 contributes nothing; M not > 0 or not finite: a row of zeros.
//
//   page_root_kernel     branch 0 of a quiz: its posterior with the zeros selected in, and its mass.  A workgroup per quiz.
//   page_expand_kernel   one workgroup per PARENT row: it streams the parent and the question's K + 1 cube rows once, 16 bytes a
//                        lane and row (two targets of a Double cube, four of a Float one), forms r_k with div_nr exactly as the gain
//                        sweep does, writes the K child rows and reduces their K masses -- a lane adds its stored values in ascending
//                        order, wave_sum adds the lanes, thread k adds the waves in wave order (prior_device.h: ordered_sum_share /
//                        ordered_sum_collect).  The question is a launch argument (a given one) or read HERE from the record the
//                        listing left (a page's pick): no pick -- a row of zeros and a mass of 0 for every child, which the later
//                        steps of that quiz then inherit.  Answer counts above kPagePiece: the same in pieces of kPagePiece answers.
//                        The expansion also notes its question in the quiz's set.  A given question that another engine holds
//                        (kPageBlockGiven) is read at the record's own pointer, a slot of a block package at the package's row
//                        pitch: the same loads, the same arithmetic, so a child row has the bits the owner's cube gives; it is
//                        noted as -1, which excludes nothing and is NOT "no pick".
//   page_combine_kernel  a thread per (quiz, question): sum_b (m_b / M) rows[b][q] over the quiz's rows of the gain sweep's output
//                        into the quiz's combined row; the first workgroup of a quiz also writes the quiz's exclusion bitmap, its
//                        asked bits | its set so far, which the listing takes for an asked bitmap.
//
// No atomics.  A value depends on the quiz's posterior, the blocks of S and of q, the listed order of S, the target gaps and K alone:
// the rows are functions of their parents element by element, every sum has a fixed order, and nothing depends on the other quizzes
// of a call, a quiz's place in it, where its rows lie in scratch, or the chunking.
#include "pqa_device.h"
#include "pqa_kernels.h"
#include "prior_device.h"

namespace pqa {

namespace {

constexpr int kPageThreads = 256, kPageWaves = kPageThreads / kWave;
constexpr int kPagePiece = 4;   // answers per pass of an expansion without an instantiation

template <typename E> struct PageVec;
template <> struct PageVec<double> {
  static constexpr int V = 2;
  static __device__ __forceinline__ void load(const double *row, int64_t t0, double (&v)[2]) {
    const double2 x = *reinterpret_cast<const double2 *>(row + t0);
    v[0] = x.x; v[1] = x.y;
  }
};
template <> struct PageVec<float> {
  static constexpr int V = 4;
  static __device__ __forceinline__ void load(const float *row, int64_t t0, double (&v)[4]) {
    const float4 x = *reinterpret_cast<const float4 *>(row + t0);
    v[0] = (double)x.x; v[1] = (double)x.y; v[2] = (double)x.z; v[3] = (double)x.w;
  }
};

template <int V>
__device__ __forceinline__ void page_load_row(const double *row, int64_t t0, double (&v)[V]) {
#pragma unroll
  for (int e = 0; e < V; e += 2) {
    const double2 x = *reinterpret_cast<const double2 *>(row + t0 + e);
    v[e] = x.x; v[e + 1] = x.y;
  }
}
template <int V>
__device__ __forceinline__ void page_store_row(double *row, int64_t t0, const double (&v)[V]) {
#pragma unroll
  for (int e = 0; e < V; e += 2) *reinterpret_cast<double2 *>(row + t0 + e) = make_double2(v[e], v[e + 1]);
}

// bit e: target t0 + e is a gap or lies behind T (t0 a multiple of V <= 4: the V bits lie in one word)
template <int V>
__device__ __forceinline__ uint32_t page_off_bits(const uint32_t *__restrict__ tgap, int64_t t0, int64_t T) {
  uint32_t off = tgap[t0 >> 5] >> (t0 & 31);
#pragma unroll
  for (int e = 0; e < V; e++)
    if (t0 + e >= T) off |= 1u << e;
  return off;
}

struct PageRows {
  const PageQuiz *quizzes;
  const void *cube;
  const uint32_t *tgap;
  double *rows, *masses;    // [row][pitch], [row]
  int64_t Q, K, T, ldT, pitch;
  int64_t blockLdT;         // the row pitch of a block package's slots in elements (kPageBlockGiven)
};

__global__ __launch_bounds__(kPageThreads) void page_root_kernel(PageRows a, TopBatchPriors priors) {
  __shared__ double waves[kPageWaves];
  const PageQuiz z = a.quizzes[blockIdx.x];
  const double *prior = priors.prior[blockIdx.x];
  double *row = a.rows + (int64_t)z.row0 * a.pitch;
  const int64_t T4 = (a.T + 3) & ~(int64_t)3;   // (the gain sweep of a Float cube reads four elements a lane)
  double acc = 0.0;
  for (int64_t t0 = (int64_t)threadIdx.x * 2; t0 < T4; t0 += (int64_t)kPageThreads * 2) {
    double p[2];
    page_load_row<2>(prior, t0, p);
    const uint32_t off = page_off_bits<2>(a.tgap, t0, a.T);
#pragma unroll
    for (int e = 0; e < 2; e++) {
      p[e] = (!((off >> e) & 1u) && p[e] > 0.0) ? p[e] : 0.0;
      acc += p[e];
    }
    page_store_row<2>(row, t0, p);
  }
  ordered_sum_share(acc, waves);
  __syncthreads();
  if (threadIdx.x == 0) a.masses[z.row0] = ordered_sum_collect(waves);
}

template <typename E, int KP>
__global__ __launch_bounds__(kPageThreads) void page_expand_kernel(PageRows a) {
  constexpr int V = PageVec<E>::V;
  __shared__ double waves[KP][kPageWaves];
  const int tid = threadIdx.x;
  const PageQuiz z = a.quizzes[blockIdx.y];
  if ((int)blockIdx.x >= z.nParents) return;
  int64_t q = z.question;
  const bool packaged = q == kPageBlockGiven;   // (workgroup-uniform) another engine's question: no local id, its block lies in a package
  if (q == kPagePickListed) q = *z.nPick > 0 ? z.pick->iTarget : -1;
  if (q < 0 || q >= a.Q) q = -1;
  if (blockIdx.x == 0 && tid == 0) z.set[z.nSet] = (int32_t)q;
  const int K = (int)a.K;
  const int64_t child0 = (int64_t)z.row0 + (int64_t)blockIdx.x * K, T4 = (a.T + 3) & ~(int64_t)3;
  if (q < 0 && !packaged) {   // (workgroup-uniform) no pick: nothing of this quiz is listed from here on
    const double zeros[V] = {};
    for (int k = 0; k < K; k++) {
      for (int64_t t0 = (int64_t)tid * V; t0 < T4; t0 += (int64_t)kPageThreads * V) page_store_row<V>(a.rows + (child0 + k) * a.pitch, t0, zeros);
      if (tid == 0) a.masses[child0 + k] = 0.0;
    }
    return;
  }
  const double *parent = a.rows + (int64_t)(z.parent0 + (int)blockIdx.x) * a.pitch;
  const int64_t ldT = packaged ? a.blockLdT : a.ldT;
  const E *block = packaged ? static_cast<const E *>(z.block) : static_cast<const E *>(a.cube) + q * (K + 1) * ldT;
  for (int k0 = 0; k0 < K; k0 += KP) {
    double acc[KP];
#pragma unroll
    for (int x = 0; x < KP; x++) acc[x] = 0.0;
    for (int64_t t0 = (int64_t)tid * V; t0 < T4; t0 += (int64_t)kPageThreads * V) {
      double p[V], d[V], v[KP][V];
      page_load_row<V>(parent, t0, p);
      PageVec<E>::load(block + (int64_t)K * ldT, t0, d);
#pragma unroll
      for (int x = 0; x < KP; x++) PageVec<E>::load(block + (int64_t)(k0 + x < K ? k0 + x : K - 1) * ldT, t0, v[x]);   // (past the last answer: read, not used)
      const uint32_t off = page_off_bits<V>(a.tgap, t0, a.T);
#pragma unroll
      for (int e = 0; e < V; e++) {
        const double inv = div_nr(1.0, d[e]);
        const bool out = (off >> e) & 1u;
#pragma unroll
        for (int x = 0; x < KP; x++) {
          const double r = v[x][e] * inv;
          v[x][e] = p[e] * (out ? 0.0 : r);
          acc[x] += v[x][e];
        }
      }
#pragma unroll
      for (int x = 0; x < KP; x++)
        if (k0 + x < K) page_store_row<V>(a.rows + (child0 + k0 + x) * a.pitch, t0, v[x]);
    }
#pragma unroll
    for (int x = 0; x < KP; x++) ordered_sum_share(acc[x], waves[x]);
    __syncthreads();
    if (tid < KP && k0 + tid < K) a.masses[child0 + k0 + tid] = ordered_sum_collect(waves[tid]);
    __syncthreads();   // (the next piece writes waves[] again)
  }
}

struct PageCombine {
  const PageQuiz *quizzes;
  const double *gains;      // [row of the sweep][gainPitch]
  const double *masses;     // [row of scratch]
  double *combined;         // [quiz][combPitch]
  uint32_t *excl;           // [quiz][exclWords], or nullptr
  int64_t Q, gainPitch, combPitch, exclWords;
};

__global__ __launch_bounds__(kPageThreads) void page_combine_kernel(PageCombine a) {
  __shared__ double weight[kTopBatchQuizzes];
  __shared__ double total;
  const int tid = threadIdx.x;
  const PageQuiz z = a.quizzes[blockIdx.y];
  if (tid == 0) {
    double M = 0.0;
    for (int b = 0; b < z.nRows; b++) M += a.masses[z.row0 + b];
    total = M;
  }
  __syncthreads();
  const double M = total;
  const bool live = M > 0.0 && M <= 1.7976931348623157e308;
  for (int b = tid; b < z.nRows; b += kPageThreads) {
    const double m = a.masses[z.row0 + b];
    weight[b] = (live && m > 0.0) ? m / M : -1.0;   // (-1: the branch contributes nothing)
  }
  __syncthreads();
  const int64_t q = (int64_t)blockIdx.x * kPageThreads + tid;
  if (q < a.Q) {
    const double *g = a.gains + (int64_t)z.gain0 * a.gainPitch + q;
    double acc = 0.0;
    for (int b = 0; b < z.nRows; b++)
      if (weight[b] >= 0.0) acc = fma(weight[b], g[(int64_t)b * a.gainPitch], acc);
    a.combined[(int64_t)blockIdx.y * a.combPitch + q] = acc;
  }
  if (blockIdx.x == 0 && a.excl != nullptr) {
    for (int64_t w = tid; w < a.exclWords; w += kPageThreads) {
      uint32_t bits = z.asked[w];
      for (int j = 0; j < z.nSet; j++) {
        const int32_t id = z.set[j];
        if (id >= 0 && (id >> 5) == w) bits |= 1u << (id & 31);
      }
      a.excl[(int64_t)blockIdx.y * a.exclWords + w] = bits;
    }
  }
}

template <typename E>
hipError_t launch_expand(const PageRows &a, int64_t nQuizzes, int64_t maxParents, hipStream_t stream) {
  const dim3 grid((unsigned)maxParents, (unsigned)nQuizzes), block(kPageThreads);
  switch (a.K) {
    case 2: hipLaunchKernelGGL((page_expand_kernel<E, 2>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((page_expand_kernel<E, 3>), grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((page_expand_kernel<E, 4>), grid, block, 0, stream, a); break;
    case 5: hipLaunchKernelGGL((page_expand_kernel<E, 5>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((page_expand_kernel<E, kPagePiece>), grid, block, 0, stream, a); break;
  }
  return hipGetLastError();
}

bool page_kb_ok(const KbView &kb, int64_t pitch) {
  return (kb.elem == 8 || kb.elem == 4) && kb.K >= 2 && kb.K <= kTopBatchQuizzes && kb.Q >= 1 && kb.T >= 1 && kb.ldT >= ((kb.T + 3) & ~(int64_t)3) && kb.ldT % 4 == 0 &&
         pitch >= ((kb.T + 3) & ~(int64_t)3) && pitch % 2 == 0;
}

}  // namespace

hipError_t LaunchPageRoots(const KbView &kb, const TopBatchPriors &priors, const PageQuiz *quizzes, int64_t nQuizzes, double *rows, int64_t pitch, double *masses,
                           hipStream_t stream) {
  if (nQuizzes <= 0 || nQuizzes > kTopBatchQuizzes || quizzes == nullptr || rows == nullptr || masses == nullptr || !page_kb_ok(kb, pitch) ||
      (reinterpret_cast<uintptr_t>(rows) & 15) != 0)
    return hipErrorInvalidValue;
  for (int64_t i = 0; i < nQuizzes; i++)
    if (priors.prior[i] == nullptr || (reinterpret_cast<uintptr_t>(priors.prior[i]) & 15) != 0) return hipErrorInvalidValue;
  const PageRows a{quizzes, kb.cube, kb.tgap, rows, masses, kb.Q, kb.K, kb.T, kb.ldT, pitch, 0};
  hipLaunchKernelGGL(page_root_kernel, dim3((unsigned)nQuizzes), dim3(kPageThreads), 0, stream, a, priors);
  return hipGetLastError();
}

hipError_t LaunchPageExpand(const KbView &kb, const PageQuiz *quizzes, int64_t nQuizzes, int64_t maxParents, double *rows, int64_t pitch, double *masses,
                            int64_t blockLdT, hipStream_t stream) {
  if (nQuizzes <= 0 || nQuizzes > kTopBatchQuizzes || maxParents <= 0 || maxParents > kTopBatchQuizzes || quizzes == nullptr || rows == nullptr || masses == nullptr ||
      !page_kb_ok(kb, pitch) || (reinterpret_cast<uintptr_t>(rows) & 15) != 0 ||
      (blockLdT != 0 && (blockLdT < ((kb.T + 3) & ~(int64_t)3) || blockLdT % 4 != 0)))   // (a slot's rows are read 16 bytes a lane up to T4, as the cube's)
    return hipErrorInvalidValue;
  const PageRows a{quizzes, kb.cube, kb.tgap, rows, masses, kb.Q, kb.K, kb.T, kb.ldT, pitch, blockLdT};
  return kb.elem == 8 ? launch_expand<double>(a, nQuizzes, maxParents, stream) : launch_expand<float>(a, nQuizzes, maxParents, stream);
}

hipError_t LaunchPageCombine(const KbView &kb, const PageQuiz *quizzes, int64_t nQuizzes, const double *gains, int64_t gainPitch, const double *masses,
                             double *combined, int64_t combPitch, uint32_t *excl, int64_t exclWords, hipStream_t stream) {
  if (nQuizzes <= 0 || nQuizzes > kTopBatchQuizzes || quizzes == nullptr || gains == nullptr || masses == nullptr || combined == nullptr || gainPitch < kb.Q ||
      combPitch < kb.Q || kb.Q < 1 || (excl != nullptr && exclWords * 32 < kb.Q))
    return hipErrorInvalidValue;
  const PageCombine a{quizzes, gains, masses, combined, excl, kb.Q, gainPitch, combPitch, exclWords};
  hipLaunchKernelGGL(page_combine_kernel, dim3((unsigned)((kb.Q + kPageThreads - 1) / kPageThreads), (unsigned)nQuizzes), dim3(kPageThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace pqa
