// gain_kernels.hip -- the information gain of every question of a quiz (include/PqaHipExt.h: PqaEngine_EvalQuestionGainsBatch and
// its neighbour; host side: hip_engine_gain.cpp).
//
// With the quiz's posterior p (0 at a gap target and where it is not > 0), r_k(t) = A[q][k][t] * (1 / D[q][t]) and f(x) = x log2 x
// (f(0) = 0), question q's joint table is J[k][t] = p_t r_k(t), its answer totals W_k = sum_t J[k][t], Z = sum_k W_k, and
//     gain(quiz, q) = max(0, (f(Z) - sum_k f(W_k) - sum_t p_t g_q(t)) / Z)   bits;  0 if Z is not > 0 or not finite
//     g_q(t)        = f(s_q(t)) - sum_k f(r_k(t)),  s_q(t) = sum_k r_k(t)
// -- the mutual information between the answer to q and the target for a target drawn from p.  g_q belongs to the knowledge base
// alone: its K + 1 logarithms per element are paid once per TILE of quizzes, and a quiz of the tile costs K + 1 fma chains.
// Everything is fp64 whatever the cube's element type (a Float engine's elements are converted exactly).
//
//   gain_sweep_kernel   one streaming pass over the cube per tile of NQ quizzes: a workgroup per (question, tile), the workgroups of a
//                       question next to each other in the grid, so that the tiles of a launch share the question's block in L2.  A
//                       lane takes 16 bytes of the D row and of each of the K A rows (two targets of a Double cube, four of a Float
//                       one), forms r_k(t) with div_nr and g_q(t) with the device's fp64 log2 once per element -- zeros through a
//                       select at gap targets and behind T --, then per quiz of the tile loads the posterior's elements, selects p
//                       once, and runs W_k = fma(p, r_k, W_k) for every k and E = fma(p, g, E).  A wave reduction by DPP (wave_sum),
//                       the waves added in wave order through LDS, and one thread per (quiz, question) finishes out of LDS: Z and
//                       sum f(W_k) in k order.  A last tile that the call does not fill repeats its last quiz and writes nothing
//                       for the repeats.  A gap question gets 0.
//   gain_sweep_generic_kernel  answer counts without an instantiation: a workgroup per (question, quiz) streams the question's rows
//                       once for E and once per piece of kGainPiece answers for their W_k.  The same element arithmetic and the same
//                       order of summation.
//   gain_slots_kernel   the listing's view of the rows (LaunchTopQuestions): slot i's priority vector is row i, its asked bitmap
//                       the quiz's own.
//
// No atomics on values.  A value is a function of the quiz's posterior, question q's block, the target gaps and K alone: a lane's
// accumulators see their targets in ascending order, the lanes are added in wave_sum's fixed tree and the waves in wave order; none
// of it depends on the other quizzes of the call, the quiz's place in the call or in its tile, the tile's width, the chunking, or
// where q falls in the grid or in a shard.
#include "pqa_device.h"
#include "pqa_kernels.h"

namespace pqa {

namespace {

constexpr int kGainThreads = 256, kGainWaves = kGainThreads / kWave;
constexpr int kGainPiece = 4;   // answers per pass of the generic sweep

template <typename E> struct GainVec;
template <> struct GainVec<double> {
  static constexpr int V = 2;
  static __device__ __forceinline__ void load(const double *row, int64_t t0, double (&v)[2]) {
    const double2 x = *reinterpret_cast<const double2 *>(row + t0);
    v[0] = x.x; v[1] = x.y;
  }
};
template <> struct GainVec<float> {
  static constexpr int V = 4;
  static __device__ __forceinline__ void load(const float *row, int64_t t0, double (&v)[4]) {
    const float4 x = *reinterpret_cast<const float4 *>(row + t0);
    v[0] = (double)x.x; v[1] = (double)x.y; v[2] = (double)x.z; v[3] = (double)x.w;
  }
};

// the posterior's V elements from t0: 0 at a gap target (bit e of g) and where it is not > 0
template <int V>
__device__ __forceinline__ void gain_load_p(const double *__restrict__ prior, int64_t t0, uint32_t g, double (&p)[V]) {
#pragma unroll
  for (int e = 0; e < V; e += 2) {
    const double2 x = *reinterpret_cast<const double2 *>(prior + t0 + e);
    p[e] = x.x; p[e + 1] = x.y;
  }
#pragma unroll
  for (int e = 0; e < V; e++) p[e] = (!((g >> e) & 1u) && p[e] > 0.0) ? p[e] : 0.0;
}

__device__ __forceinline__ double gain_f(double x) { return x > 0.0 ? x * log2(x) : 0.0; }

// (t0 is a multiple of V <= 4: the V bits lie in one word)
__device__ __forceinline__ uint32_t gain_gap_bits(const uint32_t *__restrict__ tgap, int64_t t0) { return tgap[t0 >> 5] >> (t0 & 31); }

// One (quiz, question) from its sums: Z and sum f(W_k) in k order.
__device__ __forceinline__ double gain_value(double Z, double FW, double E) {
  if (!(Z > 0.0) || !(Z <= 1.7976931348623157e308)) return 0.0;
  const double v = ((gain_f(Z) - FW) - E) / Z;
  return v > 0.0 ? v : 0.0;
}

struct GainSweep {
  const void *cube;
  const uint32_t *tgap, *qgap;
  double *rows;             // [quiz of the call][rowPitch]
  int64_t Q, K, T, ldT, rowPitch;
  int64_t qBase, qCount;    // this launch's questions
  int first, nTiles, n;     // this launch's quizzes: nTiles tiles from quiz `first`; the call has n
};

template <typename E, int K, int NQ>
__global__ __launch_bounds__(kGainThreads) void gain_sweep_kernel(GainSweep a, TopBatchPriors priors) {
  constexpr int V = GainVec<E>::V, N = NQ * (K + 1);
  __shared__ double part[kGainWaves][N];
  __shared__ double table[N];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int64_t q = a.qBase + blockIdx.x / a.nTiles;
  const int quiz0 = a.first + (int)(blockIdx.x % a.nTiles) * NQ;
  if (bit_test(a.qgap, q)) {
    if (tid < NQ && quiz0 + tid < a.n) a.rows[(int64_t)(quiz0 + tid) * a.rowPitch + q] = 0.0;
    return;
  }
  const int64_t ldT = a.ldT;
  const E *block = static_cast<const E *>(a.cube) + q * (K + 1) * ldT;
  const double *prior[NQ];
#pragma unroll
  for (int i = 0; i < NQ; i++) prior[i] = priors.prior[quiz0 + i < a.n ? quiz0 + i : a.n - 1];
  double acc[N];
#pragma unroll
  for (int e = 0; e < N; e++) acc[e] = 0.0;
  for (int64_t t0 = (int64_t)tid * V; t0 < a.T; t0 += (int64_t)kGainThreads * V) {
    double d[V], r[K][V], g[V];
    GainVec<E>::load(block + K * ldT, t0, d);
#pragma unroll
    for (int k = 0; k < K; k++) GainVec<E>::load(block + k * ldT, t0, r[k]);
    const uint32_t gap = gain_gap_bits(a.tgap, t0);
#pragma unroll
    for (int e = 0; e < V; e++) {
      const double inv = div_nr(1.0, d[e]);
      const bool off = (gap >> e) & 1u;
      double s = 0.0, F = 0.0;
#pragma unroll
      for (int k = 0; k < K; k++) {
        const double x = r[k][e] * inv;
        s += x;
        F += gain_f(x);
        r[k][e] = off ? 0.0 : x;
      }
      g[e] = off ? 0.0 : gain_f(s) - F;
    }
#pragma unroll
    for (int i = 0; i < NQ; i++) {
      double p[V];
      gain_load_p<V>(prior[i], t0, gap, p);
#pragma unroll
      for (int k = 0; k < K; k++) {
#pragma unroll
        for (int e = 0; e < V; e++) acc[i * (K + 1) + k] = fma(p[e], r[k][e], acc[i * (K + 1) + k]);
      }
#pragma unroll
      for (int e = 0; e < V; e++) acc[i * (K + 1) + K] = fma(p[e], g[e], acc[i * (K + 1) + K]);
    }
  }
#pragma unroll
  for (int e = 0; e < N; e++) {
    const double s = wave_sum(acc[e]);
    if (lane == 0) part[wave][e] = s;
  }
  __syncthreads();
  if (tid < N) {
    double s = part[0][tid];
#pragma unroll
    for (int x = 1; x < kGainWaves; x++) s += part[x][tid];
    table[tid] = s;
  }
  __syncthreads();
  if (tid < NQ && quiz0 + tid < a.n) {
    const double *w = table + tid * (K + 1);
    double Z = 0.0, FW = 0.0;
#pragma unroll
    for (int k = 0; k < K; k++) Z += w[k];
#pragma unroll
    for (int k = 0; k < K; k++) FW += gain_f(w[k]);
    a.rows[(int64_t)(quiz0 + tid) * a.rowPitch + q] = gain_value(Z, FW, w[K]);
  }
}

// Any answer count: workgroup w of the grid takes the (question, quiz) pairs w, w + gridDim.x, ... of the call.
template <typename E>
__global__ __launch_bounds__(kGainThreads) void gain_sweep_generic_kernel(GainSweep a, TopBatchPriors priors) {
  constexpr int V = GainVec<E>::V;
  __shared__ double part[kGainWaves][kGainPiece];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int K = (int)a.K;
  const int64_t ldT = a.ldT;
  for (int64_t work = blockIdx.x; work < a.Q * a.n; work += gridDim.x) {
    const int64_t q = work / a.n;
    const int quiz = (int)(work % a.n);
    if (bit_test(a.qgap, q)) {
      if (tid == 0) a.rows[(int64_t)quiz * a.rowPitch + q] = 0.0;
      continue;
    }
    const E *block = static_cast<const E *>(a.cube) + q * (K + 1) * ldT;
    const double *prior = priors.prior[quiz];
    double Z = 0.0, FW = 0.0, Etot = 0.0;   // (thread 0's)
    {   // E = sum_t p_t g_q(t)
      double acc = 0.0;
      for (int64_t t0 = (int64_t)tid * V; t0 < a.T; t0 += (int64_t)kGainThreads * V) {
        double d[V], inv[V], s[V], F[V], p[V];
        GainVec<E>::load(block + (int64_t)K * ldT, t0, d);
        const uint32_t gap = gain_gap_bits(a.tgap, t0);
#pragma unroll
        for (int e = 0; e < V; e++) { inv[e] = div_nr(1.0, d[e]); s[e] = 0.0; F[e] = 0.0; }
        for (int k = 0; k < K; k++) {
          double v[V];
          GainVec<E>::load(block + (int64_t)k * ldT, t0, v);
#pragma unroll
          for (int e = 0; e < V; e++) {
            const double x = v[e] * inv[e];
            s[e] += x;
            F[e] += gain_f(x);
          }
        }
        gain_load_p<V>(prior, t0, gap, p);
#pragma unroll
        for (int e = 0; e < V; e++) acc = fma(p[e], ((gap >> e) & 1u) ? 0.0 : gain_f(s[e]) - F[e], acc);
      }
      const double sum = wave_sum(acc);
      if (lane == 0) part[wave][0] = sum;
      __syncthreads();
      if (tid == 0) {
        Etot = part[0][0];
#pragma unroll
        for (int x = 1; x < kGainWaves; x++) Etot += part[x][0];
      }
      __syncthreads();
    }
    for (int k0 = 0; k0 < K; k0 += kGainPiece) {
      double acc[kGainPiece];
#pragma unroll
      for (int x = 0; x < kGainPiece; x++) acc[x] = 0.0;
      for (int64_t t0 = (int64_t)tid * V; t0 < a.T; t0 += (int64_t)kGainThreads * V) {
        double d[V], p[V], v[kGainPiece][V];
        GainVec<E>::load(block + (int64_t)K * ldT, t0, d);
#pragma unroll
        for (int x = 0; x < kGainPiece; x++) GainVec<E>::load(block + (int64_t)(k0 + x < K ? k0 + x : K - 1) * ldT, t0, v[x]);   // (past the last answer: read, not used)
        const uint32_t gap = gain_gap_bits(a.tgap, t0);
        gain_load_p<V>(prior, t0, gap, p);
#pragma unroll
        for (int e = 0; e < V; e++) {
          const double inv = div_nr(1.0, d[e]);
          const bool off = (gap >> e) & 1u;
#pragma unroll
          for (int x = 0; x < kGainPiece; x++) acc[x] = fma(p[e], off ? 0.0 : v[x][e] * inv, acc[x]);
        }
      }
#pragma unroll
      for (int x = 0; x < kGainPiece; x++) {
        const double s = wave_sum(acc[x]);
        if (lane == 0) part[wave][x] = s;
      }
      __syncthreads();
      if (tid == 0) {
        for (int x = 0; x < kGainPiece && k0 + x < K; x++) {
          double w = part[0][x];
#pragma unroll
          for (int y = 1; y < kGainWaves; y++) w += part[y][x];
          Z += w;
          FW += gain_f(w);
        }
      }
      __syncthreads();
    }
    if (tid == 0) a.rows[(int64_t)quiz * a.rowPitch + q] = gain_value(Z, FW, Etot);
  }
}

__global__ __launch_bounds__(256) void gain_slots_kernel(QuizSlot *slots, double *rows, int64_t rowPitch, GainAsked asked, int n) {
  const int i = threadIdx.x;
  if (i >= n) return;
  QuizSlot s{};
  s.priority = rows + (int64_t)i * rowPitch;
  s.asked = asked.asked[i];
  slots[i] = s;
}

constexpr int64_t kGainMaxWorkgroups = 1 << 22;   // of a launch
constexpr int64_t kGainGenericWorkgroups = 8192;

template <typename E, int K, int NQ>
hipError_t launch_tiles(GainSweep a, const TopBatchPriors &priors, int first, int nTiles, hipStream_t stream) {
  const int64_t tilesPer = a.Q >= kGainMaxWorkgroups ? 1 : std::min<int64_t>(nTiles, kGainMaxWorkgroups / a.Q);
  const int64_t qPer = std::min<int64_t>(a.Q, kGainMaxWorkgroups / tilesPer);
  for (int64_t t = 0; t < nTiles; t += tilesPer) {
    a.first = first + (int)t * NQ;
    a.nTiles = (int)std::min<int64_t>(tilesPer, nTiles - t);
    for (int64_t q = 0; q < a.Q; q += qPer) {
      a.qBase = q;
      a.qCount = std::min<int64_t>(qPer, a.Q - q);
      hipLaunchKernelGGL((gain_sweep_kernel<E, K, NQ>), dim3((unsigned)(a.qCount * a.nTiles)), dim3(kGainThreads), 0, stream, a, priors);
    }
  }
  return hipGetLastError();
}

// a lone quiz takes the narrow instantiation; every other call tiles of GainTileWidth(K), the last one filled with repeats
template <typename E, int K>
hipError_t launch_sweep(const GainSweep &a, const TopBatchPriors &priors, hipStream_t stream) {
  constexpr int W = GainTileWidth(K);
  if (a.n == 1) return launch_tiles<E, K, 1>(a, priors, 0, 1, stream);
  return launch_tiles<E, K, W>(a, priors, 0, (a.n + W - 1) / W, stream);
}

template <typename E>
hipError_t launch_sweep_any(const GainSweep &a, const TopBatchPriors &priors, hipStream_t stream) {
  switch (a.K) {
    case 2: return launch_sweep<E, 2>(a, priors, stream);
    case 3: return launch_sweep<E, 3>(a, priors, stream);
    case 4: return launch_sweep<E, 4>(a, priors, stream);
    case 5: return launch_sweep<E, 5>(a, priors, stream);
    default: break;
  }
  hipLaunchKernelGGL((gain_sweep_generic_kernel<E>), dim3((unsigned)std::min<int64_t>(a.Q * a.n, kGainGenericWorkgroups)), dim3(kGainThreads), 0, stream, a, priors);
  return hipGetLastError();
}

}  // namespace

hipError_t LaunchQuestionGains(const KbView &kb, const TopBatchPriors &priors, int64_t nQuizzes, double *rows, int64_t rowPitch, hipStream_t stream) {
  if (nQuizzes <= 0) return hipSuccess;
  if (nQuizzes > kTopBatchQuizzes || rows == nullptr || rowPitch < kb.Q || (kb.elem != 8 && kb.elem != 4) || kb.K < 2 || kb.K > 32767 || kb.Q < 1 || kb.T < 1 ||
      kb.ldT < ((kb.T + 3) & ~(int64_t)3) || kb.ldT % 4 != 0)
    return hipErrorInvalidValue;
  for (int64_t i = 0; i < nQuizzes; i++)
    if (priors.prior[i] == nullptr || (reinterpret_cast<uintptr_t>(priors.prior[i]) & 15) != 0) return hipErrorInvalidValue;
  GainSweep a{kb.cube, kb.tgap, kb.qgap, rows, kb.Q, kb.K, kb.T, kb.ldT, rowPitch, 0, kb.Q, 0, 1, (int)nQuizzes};
  return kb.elem == 8 ? launch_sweep_any<double>(a, priors, stream) : launch_sweep_any<float>(a, priors, stream);
}

hipError_t LaunchGainSlots(QuizSlot *slots, double *rows, int64_t rowPitch, const GainAsked &asked, int64_t nQuizzes, hipStream_t stream) {
  if (nQuizzes <= 0 || nQuizzes > kTopBatchQuizzes || slots == nullptr || rows == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gain_slots_kernel, dim3(1), dim3(256), 0, stream, slots, rows, rowPitch, asked, (int)nQuizzes);
  return hipGetLastError();
}

}  // namespace pqa
