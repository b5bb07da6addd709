// redundancy_kernels.hip -- questions whose answers a given one predicts (include/PqaHipExt.h: PqaEngine_EvalQuestionRedundancy and
// its neighbours; host side: hip_engine_sources.cpp).
//
// With w[t] = vB[t] (0 at a gap target) and p_qk(t) = A[q][k][t] * (1 / D[q][t]), a source question s and a question q have the K x K
// table  J[k][k'] = sum_t (w[t] p_sk(t)) p_qk'(t)  and the mutual information of their answers, in bits,
//     I(s, q) = sum over J > 0 of (J / Z) log2(J Z / (r[k] c[k'])),   Z = sum J, r = row sums, c = column sums;  0 if Z == 0.
// The contraction is over the TARGETS, between the source's block and every other question's block.  Everything is fp64 whatever the
// cube's element type (a Float engine's elements are converted exactly).  Two steps:
//
//   red_weights_kernel  the K rows u_k[t] = w[t] * (A[s][k][t] * div_nr(1, D[s][t])) of every source THIS cube holds into the package:
//                       slot i = K rows of `pitch` doubles, 0 at gap targets and behind T, all 0 for a gap source.  Slots of sources
//                       other ranks hold are not touched (the ranks' packages are summed: one writer per slot).  With a flag, the pack
//                       kernels' protocol (kb_kernels.hip: pack_answer_rows_kernel): the workgroup that arrives last publishes.
//   red_sweep_kernel    one streaming pass over the cube per TILE of NS sources: a workgroup per (question, tile), the workgroups of a
//                       question next to each other in the grid, so that the tiles of a launch share the question's block in L2.  A
//                       lane takes 16 bytes of the D row and of each of the K A rows (two targets of a Double cube, four of a Float
//                       one), forms v_k'(t) = A * (1 / D) once per element -- 0 through a select at gap targets and behind T -- and
//                       runs NS K K fma chains against the tile's u rows, which come from the package (L2 / Infinity Cache: they are
//                       read once per question).  A wave reduction by DPP (wave_sum), the waves added in wave order through LDS, and
//                       one thread per (source, question) finishes: Z, r, c in index order, the sum in row-major order with the
//                       device's fp64 log2.  It writes 0 for a gap question, a gap source (its u rows are zeros: Z == 0) and, for
//                       the rows that go to the listing, at the source's own entry.
//   red_sweep_generic_kernel  answer counts without an instantiation: a workgroup per (question, source) walks the table in pieces of
//                       kRedPiece entries of a row, streaming the question's rows once per piece, and keeps the table in a scratch
//                       of its own in global memory.  The same element arithmetic and the same order of summation.
//
// No atomics on values.  I(s, q) is a function of block s, block q, vB, the target gaps and the package's pitch alone: a lane's
// accumulator sees its targets in ascending order, the lanes are added in wave_sum's fixed tree and the waves in wave order; none of
// it depends on the other sources of the call, the place of s in the call or in its tile, the tile's width, or where q falls in the
// grid or in a shard.
#include "pqa_device.h"
#include "pqa_kernels.h"

namespace pqa {

namespace {

constexpr int kRedThreads = 256, kRedWaves = kRedThreads / kWave;
constexpr int kRedPiece = 4;   // table entries of a row per pass of the generic sweep

template <typename E> struct RedVec;
template <> struct RedVec<double> {
  static constexpr int V = 2;
  static __device__ __forceinline__ void load(const double *row, int64_t t0, double (&v)[2]) {
    const double2 x = *reinterpret_cast<const double2 *>(row + t0);
    v[0] = x.x; v[1] = x.y;
  }
};
template <> struct RedVec<float> {
  static constexpr int V = 4;
  static __device__ __forceinline__ void load(const float *row, int64_t t0, double (&v)[4]) {
    const float4 x = *reinterpret_cast<const float4 *>(row + t0);
    v[0] = (double)x.x; v[1] = (double)x.y; v[2] = (double)x.z; v[3] = (double)x.w;
  }
};
template <int V>
__device__ __forceinline__ void red_load_u(const double *row, int64_t t0, double (&u)[V]) {
#pragma unroll
  for (int e = 0; e < V; e += 2) {
    const double2 x = *reinterpret_cast<const double2 *>(row + t0 + e);
    u[e] = x.x; u[e + 1] = x.y;
  }
}

template <typename E>
__global__ __launch_bounds__(256) void red_weights_kernel(const E *__restrict__ cube, const double *__restrict__ vB, const uint32_t *__restrict__ tgap,
                                                          const uint32_t *__restrict__ qgap, const int64_t *__restrict__ sources, int64_t nWork, int64_t qFirst,
                                                          int64_t Q, int64_t K, int64_t T, int64_t ldT, int64_t pitch, double *dst, unsigned *counter,
                                                          unsigned expected, uint64_t *flag, uint64_t flagValue) {
  const int64_t t = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x), k = blockIdx.y, i = blockIdx.z;
  if (i < nWork && t < pitch) {   // (pitch is even)
    const int64_t s = sources[i] - qFirst;
    if (s >= 0 && s < Q) {
      double2 out{0.0, 0.0};
      if (!bit_test(qgap, s)) {
        const E *a = cube + (s * (K + 1) + k) * ldT, *d = cube + (s * (K + 1) + K) * ldT;
        if (t < T && !bit_test(tgap, t)) out.x = vB[t] * ((double)a[t] * div_nr(1.0, (double)d[t]));
        if (t + 1 < T && !bit_test(tgap, t + 1)) out.y = vB[t + 1] * ((double)a[t + 1] * div_nr(1.0, (double)d[t + 1]));
      }
      *reinterpret_cast<double2 *>(dst + (i * K + k) * pitch + t) = out;
    }
  }
  if (flag == nullptr) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope: this thread's part of the slots before the count
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != expected - 1) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  __hip_atomic_store(flag, flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct RedSweep {
  const void *cube;
  const uint32_t *tgap, *qgap;
  const double *weights;    // [source of the call][K][pitch]
  const int64_t *sources;   // GLOBAL ids of the call's sources
  double *rows;             // [source of the call][rowPitch]
  int64_t Q, K, ldT, pitch, rowPitch, qFirst;
  int64_t qBase, qCount;    // this launch's questions
  int first, nTiles;        // this launch's sources: nTiles tiles from source `first`
  int zeroSelf;
};

// One (source, question): the table's mutual information in bits.  Z, r and c in index order, then row-major.
__device__ double red_finish(const double *J, int K) {
  double Z = 0.0;
  for (int e = 0; e < K * K; e++) Z += J[e];
  if (!(Z > 0.0)) return 0.0;
  double I = 0.0;
  for (int k = 0; k < K; k++) {
    double r = 0.0;
    for (int j = 0; j < K; j++) r += J[k * K + j];
    for (int j = 0; j < K; j++) {
      const double v = J[k * K + j];
      if (!(v > 0.0)) continue;
      double c = 0.0;
      for (int kk = 0; kk < K; kk++) c += J[kk * K + j];
      I += (v / Z) * log2(v * Z / (r * c));
    }
  }
  return I;
}

// (t0 is a multiple of V <= 4: the V bits lie in one word)
__device__ __forceinline__ uint32_t red_gap_bits(const uint32_t *__restrict__ tgap, int64_t t0) { return tgap[t0 >> 5] >> (t0 & 31); }

template <typename E, int K, int NS>
__global__ __launch_bounds__(kRedThreads) void red_sweep_kernel(RedSweep a) {
  constexpr int V = RedVec<E>::V, N = NS * K * K;
  __shared__ double part[kRedWaves][N];
  __shared__ double table[N];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int64_t q = a.qBase + blockIdx.x / a.nTiles;
  const int src0 = a.first + (int)(blockIdx.x % a.nTiles) * NS;
  if (bit_test(a.qgap, q)) {
    if (tid < NS) a.rows[(int64_t)(src0 + tid) * a.rowPitch + q] = 0.0;
    return;
  }
  const int64_t ldT = a.ldT, pitch = a.pitch;
  const E *block = static_cast<const E *>(a.cube) + q * (K + 1) * ldT;
  const double *w = a.weights + (int64_t)src0 * K * pitch;
  double acc[N];
#pragma unroll
  for (int e = 0; e < N; e++) acc[e] = 0.0;
  for (int64_t t0 = (int64_t)tid * V; t0 < pitch; t0 += (int64_t)kRedThreads * V) {
    double d[V], v[K][V];
    RedVec<E>::load(block + K * ldT, t0, d);
#pragma unroll
    for (int j = 0; j < K; j++) RedVec<E>::load(block + j * ldT, t0, v[j]);
    const uint32_t g = red_gap_bits(a.tgap, t0);
#pragma unroll
    for (int e = 0; e < V; e++) {
      const double inv = div_nr(1.0, d[e]);
      const bool off = (g >> e) & 1u;
#pragma unroll
      for (int j = 0; j < K; j++) v[j][e] = off ? 0.0 : v[j][e] * inv;
    }
#pragma unroll
    for (int i = 0; i < NS; i++) {
#pragma unroll
      for (int k = 0; k < K; k++) {
        double u[V];
        red_load_u<V>(w + (int64_t)(i * K + k) * pitch, t0, u);
#pragma unroll
        for (int j = 0; j < K; j++) {
#pragma unroll
          for (int e = 0; e < V; e++) acc[(i * K + k) * K + j] = fma(u[e], v[j][e], acc[(i * K + k) * K + j]);
        }
      }
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
    for (int x = 1; x < kRedWaves; x++) s += part[x][tid];
    table[tid] = s;
  }
  __syncthreads();
  if (tid < NS) {
    double I = red_finish(table + tid * K * K, K);
    if (a.zeroSelf && a.sources[src0 + tid] == a.qFirst + q) I = 0.0;
    a.rows[(int64_t)(src0 + tid) * a.rowPitch + q] = I;
  }
}

// Any answer count: workgroup w of the grid takes the (question, source) pairs w, w + gridDim.x, ... of the launch and keeps the
// table of the pair at hand in its own K K doubles of `tables`.
template <typename E>
__global__ __launch_bounds__(kRedThreads) void red_sweep_generic_kernel(RedSweep a, int m, double *tables) {
  constexpr int V = RedVec<E>::V;
  __shared__ double part[kRedWaves][kRedPiece];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int K = (int)a.K;
  const int64_t ldT = a.ldT, pitch = a.pitch;
  double *table = tables + (int64_t)blockIdx.x * K * K;
  for (int64_t work = blockIdx.x; work < a.qCount * m; work += gridDim.x) {
    const int64_t q = a.qBase + work / m;
    const int src = a.first + (int)(work % m);
    if (bit_test(a.qgap, q)) {
      if (tid == 0) a.rows[(int64_t)src * a.rowPitch + q] = 0.0;
      continue;
    }
    const E *block = static_cast<const E *>(a.cube) + q * (K + 1) * ldT;
    const double *w = a.weights + (int64_t)src * K * pitch;
    for (int k = 0; k < K; k++) {
      for (int j0 = 0; j0 < K; j0 += kRedPiece) {
        double acc[kRedPiece];
#pragma unroll
        for (int x = 0; x < kRedPiece; x++) acc[x] = 0.0;
        for (int64_t t0 = (int64_t)tid * V; t0 < pitch; t0 += (int64_t)kRedThreads * V) {
          double d[V], u[V], v[kRedPiece][V];
          RedVec<E>::load(block + (int64_t)K * ldT, t0, d);
#pragma unroll
          for (int x = 0; x < kRedPiece; x++) RedVec<E>::load(block + (int64_t)(j0 + x < K ? j0 + x : K - 1) * ldT, t0, v[x]);   // (past the row's end: read, not used)
          red_load_u<V>(w + (int64_t)k * pitch, t0, u);
          const uint32_t g = red_gap_bits(a.tgap, t0);
#pragma unroll
          for (int e = 0; e < V; e++) {
            const double inv = div_nr(1.0, d[e]);
            const bool off = (g >> e) & 1u;
#pragma unroll
            for (int x = 0; x < kRedPiece; x++) acc[x] = fma(u[e], off ? 0.0 : v[x][e] * inv, acc[x]);
          }
        }
#pragma unroll
        for (int x = 0; x < kRedPiece; x++) {
          const double s = wave_sum(acc[x]);
          if (lane == 0) part[wave][x] = s;
        }
        __syncthreads();
        if (tid < kRedPiece && j0 + tid < K) {
          double s = part[0][tid];
#pragma unroll
          for (int x = 1; x < kRedWaves; x++) s += part[x][tid];
          table[k * K + j0 + tid] = s;
        }
        __syncthreads();
      }
    }
    // (the table's entries were stored by threads 0 .. kRedPiece - 1 of this workgroup, in front of a barrier each)
    if (tid == 0) {
      double I = red_finish(table, K);
      if (a.zeroSelf && a.sources[src] == a.qFirst + q) I = 0.0;
      a.rows[(int64_t)src * a.rowPitch + q] = I;
    }
    __syncthreads();   // the table is the next pair's
  }
}

__global__ __launch_bounds__(256) void red_slots_kernel(QuizSlot *slots, double *rows, int64_t rowPitch, const uint32_t *qgap, int n) {
  const int i = threadIdx.x;
  if (i >= n) return;
  QuizSlot s{};
  s.priority = rows + (int64_t)i * rowPitch;
  s.asked = qgap;   // (a bitmap that is there: the listing tests it beside the gap bits, which it repeats)
  slots[i] = s;
}

constexpr int64_t kRedMaxWorkgroups = 1 << 22;   // of a launch

template <typename E, int K, int NS>
hipError_t launch_tiles(RedSweep a, int first, int nTiles, hipStream_t stream) {
  const int64_t tilesPer = a.Q >= kRedMaxWorkgroups ? 1 : std::min<int64_t>(nTiles, kRedMaxWorkgroups / a.Q);
  const int64_t qPer = std::min<int64_t>(a.Q, kRedMaxWorkgroups / tilesPer);
  for (int64_t t = 0; t < nTiles; t += tilesPer) {
    a.first = first + (int)t * NS;
    a.nTiles = (int)std::min<int64_t>(tilesPer, nTiles - t);
    for (int64_t q = 0; q < a.Q; q += qPer) {
      a.qBase = q;
      a.qCount = std::min<int64_t>(qPer, a.Q - q);
      hipLaunchKernelGGL((red_sweep_kernel<E, K, NS>), dim3((unsigned)(a.qCount * a.nTiles)), dim3(kRedThreads), 0, stream, a);
    }
  }
  return hipGetLastError();
}

// the wide tiles of the call's sources first, what is left over one source a tile
template <typename E, int K>
hipError_t launch_sweep(const RedSweep &a, int n, hipStream_t stream) {
  constexpr int W = RedundancyTileWidth(K);
  const int nWide = n / W;
  if (W > 1 && nWide > 0) {
    const hipError_t e = launch_tiles<E, K, W>(a, 0, nWide, stream);
    if (e != hipSuccess) return e;
  }
  const int done = W > 1 ? nWide * W : 0;
  if (n > done) return launch_tiles<E, K, 1>(a, done, n - done, stream);
  return hipSuccess;
}

template <typename E>
hipError_t launch_sweep_any(const RedSweep &a, int n, double *tables, hipStream_t stream) {
  switch (a.K) {
    case 2: return launch_sweep<E, 2>(a, n, stream);
    case 3: return launch_sweep<E, 3>(a, n, stream);
    case 4: return launch_sweep<E, 4>(a, n, stream);
    case 5: return launch_sweep<E, 5>(a, n, stream);
    default: break;
  }
  if (tables == nullptr) return hipErrorInvalidValue;
  RedSweep g = a;
  g.first = 0; g.nTiles = 1; g.qBase = 0; g.qCount = a.Q;
  const int64_t work = a.Q * n;
  hipLaunchKernelGGL((red_sweep_generic_kernel<E>), dim3((unsigned)std::min<int64_t>(work, kRedGenericWorkgroups)), dim3(kRedThreads), 0, stream, g, n, tables);
  return hipGetLastError();
}

}  // namespace

size_t RedundancyTableBytes(const KbView &kb) {
  return kb.K >= 2 && kb.K <= 5 ? 0 : (size_t)kRedGenericWorkgroups * (size_t)(kb.K * kb.K) * sizeof(double);
}

hipError_t LaunchQuestionWeights(const KbView &kb, const int64_t *sources, int64_t nSources, int64_t qFirst, double *dst, int64_t pitch, unsigned *counter,
                                 uint64_t *flag, uint64_t flagValue, hipStream_t stream) {
  if (nSources < 0 || nSources > kTopBatchQuizzes || pitch <= 0 || pitch % 16 != 0 || pitch > kb.ldT || pitch < kb.T || (kb.elem != 8 && kb.elem != 4) ||
      kb.K < 1 || kb.K > 65535 || kb.Q < 1 || (nSources > 0 && (sources == nullptr || dst == nullptr)) || (flag != nullptr && counter == nullptr))
    return hipErrorInvalidValue;
  if (nSources == 0 && flag == nullptr) return hipSuccess;
  const dim3 grid = nSources == 0 ? dim3(1) : dim3((unsigned)(((pitch >> 1) + 255) / 256), (unsigned)kb.K, (unsigned)nSources);
  const unsigned expected = grid.x * grid.y * grid.z;
  if (kb.elem == 8)
    hipLaunchKernelGGL(red_weights_kernel<double>, grid, dim3(256), 0, stream, static_cast<const double *>(kb.cube), kb.vB, kb.tgap, kb.qgap, sources, nSources, qFirst,
                       kb.Q, kb.K, kb.T, kb.ldT, pitch, dst, counter, expected, flag, flagValue);
  else
    hipLaunchKernelGGL(red_weights_kernel<float>, grid, dim3(256), 0, stream, static_cast<const float *>(kb.cube), kb.vB, kb.tgap, kb.qgap, sources, nSources, qFirst,
                       kb.Q, kb.K, kb.T, kb.ldT, pitch, dst, counter, expected, flag, flagValue);
  return hipGetLastError();
}

hipError_t LaunchRedundancySweep(const KbView &kb, const double *weights, int64_t pitch, const int64_t *sources, int64_t nSources, int64_t qFirst, bool zeroSelf,
                                 double *rows, int64_t rowPitch, double *tables, hipStream_t stream) {
  if (nSources <= 0) return hipSuccess;
  if (nSources > kTopBatchQuizzes || weights == nullptr || sources == nullptr || rows == nullptr || pitch <= 0 || pitch % 16 != 0 || pitch > kb.ldT || pitch < kb.T ||
      rowPitch < kb.Q || (kb.elem != 8 && kb.elem != 4) || kb.K < 2 || kb.K > 32767 || kb.Q < 1 || (reinterpret_cast<uintptr_t>(weights) & 15) != 0)
    return hipErrorInvalidValue;
  RedSweep a{kb.cube, kb.tgap, kb.qgap, weights, sources, rows, kb.Q, kb.K, kb.ldT, pitch, rowPitch, qFirst, 0, kb.Q, 0, 1, zeroSelf ? 1 : 0};
  return kb.elem == 8 ? launch_sweep_any<double>(a, (int)nSources, tables, stream) : launch_sweep_any<float>(a, (int)nSources, tables, stream);
}

hipError_t LaunchRedundancySlots(QuizSlot *slots, double *rows, int64_t rowPitch, const uint32_t *qgap, int64_t nSources, hipStream_t stream) {
  if (nSources <= 0 || nSources > kTopBatchQuizzes || slots == nullptr || rows == nullptr || qgap == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(red_slots_kernel, dim3(1), dim3(256), 0, stream, slots, rows, rowPitch, qgap, (int)nSources);
  return hipGetLastError();
}

}  // namespace pqa
