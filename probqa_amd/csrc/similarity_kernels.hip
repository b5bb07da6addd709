// similarity_kernels.hip -- targets that answer like a given one (include/PqaHipExt.h: PqaEngine_EvalTargetSimilarity and its
// neighbours; host side: hip_engine_sources.cpp).
//
// With p_qk(t) = A[q][k][t] / D[q][t] the similarity of a source s and a target t is the mean over the questions that are not gaps of
// the Bhattacharyya coefficient  BC_q(s, t) = sum_k sqrt(p_qk(s)) sqrt(p_qk(t)).  Every other sweep of the engine contracts a question's
// rows over the targets; this one contracts over (question, answer) and keeps the target axis: one streaming pass over the cube
// [Q][K + 1][ldT] per TILE of up to kSimTile sources.  Everything is fp64 whatever the cube's element type (a Float engine's elements
// are converted exactly).  Three kernels per tile:
//
//   sim_sources_kernel  RS[q][k][i] = sqrt(A[q][k][s_i] * div_nr(1, D[q][s_i])) into a compact scratch: 0 for a gap question, a gap
//                       source and the entries past the tile's sources, so that none of them needs a branch in the sweep.  Q K NS
//                       scattered reads against the sweep's Q (K + 1) ldT stream.
//   sim_sweep_kernel    grid (tiles of 2 * kSimThreads targets, chunks of questions); a lane owns two neighbouring targets (a 16-byte
//                       load of a Double row, 8 bytes of a Float row) and 2 NS accumulators.  A question's D row comes first: the
//                       lane's 1 / D, once; then per answer row r_t = sqrt(A * (1 / D)), once, and one fma per source with RS[q][k][i],
//                       which is the same for every lane (uniform addresses: scalar loads).  The A rows of a chunk are one sequence,
//                       question after question, walked through a ring of kSimAhead loads in flight, whatever K is; the D row of
//                       the next question is requested when a question begins.  The accumulators see no branch: gap targets, the
//                       columns from T on (their tgap bits are set), a gap question's rows and the ring's rows past the chunk's end
//                       contribute r = 0 through a select, without their elements being used.  Each chunk leaves
//                       partial[chunk][i][ldT].
//   sim_finish_kernel   the chunks added in chunk order into the package's slots, zeros at gaps and behind T up to the slot's pitch;
//                       with a flag, the pack kernels' protocol (kb_kernels.hip: pack_answer_rows_kernel) over ALL finishing launches
//                       of a call: the workgroup that arrives last of `expected` publishes.
//
// No atomics on values, no LDS, no barrier.  The value of (s, t) is a function of columns s and t alone: the element arithmetic is
// the same for every lane, a source's accumulator sees questions and answers in ascending order within a chunk and the chunks in
// ascending order, and the chunking (SimQuestionsPerChunk) depends on Q and ldT only -- not on the number of sources, a source's
// place in the call or in its tile, nor on the width NS the tile is instantiated with.
//
// sim_rows_kernel turns a (summed) package into rows: sum / nValidQuestions (IEEE division), 0 at gaps, and -- for the rows that go
// to the listing -- 0 at the source's own entry, which the listing's "<= 0 is no candidate" rule then drops.
#include "pqa_device.h"
#include "pqa_kernels.h"

namespace pqa {

namespace {

constexpr int kSimThreads = 128;   // two waves a workgroup: 256 targets
constexpr int kSimAhead = 4;       // row loads in flight per lane

__device__ __forceinline__ double2 sim_load(const double *row, int64_t p) { return reinterpret_cast<const double2 *>(row)[p]; }
__device__ __forceinline__ double2 sim_load(const float *row, int64_t p) {
  const float2 v = reinterpret_cast<const float2 *>(row)[p];
  return double2{(double)v.x, (double)v.y};
}

template <typename E, int NS>
__global__ __launch_bounds__(256) void sim_sources_kernel(const E *__restrict__ cube, const uint32_t *__restrict__ tgap, const uint32_t *__restrict__ qgap,
                                                          const int64_t *__restrict__ sources, int m, int64_t Q, int64_t K, int64_t ldT,
                                                          double *__restrict__ rs) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= Q * K * NS) return;
  const int i = (int)(idx % NS);
  const int64_t qk = idx / NS, q = qk / K, k = qk % K;
  double v = 0.0;
  if (i < m && !bit_test(qgap, q)) {
    const int64_t s = sources[i];
    if (!bit_test(tgap, s)) {
      const E *qBase = cube + q * (K + 1) * ldT;
      v = sqrt((double)qBase[k * ldT + s] * div_nr(1.0, (double)qBase[K * ldT + s]));
    }
  }
  rs[idx] = v;
}

struct SimSweep {
  const void *cube;
  const uint32_t *tgap, *qgap;
  const double *rs;        // [Q][K][NS]
  double *partial;         // [chunk][NS][ldT]
  int64_t Q, K, ldT, qPerChunk;
};

template <typename E, int NS>
__global__ __launch_bounds__(kSimThreads) void sim_sweep_kernel(SimSweep a) {
  const int64_t p = (int64_t)blockIdx.x * kSimThreads + threadIdx.x;   // targets 2 p, 2 p + 1
  if (p >= (a.ldT >> 1)) return;
  const int K = (int)a.K, rows = K + 1;
  const int64_t ldT = a.ldT;
  const int chunk = blockIdx.y, qFirst = chunk * (int)a.qPerChunk, qEnd = qFirst + a.qPerChunk < a.Q ? qFirst + (int)a.qPerChunk : (int)a.Q;
  const bool g0 = bit_test(a.tgap, 2 * p), g1 = bit_test(a.tgap, 2 * p + 1);
  const E *cube = static_cast<const E *>(a.cube);
  double acc0[NS], acc1[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) { acc0[i] = 0.0; acc1[i] = 0.0; }
  // Two streams.  The A rows of the chunk, question after question, are one sequence walked through a ring of kSimAhead loads; its
  // load-ahead position stays on the chunk's last row once it has reached it (read again, not used).  The D row of the NEXT question
  // is requested when a question begins.  The accumulators see no branch: a row past the chunk's end, a gap question's and a gap
  // target's contribute r = 0.
  const int N = (qEnd - qFirst) * K;
  int lq = qFirst, lk = 0;
  auto issue = [&]() -> double2 {
    const double2 v = sim_load(cube + (int64_t)(lq * rows + lk) * ldT, p);
    if (lk + 1 < K) lk++;
    else if (lq + 1 < qEnd) { lq++; lk = 0; }
    return v;
  };
  double2 ring[kSimAhead];
#pragma unroll
  for (int s = 0; s < kSimAhead; s++) ring[s] = issue();
  double2 dNext = sim_load(cube + (int64_t)(qFirst * rows + K) * ldT, p);
  int cq = qFirst, ck = 0;
  double inv0 = 0.0, inv1 = 0.0;
  bool off0 = true, off1 = true;
  for (int n = 0; n < N; n += kSimAhead) {
#pragma unroll
    for (int s = 0; s < kSimAhead; s++) {
      const int q = cq < qEnd ? cq : qEnd - 1;
      if (ck == 0) {   // a question begins: 1 / D of the lane's targets, and the next question's D row
        const bool dead = cq >= qEnd || bit_test(a.qgap, q);
        off0 = g0 || dead;
        off1 = g1 || dead;
        inv0 = div_nr(1.0, dNext.x);
        inv1 = div_nr(1.0, dNext.y);
        dNext = sim_load(cube + (int64_t)((q + 1 < qEnd ? q + 1 : q) * rows + K) * ldT, p);
      }
      const double2 v = ring[s];
      const double r0 = off0 ? 0.0 : sqrt(v.x * inv0), r1 = off1 ? 0.0 : sqrt(v.y * inv1);
      const double *__restrict__ rs = a.rs + (int64_t)(q * K + ck) * NS;
#pragma unroll
      for (int i = 0; i < NS; i++) {
        const double w = rs[i];
        acc0[i] = fma(r0, w, acc0[i]);
        acc1[i] = fma(r1, w, acc1[i]);
      }
      ring[s] = issue();
      if (++ck == K) { ck = 0; cq++; }
    }
  }
  double *out = a.partial + (int64_t)chunk * NS * ldT + 2 * p;
#pragma unroll
  for (int i = 0; i < NS; i++) *reinterpret_cast<double2 *>(out + (int64_t)i * ldT) = double2{acc0[i], acc1[i]};
}

// workgroup (256 pairs of a slot's pitch, source of the tile)
__global__ __launch_bounds__(256) void sim_finish_kernel(const double *__restrict__ partial, int64_t nChunks, int NS, int64_t ldT, int64_t nWork,
                                                         const uint32_t *__restrict__ tgap, int64_t T, int64_t pitch, double *dst, unsigned *counter,
                                                         unsigned expected, uint64_t *flag, uint64_t flagValue) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (i < nWork && 2 * u < pitch) {
    const int64_t t = 2 * u;   // (pitch <= ldT: both multiples of 16)
    double2 s = *reinterpret_cast<const double2 *>(partial + i * ldT + t);
    for (int64_t c = 1; c < nChunks; c++) {
      const double2 v = *reinterpret_cast<const double2 *>(partial + (c * NS + i) * ldT + t);
      s.x += v.x;
      s.y += v.y;
    }
    if (t >= T || bit_test(tgap, t)) s.x = 0.0;
    if (t + 1 >= T || bit_test(tgap, t + 1)) s.y = 0.0;
    *reinterpret_cast<double2 *>(dst + i * pitch + t) = s;
  }
  if (flag == nullptr) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope: this thread's part of the slots before the count
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != expected - 1) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  __hip_atomic_store(flag, flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(256) void sim_rows_kernel(const double *__restrict__ sums, int64_t pitch, const int64_t *__restrict__ sources, int zeroSelf,
                                                       const uint32_t *__restrict__ tgap, int64_t T, double nValid, double *__restrict__ rows) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (t >= pitch) return;
  double v = 0.0;
  if (t < T && nValid > 0.0 && !bit_test(tgap, t) && !(zeroSelf && t == sources[i])) v = sums[i * pitch + t] / nValid;
  rows[i * pitch + t] = v;
}

constexpr int sim_tile_width(int m) { return m <= kSimTileSmall ? kSimTileSmall : kSimTile; }

template <typename E, int NS>
hipError_t launch_tile(const KbView &kb, const int64_t *sources, int m, double *rs, double *partial, int64_t qPerChunk, int64_t nChunks, hipStream_t stream) {
  const int64_t nRS = kb.Q * kb.K * NS;
  hipLaunchKernelGGL((sim_sources_kernel<E, NS>), dim3((unsigned)((nRS + 255) / 256)), dim3(256), 0, stream, static_cast<const E *>(kb.cube), kb.tgap, kb.qgap,
                     sources, m, kb.Q, kb.K, kb.ldT, rs);
  SimSweep a{kb.cube, kb.tgap, kb.qgap, rs, partial, kb.Q, kb.K, kb.ldT, qPerChunk};
  const int64_t tiles = ((kb.ldT >> 1) + kSimThreads - 1) / kSimThreads;
  hipLaunchKernelGGL((sim_sweep_kernel<E, NS>), dim3((unsigned)tiles, (unsigned)nChunks), dim3(kSimThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

// Questions per chunk of the sweep: about 2048 workgroups of two waves (two rounds at the wide tile's two waves a SIMD) where the cube
// has them, and never fewer than 16 questions a chunk, so that the partial sums stay a fraction of the cube.  A function of Q and ldT.
int64_t SimQuestionsPerChunk(int64_t Q, int64_t ldT) {
  const int64_t tiles = ((ldT >> 1) + kSimThreads - 1) / kSimThreads;
  const int64_t wanted = (2048 + tiles - 1) / tiles;
  const int64_t per = (Q + wanted - 1) / wanted;
  return per < 16 ? 16 : per;
}
int64_t SimChunks(int64_t Q, int64_t ldT) {
  const int64_t per = SimQuestionsPerChunk(Q, ldT);
  return Q <= 0 ? 1 : (Q + per - 1) / per;
}
size_t SimSourceScratchBytes(const KbView &kb) { return (size_t)kb.Q * (size_t)kb.K * kSimTile * sizeof(double); }
size_t SimPartialBytes(const KbView &kb) { return (size_t)SimChunks(kb.Q, kb.ldT) * kSimTile * (size_t)kb.ldT * sizeof(double); }

hipError_t LaunchSimilaritySums(const KbView &kb, const int64_t *sources, int64_t nSources, double *rs, double *partial, double *dst, int64_t pitch,
                                unsigned *counter, uint64_t *flag, uint64_t flagValue, hipStream_t stream) {
  if (nSources < 0 || pitch <= 0 || pitch % 16 != 0 || pitch > kb.ldT || pitch < kb.T || (kb.elem != 8 && kb.elem != 4) || (kb.ldT & 15) != 0 || kb.Q < 1 ||
      (nSources > 0 && (sources == nullptr || rs == nullptr || partial == nullptr || dst == nullptr)) || (flag != nullptr && counter == nullptr))
    return hipErrorInvalidValue;
  if (nSources == 0 && flag == nullptr) return hipSuccess;
  const int64_t qPerChunk = SimQuestionsPerChunk(kb.Q, kb.ldT), nChunks = SimChunks(kb.Q, kb.ldT);
  const unsigned finishX = (unsigned)(((pitch >> 1) + 255) / 256);
  const unsigned expected = nSources == 0 ? 1u : finishX * (unsigned)nSources;
  if (nSources == 0) {   // (a flag alone)
    hipLaunchKernelGGL(sim_finish_kernel, dim3(1), dim3(256), 0, stream, partial, nChunks, kSimTile, kb.ldT, (int64_t)0, kb.tgap, kb.T, pitch, dst, counter, expected,
                       flag, flagValue);
    return hipGetLastError();
  }
  for (int64_t first = 0; first < nSources; first += kSimTile) {
    const int m = (int)(nSources - first < kSimTile ? nSources - first : kSimTile);
    const int NS = sim_tile_width(m);
    hipError_t e;
    if (kb.elem == 8) e = NS == kSimTile ? launch_tile<double, kSimTile>(kb, sources + first, m, rs, partial, qPerChunk, nChunks, stream)
                                         : launch_tile<double, kSimTileSmall>(kb, sources + first, m, rs, partial, qPerChunk, nChunks, stream);
    else e = NS == kSimTile ? launch_tile<float, kSimTile>(kb, sources + first, m, rs, partial, qPerChunk, nChunks, stream)
                            : launch_tile<float, kSimTileSmall>(kb, sources + first, m, rs, partial, qPerChunk, nChunks, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sim_finish_kernel, dim3(finishX, (unsigned)m), dim3(256), 0, stream, partial, nChunks, NS, kb.ldT, (int64_t)m, kb.tgap, kb.T, pitch,
                       dst + first * pitch, counter, expected, flag, flagValue);
  }
  return hipGetLastError();
}

hipError_t LaunchSimilarityRows(const KbView &kb, const double *sums, int64_t pitch, const int64_t *sources, int64_t nSources, bool zeroSelf, int64_t nValidQuestions,
                                double *rows, hipStream_t stream) {
  if (nSources <= 0) return hipSuccess;
  if (sums == nullptr || rows == nullptr || sources == nullptr || pitch < kb.T) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sim_rows_kernel, dim3((unsigned)((pitch + 255) / 256), (unsigned)nSources), dim3(256), 0, stream, sums, pitch, sources, zeroSelf ? 1 : 0, kb.tgap,
                     kb.T, (double)nValidQuestions, rows);
  return hipGetLastError();
}

}  // namespace pqa
