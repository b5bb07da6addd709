// among_kernels.hip -- the sweep over a LIST of (quiz, question) pairs, and the small kernels around it (the Among calls of
// include/PqaHipExt.h; host side: hip_engine_among.cpp).
//
// Every other sweep of the engine walks the whole question axis.  eval_listed_kernel walks a list: pair i names a slot b of the
// batch's QuizSlot[] and a local question q, and the workgroup that takes it evaluates question q for quiz b and stores the priority
// to slots[b].priority[q] -- the cost of a call follows its list, not Q.  The element arithmetic is the streaming sweep's
// (eval_kernels.hip: eval_questions_f64_stream) and the fp64 re-rank's (batch_rerank_kernel): (A * div_nr(1, D)) * prior with gaps
// masked, per-lane Kahan pairs, wave_sum / row_sum, pass2_pair, eval_epilogue -- in fp64 whatever the cube's element type (a Float
// engine's rows are converted exactly).  Rows are re-read by pass 2 (from L2 / the Infinity Cache where they fit): the register-ring
// sweeps, which keep a row on chip, are the cheaper way to evaluate EVERY question.
//
// Shape.  grid.x indexes the pairs with a grid stride: a workgroup copies the Log2Hot table (16 KiB) into LDS once and then takes
// pair after pair, so a launch of hundreds of thousands of pairs copies the table once per resident workgroup, not once per pair.
// WPQ waves share a pair: two for rows of up to 2048 elements (1000 targets are 504 pairs of doubles: four strided steps a lane and
// pass, one barrier per row between two waves), four beyond (DESIGN.md has the compiler's resource report for both).  A pair that is
// another shard's (q < 0), a gap or an asked question costs its workgroup one look.
//
// E = double with a pole list: the watch of eval_questions_f64_stream (pole_device.h: kQuarterShare, kNearOneShare, kSmallV), the
// question's sums stored by list position as W_k | W_k sqrt(V_k) | sum l log2 p | lack, and pole_fixup_kernel behind the launch
// (bySlot, the quizzes' own vectors) stores the corrected priority where this kernel stored its own.
#include "pqa_device.h"
#include "eval_device.h"
#include "pqa_kernels.h"
#include "pole_device.h"

namespace pqa {

static __device__ double gLog2TableA[kLog2TableDoubles];   // this translation unit's copy of the Log2Hot table
hipError_t UploadLog2TableAmong(const double *hostTable) {
  return hipMemcpyToSymbol(HIP_SYMBOL(gLog2TableA), hostTable, kLog2TableDoubles * sizeof(double));
}

namespace {

struct ListedArgs {
  const void *cube;
  const uint32_t *tgap, *qgap;
  const QuizSlot *slots;
  const ListedPair *pairs;
  int64_t nPairs, K, ldT;
  double vCompTail;
  PoleHeader *poleList;   // null: no watch
  double *poleSums;       // [entry][2 K + 2]
};

// elements 2 p, 2 p + 1 of a row as doubles (fp32 -> fp64 is exact)
__device__ __forceinline__ double2 load_pair(const double *row, int64_t p) { return reinterpret_cast<const double2 *>(row)[p]; }
__device__ __forceinline__ double2 load_pair(const float *row, int64_t p) {
  const float2 v = reinterpret_cast<const float2 *>(row)[p];
  return double2{(double)v.x, (double)v.y};
}

constexpr size_t listed_lds_bytes(int wpq, int64_t K) {   // table | W exchange [2][WPQ] | W_k [K] | partials [K + 2][WPQ] | watch words
  return ((size_t)kLog2TableDoubles + 2 * (size_t)wpq + (size_t)K + (size_t)(K + 2) * wpq + 1) * sizeof(double);
}

template <typename E, int WPQ>
__global__ __launch_bounds__(WPQ * 64) void eval_listed_kernel(ListedArgs a) {
  constexpr int kThreads = WPQ * kWave;
  extern __shared__ double smem[];
  const int64_t ldT = a.ldT, K = a.K;
  double *tbl = smem;
  if (!lds_table_at_zero(tbl)) __builtin_trap();  // log2hot addresses the table absolutely
  double *redW = tbl + kLog2TableDoubles;
  double *wk = redW + 2 * WPQ;
  double *part = wk + K;
  const int nPart = (int)(K + 2);
  uint32_t *watchWords = reinterpret_cast<uint32_t *>(part + nPart * WPQ);   // the rows that passed the pole watch [0], its wider form [1]
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  for (int i = tid; i < kLog2TableDoubles; i += kThreads) tbl[i] = gLog2TableA[i];
  if (tid < 2) watchWords[tid] = 0;
  __syncthreads();
  const E *cube = static_cast<const E *>(a.cube);
  const int64_t qStride = (K + 1) * ldT;
  const int64_t nPairs = ldT >> 1;
  const bool watch = a.poleList != nullptr;
  int phase = 0;
  for (int64_t i = blockIdx.x; i < a.nPairs; i += gridDim.x) {
    const ListedPair lp = a.pairs[i];
    if (lp.q < 0) continue;                                    // (another shard's question)
    const QuizSlot s = a.slots[lp.b];
    const int64_t q = lp.q;
    if (bit_test(a.qgap, q) || bit_test(s.asked, q)) {
      if (tid == 0) s.priority[q] = 0.0;
      continue;
    }
    const E *qBase = cube + q * qStride;
    const E *rowD = qBase + K * ldT;
    const double2 *prior2 = reinterpret_cast<const double2 *>(s.prior);
    double accL = 0, hW = 0;
    uint32_t poleRows = 0, quarterRows = 0;
    for (int64_t k = 0; k < K; k++) {
      const E *rowA = qBase + k * ldT;
      double s0 = 0, c0 = 0, s1 = 0, c1 = 0;
      for (int64_t p = tid; p < nPairs; p += kThreads) {
        const bool g0 = bit_test(a.tgap, 2 * p), g1 = bit_test(a.tgap, 2 * p + 1);
        const double2 d = load_pair(rowD, p), av = load_pair(rowA, p), pv = prior2[p];
        const double x0 = g0 ? 0.0 : (av.x * div_nr(1.0, d.x)) * pv.x;
        const double x1 = g1 ? 0.0 : (av.y * div_nr(1.0, d.y)) * pv.y;
        { const double y = x0 - c0; const double t = s0 + y; c0 = (t - s0) - y; s0 = t; }
        { const double y = x1 - c1; const double t = s1 + y; c1 = (t - s1) - y; s1 = t; }
      }
      const double sLane = (s0 - c0) + (s1 - c1);
      double Wk = wave_sum(sLane);
      if constexpr (WPQ > 1) {
        double *buf = redW + phase * WPQ;
        if (lane == 0) buf[wave] = Wk;
        __syncthreads();
        Wk = row_sum<WPQ>(buf[lane % WPQ]);
        phase ^= 1;
      }
      // the pole watch (eval_kernels.hip: sweep_body): a lane that holds a quarter / nearly all of W_k
      if (watch && __any(sLane > Wk * kQuarterShare)) {
        quarterRows |= 1u << (k < 31 ? (int)k : 31);
        if (__any(sLane >= Wk * kNearOneShare)) poleRows |= 1u << (k < 31 ? (int)k : 31);
      }
      const double invWk = div_nr(1.0, Wk);
      double v = 0;
      for (int64_t p = tid; p < nPairs; p += kThreads) {
        const bool g0 = bit_test(a.tgap, 2 * p), g1 = bit_test(a.tgap, 2 * p + 1);
        const double2 d = load_pair(rowD, p), av = load_pair(rowA, p);
        double2 pv = prior2[p], id, lh;
        id.x = g0 ? 0.0 : div_nr(1.0, d.x);
        id.y = g1 ? 0.0 : div_nr(1.0, d.y);
        pv.x = g0 ? 0.0 : pv.x;
        pv.y = g1 ? 0.0 : pv.y;
        lh.x = (av.x * id.x) * pv.x;
        lh.y = (av.y * id.y) * pv.y;
        pass2_pair(lh, id, pv, invWk, tbl, hW, v, accL);
      }
      v = wave_sum(v);
      if (lane == 0) {
        if (wave == 0) wk[k] = Wk;
        part[k * WPQ + wave] = v;
      }
    }
    hW = wave_sum(hW);
    accL = wave_sum(accL);
    if (lane == 0) {
      part[K * WPQ + wave] = hW;
      part[(K + 1) * WPQ + wave] = accL;
      if (quarterRows != 0) { atomicOr(&watchWords[1], quarterRows); if (poleRows != 0) atomicOr(&watchWords[0], poleRows); }
    }
    __syncthreads();
    if (tid == 0) {
      for (int r = 0; r < nPart; r++) {
        double acc = part[r * WPQ];
        for (int w2 = 1; w2 < WPQ; w2++) acc += part[r * WPQ + w2];
        if (r < K && acc <= kSmallV && ((watchWords[1] >> (r < 31 ? r : 31)) & 1u)) watchWords[0] |= 1u << (r < 31 ? r : 31);   // (a vanishing velocity sum: pole_device.h)
        part[r] = r < K ? wk[r] * sqrt(acc) : acc;
      }
      s.priority[q] = eval_epilogue(wk, -part[K], part, K, part[K + 1], a.vCompTail);
      if (watch && watchWords[0] != 0) {
        // the pair's sums as they are, for the fix behind the launch (pole_kernels.hip): by list position
        const uint32_t at = pole_list_append(a.poleList, (uint32_t)q, K <= 31 ? watchWords[0] : 0u, (uint32_t)lp.b);
        double *ps = a.poleSums + (int64_t)at * (2 * K + 2);
        for (int r = 0; r < K; r++) { ps[r] = wk[r]; ps[K + r] = part[r]; }
        ps[2 * K] = part[K];
        ps[2 * K + 1] = part[K + 1];
      }
      watchWords[0] = 0;
      watchWords[1] = 0;
    }
    __syncthreads();   // (part, wk and the watch words are the next pair's)
  }
}

// out[i] = the priority the sweep (and the fix behind it) left for pair i; 0 for another shard's question
__global__ __launch_bounds__(256) void listed_gather_kernel(const QuizSlot *__restrict__ slots, const ListedPair *__restrict__ pairs, int64_t nPairs,
                                                            double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nPairs) return;
  const ListedPair lp = pairs[i];
  out[i] = lp.q < 0 ? 0.0 : slots[lp.b].priority[lp.q];
}

// blockIdx.x = quiz: the best of its listed questions -- maximum priority, lowest question on ties, NaN never wins; gaps, asked
// questions and other shards' questions are not candidates.  The record, then the flag, to the slot's host-coherent cells.
struct ListedBest { double p; int64_t i; };
__device__ __forceinline__ void listed_merge(ListedBest &b, double op, int64_t oi) {
  if (oi >= 0 && (b.i < 0 || op > b.p || (op == b.p && oi < b.i))) { b.p = op; b.i = oi; }
}
__global__ __launch_bounds__(256) void listed_argmax_kernel(const QuizSlot *__restrict__ slots, const uint32_t *__restrict__ qgap,
                                                            const int64_t *__restrict__ offsets, const ListedPair *__restrict__ pairs, int64_t outBase,
                                                            uint64_t flagValue) {
  __shared__ ListedBest wb[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const QuizSlot s = slots[b];
  ListedBest best{0.0, -1};
  for (int64_t i = offsets[b] + tid; i < offsets[b + 1]; i += 256) {
    const int64_t q = pairs[i].q;
    if (q < 0 || bit_test(qgap, q) || bit_test(s.asked, q)) continue;
    double p = s.priority[q];
    if (p != p) p = -__builtin_huge_val();
    listed_merge(best, p, q);
  }
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    const double op = __shfl_xor(best.p, m, kWave);
    const int64_t oi = __shfl_xor(best.i, m, kWave);
    listed_merge(best, op, oi);
  }
  if (lane == 0) wb[wave] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; w++) listed_merge(best, wb[w].p, wb[w].i);
    host_publish(s.out, best.i < 0 ? 0.0 : best.p, best.i < 0 ? -1 : best.i + outBase, s.seq, flagValue);
  }
}

template <typename E, int WPQ>
hipError_t launch_listed(const ListedArgs &args, hipStream_t stream) {
  const size_t shmem = listed_lds_bytes(WPQ, args.K);
  if (shmem > kLdsPerCU) return hipErrorInvalidValue;
  static LaunchCache cache;
  const int dev = DeviceSlot();
  int perCU = 0;
  const hipError_t e = cache.Residency(dev, eval_listed_kernel<E, WPQ>, WPQ * kWave, shmem, &perCU);
  if (e != hipSuccess) return e;
  const int64_t resident = (int64_t)DeviceCUs(dev) * perCU;
  const int64_t grid = args.nPairs < resident ? args.nPairs : resident;
  hipLaunchKernelGGL((eval_listed_kernel<E, WPQ>), dim3((unsigned)grid), dim3(WPQ * kWave), shmem, stream, args);
  return hipGetLastError();
}

}  // namespace

size_t EvalListedPoleBytes(const KbView &kb, int64_t nPairs) {
  if (kb.elem != 8 || kb.poleList == nullptr) return 0;
  return kBatchPoleClear + (size_t)nPairs * (sizeof(PoleEntry) + (size_t)(2 * kb.K + 2) * sizeof(double));
}

hipError_t LaunchEvalListed(const KbView &kb, const QuizSlot *slots, int nSlots, const ListedPair *pairs, int64_t nPairs, void *pole,
                            hipStream_t stream) {
  if (nPairs <= 0 || nSlots <= 0) return hipSuccess;
  if (slots == nullptr || pairs == nullptr || (kb.elem != 8 && kb.elem != 4) || (kb.ldT & 1) != 0) return hipErrorInvalidValue;
  ListedArgs args{};
  args.cube = kb.cube; args.tgap = kb.tgap; args.qgap = kb.qgap;
  args.slots = slots; args.pairs = pairs; args.nPairs = nPairs;
  args.K = kb.K; args.ldT = kb.ldT;
  args.vCompTail = VCompTail(kb);
  const bool watch = pole != nullptr && EvalListedPoleBytes(kb, nPairs) != 0;
  if (watch) {   // the head as the batched sweeps lay it out (marks | list header), then the entries and the records, nPairs of each
    char *p = static_cast<char *>(pole);
    args.poleList = reinterpret_cast<PoleHeader *>(p + 256 * sizeof(uint32_t));
    args.poleSums = reinterpret_cast<double *>(p + kBatchPoleClear + (size_t)nPairs * sizeof(PoleEntry));
  }
  const bool two = kb.ldT <= 2048;
  const hipError_t le = kb.elem == 8 ? (two ? launch_listed<double, 2>(args, stream) : launch_listed<double, 4>(args, stream))
                                     : (two ? launch_listed<float, 2>(args, stream) : launch_listed<float, 4>(args, stream));
  if (le != hipSuccess || !watch) return le;
  PoleFix f = PoleFixWV(static_cast<const double *>(kb.cube), kb.tgap, kb.qgap, kb.K, kb.T, kb.ldT);
  f.list = args.poleList; f.sums = args.poleSums;
  f.slots = slots; f.nSlots = nSlots; f.bySlot = 1;
  f.qFirst = 0; f.nQ = kb.Q; f.capacity = nPairs;
  f.vCompTail = args.vCompTail;
  return LaunchPoleFixup(f, stream);   // (fs.scratch == nullptr: it corrects the vectors and publishes nothing)
}

hipError_t LaunchListedGather(const QuizSlot *slots, const ListedPair *pairs, int64_t nPairs, double *out, hipStream_t stream) {
  if (nPairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(listed_gather_kernel, dim3((unsigned)((nPairs + 255) / 256)), dim3(256), 0, stream, slots, pairs, nPairs, out);
  return hipGetLastError();
}

hipError_t LaunchListedArgmax(const KbView &kb, const QuizSlot *slots, int nSlots, const int64_t *offsets, const ListedPair *pairs, int64_t outBase,
                              uint64_t flagValue, hipStream_t stream) {
  if (nSlots <= 0) return hipSuccess;
  hipLaunchKernelGGL(listed_argmax_kernel, dim3((unsigned)nSlots), dim3(256), 0, stream, slots, kb.qgap, offsets, pairs, outBase, flagValue);
  return hipGetLastError();
}

}  // namespace pqa
