// kb_kernels.hip -- knowledge-base construction / mutation and top-target listing on gfx950.
//   fill_fresh      : CpuEngine ctor (reference: PqaCore/CpuEngine.cpp:44-84)  A = init^2, D = init^2*K, B = init
//   fill_synthetic  : deterministic benchmark / test cube, bit-identical to probqa_amd/synth.py (numpy)
//   train           : CETrainOperation::Perform1 / Perform2 (PqaCore/CETrainOperation.cpp:15-83)
//   top_targets     : ListTopTargets (PqaCore/CEListTopTargetsAlgorithm.cpp:30-95): descending probability
#include <algorithm>
#include <type_traits>

#include "pqa_device.h"
#include "pqa_kernels.h"

namespace pqa {

namespace {

__global__ __launch_bounds__(256) void fill_fresh_kernel(void *__restrict__ cube, int elem, double *__restrict__ vB, int64_t K,
                                                         int64_t Q, int64_t T, int64_t ldT, double initAmount) {
  const double init1 = initAmount, initSqr = init1 * init1, initMD = initSqr * (double)K;  // CpuEngine.cpp:45-47
  const int64_t total = Q * (K + 1) * ldT;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = i % ldT, r = (i / ldT) % (K + 1);
    cube_st(cube, elem, i, (t < T) ? (r < K ? initSqr : initMD) : (r < K ? 0.0 : 1.0));
    if (i < ldT) vB[i] = (i < T) ? (elem == 4 ? (double)(float)init1 : init1) : 0.0;   // (Float engines: vB holds fp32 values)
  }
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
__device__ __forceinline__ double hash_unit(uint64_t seed, uint64_t idx) {  // uniform in [0,1), 53 bits
  return (double)(splitmix64(seed + idx * 0x9E3779B97F4A7C15ULL) >> 11) * 0x1.0p-53;
}

// One thread per (question, target): loops over the answers so that D = sum_k A is accumulated in k order.
__global__ __launch_bounds__(256) void fill_synth_kernel(void *__restrict__ cube, int elem, double *__restrict__ vB, int64_t K,
                                                         int64_t Q, int64_t T, int64_t ldT, int64_t qOffset,
                                                         int64_t qTotal, double initAmount, double nTrain,
                                                         double noiseAmp, uint64_t seed) {
  const int64_t total = Q * ldT;
  const int64_t w = (32 * T) / 1000 > 1 ? (32 * T) / 1000 : 1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = i / ldT, t = i % ldT;
    const int64_t col = q * (K + 1) * ldT + t;
    if (t >= T) {
      for (int64_t k = 0; k < K; k++) cube_st(cube, elem, col + k * ldT, 0.0);
      cube_st(cube, elem, col + K * ldT, 1.0);
    } else {
      const int64_t qg = qOffset + q;
      const int64_t x = (qg * T) / qTotal;
      int64_t ans;  // the +-32 "binary search" answer rule of PqaCoreTests/DichotomyTest.cpp:50-64, scaled by T/1000
      if (t < x - w) ans = 0; else if (t < x) ans = 1; else if (t == x) ans = 2; else if (t <= x + w) ans = 3; else ans = 4;
      if (ans > K - 1) ans = K - 1;
      double d = 0.0;
      for (int64_t k = 0; k < K; k++) {
        double a = initAmount;
        if (k == ans) a = a + nTrain;
        a = a + noiseAmp * hash_unit(seed, (uint64_t)((qg * K + k) * T + t));
        double a2 = a * a;  // the cube stores squares (PqaCore/CETrainOperation.cpp:15-25)
        if (elem == 4) a2 = (double)(float)a2;   // Float cube: D is the sum of the ROUNDED squares, as training would leave it
        cube_st(cube, elem, col + k * ldT, a2);
        d = d + a2;
      }
      cube_st(cube, elem, col + K * ldT, d);
    }
    if (q == 0) {
      const double b = (t < T) ? (initAmount + nTrain) + noiseAmp * hash_unit(seed ^ 0x5851F42D4C957F2DULL, (uint64_t)t) : 0.0;
      vB[t] = elem == 4 ? (double)(float)b : b;
    }
  }
}

// Training (reference PqaCore/CETrainOperation.cpp:15-83).  The host turns the call's answered questions into steps in the
// reference's own pairing order (hip_engine_update.cpp: BuildTrainSteps) and groups the steps by question: steps on different
// questions touch different cells and run in parallel, one thread per question; a question's steps run in order.
//   kind 1  Perform1 (:28-30, and either half of a Perform2 over two different questions, :56-82): a = sqrt(A); A, D += 2ab + b^2
//   kind 2  Perform2, same question and answer (:34-35): ONE step of 2b -- A, D += 4ab + 4b^2 (_inc4B, _incSquare2B)
//   kind 3  Perform2, same question, answers a1 != a2 (:37-54): each cell its own addend; D += TWICE THE FIRST cell's addend (:45-46)
__device__ __forceinline__ void train_steps_body(void *__restrict__ cube, int elem, double *__restrict__ vB, int64_t K, int64_t ldT,
                                                 const TrainStep *__restrict__ steps, const int64_t *__restrict__ chainStart, int64_t nChains,
                                                 int64_t iTarget, double amount) {
  const double twoB = 2 * amount, bSquare = amount * amount;  // CETrainTaskNumSpec.h:24-32
  const double fourB = 4 * amount, square2B = 4 * bSquare;
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nChains; c += (int64_t)gridDim.x * blockDim.x) {
    for (int64_t i = chainStart[c]; i < chainStart[c + 1]; i++) {
      const TrainStep st = steps[i];
      const int64_t iA = (st.q * (K + 1) + st.a1) * ldT + iTarget, iD = (st.q * (K + 1) + K) * ldT + iTarget;
      const double oldA = cube_ld(cube, elem, iA);
      const double a = sqrt(oldA);                               // CETrainOperation.cpp:18
      if (st.kind == 3) {
        const int64_t iA2 = (st.q * (K + 1) + st.a2) * ldT + iTarget;
        const double oldA2 = cube_ld(cube, elem, iA2);
        const double add1 = a * twoB + bSquare, add2 = sqrt(oldA2) * twoB + bSquare;   // :42-44
        cube_st(cube, elem, iA, oldA + add1);                    // :47-53
        cube_st(cube, elem, iA2, oldA2 + add2);
        cube_st(cube, elem, iD, cube_ld(cube, elem, iD) + (add1 + add1));
      } else {
        const double addend = st.kind == 2 ? a * fourB + square2B : a * twoB + bSquare;   // :19
        cube_st(cube, elem, iA, oldA + addend);                  // :23-24
        cube_st(cube, elem, iD, cube_ld(cube, elem, iD) + addend);   // :25
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double b = vB[iTarget] + amount;                   // PqaCore/CpuEngine.cpp:172, :462
    vB[iTarget] = elem == 4 ? (double)(float)b : b;
  }
}
__global__ void train_steps_kernel(void *__restrict__ cube, int elem, double *__restrict__ vB, int64_t K, int64_t ldT,
                                   const TrainStep *__restrict__ steps, const int64_t *__restrict__ chainStart, int64_t nChains,
                                   int64_t iTarget, double amount) {
  train_steps_body(cube, elem, vB, K, ldT, steps, chainStart, nChains, iTarget, amount);
}
// The same with the steps in the kernel's arguments: the training call at the end of a quiz has a handful of them, and two
// staged copies plus the wait for them (the host vectors are their sources) cost four times what the launch does.
__global__ void train_steps_inline_kernel(void *__restrict__ cube, int elem, double *__restrict__ vB, int64_t K, int64_t ldT,
                                          TrainStepsInline in, int64_t iTarget, double amount) {
  train_steps_body(cube, elem, vB, K, ldT, in.steps, in.chainStart, in.nChains, iTarget, amount);
}

// Several calls' steps, one workgroup per call (the calls' targets differ: no cell belongs to two of them).  The arithmetic of a step
// is train_steps_body's.
__global__ void train_batch_inline_kernel(void *__restrict__ cube, int elem, double *__restrict__ vB, int64_t K, int64_t ldT, TrainBatchInline in) {
  const TrainBatchCall call = in.calls[blockIdx.x];
  const int64_t iTarget = call.iTarget;
  const double amount = call.amount;
  const double twoB = 2 * amount, bSquare = amount * amount;  // CETrainTaskNumSpec.h:24-32
  const double fourB = 4 * amount, square2B = 4 * bSquare;
  // chain c of the call: steps [chainStart[firstChain + callIndex + c], chainStart[firstChain + callIndex + c + 1]) -- every call's
  // chain starts are followed by one end marker, so call b's entries begin at firstChain + b
  const uint16_t *cs = in.chainStart + call.firstChain + blockIdx.x;
  for (int c = threadIdx.x; c < call.nChains; c += blockDim.x) {
    for (int i = cs[c]; i < cs[c + 1]; i++) {
      const TrainBatchStep st = in.steps[i];
      const int64_t iA = ((int64_t)st.q * (K + 1) + st.a1) * ldT + iTarget, iD = ((int64_t)st.q * (K + 1) + K) * ldT + iTarget;
      const double oldA = cube_ld(cube, elem, iA);
      const double a = sqrt(oldA);                               // CETrainOperation.cpp:18
      if (st.kind == 3) {
        const int64_t iA2 = ((int64_t)st.q * (K + 1) + st.a2) * ldT + iTarget;
        const double oldA2 = cube_ld(cube, elem, iA2);
        const double add1 = a * twoB + bSquare, add2 = sqrt(oldA2) * twoB + bSquare;   // :42-44
        cube_st(cube, elem, iA, oldA + add1);                    // :47-53
        cube_st(cube, elem, iA2, oldA2 + add2);
        cube_st(cube, elem, iD, cube_ld(cube, elem, iD) + (add1 + add1));
      } else {
        const double addend = st.kind == 2 ? a * fourB + square2B : a * twoB + bSquare;   // :19
        cube_st(cube, elem, iA, oldA + addend);                  // :23-24
        cube_st(cube, elem, iD, cube_ld(cube, elem, iD) + addend);   // :25
      }
    }
  }
  if (threadIdx.x == 0) {
    const double b = vB[iTarget] + amount;                   // PqaCore/CpuEngine.cpp:172, :462
    vB[iTarget] = elem == 4 ? (double)(float)b : b;
  }
}

// Many records in one launch (hip_engine_train.cpp: why the result is bit-identical to consecutive training calls).  One lane per
// chain -- the steps on one (target, question) in record order -- with the step arithmetic of train_steps_body operation for
// operation, but each step with its own record's amount.  D[q][t] belongs to the chain alone: it stays in a register and is
// rounded where cube_st would round it, once per step on a Float cube.  The A cells are read and written in memory (a chain may
// come back to one).  The lanes after the chains add each target's amounts to vB[t] in record order with the rounding of
// train_steps_body.  No barriers: the kernel is latency-bound and its speed is the number of chains in flight.
__global__ __launch_bounds__(64) void train_chains_kernel(void *__restrict__ cube, int elem, double *__restrict__ vB, int64_t K,
                                                          int64_t ldT, const TrainChain *__restrict__ chains, int64_t nChains,
                                                          int64_t nTargets, const TrainChainStep *__restrict__ steps,
                                                          const double *__restrict__ amounts) {
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nChains + nTargets; c += (int64_t)gridDim.x * blockDim.x) {
    const TrainChain ch = chains[c];
    if (c >= nChains) {
      double b = vB[ch.t];
      for (int32_t i = ch.first; i < ch.end; i++) {
        b = b + amounts[i];                                  // PqaCore/CpuEngine.cpp:172, :462
        if (elem == 4) b = (double)(float)b;
      }
      vB[ch.t] = b;
      continue;
    }
    const int64_t q = steps[ch.first].q;
    const int64_t colQ = q * (K + 1) * ldT + ch.t, iD = colQ + K * ldT;
    double d = cube_ld(cube, elem, iD);
    for (int32_t i = ch.first; i < ch.end; i++) {
      const TrainChainStep st = steps[i];
      const uint32_t kind = st.kindRec & 3u;
      const double amount = amounts[st.kindRec >> 2];
      const double twoB = 2 * amount, bSquare = amount * amount;   // CETrainTaskNumSpec.h:24-32
      const double fourB = 4 * amount, square2B = 4 * bSquare;
      const int64_t iA = colQ + (int64_t)st.a1 * ldT;
      const double oldA = cube_ld(cube, elem, iA);
      const double a = sqrt(oldA);                                 // CETrainOperation.cpp:18
      if (kind == 3) {
        const int64_t iA2 = colQ + (int64_t)st.a2 * ldT;
        const double oldA2 = cube_ld(cube, elem, iA2);
        const double add1 = a * twoB + bSquare, add2 = sqrt(oldA2) * twoB + bSquare;   // :42-44
        cube_st(cube, elem, iA, oldA + add1);                      // :47-53
        cube_st(cube, elem, iA2, oldA2 + add2);
        d = d + (add1 + add1);
      } else {
        const double addend = kind == 2 ? a * fourB + square2B : a * twoB + bSquare;   // :19
        cube_st(cube, elem, iA, oldA + addend);                    // :23-24
        d = d + addend;                                            // :25
      }
      if (elem == 4) d = (double)(float)d;                         // (what cube_st and the next cube_ld would make of it)
    }
    cube_st(cube, elem, iD, d);
  }
}

// ListTopTargets on the device (top_targets_publish in pqa_device.h); T <= 16384.
static_assert(sizeof(TopOut) == sizeof(RatedTargetDev), "same record");
template <bool SMALL>
__global__ __launch_bounds__(SMALL ? 256 : 1024) void top_targets_kernel(const double *__restrict__ prior,
                                                                         const uint32_t *__restrict__ tgap, int64_t T,
                                                                         int64_t maxCount, RatedTargetDev *out, int64_t *nOut,
                                                                         uint64_t *flag, uint64_t flagValue) {
  __shared__ TopScratch scratch;
  top_targets_publish<SMALL>(prior, tgap, T, maxCount, reinterpret_cast<TopOut *>(out), nOut, flag, flagValue, &scratch);
}

unsigned grid_for(int64_t n, int threads) {
  int64_t b = (n + threads - 1) / threads;
  if (b > 256 * 32) b = 256 * 32;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// ---- maintenance (reference PqaCore/CpuEngine.cpp:468-658) ---------------------------------------------------------
// (Re)initialise whole questions: A = init^2, D = init^2 * K on real targets; padding columns A = 0, D = 1.
__global__ __launch_bounds__(256) void fill_questions_kernel(void *__restrict__ cube, int elem, int64_t K, int64_t T, int64_t ldT,
                                                             const int64_t *__restrict__ qs,
                                                             const double *__restrict__ inits, int64_t n) {
  const int64_t per = (K + 1) * ldT, total = n * per;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t iq = i / per, r = (i % per) / ldT, t = i % ldT;
    const double initSqr = inits[iq] * inits[iq], initMD = initSqr * (double)K;  // :503-510 / :548-555
    cube_st(cube, elem, qs[iq] * per + r * ldT + t, (t < T) ? (r < K ? initSqr : initMD) : (r < K ? 0.0 : 1.0));
  }
}

// (Re)initialise target columns over questions [0,nQ) except those flagged in skipQ (already initialised as questions).
__global__ __launch_bounds__(256) void fill_targets_kernel(void *__restrict__ cube, int elem, double *__restrict__ vB, int64_t K,
                                                           int64_t ldT, int64_t nQ, const uint32_t *__restrict__ skipQ,
                                                           const int64_t *__restrict__ ts,
                                                           const double *__restrict__ inits, int64_t n) {
  const int64_t total = nQ * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = i / n, it = i % n;
    if (q == 0) vB[ts[it]] = elem == 4 ? (double)(float)inits[it] : inits[it];   // :532 / :566
    if (skipQ && bit_test(skipQ, q)) continue;                                   // :558-560
    const double initSqr = inits[it] * inits[it], initMD = initSqr * (double)K;  // :517,:523 / :556-557
    const int64_t col = q * (K + 1) * ldT + ts[it];
    for (int64_t k = 0; k < K; k++) cube_st(cube, elem, col + k * ldT, initSqr);
    cube_st(cube, elem, col + K * ldT, initMD);
  }
}

// Compaction of the target axis (:619-647): column dst <- column src for every kept question and for vB.
__global__ __launch_bounds__(256) void move_targets_kernel(void *__restrict__ cube, int elem, double *__restrict__ vB, int64_t K,
                                                           int64_t ldT, int64_t nQ, const int64_t *__restrict__ moves,
                                                           int64_t n) {
  const int64_t rows = nQ * (K + 1) + 1, total = rows * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / n, m = i % n;
    // (src, dst) pairs; sources are never destinations (:604-618)
    if (row < nQ * (K + 1)) cube_st(cube, elem, row * ldT + moves[2 * m + 1], cube_ld(cube, elem, row * ldT + moves[2 * m]));
    else vB[moves[2 * m + 1]] = vB[moves[2 * m]];
  }
}

// Rebuild of a shard after a change of the dimensions (sharded_engine.cpp): question q of the new cube takes the rows of the
// block src[q] -- which may live on another device of the process (peer access) -- with its columns picked by colMap (new
// target t <- old target colMap[t]; -1: a new column, left as the fresh fill made it and initialised afterwards).
__global__ __launch_bounds__(256) void adopt_rows_kernel(void *__restrict__ dst, int elem, int64_t K, int64_t nQ, int64_t Tn, int64_t ldTn,
                                                         const void *const *__restrict__ src, int64_t ldTs,
                                                         const int64_t *__restrict__ colMap) {
  const int64_t per = (K + 1) * Tn, total = nQ * per;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = i / per, r = (i % per) / Tn, t = i % Tn;
    const void *s = src[q];
    const int64_t c = colMap[t];
    if (s != nullptr && c >= 0) cube_st(dst, elem, (q * (K + 1) + r) * ldTn + t, cube_ld(s, elem, r * ldTs + c));
  }
}
__global__ __launch_bounds__(256) void adopt_vb_kernel(double *__restrict__ dst, const double *__restrict__ src, const int64_t *__restrict__ colMap,
                                                       int64_t Tn) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < Tn; t += (int64_t)gridDim.x * blockDim.x)
    if (colMap[t] >= 0) dst[t] = src[colMap[t]];
}

// PqaHip_PackAnswerRows: workgroup (row, chunk) copies kPackChunkBytes of one row -- row 2 i the sA row of pair i, row 2 i + 1 its mD
// row, which lands rowUnits 16-byte units behind it -- as 16-byte loads, all of a thread's requested before its first store.  The
// bytes travel as they are: no element is looked at, so Float and Double cubes take the same kernel.  With a flag, every workgroup
// makes its stores visible system-wide and counts itself in; the last one to arrive publishes flagValue (the finisher of the sweeps).
// Workgroups past `nWork` (a package without a row of this engine: one workgroup) only do that.
__global__ __launch_bounds__(256) void pack_answer_rows_kernel(const PackPair *__restrict__ pairs, int64_t nWork, int64_t rowUnits, int64_t chunksPerRow,
                                                               unsigned *counter, uint64_t *flag, uint64_t flagValue) {
  constexpr int kPer = (int)(kPackChunkBytes / 16 / 256);
  if ((int64_t)blockIdx.x < nWork) {
    const int64_t row = blockIdx.x / chunksPerRow, chunk = blockIdx.x % chunksPerRow;
    const PackPair p = pairs[row >> 1];
    const uint4 *src = static_cast<const uint4 *>((row & 1) ? p.rowD : p.rowA);
    uint4 *dst = static_cast<uint4 *>(p.dst) + (row & 1) * rowUnits;
    const int64_t u0 = chunk * (kPer * 256) + threadIdx.x;
    uint4 v[kPer];
#pragma unroll
    for (int e = 0; e < kPer; e++)
      if (u0 + e * 256 < rowUnits) v[e] = src[u0 + e * 256];
#pragma unroll
    for (int e = 0; e < kPer; e++)
      if (u0 + e * 256 < rowUnits) dst[u0 + e * 256] = v[e];
  }
  if (flag == nullptr) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope: this thread's part of the rows before the count
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != gridDim.x - 1) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  __hip_atomic_store(flag, flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// PqaHip_PackQuestionBlocks / PqaEngine_CompactFromBlocks: whole question blocks between a cube and a block package, whose row pitches
// differ (the cube's ldT only ever grows; a package's pitch is that of the current T).  Workgroup (block, row, chunk) moves
// kPackChunkBytes of one row as 16-byte units, all of a thread's loads requested before its first store; rows start on 128-byte lines on
// both sides, so every unit is aligned.  A row is rowWords 4-byte words (elements are 4 or 8 bytes): its last unit may be partial.
// kZeroTail (packing): the partial unit's other words and every unit behind it up to the destination's pitch are stored as zeros, so a
// slot is a function of the row's T elements alone.  Otherwise (unpacking into a cube) the partial unit goes word by word and nothing
// behind it is written: the cube's columns from T on stay as they are.  The flag protocol is pack_answer_rows_kernel's.
template <bool kZeroTail>
__global__ __launch_bounds__(256) void copy_question_blocks_kernel(const BlockCopy *__restrict__ blocks, int64_t nWork, int64_t rows, int64_t rowWords,
                                                                   int64_t srcPitchUnits, int64_t dstPitchUnits, int64_t chunksPerRow, unsigned *counter,
                                                                   uint64_t *flag, uint64_t flagValue) {
  constexpr int kPer = (int)(kPackChunkBytes / 16 / 256);
  if ((int64_t)blockIdx.x < nWork) {
    const int64_t rowIndex = blockIdx.x / chunksPerRow, chunk = blockIdx.x % chunksPerRow;
    const BlockCopy b = blocks[rowIndex / rows];
    const int64_t r = rowIndex % rows;
    const uint4 *src = static_cast<const uint4 *>(b.src) + r * srcPitchUnits;
    uint4 *dst = static_cast<uint4 *>(b.dst) + r * dstPitchUnits;
    const int64_t fullUnits = rowWords >> 2;
    const int tailWords = (int)(rowWords & 3);
    const int64_t dataUnits = fullUnits + (tailWords != 0 ? 1 : 0), dstUnits = kZeroTail ? dstPitchUnits : dataUnits;
    const int64_t u0 = chunk * (kPer * 256) + threadIdx.x;
    uint4 v[kPer];
#pragma unroll
    for (int e = 0; e < kPer; e++) {
      const int64_t u = u0 + e * 256;
      v[e] = u < dataUnits ? src[u] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < kPer; e++) {
      const int64_t u = u0 + e * 256;
      if (u >= dstUnits) continue;
      if (u != fullUnits || tailWords == 0) { dst[u] = v[e]; continue; }
      if constexpr (kZeroTail) {
        dst[u] = make_uint4(v[e].x, tailWords > 1 ? v[e].y : 0u, tailWords > 2 ? v[e].z : 0u, 0u);
      } else {
        uint32_t *w = reinterpret_cast<uint32_t *>(dst + u);
        w[0] = v[e].x;
        if (tailWords > 1) w[1] = v[e].y;
        if (tailWords > 2) w[2] = v[e].z;
      }
    }
  }
  if (flag == nullptr) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope: this thread's part of the blocks before the count
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != gridDim.x - 1) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  __hip_atomic_store(flag, flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// PqaHip_PackAnswerPosteriors / PqaEngine_RecordAnswerBatchFromPosteriors: one posterior -- T doubles -- between the engine and a slot
// of a posterior package, whose pitch is that of the current T.  A workgroup moves chunk `chunk` (kPackChunkBytes) of the vector as
// 16-byte units, all of a thread's loads requested before its first store; both sides start on 16-byte bounds.  An odd T leaves a
// partial last unit.  kZeroTail (packing): its other half and every unit behind it up to dstUnits are stored as zeros, so a slot is
// a function of the T doubles alone.  Otherwise (into a quiz's posterior) its half goes word by word and nothing behind it is
// written: the elements from T on stay as they are.
template <bool kZeroTail>
__device__ __forceinline__ void copy_posterior_chunk(const uint4 *__restrict__ src, uint4 *__restrict__ dst, int64_t T, int64_t dstUnits, int64_t chunk) {
  constexpr int kPer = (int)(kPackChunkBytes / 16 / 256);
  const int64_t fullUnits = T >> 1;
  const bool tail = (T & 1) != 0;
  const int64_t dataUnits = fullUnits + (tail ? 1 : 0), lastUnit = kZeroTail ? dstUnits : dataUnits;
  const int64_t u0 = chunk * (kPer * 256) + threadIdx.x;
  uint4 v[kPer];
#pragma unroll
  for (int e = 0; e < kPer; e++) {
    const int64_t u = u0 + e * 256;
    v[e] = u < dataUnits ? src[u] : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int e = 0; e < kPer; e++) {
    const int64_t u = u0 + e * 256;
    if (u >= lastUnit) continue;
    if (u != fullUnits || !tail) { dst[u] = v[e]; continue; }
    if constexpr (kZeroTail) {
      dst[u] = make_uint4(v[e].x, v[e].y, 0u, 0u);
    } else {
      uint32_t *w = reinterpret_cast<uint32_t *>(dst + u);
      w[0] = v[e].x;
      w[1] = v[e].y;
    }
  }
}

// Workgroup (entry, chunk of the slot's pitch).  The flag protocol is pack_answer_rows_kernel's; workgroups past `nWork` (a batch
// without a question of this engine: one workgroup) only take part in that.
__global__ __launch_bounds__(256) void pack_posteriors_kernel(const PosteriorCopy *__restrict__ copies, int64_t nWork, int64_t T, int64_t pitchUnits,
                                                              int64_t chunksPerSlot, unsigned *counter, uint64_t *flag, uint64_t flagValue) {
  if ((int64_t)blockIdx.x < nWork) {
    const PosteriorCopy c = copies[blockIdx.x / chunksPerSlot];
    copy_posterior_chunk<true>(static_cast<const uint4 *>(c.src), static_cast<uint4 *>(c.dst), T, pitchUnits, blockIdx.x % chunksPerSlot);
  }
  if (flag == nullptr) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope: this thread's part of the slots before the count
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != gridDim.x - 1) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  __hip_atomic_store(flag, flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Workgroup (entry, chunk of the T doubles).  The entry's first workgroup also marks the answered question as asked where this engine
// holds it (CEQuiz::RecordAnswer, PqaCore/CEQuiz.h:92): the batch's quizzes are distinct, so the word has one writer.
__global__ __launch_bounds__(256) void take_posteriors_kernel(const PosteriorCopy *__restrict__ copies, int64_t T, int64_t chunksPerVector) {
  const int64_t chunk = blockIdx.x % chunksPerVector;
  const PosteriorCopy c = copies[blockIdx.x / chunksPerVector];
  copy_posterior_chunk<false>(static_cast<const uint4 *>(c.src), static_cast<uint4 *>(c.dst), T, 0, chunk);
  if (chunk == 0 && threadIdx.x == 0 && c.asked != nullptr) c.asked[c.askedBit >> 5] |= 1u << (c.askedBit & 31);
}

// ---- .kb rows between the file's dense layout in one number type and the cube's padded layout in another -------------------------------
// A thread moves four consecutive elements of one row, columns [4 g, 4 g + 4): on the cube's side that is a 16-byte aligned unit of a
// Float row (two of a Double row), whatever the row -- rows start on 128-byte lines.  The dense side is only element-aligned: row r
// starts r T elements into the block, so with an odd T every other row is 8 (fp64) or 4, 8, 12 (fp32) bytes off.  The quad is moved by
// the widest access its address allows -- 16 bytes where both sides allow it, 8 or 4 on the dense side otherwise; consecutive lanes
// stay on consecutive addresses either way.  A row's last 1..3 elements go one by one, so nothing outside [0, T) of a row is read
// or written on either side: the cube's padding stays as Create left it, and the dense neighbours are other rows.
// 256 threads = rowsPerBlock rows x lanesPerRow quads (a power of two: short rows share a workgroup); grid.x strides along the row,
// grid.y over the rows.  No LDS, no barrier: a streaming copy whose speed is the loads in flight.
template <typename E>
__device__ __forceinline__ void quad_load(const E *p, E (&v)[4]) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if constexpr (sizeof(E) == 8) {
    if ((a & 15) == 0) {
      const double2 x = reinterpret_cast<const double2 *>(p)[0], y = reinterpret_cast<const double2 *>(p)[1];
      v[0] = x.x; v[1] = x.y; v[2] = y.x; v[3] = y.y;
    } else { v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3]; }
  } else {
    if ((a & 15) == 0) {
      const float4 x = reinterpret_cast<const float4 *>(p)[0];
      v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else if ((a & 7) == 0) {
      const float2 x = reinterpret_cast<const float2 *>(p)[0], y = reinterpret_cast<const float2 *>(p)[1];
      v[0] = x.x; v[1] = x.y; v[2] = y.x; v[3] = y.y;
    } else { v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3]; }
  }
}
template <typename E>
__device__ __forceinline__ void quad_store(E *p, const E (&v)[4]) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if constexpr (sizeof(E) == 8) {
    if ((a & 15) == 0) {
      reinterpret_cast<double2 *>(p)[0] = make_double2(v[0], v[1]);
      reinterpret_cast<double2 *>(p)[1] = make_double2(v[2], v[3]);
    } else { p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3]; }
  } else {
    if ((a & 15) == 0) reinterpret_cast<float4 *>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
    else if ((a & 7) == 0) {
      reinterpret_cast<float2 *>(p)[0] = make_float2(v[0], v[1]);
      reinterpret_cast<float2 *>(p)[1] = make_float2(v[2], v[3]);
    } else { p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3]; }
  }
}
// One element on its way: fp64 -> fp32 rounds to nearest even (the conversion instruction's default mode, what (float)x is on the host);
// fp32 -> fp64 is exact; kRound: fp64 words that are to hold fp32 values.  A finite value that does not stay finite is counted.
template <typename D, typename S, bool kRound>
__device__ __forceinline__ D convert_element(S x, unsigned &bad) {
  if constexpr (sizeof(S) == 8 && (sizeof(D) == 4 || kRound)) {
    const float y = (float)x;
    if (fabs(x) < HUGE_VAL && !(fabsf(y) < HUGE_VALF)) bad++;
    return (D)y;
  } else {
    return (D)x;
  }
}
template <typename DenseT, typename CubeT, bool kToCube, bool kRound>
__global__ __launch_bounds__(256) void convert_rows_kernel(DenseT *__restrict__ dense, CubeT *__restrict__ cube, int64_t T, int64_t ldT, int64_t nRows,
                                                           unsigned rowsPerQ, unsigned rowBase, unsigned qStride, int laneBits, unsigned *overflow) {
  using Src = typename std::conditional<kToCube, DenseT, CubeT>::type;
  using Dst = typename std::conditional<kToCube, CubeT, DenseT>::type;
  const int lanesPerRow = 1 << laneBits, lane = threadIdx.x & (lanesPerRow - 1), rowInBlock = threadIdx.x >> laneBits, rowsPerBlock = 256 >> laneBits;
  unsigned bad = 0;
  for (int64_t r = (int64_t)blockIdx.y * rowsPerBlock + rowInBlock; r < nRows; r += (int64_t)gridDim.y * rowsPerBlock) {
    const unsigned ru = (unsigned)r;   // (the launcher: nRows < 2^31)
    const int64_t cubeRow = (int64_t)(ru / rowsPerQ) * qStride + (ru % rowsPerQ) + rowBase;
    DenseT *d = dense + r * T;
    CubeT *c = cube + cubeRow * ldT;
    const Src *src;
    Dst *dst;
    if constexpr (kToCube) { src = d; dst = c; } else { src = c; dst = d; }
    for (int64_t t = ((int64_t)blockIdx.x * lanesPerRow + lane) * 4; t < T; t += (int64_t)gridDim.x * lanesPerRow * 4) {
      if (t + 4 <= T) {
        Src s[4];
        Dst o[4];
        quad_load(src + t, s);
#pragma unroll
        for (int e = 0; e < 4; e++) o[e] = convert_element<Dst, Src, kRound>(s[e], bad);
        quad_store(dst + t, o);
      } else {
        for (int64_t e = t; e < T; e++) dst[e] = convert_element<Dst, Src, kRound>(src[e], bad);
      }
    }
  }
  if (bad != 0) atomicAdd(overflow, bad);
}

}  // namespace

hipError_t LaunchConvertRows(const ConvertRows &c, hipStream_t stream) {
  if (c.dense == nullptr || c.cube == nullptr || c.overflow == nullptr || c.T < 1 || c.ldT < c.T || c.nRows < 0 || c.nRows > 0x7fffffff || c.rowsPerQ < 1 ||
      c.rowsPerQ > 0x7fffffff || c.rowBase < 0 || c.rowBase > 0x7fffffff || c.qStride < 0 || c.qStride > 0x7fffffff)
    return hipErrorInvalidValue;
  if (c.nRows == 0) return hipSuccess;
  const int64_t quads = (c.T + 3) / 4;
  int laneBits = 0;
  while (laneBits < 8 && ((int64_t)1 << laneBits) < quads) laneBits++;
  const int64_t lanesPerRow = (int64_t)1 << laneBits, rowsPerBlock = 256 / lanesPerRow;
  const dim3 grid((unsigned)std::min<int64_t>((quads + lanesPerRow - 1) / lanesPerRow, 64), (unsigned)std::min<int64_t>((c.nRows + rowsPerBlock - 1) / rowsPerBlock, 65535));
#define PQA_CONVERT(DenseT, CubeT, TO_CUBE, ROUND)                                                                                                          \
  hipLaunchKernelGGL((convert_rows_kernel<DenseT, CubeT, TO_CUBE, ROUND>), grid, dim3(256), 0, stream, static_cast<DenseT *>(c.dense), static_cast<CubeT *>(c.cube), \
                     c.T, c.ldT, c.nRows, (unsigned)c.rowsPerQ, (unsigned)c.rowBase, (unsigned)c.qStride, laneBits, c.overflow)
  if (c.denseElem == 8 && c.cubeElem == 4 && !c.roundF32) { if (c.toCube) PQA_CONVERT(double, float, true, false); else PQA_CONVERT(double, float, false, false); }
  else if (c.denseElem == 4 && c.cubeElem == 8 && !c.roundF32) { if (c.toCube) PQA_CONVERT(float, double, true, false); else PQA_CONVERT(float, double, false, false); }
  else if (c.denseElem == 8 && c.cubeElem == 8 && c.roundF32 && c.toCube) PQA_CONVERT(double, double, true, true);
  else return hipErrorInvalidValue;   // (equal types move by plain copies: hip_engine_kb.cpp)
#undef PQA_CONVERT
  return hipGetLastError();
}

hipError_t LaunchPackAnswerRows(const PackPair *pairs, int64_t n, int64_t rowBytes, unsigned *counter, uint64_t *flag, uint64_t flagValue,
                                hipStream_t stream) {
  if (n < 0 || rowBytes <= 0 || rowBytes % 16 != 0 || (flag != nullptr && counter == nullptr)) return hipErrorInvalidValue;
  if (n == 0 && flag == nullptr) return hipSuccess;
  const int64_t rowUnits = rowBytes / 16, chunksPerRow = (rowBytes + kPackChunkBytes - 1) / kPackChunkBytes;   // (a short row: one workgroup)
  const int64_t nWork = 2 * n * chunksPerRow;
  if (nWork > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_answer_rows_kernel, dim3((unsigned)std::max<int64_t>(nWork, 1)), dim3(256), 0, stream, pairs, nWork, rowUnits, chunksPerRow,
                     counter, flag, flagValue);
  return hipGetLastError();
}

hipError_t LaunchCopyQuestionBlocks(const BlockCopy *blocks, int64_t n, int64_t rows, int64_t rowWords, int64_t srcPitchBytes, int64_t dstPitchBytes,
                                    bool zeroTail, unsigned *counter, uint64_t *flag, uint64_t flagValue, hipStream_t stream) {
  const int64_t dataBytes = (rowWords + 3) / 4 * 16;   // the row, rounded up to the unit
  if (n < 0 || rows < 1 || rowWords < 1 || srcPitchBytes % 16 != 0 || dstPitchBytes % 16 != 0 || srcPitchBytes < dataBytes || dstPitchBytes < dataBytes ||
      (n > 0 && blocks == nullptr) || (flag != nullptr && counter == nullptr))
    return hipErrorInvalidValue;
  if (n == 0 && flag == nullptr) return hipSuccess;
  const int64_t dstBytes = zeroTail ? dstPitchBytes : dataBytes, chunksPerRow = (dstBytes + kPackChunkBytes - 1) / kPackChunkBytes;
  if (n > 0x7fffffff / (rows * chunksPerRow)) return hipErrorInvalidValue;
  const int64_t nWork = n * rows * chunksPerRow;
  const dim3 grid((unsigned)std::max<int64_t>(nWork, 1));
  if (zeroTail)
    hipLaunchKernelGGL(copy_question_blocks_kernel<true>, grid, dim3(256), 0, stream, blocks, nWork, rows, rowWords, srcPitchBytes / 16, dstPitchBytes / 16,
                       chunksPerRow, counter, flag, flagValue);
  else
    hipLaunchKernelGGL(copy_question_blocks_kernel<false>, grid, dim3(256), 0, stream, blocks, nWork, rows, rowWords, srcPitchBytes / 16, dstPitchBytes / 16,
                       chunksPerRow, counter, flag, flagValue);
  return hipGetLastError();
}

hipError_t LaunchPackPosteriors(const PosteriorCopy *copies, int64_t n, int64_t T, int64_t pitchBytes, unsigned *counter, uint64_t *flag,
                                uint64_t flagValue, hipStream_t stream) {
  if (n < 0 || T < 1 || pitchBytes % 16 != 0 || pitchBytes < (T + 1) / 2 * 16 || (n > 0 && copies == nullptr) || (flag != nullptr && counter == nullptr))
    return hipErrorInvalidValue;
  if (n == 0 && flag == nullptr) return hipSuccess;
  const int64_t chunksPerSlot = (pitchBytes + kPackChunkBytes - 1) / kPackChunkBytes;
  if (n > 0x7fffffff / chunksPerSlot) return hipErrorInvalidValue;
  const int64_t nWork = n * chunksPerSlot;
  hipLaunchKernelGGL(pack_posteriors_kernel, dim3((unsigned)std::max<int64_t>(nWork, 1)), dim3(256), 0, stream, copies, nWork, T, pitchBytes / 16,
                     chunksPerSlot, counter, flag, flagValue);
  return hipGetLastError();
}

hipError_t LaunchTakePosteriors(const PosteriorCopy *copies, int64_t n, int64_t T, hipStream_t stream) {
  if (n < 0 || T < 1 || (n > 0 && copies == nullptr)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const int64_t chunksPerVector = ((T + 1) / 2 * 16 + kPackChunkBytes - 1) / kPackChunkBytes;
  if (n > 0x7fffffff / chunksPerVector) return hipErrorInvalidValue;
  hipLaunchKernelGGL(take_posteriors_kernel, dim3((unsigned)(n * chunksPerVector)), dim3(256), 0, stream, copies, T, chunksPerVector);
  return hipGetLastError();
}

hipError_t LaunchAdoptRows(void *dst, int elem, double *dstVB, int64_t K, int64_t nQ, int64_t Tn, int64_t ldTn, const void *const *src,
                           int64_t ldTs, const double *srcVB, const int64_t *colMap, hipStream_t stream) {
  if (nQ <= 0 || Tn <= 0) return hipSuccess;
  hipLaunchKernelGGL(adopt_rows_kernel, dim3(grid_for(nQ * (K + 1) * Tn, 256)), dim3(256), 0, stream, dst, elem, K, nQ, Tn, ldTn, src, ldTs, colMap);
  hipLaunchKernelGGL(adopt_vb_kernel, dim3(grid_for(Tn, 256)), dim3(256), 0, stream, dstVB, srcVB, colMap, Tn);
  return hipGetLastError();
}

hipError_t LaunchFillQuestions(void *cube, int elem, int64_t K, int64_t T, int64_t ldT, const int64_t *qs, const double *inits,
                               int64_t n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fill_questions_kernel, dim3(grid_for(n * (K + 1) * ldT, 256)), dim3(256), 0, stream, cube, elem, K, T, ldT,
                     qs, inits, n);
  return hipGetLastError();
}

hipError_t LaunchFillTargets(void *cube, int elem, double *vB, int64_t K, int64_t ldT, int64_t nQ, const uint32_t *skipQ,
                             const int64_t *ts, const double *inits, int64_t n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fill_targets_kernel, dim3(grid_for(nQ * n, 256)), dim3(256), 0, stream, cube, elem, vB, K, ldT, nQ, skipQ, ts,
                     inits, n);
  return hipGetLastError();
}

hipError_t LaunchMoveTargets(void *cube, int elem, double *vB, int64_t K, int64_t ldT, int64_t nQ, const int64_t *moves,
                             int64_t n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(move_targets_kernel, dim3(grid_for((nQ * (K + 1) + 1) * n, 256)), dim3(256), 0, stream, cube, elem, vB, K,
                     ldT, nQ, moves, n);
  return hipGetLastError();
}

hipError_t LaunchFillFresh(void *cube, int elem, double *vB, int64_t K, int64_t Q, int64_t T, int64_t ldT, double initAmount,
                           hipStream_t stream) {
  hipLaunchKernelGGL(fill_fresh_kernel, dim3(grid_for(Q * (K + 1) * ldT, 256)), dim3(256), 0, stream, cube, elem, vB, K, Q, T,
                     ldT, initAmount);
  return hipGetLastError();
}

hipError_t LaunchFillSynthetic(void *cube, int elem, double *vB, int64_t K, int64_t Q, int64_t T, int64_t ldT, int64_t qOffset,
                               int64_t qTotal, double initAmount, double nTrain, double noiseAmp, uint64_t seed,
                               hipStream_t stream) {
  hipLaunchKernelGGL(fill_synth_kernel, dim3(grid_for(Q * ldT, 256)), dim3(256), 0, stream, cube, elem, vB, K, Q, T, ldT,
                     qOffset, qTotal, initAmount, nTrain, noiseAmp, seed);
  return hipGetLastError();
}

hipError_t LaunchTrainSteps(void *cube, int elem, double *vB, int64_t K, int64_t ldT, const TrainStep *steps,
                            const int64_t *chainStart, int64_t nChains, int64_t iTarget, double amount, hipStream_t stream) {
  hipLaunchKernelGGL(train_steps_kernel, dim3(grid_for(nChains, 64)), dim3(64), 0, stream, cube, elem, vB, K, ldT, steps, chainStart,
                     nChains, iTarget, amount);
  return hipGetLastError();
}

hipError_t LaunchTrainStepsInline(void *cube, int elem, double *vB, int64_t K, int64_t ldT, const TrainStepsInline &in,
                                  int64_t iTarget, double amount, hipStream_t stream) {
  hipLaunchKernelGGL(train_steps_inline_kernel, dim3(1), dim3(64), 0, stream, cube, elem, vB, K, ldT, in, iTarget, amount);
  return hipGetLastError();
}

hipError_t LaunchTrainChains(void *cube, int elem, double *vB, int64_t K, int64_t ldT, const TrainChain *chains, int64_t nChains,
                             int64_t nTargets, const TrainChainStep *steps, const double *amounts, hipStream_t stream) {
  if (nChains + nTargets <= 0) return hipSuccess;
  hipLaunchKernelGGL(train_chains_kernel, dim3(grid_for(nChains + nTargets, 64)), dim3(64), 0, stream, cube, elem, vB, K, ldT, chains,
                     nChains, nTargets, steps, amounts);
  return hipGetLastError();
}

hipError_t LaunchTrainBatchInline(void *cube, int elem, double *vB, int64_t K, int64_t ldT, const TrainBatchInline &in, hipStream_t stream) {
  if (in.nCalls < 1 || in.nCalls > kTrainBatchCalls) return hipErrorInvalidValue;
  hipLaunchKernelGGL(train_batch_inline_kernel, dim3((unsigned)in.nCalls), dim3(64), 0, stream, cube, elem, vB, K, ldT, in);
  return hipGetLastError();
}

hipError_t LaunchTopTargets(const KbView &kb, const double *prior, int64_t maxCount, RatedTargetDev *out,
                            int64_t *nOut, uint64_t *flag, uint64_t flagValue, hipStream_t stream) {
  if (kb.T > 16384) return hipErrorInvalidValue;  // LaunchTopTargetsBatch takes over (hip_engine_update.cpp)
  if (kb.smallLaunches && kb.T <= 1024)   // beside the resident sweep (prior_kernels.hip: kSmallThreads)
    hipLaunchKernelGGL(top_targets_kernel<true>, dim3(1), dim3(256), 0, stream, prior, kb.tgap, kb.T, maxCount, out, nOut, flag,
                       flagValue);
  else
    hipLaunchKernelGGL(top_targets_kernel<false>, dim3(1), dim3(1024), 0, stream, prior, kb.tgap, kb.T, maxCount, out, nOut, flag,
                       flagValue);
  return hipGetLastError();
}

// ---- ListTopTargets over rows of any length, for many quizzes at once ----------------------------------------------------
// Level 0: every WAVE holds 1024 targets of a quiz's posterior in registers (16 per lane) and lists ITS best maxCount by itself -- no
// LDS, no barrier: a round is two wave all-reduces, and the lane that held the winner looks at its 16 again.  The best maxCount of the
// whole row under the order (probability descending, target ascending) are among the waves' bests under the same order.  Then merges
// of up to 16384 / maxCount candidate lists per workgroup until one list per quiz is left; the last level writes the caller's records
// and counts.  What crosses to the host is nQuizzes x maxCount records -- the reference's GPU engine copies all T posteriors per quiz
// and heapifies on the host (PqaCore/CudaEngine.cpp:251-289).
namespace {
constexpr int kTopChunkThreads = 256, kTopWaveTargets = 16 * kWave;
static_assert(kTopChunkThreads / kWave * kTopWaveTargets == kTopChunkTargets, "four waves of 1024 targets per workgroup");

__global__ __launch_bounds__(kTopChunkThreads) void top_chunks_kernel(TopBatchPriors priors, const uint32_t *__restrict__ tgap, int64_t T,
                                                                      int64_t maxCount, TopOut *lists) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int64_t quiz = blockIdx.y, nLists = (int64_t)gridDim.x * (kTopChunkThreads / kWave);
  const int64_t list = (int64_t)blockIdx.x * (kTopChunkThreads / kWave) + wave;
  const int64_t tFirst = list * kTopWaveTargets;
  const double *prior = priors.prior[quiz];
  double p[16];
  int t[16];
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int64_t tt = tFirst + lane + e * kWave;
    const bool ok = tt < T && !bit_test(tgap, tt);
    p[e] = ok ? prior[tt] : -1.0;
    if (!(p[e] > 0.0)) p[e] = -1.0;       // gaps and probabilities <= 0 are no candidates (pqa_device.h)
    t[e] = (int)tt;
  }
  TopOut *mine = lists + (quiz * nLists + list) * maxCount;
  const int64_t listed = top_rounds_wave<16>(p, t, maxCount, mine);
  for (int64_t i = listed + lane; i < maxCount; i += kWave) mine[i] = TopOut{-1, -1.0};   // the rest of the list says "no candidate"
}

__device__ __forceinline__ void top_scratch_init(TopScratch *scratch) {
  if (threadIdx.x < 32) {   // waves that do not exist never win a round
    scratch->sp[threadIdx.x >> 4][threadIdx.x & 15] = -1.0;
    scratch->st[threadIdx.x >> 4][threadIdx.x & 15] = kTopNone;
  }
  __syncthreads();
}
template <int E, bool ORDERED>
__device__ __forceinline__ int64_t top_merge_rounds(const TopOut *cand, int64_t n, int64_t maxCount, TopScratch *scratch) {
  double p[E];
  int t[E];
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int64_t i = threadIdx.x + (int64_t)e * blockDim.x;
    const TopOut c = i < n ? cand[i] : TopOut{-1, -1.0};
    p[e] = c.prob > 0.0 ? c.prob : -1.0;
    t[e] = (int)c.iTarget;
  }
  return top_rounds<E, ORDERED>(p, t, maxCount, scratch->staged, scratch->sp, scratch->st);
}
// workgroup (group, quiz): lists [group * fanIn, ...) of the quiz's nLists lists of maxCount records -> list `group` of the next level
// (256 threads for up to 4096 candidates, 1024 beyond: a round costs every wave its all-reduces, whatever it holds).  The winners are
// staged in LDS and leave in one burst: the last level's list goes to host-coherent memory, where a store per round would cost more
// than the round.  ORDERED = false: the lists of a listing among a listed set, whose targets follow the caller's list (lane_best).
template <bool ORDERED>
__global__ __launch_bounds__(1024) void top_merge_kernel(const TopOut *__restrict__ lists, int64_t nLists, int64_t fanIn, int64_t maxCount,
                                                         TopOut *outLists, int64_t *nOut, uint64_t *flag, uint64_t flagValue) {
  __shared__ TopScratch scratch;
  top_scratch_init(&scratch);
  const int64_t group = blockIdx.x, quiz = blockIdx.y;
  const int64_t first = group * fanIn, limit = first + fanIn < nLists ? first + fanIn : nLists;
  const TopOut *cand = lists + (quiz * nLists + first) * maxCount;
  const int64_t n = (limit - first) * maxCount;
  int64_t listed;
  if (n <= blockDim.x) listed = top_merge_rounds<1, ORDERED>(cand, n, maxCount, &scratch);
  else if (n <= 4 * (int64_t)blockDim.x) listed = top_merge_rounds<4, ORDERED>(cand, n, maxCount, &scratch);
  else listed = top_merge_rounds<16, ORDERED>(cand, n, maxCount, &scratch);
  __syncthreads();
  TopOut *list = outLists + (quiz * gridDim.x + group) * maxCount;
  for (int64_t i = threadIdx.x; i < maxCount; i += blockDim.x) list[i] = i < listed ? scratch.staged[i] : TopOut{-1, -1.0};
  if (nOut != nullptr || flag != nullptr) {   // (the last level)
    __syncthreads();
    if (threadIdx.x == 0) {
      if (nOut != nullptr) nOut[quiz] = listed;
      if (flag != nullptr) {   // (one flag per quiz: flag[0] where one quiz is listed)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __hip_atomic_store(flag + quiz, flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}
// ---- ListTopTargetsAmongBatch: the best targets within a LISTED set ---------------------------------------------------------------------
// Level 0 that gathers instead of streaming: grid (chunks of the group's longest list, quiz).  Every wave takes 1024 consecutive entries
// of its quiz's list, 16 per lane: the ids loaded coalesced (int32, staged by the host: in [0, T), no id twice in a list), prior[id] and
// the gap word gathered -- sixteen independent loads a lane, issued before the first is used.  The candidates (no gap, probability > 0)
// go through the wave's rounds with t = the id; nothing ascends along a caller's list, hence the rounds' unordered form.  A wave past
// the end of its quiz's list holds no candidate and writes only the padding.  partial[quiz][list]: the sum of the wave's candidates --
// a lane's sixteen in order, then the wave's butterfly: a fixed order, and no atomics.
struct TopAmongQuizzes { int32_t listOf[kTopBatchQuizzes]; };
__global__ __launch_bounds__(kTopChunkThreads) void top_among_chunks_kernel(TopBatchPriors priors, TopAmongQuizzes quizzes, const int64_t *__restrict__ offsets,
                                                                            const int32_t *__restrict__ ids, const uint32_t *__restrict__ tgap,
                                                                            int64_t maxCount, TopOut *lists, double *__restrict__ partial) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int64_t quiz = blockIdx.y, nLists = (int64_t)gridDim.x * (kTopChunkThreads / kWave);
  const int64_t list = (int64_t)blockIdx.x * (kTopChunkThreads / kWave) + wave;
  const int64_t first = offsets[quizzes.listOf[quiz]], len = offsets[quizzes.listOf[quiz] + 1] - first;
  const int64_t iFirst = list * kTopWaveTargets;
  const double *prior = priors.prior[quiz];
  double p[16];
  int t[16];
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int64_t i = iFirst + lane + e * kWave;
    t[e] = i < len ? ids[first + i] : -1;
  }
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const bool ok = t[e] >= 0 && !bit_test(tgap, t[e]);
    p[e] = ok ? prior[t[e]] : -1.0;
    if (!(p[e] > 0.0)) p[e] = -1.0;       // gaps and probabilities <= 0 are no candidates (pqa_device.h)
  }
  double sum = 0.0;
#pragma unroll
  for (int e = 0; e < 16; e++) sum += p[e] > 0.0 ? p[e] : 0.0;
  sum = wave_sum(sum);
  if (lane == 0) partial[quiz * nLists + list] = sum;
  TopOut *mine = lists + (quiz * nLists + list) * maxCount;
  const int64_t listed = top_rounds_wave<16, false>(p, t, maxCount, mine);
  for (int64_t i = listed + lane; i < maxCount; i += kWave) mine[i] = TopOut{-1, -1.0};   // the rest of the list says "no candidate"
}
// mass[quiz] = the quiz's partial sums, list 0 first: one thread per quiz, into the host-coherent result lines.  (A wave beyond the quiz's
// own list has left +0: the sum does not depend on how long the group's longest list is.)
__global__ __launch_bounds__(kWave) void top_among_mass_kernel(const double *__restrict__ partial, int64_t nLists, int64_t nQuizzes, double *mass) {
  const int64_t quiz = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (quiz >= nQuizzes) return;
  double sum = 0.0;
  for (int64_t l = 0; l < nLists; l++) sum += partial[quiz * nLists + l];
  mass[quiz] = sum;
}
// Lists of more than 256 records a quiz: out[quiz * pitch + i] = the posterior of entry i of the quiz's list, -1 for a gap -- what the
// host then selects from.  grid (chunks of 256 entries of the group's longest list, quiz).
__global__ __launch_bounds__(256) void top_among_gather_kernel(TopBatchPriors priors, TopAmongQuizzes quizzes, const int64_t *__restrict__ offsets,
                                                               const int32_t *__restrict__ ids, const uint32_t *__restrict__ tgap, int64_t pitch,
                                                               double *__restrict__ out) {
  const int64_t quiz = blockIdx.y, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t first = offsets[quizzes.listOf[quiz]], len = offsets[quizzes.listOf[quiz] + 1] - first;
  if (i >= len) return;
  const int id = ids[first + i];
  out[quiz * pitch + i] = bit_test(tgap, id) ? -1.0 : priors.prior[quiz][id];
}

// ---- ListTopQuestions: the best next questions of a quiz, by priority ------------------------------------------------------------------
// The question-side twin of the listing above, over the priorities a sweep has left on the device: descending priority, ascending
// question among equal priorities.  A question is a candidate if its bit is clear in the question-gap bitmap AND in the quiz's asked
// bitmap and its priority is > 0 -- the sweeps write 0 for asked questions and gaps, but the bits are tested here all the same, so that
// a stale word of the vector is never listed; a NaN is no candidate.  Level 0 leaves a list per wave of 1024 questions, the merge
// levels above do the rest.  Indices are 32-bit and LOCAL (Q < 2^31); the host adds the shard's first question.
// Level 0 over a priority VECTOR (one quiz: the engine's own; a grid.y = quiz batch: blockIdx.y's, from its slot): top_chunks_kernel's
// shape -- every wave holds 1024 consecutive questions, 16 per lane, loaded coalesced, and lists its own best by itself.
// Bytes per quiz: 8 Q of priorities and Q / 4 of the two bitmaps.
__global__ __launch_bounds__(kTopChunkThreads) void top_questions_chunks_kernel(const QuizSlot *__restrict__ slots, const double *__restrict__ priority,
                                                                                const uint32_t *__restrict__ asked, const uint32_t *__restrict__ qgap,
                                                                                int64_t Q, int64_t maxCount, TopOut *lists) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int64_t quiz = blockIdx.y, nLists = (int64_t)gridDim.x * (kTopChunkThreads / kWave);
  const int64_t list = (int64_t)blockIdx.x * (kTopChunkThreads / kWave) + wave;
  const int64_t qFirst = list * kTopWaveTargets;
  if (slots != nullptr) {
    priority = slots[quiz].priority;
    asked = slots[quiz].asked;
  }
  double p[16];
  int t[16];
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int64_t qq = qFirst + lane + e * kWave;
    const bool ok = qq < Q && !bit_test(qgap, qq) && !bit_test(asked, qq);
    p[e] = ok ? priority[qq] : -1.0;
    if (!(p[e] > 0.0)) p[e] = -1.0;
    t[e] = (int)qq;
  }
  TopOut *mine = lists + (quiz * nLists + list) * maxCount;
  const int64_t listed = top_rounds_wave<16>(p, t, maxCount, mine);
  for (int64_t i = listed + lane; i < maxCount; i += kWave) mine[i] = TopOut{-1, -1.0};
}

// Level 0 over the quiz-minor priority MATRIX [Q][Bp] of the row-sharing and (quiz, chunk) sweeps.  A wave that walked its quiz's
// column would touch a 64-byte line per question and use 8 bytes of it -- every line pulled through the caches by eight waves.  Here
// a workgroup takes 1024 questions x 8 adjacent quiz columns: one 64-byte line per question, requested by this workgroup only, eight
// lanes along the quiz axis per line and eight lines per wave load; the tile is turned in LDS (64 KB: two workgroups per CU) and wave w
// then lists column w from LDS exactly as the vector form lists from registers.  The LDS index is swizzled (row ^ 8 * column) so that
// the eight columns of a row fall into different banks on the way in and a column reads without conflicts on the way out.
// Bytes per batch of n quizzes: 64 Q ceil(n / 8) of priorities -- grid.y has a column group per eight quizzes, so of a row's Bp columns
// (the batch rounded up to 64) only the lines that hold a quiz of the batch are read, each once: 16 of 64 columns at 9 quizzes; the
// last group's columns beyond the batch come with their line and are not listed -- and Q / 8 per quiz and bitmap.
constexpr int kTopQTileQuizzes = 8, kTopQTileThreads = kTopQTileQuizzes * kWave;
__global__ __launch_bounds__(kTopQTileThreads) void top_questions_tile_kernel(const double *__restrict__ priorityT, int64_t Bp, const QuizSlot *__restrict__ slots,
                                                                              int nSlots, const uint32_t *__restrict__ qgap, int64_t Q, int64_t maxCount,
                                                                              TopOut *lists) {
  __shared__ double tile[kTopQTileQuizzes * kTopWaveTargets];
  const int64_t chunk = blockIdx.x, nLists = gridDim.x, qFirst = chunk * kTopWaveTargets;
  const int col0 = (int)blockIdx.y * kTopQTileQuizzes;
  {
    const int c = threadIdx.x % kTopQTileQuizzes, r0 = threadIdx.x / kTopQTileQuizzes;
    constexpr int kRowsPerPass = kTopQTileThreads / kTopQTileQuizzes;
#pragma unroll 4
    for (int r = r0; r < kTopWaveTargets; r += kRowsPerPass) {
      const int64_t qq = qFirst + r;
      tile[c * kTopWaveTargets + (r ^ (c << 3))] = qq < Q ? priorityT[qq * Bp + col0 + c] : -1.0;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int quiz = col0 + wave;
  if (quiz >= nSlots) return;
  const uint32_t *asked = slots[quiz].asked;
  double p[16];
  int t[16];
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int r = lane + e * kWave;
    const int64_t qq = qFirst + r;
    const bool ok = qq < Q && !bit_test(qgap, qq) && !bit_test(asked, qq);
    p[e] = ok ? tile[wave * kTopWaveTargets + (r ^ (wave << 3))] : -1.0;
    if (!(p[e] > 0.0)) p[e] = -1.0;
    t[e] = (int)qq;
  }
  TopOut *mine = lists + ((int64_t)quiz * nLists + chunk) * maxCount;
  const int64_t listed = top_rounds_wave<16>(p, t, maxCount, mine);
  for (int64_t i = listed + lane; i < maxCount; i += kWave) mine[i] = TopOut{-1, -1.0};
}
}  // namespace

// ---- ListTopTargets in the REFERENCE'S order among equal probabilities (round 6) --------------------------------------------------
// Where the listing above shows equal probabilities among the listed targets, or between the last listed and the next, what the
// reference returns is decided by its heaps (PqaCore/CEListTopTargetsAlgorithm.cpp:30-95): the target axis in one piece per worker
// thread (CalcSplit), every piece's candidates -- no gaps, prob > 0 -- in index order made a heap (std::make_heap,
// CEHeapifyPriorsSubtaskMake.cpp:56-88), then a head heap over the pieces' tops that pops maxCount times.  Reproduced step for step:
//   * top_pieces_kernel, a workgroup per (piece, quiz): the candidates compacted in index order into LDS (a piece of more than 8192
//     candidates: into global scratch); std::make_heap level by level -- the library sifts the holes n/2 - 1 ... 0 in turn, deeper
//     levels before shallower ones, and the subtrees of one level are disjoint: a level's holes sift side by side, a barrier between
//     levels, the same heap --; then ONE thread pops the piece's first maxCount tops, which are what the piece yields whatever the
//     other pieces do (a piece's heap changes only when its own top is taken);
//   * top_heads_kernel, a thread per quiz: the head heap over the pieces' first tops (std::make_heap), maxCount times the top, the
//     piece's next key and SRHeapHelper::Down (SRPlatform/Interface/SRHeap.h:16-39) -- or std::pop_heap when the piece is exhausted.
// The heap steps are the algorithm MSVC's and libstdc++'s libraries share (the oracle's restatement is held to libstdc++'s).
namespace {
struct HeapRec { double prob; int64_t id; };
__device__ __forceinline__ void heap_push_by_index(HeapRec *first, int64_t hole, int64_t top, HeapRec val) {
  for (int64_t idx = (hole - 1) >> 1; top < hole && first[idx].prob < val.prob; idx = (hole - 1) >> 1) {
    first[hole] = first[idx];
    hole = idx;
  }
  first[hole] = val;
}
__device__ __forceinline__ void heap_adjust(HeapRec *first, int64_t hole, int64_t bottom, HeapRec val) {
  const int64_t top = hole;
  int64_t idx = hole;
  const int64_t maxNonLeaf = (bottom - 1) >> 1;
  while (idx < maxNonLeaf) {                         // the hole moves down to the larger child (the right one unless it is less)
    idx = 2 * idx + 2;
    if (first[idx].prob < first[idx - 1].prob) --idx;
    first[hole] = first[idx];
    hole = idx;
  }
  if (idx == maxNonLeaf && bottom % 2 == 0) {        // an only child at the bottom
    first[hole] = first[bottom - 1];
    hole = bottom - 1;
  }
  heap_push_by_index(first, hole, top, val);
}
__device__ __forceinline__ void heap_pop(HeapRec *first, int64_t n) {   // std::pop_heap: the top goes to first[n - 1]
  if (n < 2) return;
  const HeapRec val = first[n - 1];
  first[n - 1] = first[0];
  heap_adjust(first, 0, n - 1, val);
}
__device__ __forceinline__ void heap_down(HeapRec *first, int64_t n) {  // SRHeapHelper::Down
  int64_t cur = 0;
  for (;;) {
    const int64_t c1 = 2 * cur + 1;
    if (c1 >= n) return;
    const int64_t c2 = c1 + 1;
    if (c2 >= n) {
      if (first[cur].prob < first[c1].prob) { const HeapRec t = first[cur]; first[cur] = first[c1]; first[c1] = t; }
      return;
    }
    const int64_t hi = first[c2].prob < first[c1].prob ? c1 : c2;
    if (!(first[cur].prob < first[hi].prob)) return;
    const HeapRec t = first[cur]; first[cur] = first[hi]; first[hi] = t;
    cur = hi;
  }
}

constexpr int kTopPieceThreads = 256;
constexpr int64_t kTopPieceLds = 8192;               // candidates of a piece held in LDS (128 KB)
struct TopExactArgs {
  TopBatchPriors priors;
  const uint32_t *tgap;
  int64_t T, quot, rem, nSub, maxCount;              // CalcSplit(T, nWorkers): piece i = [i quot + min(i, rem), ...) of quot + (i < rem) targets
  HeapRec *heaps;                                    // [quiz][T]: the pieces that do not fit LDS (null: all fit)
  TopOut *lists;                                     // [quiz][nSub][maxCount]: a piece's first tops, in the order it yields them
  int32_t *counts;                                   // [quiz][nSub]: min(candidates of the piece, maxCount + 1)
  TopOut *out;                                       // [quiz][maxCount]
  int64_t *nOut;                                     // [quiz]
  uint64_t *flag;                                    // (one quiz) set to flagValue behind the results
  uint64_t flagValue;
};

__global__ __launch_bounds__(kTopPieceThreads) void top_pieces_kernel(TopExactArgs a) {
  extern __shared__ double smem[];
  __shared__ int64_t waveCount[kTopPieceThreads / kWave];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int64_t piece = blockIdx.x, quiz = blockIdx.y;
  const int64_t first = piece * a.quot + (piece < a.rem ? piece : a.rem), size = a.quot + (piece < a.rem ? 1 : 0), limit = first + size;
  const double *prior = a.priors.prior[quiz];
  HeapRec *h = a.heaps == nullptr ? reinterpret_cast<HeapRec *>(smem) : a.heaps + quiz * a.T + first;   // (the launcher's choice, by the largest piece)
  // ---- the candidates, in index order (CEHeapifyPriorsSubtaskMake.cpp:42-52, :66-83)
  int64_t m = 0;
  for (int64_t base = first; base < limit; base += kTopPieceThreads) {
    const int64_t t = base + tid;
    double p = 0.0;
    bool ok = t < limit && !bit_test(a.tgap, t);
    if (ok) { p = prior[t]; ok = p > 0.0; }
    const unsigned long long mask = __ballot(ok);
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) waveCount[wave] = __popcll(mask);
    __syncthreads();
    int64_t off = m;
    for (int w = 0; w < wave; w++) off += waveCount[w];
    if (ok) h[off + rank] = HeapRec{p, t};
    int64_t all = 0;
    for (int w = 0; w < kTopPieceThreads / kWave; w++) all += waveCount[w];
    m += all;
    __syncthreads();
  }
  // ---- std::make_heap (:87), level by level
  if (m >= 2) {
    const int64_t lastInternal = m / 2 - 1;
    int L = 0;
    while (((int64_t)2 << L) - 1 <= lastInternal) L++;          // the deepest level with an internal node: 2^L - 1 <= lastInternal
    for (; L >= 0; L--) {
      const int64_t lo = ((int64_t)1 << L) - 1, hiNode = ((int64_t)2 << L) - 2 < lastInternal ? ((int64_t)2 << L) - 2 : lastInternal;
      for (int64_t j = lo + tid; j <= hiNode; j += kTopPieceThreads) heap_adjust(h, j, m, h[j]);
      __syncthreads();
    }
  }
  // ---- what the piece yields, in turn: its top, then std::pop_heap (CEListTopTargetsAlgorithm.cpp:74-91)
  if (tid == 0) {
    const int64_t cnt = m < a.maxCount ? m : a.maxCount;
    TopOut *mine = a.lists + (quiz * a.nSub + piece) * a.maxCount;
    int64_t n = m;
    for (int64_t r = 0; r < cnt; r++) {
      mine[r] = TopOut{h[0].id, h[0].prob};
      if (r + 1 < cnt) { heap_pop(h, n); n--; }
    }
    a.counts[quiz * a.nSub + piece] = (int32_t)(m < a.maxCount + 1 ? m : a.maxCount + 1);
  }
}

__global__ __launch_bounds__(kWave) void top_heads_kernel(TopExactArgs a) {
  extern __shared__ double smem[];
  HeapRec *head = reinterpret_cast<HeapRec *>(smem);           // [nSub]
  int32_t *taken = reinterpret_cast<int32_t *>(head + a.nSub); // [nSub]
  const int64_t quiz = blockIdx.x;
  if (threadIdx.x != 0) return;
  const TopOut *lists = a.lists + quiz * a.nSub * a.maxCount;
  const int32_t *counts = a.counts + quiz * a.nSub;
  int64_t nHh = 0;
  for (int64_t i = 0; i < a.nSub; i++) {                        // :58-66: the pieces that have a candidate, in piece order
    taken[i] = 0;
    if (counts[i] == 0) continue;
    head[nHh++] = HeapRec{lists[i * a.maxCount].prob, i};
  }
  for (int64_t hole = nHh >> 1; hole > 0;) { --hole; heap_adjust(head, hole, nHh, head[hole]); }   // std::make_heap :67
  TopOut *out = a.out + quiz * a.maxCount;
  int64_t listed = a.maxCount;
  for (int64_t i = 0; i < a.maxCount; i++) {                    // :69-95
    if (nHh == 0) { listed = i; break; }
    const int64_t piece = head[0].id;
    out[i] = lists[piece * a.maxCount + taken[piece]];
    taken[piece]++;
    if (taken[piece] == counts[piece]) {                        // the piece is exhausted (:81-88)
      heap_pop(head, nHh);
      nHh--;
      continue;
    }
    if (i + 1 == a.maxCount) break;                             // (the key behind the last listed target is never looked at)
    head[0].prob = lists[piece * a.maxCount + taken[piece]].prob;   // :93
    heap_down(head, nHh);                                       // :94
  }
  for (int64_t i = listed; i < a.maxCount; i++) out[i] = TopOut{-1, -1.0};
  a.nOut[quiz] = listed;
  if (a.flag != nullptr) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __hip_atomic_store(a.flag, a.flagValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
}  // namespace

// scratch of the exact listing for nQuizzes quizzes: bytes of {the pieces' lists, their counts, the heaps of pieces beyond LDS}
size_t TopExactScratchBytes(int64_t T, int64_t nWorkers, int64_t maxCount, int64_t nQuizzes) {
  const int64_t quot = T / nWorkers, rem = T % nWorkers, nSub = quot == 0 ? rem : nWorkers;
  const bool big = quot + (rem ? 1 : 0) > kTopPieceLds;
  return (size_t)nQuizzes * ((size_t)nSub * (size_t)maxCount * sizeof(TopOut) + (size_t)nSub * sizeof(int32_t) + 16 + (big ? (size_t)T * sizeof(HeapRec) : 0));
}
hipError_t LaunchTopTargetsExact(const KbView &kb, const TopBatchPriors &priors, int64_t nQuizzes, int64_t nWorkers, int64_t maxCount, void *scratch,
                                 RatedTargetDev *out, int64_t *nOut, uint64_t *flag, uint64_t flagValue, hipStream_t stream) {
  if (nQuizzes <= 0 || nQuizzes > kTopBatchQuizzes || maxCount <= 0 || nWorkers < 1 || scratch == nullptr || (flag != nullptr && nQuizzes != 1)) return hipErrorInvalidValue;
  TopExactArgs a{};
  a.priors = priors; a.tgap = kb.tgap; a.T = kb.T; a.maxCount = maxCount;
  a.quot = kb.T / nWorkers; a.rem = kb.T % nWorkers; a.nSub = a.quot == 0 ? a.rem : nWorkers;   // SRPoolRunner::CalcSplit, SRPoolRunner.h:96-110
  const int64_t pieceMax = a.quot + (a.rem ? 1 : 0);
  const bool big = pieceMax > kTopPieceLds;
  char *p = static_cast<char *>(scratch);
  a.lists = reinterpret_cast<TopOut *>(p);
  p += (size_t)nQuizzes * a.nSub * maxCount * sizeof(TopOut);
  a.heaps = big ? reinterpret_cast<HeapRec *>(p) : nullptr;
  if (big) p += (size_t)nQuizzes * kb.T * sizeof(HeapRec);
  a.counts = reinterpret_cast<int32_t *>(p);
  a.out = reinterpret_cast<TopOut *>(out); a.nOut = nOut; a.flag = flag; a.flagValue = flagValue;
  const size_t shPieces = big ? 16 : (size_t)pieceMax * sizeof(HeapRec);
  if (shPieces > kLdsNoOptIn) {   // (the opt-in to more than 64 KiB of dynamic LDS: once per device, for the largest size)
    static LaunchCache cache;
    const hipError_t e = cache.OptIn(DeviceSlot(), top_pieces_kernel, kTopPieceLds * sizeof(HeapRec));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(top_pieces_kernel, dim3((unsigned)a.nSub, (unsigned)nQuizzes), dim3(kTopPieceThreads), shPieces, stream, a);
  const size_t shHeads = (size_t)a.nSub * (sizeof(HeapRec) + sizeof(int32_t)) + 16;
  hipLaunchKernelGGL(top_heads_kernel, dim3((unsigned)nQuizzes), dim3(kWave), shHeads, stream, a);
  return hipGetLastError();
}

static int64_t TopBatchLists(int64_t T) { return (T <= 0 ? 1 : (T + kTopChunkTargets - 1) / kTopChunkTargets) * (kTopChunkThreads / kWave); }
static int64_t TopFanIn(int64_t maxCount) { const int64_t f = kTopMergeCapacity / maxCount; return f < 2 ? 2 : f; }
// The merge levels over nLists lists of maxCount records per quiz in scratchA: 16384 / maxCount lists per workgroup and level, until one
// list per quiz is left; that level writes out / nOut (and flag[quiz], where a flag is given).
template <bool ORDERED = true>
static hipError_t LaunchTopMerges(int64_t nLists, int64_t nQuizzes, int64_t maxCount, RatedTargetDev *scratchA, RatedTargetDev *scratchB,
                                  RatedTargetDev *out, int64_t *nOut, uint64_t *flag, uint64_t flagValue, hipStream_t stream) {
  const int64_t fanIn = TopFanIn(maxCount);
  RatedTargetDev *src = scratchA, *dst = scratchB;
  for (;;) {
    const int64_t nGroups = (nLists + fanIn - 1) / fanIn;
    const bool last = nGroups == 1;
    const int threads = (nLists < fanIn ? nLists : fanIn) * maxCount <= 4096 ? 256 : 1024;
    hipLaunchKernelGGL(top_merge_kernel<ORDERED>, dim3((unsigned)nGroups, (unsigned)nQuizzes), dim3(threads), 0, stream, reinterpret_cast<const TopOut *>(src), nLists,
                       fanIn, maxCount, reinterpret_cast<TopOut *>(last ? out : dst), last ? nOut : nullptr, last ? flag : nullptr, flagValue);
    if (last) break;
    nLists = nGroups;
    RatedTargetDev *t = src; src = dst; dst = t;
  }
  return hipGetLastError();
}
// records per quiz each of the two scratch buffers must hold
int64_t TopBatchScratchRecords(int64_t T, int64_t maxCount) { return TopBatchLists(T) * maxCount; }
hipError_t LaunchTopTargetsBatch(const KbView &kb, const TopBatchPriors &priors, int64_t nQuizzes, int64_t maxCount, RatedTargetDev *scratchA,
                                 RatedTargetDev *scratchB, RatedTargetDev *out, int64_t *nOut, uint64_t *flag, uint64_t flagValue,
                                 hipStream_t stream) {
  if (nQuizzes <= 0 || nQuizzes > kTopBatchQuizzes || maxCount <= 0 || maxCount > 256 || (flag != nullptr && nQuizzes != 1)) return hipErrorInvalidValue;
  int64_t nLists = TopBatchLists(kb.T);
  hipLaunchKernelGGL(top_chunks_kernel, dim3((unsigned)(nLists / (kTopChunkThreads / kWave)), (unsigned)nQuizzes), dim3(kTopChunkThreads), 0, stream, priors,
                     kb.tgap, kb.T, maxCount, reinterpret_cast<TopOut *>(scratchA));
  return LaunchTopMerges(nLists, nQuizzes, maxCount, scratchA, scratchB, out, nOut, flag, flagValue, stream);
}

// ListTopQuestions: level 0 in the form the priorities lie in, then the merges.  The scratch buffers hold what LaunchTopTargetsBatch's
// would for rows of Q elements.
int64_t TopQuestionsScratchRecords(int64_t Q, int64_t maxCount) { return TopBatchLists(Q) * maxCount; }
hipError_t LaunchTopQuestions(const TopQuestions &a, int64_t maxCount, RatedTargetDev *scratchA, RatedTargetDev *scratchB, RatedTargetDev *out,
                              int64_t *nOut, uint64_t *flags, uint64_t flagValue, hipStream_t stream) {
  if (a.nQuizzes <= 0 || a.nQuizzes > kTopBatchQuizzes || maxCount <= 0 || maxCount > 256 || a.Q <= 0 || a.Q > 0x7FFFFFFF || a.qgap == nullptr) return hipErrorInvalidValue;
  if (a.slots == nullptr ? (a.nQuizzes != 1 || a.priority == nullptr || a.asked == nullptr || a.Bp != 0) : (a.Bp != 0 && a.priority == nullptr)) return hipErrorInvalidValue;
  int64_t nLists;
  if (a.Bp == 0) {
    nLists = TopBatchLists(a.Q);
    hipLaunchKernelGGL(top_questions_chunks_kernel, dim3((unsigned)(nLists / (kTopChunkThreads / kWave)), (unsigned)a.nQuizzes), dim3(kTopChunkThreads), 0, stream,
                       a.slots, a.priority, a.asked, a.qgap, a.Q, maxCount, reinterpret_cast<TopOut *>(scratchA));
  } else {
    if (a.Bp % kTopQTileQuizzes != 0 || a.nQuizzes > a.Bp) return hipErrorInvalidValue;
    nLists = (a.Q + kTopWaveTargets - 1) / kTopWaveTargets;
    hipLaunchKernelGGL(top_questions_tile_kernel, dim3((unsigned)nLists, (unsigned)((a.nQuizzes + kTopQTileQuizzes - 1) / kTopQTileQuizzes)), dim3(kTopQTileThreads), 0,
                       stream, a.priority, (int64_t)a.Bp, a.slots, a.nQuizzes, a.qgap, a.Q, maxCount, reinterpret_cast<TopOut *>(scratchA));
  }
  return LaunchTopMerges(nLists, a.nQuizzes, maxCount, scratchA, scratchB, out, nOut, flags, flagValue, stream);
}

// ListTopTargetsAmongBatch: level 0 over the staged lists (offsets | ids on the device, listOf[quiz] the quiz's list), the masses, then
// the merges.  nLists lists a quiz: a wave per 1024 entries of the group's longest list.
static int64_t TopAmongLists(int64_t longest) { return TopBatchLists(longest); }
int64_t TopAmongScratchRecords(int64_t longest, int64_t maxCount) { return TopAmongLists(longest) * maxCount; }
int64_t TopAmongPartials(int64_t longest) { return TopAmongLists(longest); }
hipError_t LaunchTopTargetsAmong(const KbView &kb, const TopBatchPriors &priors, const int32_t *listOf, int64_t nQuizzes, const int64_t *offsets,
                                 const int32_t *ids, int64_t longest, int64_t maxCount, RatedTargetDev *scratchA, RatedTargetDev *scratchB,
                                 double *partial, RatedTargetDev *out, int64_t *nOut, double *mass, hipStream_t stream) {
  if (nQuizzes <= 0 || nQuizzes > kTopBatchQuizzes || maxCount <= 0 || maxCount > 256 || longest <= 0 || longest > kb.T || offsets == nullptr || ids == nullptr ||
      listOf == nullptr || partial == nullptr || mass == nullptr)
    return hipErrorInvalidValue;
  TopAmongQuizzes qs;
  for (int64_t i = 0; i < nQuizzes; i++) qs.listOf[i] = listOf[i];
  const int64_t nLists = TopAmongLists(longest);
  hipLaunchKernelGGL(top_among_chunks_kernel, dim3((unsigned)(nLists / (kTopChunkThreads / kWave)), (unsigned)nQuizzes), dim3(kTopChunkThreads), 0, stream, priors,
                     qs, offsets, ids, kb.tgap, maxCount, reinterpret_cast<TopOut *>(scratchA), partial);
  hipLaunchKernelGGL(top_among_mass_kernel, dim3((unsigned)((nQuizzes + kWave - 1) / kWave)), dim3(kWave), 0, stream, partial, nLists, nQuizzes, mass);
  return LaunchTopMerges<false>(nLists, nQuizzes, maxCount, scratchA, scratchB, out, nOut, nullptr, 0, stream);
}
hipError_t LaunchTopAmongGather(const KbView &kb, const TopBatchPriors &priors, const int32_t *listOf, int64_t nQuizzes, const int64_t *offsets,
                                const int32_t *ids, int64_t longest, double *out, hipStream_t stream) {
  if (nQuizzes <= 0 || nQuizzes > kTopBatchQuizzes || longest <= 0 || longest > kb.T || offsets == nullptr || ids == nullptr || listOf == nullptr || out == nullptr)
    return hipErrorInvalidValue;
  TopAmongQuizzes qs;
  for (int64_t i = 0; i < nQuizzes; i++) qs.listOf[i] = listOf[i];
  hipLaunchKernelGGL(top_among_gather_kernel, dim3((unsigned)((longest + 255) / 256), (unsigned)nQuizzes), dim3(256), 0, stream, priors, qs, offsets, ids, kb.tgap,
                     longest, out);
  return hipGetLastError();
}
}  // namespace pqa
