// pqa_kernels.h -- launch wrappers for the CDNA4 (gfx950) kernels of the ProbQA question-evaluation hot path.
// Host code (hip_engine.cpp) only sees these plain functions; everything runs on the stream it is given.
//
// Device layout of the knowledge base (one allocation, "cube"):
//   cube[q][r][t],  q in [0,Q), r in [0,K] , t in [0,ldT)      -- fp64
//     r <  K : sA[q][r][t]   squared answer counts        (reference: PqaCore/CpuEngine.decl.h:31-37 `_sA`)
//     r == K : mD[q][t]      sum over answers of sA       (reference: `_mD`)
//   ldT = T rounded up to 16 doubles (128 B) so every row starts on a cache line and 16-byte lane loads never straddle
//   rows.  Padding columns t in [T,ldT) hold A=0, D=1 and are flagged as gaps in the target-gap bitmap.
//   vB[t] (ldT doubles) is separate.  Bitmaps are uint32 words, LSB-first, bits past the size set (gap) as in
//   PqaCore/GapTracker.h:9-15; the "asked" bitmap of a quiz has bits past Q clear.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "select_record.h"

namespace pqa {

constexpr size_t kLdsPerCU = 160 * 1024;     // LDS of a CU (gfx950)
constexpr size_t kLdsNoOptIn = 64 * 1024;    // dynamic LDS a launch gets without opting in (hipFuncAttributeMaxDynamicSharedMemorySize)
constexpr double kLnSqrt2 = 0.34657359027997265470861606072909;   // SRMath::_cLnSqrt2 (host and device)

constexpr int kMaxDevices = 64;
inline int DeviceSlot() { int d = 0; return hipGetDevice(&d) == hipSuccess ? (d & (kMaxDevices - 1)) : 0; }
// CUs of the current device, whose slot is `dev` (256 where the runtime does not say); asked once per process and device
inline int DeviceCUs(int dev) {
  static std::atomic<int> numCUs[kMaxDevices];
  int n = numCUs[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    int d = 0;
    n = (hipGetDevice(&d) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && n > 0) ? n : 256;
    numCUs[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}
inline int DeviceCUs() { return DeviceCUs(DeviceSlot()); }

// What a launch wrapper has asked the runtime about one kernel instantiation, PER DEVICE: the opt-in to more than 64 KiB of
// dynamic LDS (hipFuncSetAttribute) belongs to the device that was current when it was made, and one process drives
// several devices (sharded_engine.cpp).  One function-local static per instantiation; engines on different threads may
// race for a slot -- they would store the same value.
struct LaunchCache {
  std::atomic<uint64_t> slot[kMaxDevices];   // (key << 16) | (workgroups per CU + 1); 0 = nothing asked yet
  bool Get(int dev, size_t key, int *perCU) const {
    const uint64_t v = slot[dev].load(std::memory_order_acquire);
    if (v == 0 || (v >> 16) != (uint64_t)key) return false;
    *perCU = (int)(v & 0xFFFF) - 1;
    return true;
  }
  void Put(int dev, size_t key, int perCU) { slot[dev].store(((uint64_t)key << 16) | (uint64_t)(perCU + 1), std::memory_order_release); }
  // Uncached: the opt-in where shmem needs one -- its error is the result -- then the runtime's workgroups per CU (0: it did not say).
  static hipError_t Ask(const void *kern, int threads, size_t shmem, int *perCU) {
    *perCU = 0;
    if (shmem > kLdsNoOptIn) {
      const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
      if (e != hipSuccess) return e;
    }
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(perCU, kern, threads, shmem) != hipSuccess) *perCU = 0;
    return hipSuccess;
  }
  // Workgroups of `threads` threads and `shmem` bytes of dynamic LDS that a CU of the current device holds (at least 1).  Attribute
  // and occupancy are properties of (kernel, LDS size, device): asked once per device and `key` -- the LDS size, or what else the
  // caller's shape depends on -- not on every launch.  A failed opt-in is returned and not remembered.  dev: DeviceSlot().
  template <typename Kern>
  hipError_t Residency(int dev, Kern *kern, int threads, size_t shmem, size_t key, int *perCU) {
    if (Get(dev, key, perCU)) return hipSuccess;
    const hipError_t e = Ask(reinterpret_cast<const void *>(kern), threads, shmem, perCU);
    if (e != hipSuccess) return e;
    if (*perCU < 1) *perCU = 1;
    Put(dev, key, *perCU);
    return hipSuccess;
  }
  template <typename Kern>
  hipError_t Residency(int dev, Kern *kern, int threads, size_t shmem, int *perCU) { return Residency(dev, kern, threads, shmem, shmem, perCU); }
  // The opt-in alone, once per device (and key), for a kernel whose grid does not depend on the occupancy: up to maxShmem bytes.
  template <typename Kern>
  hipError_t OptIn(int dev, Kern *kern, size_t maxShmem, size_t key = 1) {
    int done = 0;
    if (Get(dev, key, &done)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)maxShmem);
    if (e == hipSuccess) Put(dev, key, 1);
    return e;
  }
};

struct KbView {
  const void *cube;       // [Q][K+1][ldT], elements of `elem` bytes: double (Double engines) or float (Float engines)
  int elem;               // 8 | 4
  const double *vB;       // [ldT]
  const uint32_t *tgap;   // target gap bits, ldT bits (+ slack), bits >= T set
  const uint32_t *qgap;   // question gap bits, bits >= Q set
  int64_t K, Q, T, ldT;
  int64_t nValidTargets;  // T - #target gaps (PqaCore/CpuEngine.cpp:352)
  int smallLaunches;      // the engine runs the resident sweep: posterior kernels over <= 1024 targets use 256 threads
  double *priorScratch;   // 8 * kMaxWorkers + 2 doubles (device): the subtasks' sums of the long-row posterior kernels (prior_kernels.hip); may be null
  int maxGrid;            // test hook (engine option "eval_max_grid"): cap the workgroups of a sweep, so that a small cube makes
                          // every workgroup stream dozens of questions; 0 = no cap
  int clusterForm;        // long rows (cluster_kernels.hip): 0 = default, 1 = question by question, 2 = pass 1 a question ahead (option cluster_form)
  int clusterShape;       // ... the shape of the form that runs ahead: 0 = default, 1 = 512 threads x 1 unit, 2 = 256 x 2 (option cluster_shape)
  int64_t clusterFrom;    // rows LONGER than this many elements take the cluster sweep (engine option cluster_from)
  double *poleScratch;    // Q x (2 K + 2) doubles (device): the sums of questions with a row at the pole of the lack term, between the
                          // sweep and the fix launched behind it (pole_kernels.hip); may be null (then such questions keep the sweep's own sums)
  struct PoleHeader *poleList;   // ... and the list of those questions: PoleListBytes(Q) bytes, zeroed once (every launch leaves it empty)
  int poleNoFollow;       // measurement hook (engine option "pole_follow" = 0): the watching sweep WITHOUT the launch behind it -- for timing the sweep
                          // kernel by itself in a quiz state that lists nothing; anything listed would stay listed
  int poleGate;           // engine option "pole_gate" (default 1): where only the ARGMAX leaves the engine (a fused single-quiz argmax), the fix
                          // redoes only the listed questions that can still win (pole_kernels.hip: pole_bounds_kernel) -- the register-shape
                          // sweeps then track, per listed question, how close to 1 its largest posterior element can be
};

// vCompTail of the epilogue (eval_device.h): ln(sqrt 2) / (nValidTargets + 1)^2, PqaCore/CEEvalQsSubtaskConsider.cpp:191, with the
// reference's two operations
inline double VCompTail(const KbView &kb) {
  const double nT = (double)(kb.nValidTargets + 1);
  return kLnSqrt2 / (nT * nT);
}

// ---- questions with a row at the pole of the lack term: listed by the sweeps, redone in the reference's order behind them
// (pole_kernels.hip).  A list is a header and `capacity` entries; a sweep appends at most one entry per question (and quiz).
struct PoleHeader { uint32_t count, arrived; unsigned long long floorBits; };   // floorBits: see PoleFix::gate
struct PoleEntry {
  uint32_t q;             // position in the priority vector (question qFirst + q of the cube)
  uint32_t rowMask;       // the answer rows that passed the sweep's watch, a bit each (0: not known -- every row is redone)
  uint32_t b;             // the quiz (batched sweeps; 0 otherwise)
  uint32_t gap;           // float bits.  From a sweep that tracks it (KbView::poleGate): a lower bound of 1 - p for the largest posterior
                          // element of the question's listed rows (0: not known); then, from pole_bounds_kernel: how far the fix can move
                          // the question's priority, relative (+inf: not known)
};
static_assert(sizeof(PoleHeader) == 16, "header and entries are 16 bytes each");
size_t PoleListBytes(int64_t capacity);
hipError_t UploadLog2TablePole(const double *hostTable);

struct SelectResult {     // 16 bytes, written by the select kernels
  double priority;        // argmax: winning priority; sampled: grand total of priorities
  int64_t index;          // selected question (global index) or -1
};

// Upload the Log2Hot table (1024 x {log2 midpoint, 1/(2 midpoint)}, built by the host); once per process and device.
hipError_t UploadLog2Table(const double *hostTable);
// out[i] = the device log2hot(x[i]) (device pointers); test hook for the function the sweep applies per element.
hipError_t LaunchLog2HotArray(const double *x, double *out, int64_t n, hipStream_t stream);

// ---- a1: priority sweep.  priority[q - qFirst] for q in [qFirst,qLimit); 0 for gap / asked questions.
// Returns hipSuccess or the launch error.  `variant`: 0 = auto, otherwise forces a kernel shape (tests/bench).
// `fused` (optional): let the sweep's last workgroup also pick the argmax, so that a selection is one launch.
constexpr int kFusedMaxGrid = 4096;     // workgroups of a fused launch (one record each)
struct alignas(16) TaggedPriority { double priority; uint64_t tag; };

struct FusedSelect {
  SelectResult *scratch;  // records (16-byte aligned): the workgroups' winners, tagged per launch; kFusedMaxGrid of them
                          // for a single sweep, scratchStride per quiz for a batch
  SelectResult *out;      // device or host-coherent memory; index = position in priority[] + outBase
  uint64_t *seq;          // optional host-coherent flag, set to flagValue after `out` is visible
  uint64_t seqValue;      // launch tag: its low 32 bits must differ from those of the previous fused launch on `scratch`
  int64_t outBase;
  int64_t scratchStride;  // batch only: records per quiz in `scratch` (the launch uses at most that many workgroups)
  uint64_t flagValue;     // what *seq receives (the engine's own callers pass the launch tag)
  // Launches replayed from a HIP graph have constant arguments: with tagCell != nullptr both the launch tag and the flag
  // value are read from this device word instead, and the finisher advances it for the next replay.
  uint64_t *tagCell;
  // The reference's sampled selector instead of the argmax, in the same launch: once the finisher has seen every
  // workgroup's record, workgroup 0 runs the selection (select_sampled_wg_impl, pqa_device.h) over the priority vector and
  // writes {sum of priorities, selected position} to `out`.  sampleSubtasks > 0 switches it on; priorities, run lengths and
  // totals are staged in the LDS that held the Log2Hot table (EvalVariantFusesSampled says whether they fit).
  int64_t sampleSubtasks;
  uint64_t sampleRnd;
  double *runLength;
  // ... or, with hostPriority != nullptr (and sampleSubtasks > 0): the host runs the selector (O(Q) scalar Kahan steps,
  // microseconds) instead of a second kernel whose dispatch alone costs more.  Every workgroup stores the priorities of its own
  // questions into this host-coherent array as 16-byte records {priority, launch tag} (one store each, nothing waited for); the
  // finisher raises the flag once it has seen every workgroup's record; the host takes an entry when it carries the launch's tag
  // (it almost always does by then; a straggling store is waited for there, not by two thousand waves on the device).
  TaggedPriority *hostPriority;
  // A synchronous caller that waits on `seq` right behind its launch may ask for the fix of pole_kernels.hip only when the sweep
  // has listed something (lazyFix != 0; argmax and hostPriority forms): nothing is launched behind the sweep, and a finisher
  // that saw suspects publishes index -4 instead of leaving the publication to the fix; the caller then launches
  // LaunchEvalPoleFixup (same arguments, a new flagValue) and waits again.  A fresh quiz's selections so cost one launch, not two.
  int64_t lazyFix;
  // The engine's own pinned cell as destination (select_record.h): `out` is a PackedSelection -- {priority, low 32 bits of flagValue :
  // local index or code} in ONE write-through store, no fence, no flag (`seq` is not written), outBase added by the host.
  int64_t packed;
  // The forms the host builds, by name (the struct stays an aggregate of the fields above, in that order; FusedSelect{}: no selection):
  // the engine's own packed cell (select_record.h), waited for by its tag; an outside reader's record, index + outBase, with flagValue
  // to *flag behind it (flag may be null); a batch (grid.y = quiz: records and flags are the slots'); a graph replay into a packed cell
  static FusedSelect OwnCell(SelectResult *scratch, SelectResult *cell, uint64_t *seq, uint64_t tag) { FusedSelect f = Record(scratch, cell, seq, tag, tag, 0); f.packed = 1; return f; }
  static FusedSelect Record(SelectResult *scratch, SelectResult *out, uint64_t *flag, uint64_t tag, uint64_t flagValue, int64_t outBase) {
    FusedSelect f{};
    f.scratch = scratch; f.out = out; f.seq = flag; f.seqValue = tag; f.flagValue = flagValue; f.outBase = outBase;
    return f;
  }
  static FusedSelect Batch(SelectResult *scratch, int64_t scratchStride, uint64_t tag) { FusedSelect f = Record(scratch, nullptr, nullptr, tag, tag, 0); f.scratchStride = scratchStride; return f; }
  static FusedSelect Graph(SelectResult *scratch, SelectResult *cell, uint64_t *seq, uint64_t *tagCell) { FusedSelect f = OwnCell(scratch, cell, seq, 0); f.tagCell = tagCell; return f; }
  FusedSelect Sampled(int64_t nSub, uint64_t rnd, double *run) const { FusedSelect f = *this; f.sampleSubtasks = nSub; f.sampleRnd = rnd; f.runLength = run; return f; }
  FusedSelect HostPriority(TaggedPriority *buf) const { FusedSelect f = *this; f.sampleSubtasks = buf ? 1 : 0; f.hostPriority = buf; return f; }   // (null: the argmax stays)
  FusedSelect Lazy(bool on) const { FusedSelect f = *this; f.lazyFix = on ? 1 : 0; return f; }
};
// One quiz of a batched sweep (blockIdx.y selects it): everything that differs between the quizzes of one launch.
struct QuizSlot {
  const double *prior;
  const uint32_t *asked;
  double *priority;       // this quiz's priority vector
  SelectResult *out;      // host-coherent record of this quiz's winner
  uint64_t *seq;          // host-coherent flag of this quiz
  TaggedPriority *hostPriority;   // optional (grid.y = quiz launches with FusedSelect::sampleSubtasks > 0): this quiz's priorities go to
                                  // the host as tagged records, as FusedSelect::hostPriority delivers a single quiz's
};
hipError_t LaunchEvalQuestions(const KbView &kb, const double *prior, const uint32_t *asked, int64_t qFirst,
                               int64_t qLimit, double *priority, int variant, const FusedSelect *fused,
                               hipStream_t stream);
// the fix behind a sweep launched with FusedSelect::lazyFix whose answer was -4 (the sweep's own arguments; fused.flagValue: what the caller waits for now)
hipError_t LaunchEvalPoleFixup(const KbView &kb, const double *prior, const uint32_t *asked, double *priority, const FusedSelect &fused,
                               hipStream_t stream);
// The fix behind a watching sweep.  A record of sums is `sumsStride` doubles: W_k [K] at wOff, W_k sqrt(V_k) (secondIsWV) or V_k [K]
// at vOff, sum l log2 p at hOff, the lack sum at lOff; record of entry e: e itself (bySlot) or its question.  priority (or priorityT
// [q][Bp], or the quizzes' own vectors: slots) receives the corrected priorities -- all null: the records are corrected in place
// and the caller's epilogue follows.  fs: the sweep's own fused selection; when the list is not empty the sweep's finisher has left
// its publication to this launch.
struct PoleFix {
  const double *cube;
  const uint32_t *tgap, *qgap, *asked;
  const double *prior;            // single quiz
  const QuizSlot *slots;          // batched sweeps: entry.b selects the quiz
  int nSlots;                     // ... of a grid.y = quiz launch (fs set): this launch publishes every quiz's result when it has work
  PoleHeader *list;
  uint32_t *maskDense;            // optional [nQ]: the rows per question where several workgroups watch one question (cleared here)
  uint32_t *dirty;                // optional [quizzes]: set to 1 for every quiz with a corrected priority (batched sweeps: the pick reads it)
  double *sums;
  int64_t sumsStride;
  int bySlot, wOff, vOff, hOff, lOff, secondIsWV;
  double *priority, *priorityT;
  int Bp;
  TaggedPriority *hostPriority;   // optional: the corrected priorities also go to the host as {priority, hostTag} records
  uint64_t hostTag;
  int64_t K, T, ldT, qFirst, nQ, capacity;
  double vCompTail;
  FusedSelect fs;
  int rows, waveLds;              // (set by the launcher)
  // gate: only the argmax leaves the engine (fs names a fused argmax of ONE quiz, `priority` holds the sweep's vector, the entries carry
  // the sweep's gaps): a kernel ahead of the fix bounds, per listed question, how far the fix can move its priority, and the fix skips
  // the questions whose upper bound stays below the best lower bound (PoleHeader::floorBits) -- they cannot be the maximum.
  int gate;
};
hipError_t LaunchPoleFixup(const PoleFix &fix, hipStream_t stream);
// The fix behind a Double engine's sweep that leaves a record as W_k [K] | W_k sqrt(V_k) [K] | sum l log2 p | lack sum: the cube and what
// describes the record; the caller adds where the records, the list and the priorities lie.
inline PoleFix PoleFixWV(const double *cube, const uint32_t *tgap, const uint32_t *qgap, int64_t K, int64_t T, int64_t ldT) {
  PoleFix f{};
  f.cube = cube; f.tgap = tgap; f.qgap = qgap;
  f.K = K; f.T = T; f.ldT = ldT;
  f.sumsStride = 2 * K + 2;
  f.wOff = 0; f.vOff = (int)K; f.hOff = (int)(2 * K); f.lOff = (int)(2 * K + 1); f.secondIsWV = 1;
  return f;
}
// The same sweep for nSlots quizzes in one launch (grid.y = quiz): `slots` is a DEVICE array; fused->scratch holds
// nSlots * fused->scratchStride records; fused->out / seq are ignored (each slot has its own).
// pole (optional): EvalBatchPoleBytes(kb, nSlots) bytes of device memory, the first kBatchPoleClear cleared once after allocation -- the
// batch's suspect list and records (pole_kernels.hip); without it the quizzes of the launch keep the sweep's own sums at the pole.
size_t EvalBatchPoleBytes(const KbView &kb, int nSlots);
hipError_t LaunchEvalQuestionsBatch(const KbView &kb, const QuizSlot *slots, int nSlots, int64_t qFirst, int64_t qLimit,
                                    int variant, const FusedSelect &fused, hipStream_t stream, void *pole = nullptr);
// ---- many quizzes per sweep, one cube read per batch (batch_kernels.hip): lane = quiz, the cube tile staged in LDS is shared by
// all quizzes of the batch.  Double and Float engines.  nSlots <= 256.
constexpr int kBatchMaxGrid = 2048;
struct BatchRecord { double priority; int64_t index; };   // a workgroup's best question of one quiz (index < 0: none)
struct BatchPlan {
  int tileTargets;        // in: targets per LDS tile (0 = default)
  int questionsPerBlock;  // in: questions staged together (0 = default: 4 fp32, 2 fp64; else the largest built shape <= this)
  int splitTail;          // in: 1 = the questions of the last, partial round of the persistent grid go to a second launch with fewer questions per group (LaunchEvalBatch)
  int questionGroups;     // in: question groups side by side in a workgroup of a small batch (0 = automatic; see eval_batch_kernel)
  int grid, Bp;           // out: workgroups of the sweep; quizzes rounded up to whole waves
  size_t ptBytes, accBytes, recBytes;   // out: sizes of the scratch buffers PT / acc / recs the caller provides
  size_t poleBytes;       // out: ... and of `pole` (0: the sweep does not watch for rows at the pole of the lack term -- pole_kernels.hip)
  void *pole;             // in: poleBytes of device memory whose first kBatchPoleClear bytes were cleared once after allocation; the
                          //     caller then also provides priorityT (the fix corrects the priority matrix, the pick reads it)
};
constexpr size_t kBatchPoleClear = 1024 + 16;
// The pole scratch of a batched sweep (BatchPlan::pole, LaunchEvalQuestionsBatch's `pole`): marks of the quizzes the fix changed [256] |
// list header | entries [Q x quizzes] | the listed pairs' sums [Q x quizzes][2 K + 2].  The caller clears the first kBatchPoleClear
// bytes once; every launch leaves them cleared.
static_assert(kBatchPoleClear == 256 * sizeof(uint32_t) + sizeof(PoleHeader), "marks and list header");
inline size_t batch_pole_bytes(const KbView &kb, int quizzes) {
  const size_t cap = (size_t)kb.Q * (size_t)quizzes;
  return kBatchPoleClear + cap * sizeof(PoleEntry) + cap * (size_t)(2 * kb.K + 2) * sizeof(double);
}
struct BatchPole { PoleHeader *list; uint32_t *dirty; double *sums; };
inline BatchPole batch_pole(const KbView &kb, int quizzes, void *pole) {
  char *p = static_cast<char *>(pole);
  const size_t cap = (size_t)kb.Q * (size_t)quizzes;
  return BatchPole{reinterpret_cast<PoleHeader *>(p + 256 * sizeof(uint32_t)), reinterpret_cast<uint32_t *>(p),
                   reinterpret_cast<double *>(p + kBatchPoleClear + cap * sizeof(PoleEntry))};
}
// queryOnly: only fill `plan`.  Otherwise: transposed masked priors -> PT, the sweep, and every quiz's winner {priority,
// local index + outBase} to its slot's `out`, then flagValue to its `seq` (host-coherent).  priorityT (optional):
// [Q][plan->Bp] priorities, quiz-minor.
hipError_t LaunchEvalBatch(const KbView &kb, const QuizSlot *slots, int nSlots, BatchPlan *plan, void *PT, double *acc,
                           BatchRecord *recs, double *priorityT, int64_t outBase, uint64_t flagValue, bool queryOnly, hipStream_t stream,
                           bool skipPick = false);   // skipPick: the caller picks (LaunchBatchRerank)
// The sweep for a few dozen quizzes (batch_kernels.hip: eval_midbatch_kernel; Double engines, K == 5, short rows): a lane is a
// (quiz, chunk of the row).  plan / PT / recs / priorityT / flags as LaunchEvalBatch; slots with hostPriority get tagged records.
bool EvalMidBatchSupported(const KbView &kb);
hipError_t LaunchEvalMidBatch(const KbView &kb, const QuizSlot *slots, int nSlots, BatchPlan *plan, void *PT, BatchRecord *recs,
                              double *priorityT, int64_t outBase, uint64_t flagValue, bool queryOnly, hipStream_t stream);
// skipPick (LaunchEvalBatch's flagValue == 0 is not used for this: see the argument): Float engines' batched ARGMAX -- the fp32
// sweep nominates, fp64 decides (eval_kernels.hip: batch_rerank_kernel).  priorityT: the sweep's [Q][Bp] matrix; scratch:
// BatchRerankScratchBytes() of device memory.  Writes every quiz's winner and flag like LaunchEvalBatch's own pick.
size_t BatchRerankScratchBytes();
hipError_t LaunchBatchRerank(const KbView &kb, const QuizSlot *slots, int nSlots, int Bp, const double *priorityT, void *scratch,
                             int64_t outBase, uint64_t flagValue, hipStream_t stream);
// ---- the sweep over a LIST of (quiz, question) pairs (among_kernels.hip; the Among calls): pair i = {slot b of `slots`, LOCAL
// question q, or q < 0: a question another shard holds -- nothing is evaluated}.  One launch for all pairs; the priority of pair i
// goes to slots[b].priority[q] (0 for a gap or an asked question -- slots[b].asked is tested), in fp64 on either cube type.
// pole (optional, Double engines with a pole list): EvalListedPoleBytes(kb, nPairs) bytes whose first kBatchPoleClear bytes were cleared
// once after allocation (every launch leaves them cleared: the batched sweeps' scratch serves) -- the sweep then watches for rows at the
// pole of the lack term and pole_fixup_kernel runs behind it, storing the corrected priorities to the same places.
struct ListedPair { int32_t b, q; };
hipError_t UploadLog2TableAmong(const double *hostTable);
size_t EvalListedPoleBytes(const KbView &kb, int64_t nPairs);   // 0: this engine's listed sweep does not watch
hipError_t LaunchEvalListed(const KbView &kb, const QuizSlot *slots, int nSlots, const ListedPair *pairs, int64_t nPairs, void *pole,
                            hipStream_t stream);
// out[i] = slots[b].priority[q] of pair i (0 where q < 0): what EvalPrioritiesAmongBatch copies to the host
hipError_t LaunchListedGather(const QuizSlot *slots, const ListedPair *pairs, int64_t nPairs, double *out, hipStream_t stream);
// Quiz b's best question among its pairs [offsets[b], offsets[b + 1]) -- maximum priority, lowest question among equals, NaN never wins;
// gaps, asked and other shards' questions are no candidates -- as {priority, q + outBase or -1} to slots[b].out, then flagValue to
// slots[b].seq (host-coherent).
hipError_t LaunchListedArgmax(const KbView &kb, const QuizSlot *slots, int nSlots, const int64_t *offsets, const ListedPair *pairs, int64_t outBase,
                              uint64_t flagValue, hipStream_t stream);
// Single-quiz sweep of a Float engine: priority[q] for every local question (0 for gap / asked).
hipError_t LaunchEvalQuestionsF32(const KbView &kb, const double *prior, const uint32_t *asked, double *priority, hipStream_t stream);
// ... with the question's rows held in registers (eval_f32_kernels.hip): rows of up to 16384 targets, up to 16 answers
bool EvalF32RegisterShape(const KbView &kb, int variant);
const char *EvalF32KernelName(const KbView &kb, int variant);
hipError_t LaunchEvalQuestionsF32Reg(const KbView &kb, const double *prior, const uint32_t *asked, double *priority, int variant,
                                     hipStream_t stream);
hipError_t UploadLog2TableBatch(const double *hostTable);
// The single-quiz sweep for rows beyond the register shapes (ldT > 16384), fp32 and fp64: a question split over a cluster of
// workgroups (cluster_kernels.hip).  `scratch`: EvalClusterScratchBytes(kb) bytes of device memory (exchange + totals).
hipError_t UploadLog2TableCluster(const double *hostTable);
bool EvalClusterSupported(const KbView &kb);
const char *EvalClusterKernelName(const KbView &kb);
size_t EvalClusterScratchBytes(const KbView &kb);
hipError_t LaunchEvalCluster(const KbView &kb, const double *prior, const uint32_t *asked, double *priority, void *scratch, hipStream_t stream);
const char *EvalVariantName(const KbView &kb, int variant);
bool EvalVariantFusesSampled(const KbView &kb, int variant, int64_t nSubtasks);   // the launch can run the sampled selector itself
bool EvalVariantHasFinisherWorkgroup(const KbView &kb, int variant);              // ... or hand the priority vector to the host (hostPriority)

// ---- resident sweep ("server"): ONE launch serves many selections.  The host posts a request in pinned memory; workgroup
// 0 sees it, hands it to the other workgroups through a device word, everybody sweeps, the finisher answers straight into
// host-coherent memory.  What a step saves is the launch + dispatch + ramp of one kernel (~8 us of a 26 us selection at
// 1000 x 5 x 1000).  The kernel leaves by itself after idleTicks (100 MHz) without a request, or when asked to.
struct ServerMailbox {            // host-coherent (pinned) memory, 128 bytes
  // host -> device; the request fields are written before `req`
  uint64_t req;                   // sequence number of the newest request (never 0 / ~0)
  const double *prior;            // the quiz
  const uint32_t *asked;
  SelectResult *out;              // where the finisher writes {priority, index + outBase}
  uint64_t *flag;                 // ... and then flagValue
  uint64_t flagValue;
  int64_t outBase;
  uint64_t stop;                  // non-zero: leave now
  // device -> host
  uint64_t state;                 // kServerRunning / kServerExiting / kServerExited
  uint64_t taken;                 // newest request the kernel has started on
  uint64_t done;                  // newest request whose step has finished (its result was published before)
  uint64_t pad[5];
};
constexpr uint64_t kServerRunning = 1, kServerExiting = 2, kServerExited = 3;
struct ServerCtl {                // device memory, one line; zeroed before each launch: workgroup 0 -> the other workgroups
  uint64_t go;                    // newest request (the line's fields belong to it); ~0: leave
  const double *prior;
  const uint32_t *asked;
  SelectResult *out;
  uint64_t *flag;
  uint64_t flagValue;
  int64_t outBase;
  uint64_t pad;
};
// Only the short-row register shapes have a resident form (that is where a launch is a large part of a selection):
// returns hipErrorNotSupported otherwise.  `scratch`: kFusedMaxGrid records.  lastSeq: the kernel serves requests != lastSeq.
// requestLine: the 64-byte line the host writes requests to -- the mailbox's own first line, or a line of host-visible device
// memory (everyonePolls: every workgroup watches it; the host then waits for `done`, not `taken`, before the next request).
// hostPriority (optional, host-coherent, qLimit - qFirst doubles): a request whose outBase carries kServerHandOver is answered
// with the priority vector itself (for the host's sampled selector) instead of the argmax.
constexpr uint64_t kServerHandOver = 1ull << 62;
// watch: the resident sweep watches for rows at the pole of the lack term (pole_kernels.hip) and answers
// a step that found one with index -4 -- the caller then takes the launched path, behind which the fix can run; a request whose outBase
// carries kServerNoWatch is answered as if nothing had been found.
constexpr uint64_t kServerNoWatch = 1ull << 61;
// ... kServerPacked: `out` is a PackedSelection (FusedSelect::packed), tagged with the low 32 bits of flagValue.
constexpr uint64_t kServerPacked = 1ull << 60;
hipError_t LaunchEvalServer(const KbView &kb, int64_t qFirst, int64_t qLimit, double *priority, int variant,
                            SelectResult *scratch, ServerMailbox *mailbox, void *requestLine, bool everyonePolls,
                            ServerCtl *ctl, uint64_t lastSeq, uint64_t idleTicks, TaggedPriority *hostPriority, hipStream_t stream,
                            bool watch = false);
bool EvalServerSupported(const KbView &kb, int variant);


struct RatedTargetDev { int64_t iTarget; double prob; };  // == CiRatedTarget
// RecordAnswer's posterior update in the prologue of the sweep that follows it (eval_kernels.hip: eval_questions_f64_upd): one
// launch does what LaunchRecordAnswer + LaunchEvalQuestions do (same posterior bits, same priorities), and the sweep does not wait
// for a posterior kernel.  `fused` must name a selection (scratch != nullptr); the listing arguments as LaunchRecordAnswer's.
bool EvalFusesUpdate(const KbView &kb, int variant, int64_t nWorkers);
hipError_t LaunchEvalQuestionsWithUpdate(const KbView &kb, double *prior, uint32_t *asked, double *priority, int variant, const FusedSelect &fused,
                                         int64_t iQuestion, int64_t iAnswer, int64_t nWorkers, RatedTargetDev *topOut, int64_t *topN,
                                         uint64_t *topFlag, uint64_t topFlagValue, int64_t topCount, hipStream_t stream);

// ---- selectors over priority[0..n) (questions qFirst..qFirst+n of the bitmaps); the reported index is
// (position in priority[]) + outBase
hipError_t LaunchSelectArgmax(const double *priority, const uint32_t *qgap, const uint32_t *asked, int64_t qFirst,
                              int64_t n, int64_t outBase, SelectResult *out, uint64_t *flag, uint64_t flagValue,
                              hipStream_t stream, bool packed = false);   // flag (optional, host-coherent): receives flagValue after `out`;
                                                                          // packed: `out` is a PackedSelection instead (FusedSelect::packed)
// Reference selector (PqaCore/CpuEngine.cpp:362-400): per-subtask Kahan run lengths, grand totals, upper_bound.
// runLength: scratch of n doubles. rnd: the 64-bit random number the reference would draw.
hipError_t LaunchSelectSampled(const double *priority, const uint32_t *qgap, const uint32_t *asked, int64_t qFirst,
                               int64_t n, int64_t nSubtasks, uint64_t rnd, double *runLength, SelectResult *out,
                               uint64_t *flag, uint64_t flagValue, hipStream_t stream);
// The same selection for every quiz of a batched sweep, behind it on its stream (NextQuestionSampledBatch): quiz b's priorities
// are its own vector slots[b].priority (priorityT == nullptr; grid.y = quiz) or column b of the quiz-minor matrix
// priorityT[q * Bp + b] (row-sharing and mid-batch sweeps; Bp a multiple of 64), its asked bits slots[b].asked, its random number
// rnd[b].  Quiz b's {grand total, position + outBase} goes to out[b] and then flagValue to seq[b] (host-coherent, as rnd).
// grand / run: device scratch of SelectSampledBatchScratch's sizes (a size of 0: not needed).
constexpr size_t kSampledBatchLdsBytes = kLdsPerCU;   // per-quiz vectors are staged in LDS up to this much
struct SampledBatch {
  const QuizSlot *slots;          // device array
  int nSlots, Bp;
  const double *priorityT;
  const uint32_t *qgap;
  int64_t n, nWorkers;            // questions; eval_subtasks
  const uint64_t *rnd;
  double *grand, *run;
  SelectResult *out;
  uint64_t *seq;
  uint64_t flagValue;
  int64_t outBase;
};
void SelectSampledBatchScratch(int64_t n, int64_t nSubtasks, int nSlots, int Bp, size_t *grandDoubles, size_t *runDoubles);
hipError_t LaunchSelectSampledBatch(const SampledBatch &a, hipStream_t stream);
// The same selection over shards that separate processes drive, in two launches with an exchange between them (sampled_part.h has
// the layout).  LaunchSampledPackParts, behind a batched sweep on its stream: quiz b's part goes to dst + b * partBytes (any
// device-visible, 16-byte aligned address), the run lengths of the shard's whole subtasks to `run` -- run[j * Bq + b] beside the
// quiz-minor matrix (Bq = its Bp), run[b * nLocal + j] beside the quizzes' own vectors (Bq = the quiz count rounded up to a wave) --
// and seq to stamp[b] as to the part's header; flag (optional): flagValue once every part is visible system-wide (counter: a zeroed
// word in device memory).
struct SampledPartsPack {
  const QuizSlot *slots;          // device array
  int nSlots, Bq;
  const double *priorityT;        // the matrix, or nullptr: slots[b].priority
  const uint32_t *qgap;           // over LOCAL questions, as slots[b].asked
  int64_t qFirst, nLocal, qTotal, nWorkers;
  char *dst;
  int64_t partBytes;
  double *run;
  uint64_t *stamp;
  uint64_t seq;
  unsigned *counter;
  uint64_t *flag;
  uint64_t flagValue;
};
hipError_t LaunchSampledPackParts(const SampledPartsPack &a, hipStream_t stream);
// LaunchSampledPickParts: parts = world x nSlots parts, rank-major.  Quiz b's {grand total, GLOBAL pick or -1 (the chosen subtask lies
// whole on another rank)} goes to out[b] and then flagValue to seq[b] (host-coherent, as rnd).  Index -2: the part of `rank` or the
// saved run lengths do not carry `seq`; -3: the headers' ranges do not tile [0, qTotal) or name another subtask count.
// grand: nSlots x nS doubles, run: nSlots x L doubles of device scratch.
constexpr int kSampledMaxWorld = 64;
struct SampledPartsPick {
  int nSlots, world, rank;
  const char *parts;
  int64_t partBytes, qTotal, nWorkers;
  const uint64_t *rnd;
  const double *packRun;
  int64_t packRunQuiz, packRunStride;   // quiz b's run length j of this rank's questions: packRun[b * packRunQuiz + j * packRunStride]
  const uint64_t *stamp;
  uint64_t seq;
  double *grand, *run;
  SelectResult *out;
  uint64_t *flags;
  uint64_t flagValue;
};
hipError_t LaunchSampledPickParts(const SampledPartsPick &a, hipStream_t stream);

// ---- prior updates (single workgroup, O(T)); nWorkers = emulated CPU worker count that fixes the summation order.
// The subtasks' partial sums live in (8 nWorkers + 1) doubles of LDS, within the 64 KiB a launch gets without opting in.
constexpr int64_t kMaxWorkers = 1000;
hipError_t LaunchStartQuiz(const KbView &kb, double *prior, uint32_t *asked, int64_t askedWords, int64_t nWorkers, hipStream_t stream);
// topOut (optional, host-coherent with topN / topFlag): also list the new posterior's topCount best targets, then store
// topFlagValue to *topFlag.
// rowA / rowD (optional): the rows of an answered question that ANOTHER shard of the question axis holds (sharded_engine.cpp), read
// where they are; iQuestion is then not used and no bit of `asked` is set.
hipError_t LaunchRecordAnswer(const KbView &kb, double *prior, uint32_t *asked, int64_t iQuestion, int64_t iAnswer,
                              int64_t nWorkers, RatedTargetDev *topOut, int64_t *topN, uint64_t *topFlag,
                              uint64_t topFlagValue, int64_t topCount, hipStream_t stream, const void *rowA = nullptr,
                              const void *rowD = nullptr);
// Several quizzes' RecordAnswer in ONE launch (grid.x = update; the same workgroup code and summation order per quiz as
// LaunchRecordAnswer, so every posterior is bit-identical to the one-by-one result): up to kRecordInline updates travel in the
// kernel's arguments.  CERecordAnswerSubtaskMul.cpp:15-42 per quiz; the reference runs concurrent quizzes' updates side by side.
constexpr int kRecordInline = 256;
struct RecordSlot {               // 56 bytes: 256 of them are 14 KB of kernel arguments
  double *prior;
  uint32_t *asked;
  void *pin;                      // the quiz's host-coherent lines {RatedTargetDev top[kQuizTopDev]; int64 nOut; uint64 topFlag} (optional: no listing without)
  int32_t iQuestion, iAnswer;     // local question
  uint64_t topFlagValue;
  const void *rowA, *rowD;        // non-null: another shard's question -- its rows where they are (then iQuestion is unused)
};
constexpr int kQuizTopDev = 32;   // == kQuizTop (hip_engine.h)
struct RecordBatchInline {
  int32_t n, topCount;
  RecordSlot s[kRecordInline];
};
hipError_t LaunchRecordAnswerBatch(const KbView &kb, const RecordBatchInline &batch, int64_t nWorkers, hipStream_t stream);
// A PAGE of answers per quiz in ONE launch (grid.x = quiz): workgroup i gives quiz i its `count` answers one after another -- per
// answer RecordAnswer's element step, reference-order sum and division, the same device functions in the same order as
// LaunchRecordAnswer, so the posterior is bit-identical to `count` consecutive launches -- with the posterior read once and written
// once where a row fits the LDS stage, and in place in memory where it does not.  Slot i lies in device memory.
constexpr int kRecordPageChunk = 256;      // quizzes per launch
constexpr int64_t kRecordPageMax = 4096;   // answers per quiz: a chunk's pointer table stays within 16 MiB
struct RecordPageSlot {
  double *prior;
  uint32_t *asked;
  void *pin;                      // as RecordSlot's (optional: no listing without)
  uint64_t topFlagValue;
  const void *const *rows;        // 2 count row pointers, {sA[q_j][a_j], mD[q_j]} per answer, as ResumeSlot's
  const int32_t *qLocal;          // count local question indices; -1: another shard's question, no bit of `asked` to set
  double *likelihood;             // count doubles: step j's total, the predictive probability of answer j (optional)
  int64_t count;                  // >= 1
};
hipError_t LaunchRecordAnswerPage(const KbView &kb, const RecordPageSlot *slots, int64_t n, int64_t nWorkers, int64_t topCount, hipStream_t stream);
// Several quizzes' StartQuiz in ONE launch (grid.x = quiz; every workgroup runs CESetPriorsSubtaskSum exactly as LaunchStartQuiz).
constexpr int kStartInline = 256;
struct StartBatchInline {
  int32_t n;
  int64_t askedWords;
  double *prior[kStartInline];
  uint32_t *asked[kStartInline];
};
hipError_t LaunchStartQuizBatch(const KbView &kb, const StartBatchInline &batch, int64_t nWorkers, hipStream_t stream);
// rows: device array of 2 nAnswered row pointers, {sA[q_i][a_i], mD[q_i]} per answered question (rows of kb.elem-byte elements,
// ldT long; they may live on another device of the process).  exps: scratch of ldT int64.  status: device int64[2]
// {error code (0 / 16 = I64Underflow), fullMax}.  bugCompat reproduces PqaCore/CEUpdatePriorsSubtaskMul.cpp:53.
hipError_t LaunchResumeQuiz(const KbView &kb, double *prior, int64_t *exps, const void *const *rows, int64_t nAnswered,
                            int64_t nWorkers, int bugCompat, int64_t *status, hipStream_t stream);
// Several quizzes' ResumeQuiz in one launch sequence: slot i (device memory) is quiz i's LaunchResumeQuiz, every posterior
// bit-identical to it.  The kernels also copy askedSrc (askedWords words) into asked.  Rows of up to 16384 targets: one workgroup
// per quiz (grid.x = quiz).  Longer rows with kb.priorScratch set (option long_row_form): three launches over (part of the row,
// quiz) -- products and the exponent maximum, normalisation and the reference's subtask sums, division -- with longScratch:
// n * ResumeLongStride(nWorkers) words, zeroed by the caller before the launch.  n <= kResumeChunk.
constexpr int kResumeChunk = 256;
struct ResumeSlot {
  double *prior;
  uint32_t *asked;
  const uint32_t *askedSrc;
  const void *const *rows;        // 2 nAnswered row pointers, as LaunchResumeQuiz's
  int64_t *exps;                  // ldT int64 of scratch
  int64_t *status;                // int64[2], as LaunchResumeQuiz's
  int64_t nAnswered;              // >= 1
  int64_t pad;
};
inline int64_t ResumeLongStride(int64_t nWorkers) { return 8 + 8 * nWorkers; }
inline bool ResumeTakesLongRow(const KbView &kb) { return kb.ldT > 16384 && kb.priorScratch != nullptr; }
hipError_t LaunchResumeQuizBatch(const KbView &kb, const ResumeSlot *slots, int64_t n, int64_t askedWords, int64_t nWorkers,
                                 int bugCompat, uint64_t *longScratch, hipStream_t stream);

// ---- KB construction / mutation
hipError_t LaunchFillFresh(void *cube, int elem, double *vB, int64_t K, int64_t Q, int64_t T, int64_t ldT, double initAmount,
                           hipStream_t stream);
// Deterministic synthetic "binary-search trained + hash noise" cube (see probqa_amd/synth.py for the definition).
hipError_t LaunchFillSynthetic(void *cube, int elem, double *vB, int64_t K, int64_t Q, int64_t T, int64_t ldT, int64_t qOffset,
                               int64_t qTotal, double initAmount, double nTrain, double noiseAmp, uint64_t seed,
                               hipStream_t stream);
// Train / RecordQuizTarget (PqaCore/CETrainOperation.cpp:15-83).  steps: device array in execution order, grouped by question;
// chain c = steps[chainStart[c] .. chainStart[c + 1]) all on one question (chainStart: nChains + 1 entries).  Always adds
// `amount` to vB[iTarget], also with no steps.
struct TrainStep { int64_t kind, q, a1, a2; };   // kind 1 | 2 | 3, see kb_kernels.hip; q local
hipError_t LaunchTrainSteps(void *cube, int elem, double *vB, int64_t K, int64_t ldT, const TrainStep *steps,
                            const int64_t *chainStart, int64_t nChains, int64_t iTarget, double amount, hipStream_t stream);
// Up to kTrainInlineSteps steps travel in the kernel's arguments (no staging copy, nothing for the host to wait for).
constexpr int kTrainInlineSteps = 48;
struct TrainStepsInline {
  int64_t nChains;
  int64_t chainStart[kTrainInlineSteps + 1];
  TrainStep steps[kTrainInlineSteps];
};
hipError_t LaunchTrainStepsInline(void *cube, int elem, double *vB, int64_t K, int64_t ldT, const TrainStepsInline &in,
                                  int64_t iTarget, double amount, hipStream_t stream);
// Several training calls -- each with its own target and amount, DIFFERENT targets (their cells are disjoint then) -- in one launch:
// workgroup c runs call c's chains exactly as train_steps_inline_kernel would.  What a server's clients' RecordQuizTarget calls
// become when they arrive together (hip_engine_combine.cpp: DrainPosted).
constexpr int kTrainBatchCalls = 24, kTrainBatchSteps = 192;
struct TrainBatchStep { int32_t q; uint8_t kind, a1, a2, pad; };
struct TrainBatchCall { int64_t iTarget; double amount; int32_t firstChain, nChains; };
struct TrainBatchInline {
  int32_t nCalls, nChainsTotal, nSteps, pad;
  TrainBatchCall calls[kTrainBatchCalls];
  uint16_t chainStart[kTrainBatchSteps + kTrainBatchCalls + 8];   // per call: its chains' starts and one end, indices into steps[]
  TrainBatchStep steps[kTrainBatchSteps];
};
hipError_t LaunchTrainBatchInline(void *cube, int elem, double *vB, int64_t K, int64_t ldT, const TrainBatchInline &in, hipStream_t stream);
// Many training records -- any targets, repeated ones too -- in one launch (TrainBatch / RecordQuizTargetBatch,
// hip_engine_train.cpp).  Lane c < nChains runs chain c: the steps on one (target t, question) cell column, in record order;
// lane nChains + j adds amounts[first .. end) to vB[t] of target slot j, in that order.  Every step names the amount of its
// record: amounts[rec].  No two lanes touch the same cell.
struct TrainChain { int64_t t; int32_t first, end; };   // chain: steps [first, end); target slot: amounts [first, end)
struct TrainChainStep {                                 // kind 1 | 2 | 3 as TrainStep; q local
  int32_t q;
  uint32_t kindRec;                                     // rec << 2 | kind
  int32_t a1, a2;
};
hipError_t LaunchTrainChains(void *cube, int elem, double *vB, int64_t K, int64_t ldT, const TrainChain *chains, int64_t nChains,
                             int64_t nTargets, const TrainChainStep *steps, const double *amounts, hipStream_t stream);
// Maintenance (PqaCore/CpuEngine.cpp:468-658): (re)initialise whole questions / whole target columns; compact the target
// axis with (src,dst) column moves.  qs/ts/inits/moves are device arrays.
hipError_t LaunchFillQuestions(void *cube, int elem, int64_t K, int64_t T, int64_t ldT, const int64_t *qs, const double *inits,
                               int64_t n, hipStream_t stream);
hipError_t LaunchFillTargets(void *cube, int elem, double *vB, int64_t K, int64_t ldT, int64_t nQ, const uint32_t *skipQ,
                             const int64_t *ts, const double *inits, int64_t n, hipStream_t stream);
// src: device array of nQ block pointers (question q's K + 1 rows, ldTs apart; nullptr: nothing to take), colMap: device array of
// Tn old column indices (-1: a new column).  vB likewise.
hipError_t LaunchAdoptRows(void *dst, int elem, double *dstVB, int64_t K, int64_t nQ, int64_t Tn, int64_t ldTn, const void *const *src,
                           int64_t ldTs, const double *srcVB, const int64_t *colMap, hipStream_t stream);
hipError_t LaunchMoveTargets(void *cube, int elem, double *vB, int64_t K, int64_t ldT, int64_t nQ, const int64_t *moves,
                             int64_t n, hipStream_t stream);
// The rows of answered questions packed for another engine (PqaHip_PackAnswerRows): pair i of `pairs` (device memory) is copied as
// it lies -- rowBytes of sA[q][k][.] and then rowBytes of mD[q][.], padding included -- to pair i's dst, which may be any
// device-visible address.  rowBytes: a multiple of 16, every address 16-byte aligned.  One launch: a workgroup per (row, chunk of
// kPackChunkBytes).  flag != nullptr: `counter` (device memory, zero at launch) counts the workgroups in, and the last one stores
// flagValue to flag once every row is visible system-wide; n == 0 then launches that store alone.
struct PackPair { const void *rowA, *rowD; void *dst; };
constexpr int64_t kPackChunkBytes = 16384;
hipError_t LaunchPackAnswerRows(const PackPair *pairs, int64_t n, int64_t rowBytes, unsigned *counter, uint64_t *flag, uint64_t flagValue,
                                hipStream_t stream);
// Whole question blocks between a cube and a BLOCK PACKAGE (PqaHip_PackQuestionBlocks, PqaEngine_CompactFromBlocks): block i of
// `blocks` (device memory) is `rows` (K + 1) rows of rowWords 4-byte words -- T elements -- that lie srcPitchBytes apart at src and
// dstPitchBytes apart at dst; both pitches are multiples of 128, every block starts on a 128-byte line, and a pitch holds the row
// rounded up to 16 bytes.  zeroTail (packing): the rest of every dst row, up to its pitch, is zero-filled; otherwise (unpacking into a
// cube) nothing behind the row's last word is written.  One launch: a workgroup per (block, row, chunk of kPackChunkBytes), 16-byte
// accesses except the words of a row's last, partial unit.  counter / flag / flagValue as LaunchPackAnswerRows.
struct BlockCopy { const void *src; void *dst; };
hipError_t LaunchCopyQuestionBlocks(const BlockCopy *blocks, int64_t n, int64_t rows, int64_t rowWords, int64_t srcPitchBytes, int64_t dstPitchBytes,
                                    bool zeroTail, unsigned *counter, uint64_t *flag, uint64_t flagValue, hipStream_t stream);
// Posteriors between the engine and a POSTERIOR PACKAGE (PqaHip_PackAnswerPosteriors, PqaEngine_RecordAnswerBatchFromPosteriors):
// slot = T doubles at a pitch of pitchBytes (a multiple of 128), zeros behind them.  Entry i of `copies` (device memory) moves one
// posterior from src to dst, both 16-byte aligned.  One launch each: a workgroup per (entry, chunk of kPackChunkBytes), 16-byte
// accesses except the words of an odd T's last, partial unit.
//   LaunchPackPosteriors: dst is the slot -- the partial unit's other half and every unit behind it up to the pitch are stored as
//     zeros.  counter / flag / flagValue as LaunchPackAnswerRows.
//   LaunchTakePosteriors: dst is a quiz's posterior -- elements from T on stay as they are -- and where `asked` is not null, one
//     lane of the entry's first workgroup sets bit askedBit there (CEQuiz::RecordAnswer, PqaCore/CEQuiz.h:92, on the holder).
struct PosteriorCopy { const void *src; void *dst; uint32_t *asked; int64_t askedBit; };
hipError_t LaunchPackPosteriors(const PosteriorCopy *copies, int64_t n, int64_t T, int64_t pitchBytes, unsigned *counter, uint64_t *flag,
                                uint64_t flagValue, hipStream_t stream);
hipError_t LaunchTakePosteriors(const PosteriorCopy *copies, int64_t n, int64_t T, hipStream_t stream);
// Rows between a .kb file's dense layout in one number type and the cube's padded layout in another (kb_kernels.hip:
// convert_rows_kernel).  `dense`: nRows rows of T elements back to back, denseElem (4 | 8) bytes each, only element-aligned.
// `cube`: the first row's question block; dense row r is the cube's row (r / rowsPerQ) * qStride + r % rowsPerQ + rowBase, rows ldT
// elements of cubeElem bytes apart, 16-byte aligned -- rowsPerQ = K, rowBase = 0, qStride = K + 1: the sA rows of consecutive
// questions; rowsPerQ = 1, rowBase = K: their mD rows; rowsPerQ = 1, qStride = 0: vB.  toCube: dense -> cube (a load), else a save.
// roundF32 (denseElem == cubeElem == 8, vB into a Float engine): every value rounded through fp32 on its way.
// fp64 -> fp32 rounds to nearest even; each finite value that does not stay finite adds one to *overflow (device memory).
// Only [0, T) of a row is read or written on either side.
struct ConvertRows {
  void *dense; void *cube;
  int denseElem, cubeElem;
  int64_t T, ldT, nRows, rowsPerQ, rowBase, qStride;
  bool toCube, roundF32;
  unsigned *overflow;
};
hipError_t LaunchConvertRows(const ConvertRows &c, hipStream_t stream);
// ListTopTargets (PqaCore/CEListTopTargetsAlgorithm.cpp): top maxCount (prob,target) pairs, descending, gaps skipped.
// (flag != nullptr: out / nOut / flag are host-coherent; the kernel stores flagValue to *flag after its results)
hipError_t LaunchTopTargets(const KbView &kb, const double *prior, int64_t maxCount, RatedTargetDev *out,
                            int64_t *nOut, uint64_t *flag, uint64_t flagValue, hipStream_t stream);
// ... over rows of any length and for up to kTopBatchQuizzes quizzes per launch (maxCount <= 256): a list per wave of 1024 targets,
// then merges; out[quiz][maxCount] records (unused ones {-1, -1}) and nOut[quiz], device or host-coherent; `flag` only with ONE quiz.
// The two scratch buffers hold nQuizzes * TopBatchScratchRecords(T, maxCount) records each.
constexpr int kTopBatchQuizzes = 256;
constexpr int64_t kTopChunkTargets = 4096, kTopMergeCapacity = 16384;
struct TopBatchPriors { const double *prior[kTopBatchQuizzes]; };
int64_t TopBatchScratchRecords(int64_t T, int64_t maxCount);
// ... and in the reference's order among EQUAL probabilities (its per-worker heaps and head heap, reproduced step for step; nWorkers:
// the emulated thread count): what ListTopTargets returns where the listing above shows a tie.  `scratch`: TopExactScratchBytes bytes.
size_t TopExactScratchBytes(int64_t T, int64_t nWorkers, int64_t maxCount, int64_t nQuizzes);
hipError_t LaunchTopTargetsExact(const KbView &kb, const TopBatchPriors &priors, int64_t nQuizzes, int64_t nWorkers, int64_t maxCount, void *scratch,
                                 RatedTargetDev *out, int64_t *nOut, uint64_t *flag, uint64_t flagValue, hipStream_t stream);
hipError_t LaunchTopTargetsBatch(const KbView &kb, const TopBatchPriors &priors, int64_t nQuizzes, int64_t maxCount, RatedTargetDev *scratchA,
                                 RatedTargetDev *scratchB, RatedTargetDev *out, int64_t *nOut, uint64_t *flag, uint64_t flagValue,
                                 hipStream_t stream);

// ListTopQuestions: the best maxCount (<= 256) questions of nQuizzes (<= kTopBatchQuizzes) quizzes by the priorities a sweep has left on
// the device -- descending priority, ascending LOCAL question among equal priorities; gaps, asked questions (both bitmaps are tested)
// and priorities that are not > 0 are never listed.  Where the priorities lie:
//   one quiz          slots == nullptr, Bp == 0: `priority` is its vector, `asked` its bitmap;
//   grid.y = quiz     slots (device), Bp == 0: every slot's own priority vector and asked bitmap;
//   quiz-minor matrix slots (device, for the asked bitmaps), Bp > 0: `priority` is [Q][Bp], quiz i in column i.
// out[quiz][maxCount], nOut[quiz] and flags[quiz] (optional: flagValue once the quiz's records are visible) are device or host-coherent.
// The two scratch buffers hold nQuizzes * TopQuestionsScratchRecords(Q, maxCount) records each.
struct TopQuestions {
  const QuizSlot *slots;
  const double *priority;
  const uint32_t *asked, *qgap;
  int nQuizzes, Bp;
  int64_t Q;
};
int64_t TopQuestionsScratchRecords(int64_t Q, int64_t maxCount);
hipError_t LaunchTopQuestions(const TopQuestions &a, int64_t maxCount, RatedTargetDev *scratchA, RatedTargetDev *scratchB, RatedTargetDev *out,
                              int64_t *nOut, uint64_t *flags, uint64_t flagValue, hipStream_t stream);

// ListTopTargetsAmongBatch: the best maxCount (<= 256) targets of nQuizzes (<= kTopBatchQuizzes) quizzes within LISTED sets -- the lists
// staged on the device as offsets[nLists + 1] | ids (int32, in [0, T), no id twice in a list), listOf[quiz] (host) the quiz's list,
// `longest` the longest list of the launch's quizzes.  The order is the batched listing's (probability descending, target ascending)
// whatever the lists' order.  out[quiz][maxCount], nOut[quiz] and mass[quiz] (the sum of the quiz's candidates, in a fixed order) are
// device or host-coherent.  The two scratch buffers hold nQuizzes * TopAmongScratchRecords(longest, maxCount) records each, `partial`
// nQuizzes * TopAmongPartials(longest) doubles.
int64_t TopAmongScratchRecords(int64_t longest, int64_t maxCount);
int64_t TopAmongPartials(int64_t longest);
hipError_t LaunchTopTargetsAmong(const KbView &kb, const TopBatchPriors &priors, const int32_t *listOf, int64_t nQuizzes, const int64_t *offsets,
                                 const int32_t *ids, int64_t longest, int64_t maxCount, RatedTargetDev *scratchA, RatedTargetDev *scratchB,
                                 double *partial, RatedTargetDev *out, int64_t *nOut, double *mass, hipStream_t stream);
// ... and for longer listings: out[quiz * longest + i] = the posterior of entry i of the quiz's list (-1 for a gap), for the host to select from
hipError_t LaunchTopAmongGather(const KbView &kb, const TopBatchPriors &priors, const int32_t *listOf, int64_t nQuizzes, const int64_t *offsets,
                                const int32_t *ids, int64_t longest, double *out, hipStream_t stream);

// PreviewAnswersBatch (preview_kernels.hip): the posteriors RecordAnswer WOULD leave, one workgroup per row.  Row r: the quiz's
// posterior `prior` (read only) under the rows sA[q][k][.] and mD[q][.] of one question block -- p = x / total, bit for bit
// RecordAnswer's (nWorkers: its reference-order sum's).  likelihood[r] = total, entropy[r] = -sum p log2 p in bits over the p > 0
// (either may be null; device or host-coherent); writeRows: p into scratch[r][pitch] (pitch >= ldT), where LaunchTopTargetsBatch
// takes it for a posterior.  A dead answer (total 0 or not finite): a row of zeros, a quiet NaN for an entropy.  `scratch` is also
// where x is staged when a row does not fit LDS (PreviewStagesInLds false); otherwise it may be null without writeRows.
// nRows <= kTopBatchQuizzes; `rows` in device memory.
struct PreviewRow { const double *prior; const void *rowA, *rowD; };
bool PreviewStagesInLds(const KbView &kb, int64_t nWorkers);
hipError_t LaunchPreviewRows(const KbView &kb, const PreviewRow *rows, int64_t nRows, int64_t nWorkers, double *scratch, int64_t pitch, bool writeRows,
                             double *likelihood, double *entropy, hipStream_t stream);

// ReviewAnswersBatch (review_kernels.hip): the posteriors ResumeQuiz would leave with one answer left out.  Row r of a chunk has ldT-long
// (pitch >= ldT) lines mants[r] and exps[r].
//   LaunchReviewChains: grid.y = a distinct quiz of the chunk.  `rows`: its 2 nAnswered row pointers as ResumeSlot's; `requests`: its
//     requested (position, row of the chunk) pairs, position ascending, a position may repeat; `ratios`: nAnswered x ldT doubles of scratch,
//     or null when nAnswered <= maxLdsAnswers (<= kReviewLdsAnswers) and the ratios stay in LDS.  Leaves every requested row's mantissas
//     and exponent sums; rows without remaining answers (nAnswered == 1) are written too and ignored by the rows kernel.
//   LaunchReviewRows: a workgroup per row normalises it as resume_quiz_body does (nWorkers subtasks), leaves the divided row in mants[r]
//     (a posterior for LaunchTopTargetsBatch), the entropy in bits, and the likelihood of the left-out answer (rowA / rowD) under it as
//     PreviewAnswersBatch computes it (max(1, nWorkers - 1) subtasks).  likelihood / entropy: device or host-coherent, either may be null.
//     nRemaining == 0: StartQuiz's posterior.  A dead row: zeros, two quiet NaNs.
// Everything in device memory; nQuizzes, nRows <= kTopBatchQuizzes.
constexpr int64_t kReviewLdsAnswers = 24;   // 24 x 256 doubles = 48 KiB: three chains workgroups per CU
struct ReviewRequest { int32_t position, row; };
struct ReviewQuiz { const void *const *rows; const ReviewRequest *requests; double *ratios; int64_t nAnswered, nRequests; };
struct ReviewRow { const void *rowA, *rowD; int64_t nRemaining; };
hipError_t LaunchReviewChains(const KbView &kb, const ReviewQuiz *quizzes, int64_t nQuizzes, int64_t maxLdsAnswers, bool bugCompat, double *mants, int64_t *exps,
                              int64_t pitch, hipStream_t stream);
hipError_t LaunchReviewRows(const KbView &kb, const ReviewRow *rows, int64_t nRows, int64_t nWorkers, double *mants, int64_t *exps, int64_t pitch,
                            double *likelihood, double *entropy, hipStream_t stream);

// QuizStatusBatch / RankTargetsBatch (status_kernels.hip): where a quiz stands, read off its posterior; a CANDIDATE is a target that is no
// gap and holds p > 0.  Only [0, T) of a posterior is read.
//   LaunchQuizStatus: a workgroup per quiz (nQuizzes <= kTopBatchQuizzes).  Quiz i's line, kStatusLineWords 8-byte words at
//     lines + i * kStatusLineWords (device or host-coherent): the entropy in bits over the candidates -- preview_rows_kernel's partition
//     and order, so the bits PreviewAnswersBatch promised for this posterior --, their mass in the same order, the largest probability (0
//     without a candidate), its target (the lowest among equals; -1), the number of candidates; from kStatusLineCounts on, per level j <
//     levels.n the number of candidates with p >= level[j], and from kStatusLineMasses on their sum in the entropy's order.  The words of
//     the levels beyond levels.n are not written.
//   LaunchRankTargets: a workgroup per tile (nTiles <= kTopBatchQuizzes; `tiles` and `ids` in device memory): tile = {the quiz's
//     posterior, first, count <= kRankTile}, its named targets ids[first .. first + count), each in [0, T).  out[first + x] = {the
//     number of candidates before the named target by (probability descending, target ascending) or -1 where it is no candidate
//     itself, the posterior's own value there} (device or host-coherent).
constexpr int kStatusLevels = 16, kRankTile = 32;
constexpr int kStatusLineCounts = 5, kStatusLineMasses = kStatusLineCounts + kStatusLevels, kStatusLineWords = 40;
static_assert(kStatusLineMasses + kStatusLevels <= kStatusLineWords, "a line holds the record and both level vectors");
struct StatusLevels { int32_t n, pad; double level[kStatusLevels]; };
struct RankTile { const double *prior; int32_t first, count; };
hipError_t LaunchQuizStatus(const KbView &kb, const TopBatchPriors &priors, int64_t nQuizzes, const StatusLevels &levels, int64_t *lines, hipStream_t stream);
hipError_t LaunchRankTargets(const KbView &kb, const RankTile *tiles, int64_t nTiles, const int32_t *ids, RatedTargetDev *out, hipStream_t stream);

// Target similarity (similarity_kernels.hip): per source s_i and target t the sum over this cube's questions that are not gaps of
// sum_k sqrt(p_qk(s_i)) sqrt(p_qk(t)), p_qk(t) = A[q][k][t] / D[q][t], in fp64 whatever the cube's element type.
//   LaunchSimilaritySums: `sources` (device memory, ids in [0, T)) in tiles of kSimTile -- per tile the sources' columns into `rs`
//     (SimSourceScratchBytes), one streaming pass over the cube into `partial` (SimPartialBytes) and the chunks added in order into
//     dst[i][pitch]: slot i = T sums, 0 at gap targets, all 0 for a gap source, zeros behind T up to `pitch` doubles (a multiple of
//     16, T <= pitch <= ldT).  dst may be any device-visible address.  counter / flag / flagValue as LaunchPackAnswerRows, over all
//     the launches of the call; nSources == 0 with a flag launches that store alone.  A tile of up to kSimTileSmall sources runs the
//     narrow instantiation: the same arithmetic per (source, target), fewer accumulators.
//   LaunchSimilarityRows: rows[i][pitch] = sums[i][pitch] / nValidQuestions (0 where that is 0), 0 at gaps and behind T, and with
//     zeroSelf at t == sources[i] -- the rows the listing takes (LaunchTopTargetsBatch: what is <= 0 is no candidate).
constexpr int kSimTile = 32, kSimTileSmall = 4;
int64_t SimQuestionsPerChunk(int64_t Q, int64_t ldT);
int64_t SimChunks(int64_t Q, int64_t ldT);
size_t SimSourceScratchBytes(const KbView &kb);
size_t SimPartialBytes(const KbView &kb);
hipError_t LaunchSimilaritySums(const KbView &kb, const int64_t *sources, int64_t nSources, double *rs, double *partial, double *dst, int64_t pitch,
                                unsigned *counter, uint64_t *flag, uint64_t flagValue, hipStream_t stream);
hipError_t LaunchSimilarityRows(const KbView &kb, const double *sums, int64_t pitch, const int64_t *sources, int64_t nSources, bool zeroSelf, int64_t nValidQuestions,
                                double *rows, hipStream_t stream);

// Question redundancy (redundancy_kernels.hip): I(s, q), the mutual information in bits between the answers to a source question s
// and a question q of this cube for a target drawn from vB, in fp64 whatever the cube's element type.
//   LaunchQuestionWeights: `sources` (device memory, GLOBAL ids; this cube holds [qFirst, qFirst + Q)) -- slot i of dst = K rows of
//     `pitch` doubles (a multiple of 16, T <= pitch <= ldT), u_k[t] = vB[t] * (A[s][k][t] * (1 / D[s][t])), 0 at gap targets and
//     behind T, all 0 for a gap source; the slots of sources this cube does not hold are NOT touched.  dst may be any device-visible
//     address.  counter / flag / flagValue as LaunchPackAnswerRows; nSources == 0 with a flag launches that store alone.
//   LaunchRedundancySweep: rows[i][rowPitch], column j = I(sources[i], qFirst + j) from the package at `weights` (16-byte aligned): 0
//     for a gap question and a source whose rows are zeros, and with zeroSelf where qFirst + j == sources[i] -- the rows the listing
//     takes (LaunchTopQuestions: what is <= 0 is no candidate).  A tile of RedundancyTileWidth(K) sources per workgroup where the
//     call has as many, one source a tile for the rest: the value of a pair is the same either way.  Answer counts without an
//     instantiation (K > 5) need `tables`, RedundancyTableBytes bytes of device scratch.
//   LaunchRedundancySlots: the listing's view of the rows -- slot i's priority vector is row i.
constexpr int RedundancyTileWidth(int K) { return K == 2 ? 8 : K <= 4 ? 4 : K == 5 ? 2 : 1; }   // NS K K accumulators <= 64 doubles a lane
constexpr int64_t kRedGenericWorkgroups = 2048;
size_t RedundancyTableBytes(const KbView &kb);
hipError_t LaunchQuestionWeights(const KbView &kb, const int64_t *sources, int64_t nSources, int64_t qFirst, double *dst, int64_t pitch, unsigned *counter,
                                 uint64_t *flag, uint64_t flagValue, hipStream_t stream);
hipError_t LaunchRedundancySweep(const KbView &kb, const double *weights, int64_t pitch, const int64_t *sources, int64_t nSources, int64_t qFirst, bool zeroSelf,
                                 double *rows, int64_t rowPitch, double *tables, hipStream_t stream);
hipError_t LaunchRedundancySlots(QuizSlot *slots, double *rows, int64_t rowPitch, const uint32_t *qgap, int64_t nSources, hipStream_t stream);

// Target separation (separation_kernels.hip): sep(G, q), the Jensen-Shannon divergence in bits of the answer distributions of the
// targets of a group G at a question q of this cube, equal weights, in fp64 whatever the cube's element type.
//   LaunchSeparationSweep: rows[g][rowPitch], column j = sep(group g, question j) for the nGroups (<= kTopBatchQuizzes) groups staged on
//     the device as groupStart[nGroups + 1] | tileGroup[nTiles + 1] | tileWidth[nTiles] | entries (ids in [0, T), 2 .. kSepMaxGroup a
//     group): 0 for a gap question and for a group with a gap member -- the rows the listing takes.  The tiles are kb_plan.h's
//     PlanGroupTiles over kSepTileEntries and kSepTileGroups: runs of whole groups; a tile's width is a power of two that holds its
//     longest group (it sets how many groups a wave reduces side by side, not a bit of any value).
constexpr int kSepMaxGroup = 64, kSepTileEntries = 256, kSepTileGroups = 128;
hipError_t LaunchSeparationSweep(const KbView &kb, const int64_t *groupStart, const int64_t *tileGroup, const int64_t *tileWidth, const int64_t *entries,
                                 int64_t nGroups, int64_t nTiles, double *rows, int64_t rowPitch, hipStream_t stream);

// Question gains (gain_kernels.hip): gain(quiz, q), the mutual information in bits between the answer to question q of this cube and
// the target for a target drawn from the quiz's posterior (0 at a gap target and where it is not > 0), in fp64 whatever the cube's
// element type.  Only [0, T) of a posterior is read, in 16-byte pieces (the posteriors are 16-byte aligned, ldT doubles long).
//   LaunchQuestionGains: rows[i][rowPitch], column j = gain(quiz i, question j) for nQuizzes (<= kTopBatchQuizzes) posteriors: 0 for a
//     gap question and for a quiz whose table's total is 0 or not finite -- the rows the listing takes (LaunchTopQuestions: what is
//     <= 0 is no candidate).  One streaming pass over the cube per tile of GainTileWidth(K) quizzes -- the K + 1 logarithms of an
//     element are paid once per tile --, a lone quiz in a tile of one; a value is the same bits at either width.  Answer counts
//     without an instantiation (K > 5) go (question, quiz) by (question, quiz).
//   LaunchGainSlots: the listing's view of the rows -- slot i's priority vector is row i, its asked bitmap asked.asked[i].
constexpr int GainTileWidth(int K) { return K == 2 ? 16 : K == 3 ? 12 : K <= 5 ? 8 : 1; }   // NQ (K + 1) accumulators <= 48 doubles a lane
struct GainAsked { const uint32_t *asked[kTopBatchQuizzes]; };
hipError_t LaunchQuestionGains(const KbView &kb, const TopBatchPriors &priors, int64_t nQuizzes, double *rows, int64_t rowPitch, hipStream_t stream);
hipError_t LaunchGainSlots(QuizSlot *slots, double *rows, int64_t rowPitch, const GainAsked &asked, int64_t nQuizzes, hipStream_t stream);

// Question pages (page_kernels.hip): the BRANCH rows of a quiz under a set of questions -- its posterior times the answer ratios of
// every combination of the set's answers, not normalised, branch b = ((k_1 K + k_2) K + ...) + k_j --, their masses, and the
// conditional gain CG(q | S) = sum_b (m_b / M) gain(row b, q) over LaunchQuestionGains' rows for them.  rows[row][pitch] and
// masses[row] are one scratch area of a call's chunk; a quiz's rows of a step lie next to each other, b ascending.  PageQuiz, in device
// memory, is one quiz of ONE launch (the host writes a list per launch):
//   LaunchPageRoots    row0 <- the quiz's posterior, 0 at gap targets, where it is not > 0 and behind T; masses[row0] its sum.
//   LaunchPageExpand   a workgroup per parent row (grid.x = maxParents >= every nParents; a quiz with nParents == 0 sits the launch
//                      out): rows [row0 + x K, row0 + (x + 1) K) <- parent parent0 + x times r_k of `question`, a LOCAL id, or with
//                      kPagePickListed the id in pick->iTarget where *nPick > 0 -- no pick: zero rows, zero masses.  set[nSet] <- the
//                      question (-1: none).  Parents and children must not overlap.  With kPageBlockGiven the question is one this
//                      engine does not hold: its K + 1 rows are read at `block`, a slot of a block package (pitch blockLdT elements,
//                      zeros behind T), set[nSet] <- -1 -- it has no local id and excludes nothing here.
//   LaunchPageCombine  combined[i][j] = sum_b (m_b / M) gains[gain0 + b][j] over the quiz's nRows rows at row0 (masses) and gain0
//                      (gains): b ascending in one fma chain, a branch with a mass not > 0 left out, zeros where M is not > 0 or not
//                      finite.  excl (optional): excl[i][exclWords] = the quiz's asked words | the bits of set[0 .. nSet).
// All sums in a fixed order; no atomics.  K <= kTopBatchQuizzes; nRows <= kTopBatchQuizzes.
constexpr int32_t kPagePickListed = -2, kPageBlockGiven = -3;
struct PageQuiz {
  const uint32_t *asked;         // the combine's exclusion bitmap starts from it
  union {
    const RatedTargetDev *pick;  // kPagePickListed: where the listing left the question ...
    const void *block;           // kPageBlockGiven: the question's block in a block package, 16-byte aligned
  };
  const int64_t *nPick;          // ... and how many it listed
  int32_t *set;                  // the quiz's set so far, LOCAL ids in listed order (-1: a step without a pick)
  int32_t parent0, nParents, row0, nRows, gain0, question, nSet, pad;
};
hipError_t LaunchPageRoots(const KbView &kb, const TopBatchPriors &priors, const PageQuiz *quizzes, int64_t nQuizzes, double *rows, int64_t pitch, double *masses,
                           hipStream_t stream);
hipError_t LaunchPageExpand(const KbView &kb, const PageQuiz *quizzes, int64_t nQuizzes, int64_t maxParents, double *rows, int64_t pitch, double *masses,
                            int64_t blockLdT /* 0: no record of the list is kPageBlockGiven */, hipStream_t stream);
hipError_t LaunchPageCombine(const KbView &kb, const PageQuiz *quizzes, int64_t nQuizzes, const double *gains, int64_t gainPitch, const double *masses,
                             double *combined, int64_t combPitch, uint32_t *excl, int64_t exclWords, hipStream_t stream);

}  // namespace pqa
