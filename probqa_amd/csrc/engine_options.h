// engine_options.h -- every option of PqaHip_SetOption / PqaHip_GetOption in one place: its field and default (EngineOptions),
// its name, accepted values, side effects and PQA_* variable (kOptions).  HipEngine::SetOption, GetOption and ApplyEnvironment,
// the sharded engine's own two options and the "option_spec:" probe of c_abi.cpp all read this table; a new option is one field
// and one row.  Also here, because both engines share them: the selector's random number generator and the reader of PQA_SEED.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pqa_kernels.h"   // kMaxWorkers

namespace pqa {

struct EngineOptions {
  // ---- resident sweep (pqa_kernels.h: ServerMailbox)
  int64_t server = 0;                 // argmax selections through the resident sweep kernel
  int64_t serverIdleUs = 500;         // that kernel leaves after this long without a request
  int64_t serverVramMailbox = 1;      // requests are written to host-visible device memory where the platform maps it (until the first selection)
  // ResumeQuiz seeds the first answered question's product from vector 0 of vB for every target vector, as the reference binary
  // does (PqaCore/CEUpdatePriorsSubtaskMul.cpp:53 loads pvB, not pvB + j): the drop-in default.  0 = the evident intent.
  int64_t bugCompat = 1;
  int64_t speculate = 1;              // the next sweep ahead of its request (HipEngine::Speculation)
  int64_t fuseUpdate = 1;             // RecordAnswer's posterior update inside the speculative sweep's launch
  // ---- concurrent callers
  int64_t combine = 1;                // 0 = every call by itself
  int64_t combineSpin = 1;            // 1 = waiting clients spin while they are fewer than the allowed CPUs, 0 = they always sleep
  int64_t lingerUs = 20;              // how long a ListTopTargets waits for the other clients' RecordAnswers before it launches the updates
  int64_t postAlways = 0;             // test hook: the posted form of every call that can be posted (HipEngine::TakeOrPost) even when the engine is free
  // ---- rows at the pole of the lack term (pole_kernels.hip)
  int64_t poleFix = 1;                // 0: questions with a row at the pole keep the sweep's own sums
  int64_t poleGate = 1;               // a fused single-quiz ARGMAX has only the listed questions redone that can still win (pole_bounds_kernel); 0: every listed question
  int64_t poleLazy = 1;               // synchronous single-quiz selections launch the fix only when the sweep listed something (FusedSelect::lazyFix)
  int64_t poleFollow = 1;             // measurement hook: 0 = the watching sweeps without the fix launched behind them (KbView::poleNoFollow)
  int64_t lateEager = 3;              // see Quiz::lateStreak (0: speculative sweeps always with the fix-up behind them)
  // ---- selection
  int64_t select = 0;                 // NextQuestion's selector: 0 = the reference's weighted draw, 1 = argmax
  int64_t workers = 16;               // emulated thread-pool size (summation order of the posterior updates, training buckets)
  int64_t evalSubtasks = 0;           // question subtasks of the sampled selector; 0 = 8 * workers (PqaCore/CpuEngine.cpp:339)
  int64_t evalVariant = 0;            // the sweep's kernel shape, 0 = automatic
  int64_t evalMaxGrid = 0;            // test hook: KbView::maxGrid
  int64_t useGraph = 0;               // NextQuestion (argmax) replays a per-quiz HIP graph instead of launching
  int64_t timeSweeps = 0;             // measurement hook: events around every launched fp64 sweep; read-only "last_sweep_ns"
  int64_t hostSampled = 1;            // the sampled NextQuestion as ONE launch + the selector on the host (the finisher workgroup hands over the priority vector)
  int64_t fusedSampled = 0;           // the sampled NextQuestion as ONE launch (the sweep's finisher workgroup runs the selector): correct,
                                      // but 38.3 vs 36.4 us at 1000 x 5 x 1000 -- one workgroup's serial selection costs more than a launch
  int64_t sampledBatchHost = 0;       // 1 = NextQuestionSampledBatch by the host's selector over the copied priorities (the A/B leg)
  // ---- batched sweeps (batch_kernels.hip)
  int64_t batchMin = 0;               // batches of at least this many quizzes take the row-sharing sweep (lane = quiz), smaller ones grid.y = quiz; 0 = by the number of waves the batch gives the row-sharing sweep
  int64_t batchForm = 0;              // 0: the batch's form by its size and the cube's shape; 1 grid.y = quiz, 2 row-sharing, 3 (quiz, chunk) lanes
  int64_t batchQb = 0;                // questions per block of that sweep (0 = default)
  int64_t batchTile = 0;              // targets per LDS tile of that sweep (0 = default)
  int64_t batchGroups = 0;            // question groups per workgroup of that sweep for batches under 129 quizzes (0 = automatic)
  int64_t batchTail = 1;              // that sweep's last, partial round as a launch of its own with fewer questions per group (LaunchEvalBatch)
  int64_t rerank = 1;                 // Float engines' batched argmax: the fp32 sweep's best 8 questions per quiz re-ranked in fp64
  // ---- long rows (cluster_kernels.hip)
  // Rows longer than this many elements take the cluster sweep.  10240: what the register shapes hold without spilling -- the
  // 16-wave shapes behind them (128 registers a lane) ran 10500^2 at 2552 us against the cluster's 1597, 12000^2 at 3004 against
  // 1974, 16000^2 at 4230 against 3430 (round 6, one box); they stay selectable (eval_variant 6, 7, 11).
  int64_t clusterFrom = 10240;
  int64_t clusterForm = 0;            // one quiz: 0 = default, 1 = question by question, 2 = pass 1 a question ahead
  int64_t clusterShape = 0;           // the shape of the form that runs ahead (kAheadVariants), 0 = default
  int64_t longRowForm = 1;            // StartQuiz / RecordAnswer over rows beyond 16384 targets as one workgroup per subtask of the sum; 0: the one-workgroup kernels there too
  // ---- listings, resumed quizzes, training
  int64_t topExact = 1;               // ListTopTargets: the reference's order among equal probabilities; 0: always by ascending target (the fast listing alone)
  int64_t topCache = 10;              // targets RecordAnswer's kernel lists ahead of the ListTopTargets that follows it (0: none)
  int64_t rowsStage = 1;              // ResumeQuizFromRows: 1 = a package in host memory is copied to the device before it is read, 0 = read in place
  int64_t trainChunkSteps = int64_t(1) << 22;   // test hook: the most steps one launch of a training batch carries
};

// Side effects that options share.  The first two run before the new value is stored, the last one after it.
enum : uint8_t {
  kOptStopServer = 1,       // the resident sweep leaves: its launch arguments hold the old value
  kOptSettlePoleList = 2,   // the suspect list is emptied while it is still in view
  kOptBumpKbVersion = 4,    // captured graphs hold the old value
};

struct OptionSpec {
  const char *name;
  int64_t EngineOptions::*field;
  int64_t lo, hi;     // accepted values; anything else is refused
  bool flag;          // SetOption stores any non-zero value as 1 and refuses nothing (the environment still wants 0 or 1)
  uint8_t effects;
  const char *env;    // the PQA_* variable that presets it at creation (stored as it is, without the effects), or nullptr
};

// What this table cannot say stays in HipEngine::SetOption / GetOption: "top_cache" also resets what ListTopTargets has been asked
// for lately, "speculate" drops the speculation in flight, "server_vram_mailbox" is refused once the resident sweep's stream
// exists and reads as the live state from then on, "eval_subtasks" reads as 8 * workers while 0, "eval_max_grid" reads as -1;
// "seed" (write-only, PQA_SEED) and PQA_SELECT's words have no row.
inline constexpr OptionSpec kOptions[] = {
    {"server", &EngineOptions::server, 0, 1, true, kOptStopServer, "PQA_SERVER"},
    {"server_idle_us", &EngineOptions::serverIdleUs, 10, 1000000, false, kOptStopServer, nullptr},
    {"server_vram_mailbox", &EngineOptions::serverVramMailbox, 0, 1, true, 0, nullptr},
    {"bug_compat", &EngineOptions::bugCompat, 0, 1, true, 0, "PQA_BUG_COMPAT"},
    {"speculate", &EngineOptions::speculate, 0, 1, true, 0, "PQA_SPECULATE"},
    {"fuse_update", &EngineOptions::fuseUpdate, 0, 1, true, 0, nullptr},
    {"combine", &EngineOptions::combine, 0, 1, true, 0, "PQA_COMBINE"},
    {"combine_spin", &EngineOptions::combineSpin, 0, 1, true, 0, nullptr},
    {"combine_linger_us", &EngineOptions::lingerUs, 0, 10000, false, 0, nullptr},
    {"post_always", &EngineOptions::postAlways, 0, 1, true, 0, nullptr},
    {"pole_fix", &EngineOptions::poleFix, 0, 1, true, kOptStopServer | kOptSettlePoleList | kOptBumpKbVersion, "PQA_POLE_FIX"},
    {"pole_gate", &EngineOptions::poleGate, 0, 1, true, kOptStopServer | kOptSettlePoleList, nullptr},
    {"pole_lazy", &EngineOptions::poleLazy, 0, 1, true, kOptStopServer | kOptSettlePoleList, nullptr},
    {"pole_follow", &EngineOptions::poleFollow, 0, 1, true, kOptStopServer | kOptSettlePoleList, nullptr},
    {"late_eager", &EngineOptions::lateEager, 0, 1000000, false, 0, nullptr},
    {"select", &EngineOptions::select, 0, 1, false, 0, nullptr},
    {"workers", &EngineOptions::workers, 1, kMaxWorkers, false, 0, "PQA_WORKERS"},
    {"eval_subtasks", &EngineOptions::evalSubtasks, 0, 8192, false, 0, nullptr},
    {"eval_variant", &EngineOptions::evalVariant, 0, INT64_MAX, false, 0, nullptr},
    {"eval_max_grid", &EngineOptions::evalMaxGrid, 0, 65535, false, kOptStopServer | kOptBumpKbVersion, nullptr},
    {"use_graph", &EngineOptions::useGraph, 0, 1, true, 0, nullptr},
    {"time_sweeps", &EngineOptions::timeSweeps, 0, 1, true, 0, nullptr},
    {"host_sampled", &EngineOptions::hostSampled, 0, 1, true, 0, nullptr},
    {"fused_sampled", &EngineOptions::fusedSampled, 0, 1, true, 0, nullptr},
    {"sampled_batch_host", &EngineOptions::sampledBatchHost, 0, 1, true, 0, nullptr},
    {"batch_min", &EngineOptions::batchMin, 0, 257, false, 0, nullptr},
    {"batch_form", &EngineOptions::batchForm, 0, 3, false, 0, nullptr},
    {"batch_qb", &EngineOptions::batchQb, 0, 4, false, 0, nullptr},
    {"batch_tile", &EngineOptions::batchTile, 0, 8192, false, 0, nullptr},
    {"batch_groups", &EngineOptions::batchGroups, 0, 8, false, 0, nullptr},
    {"batch_tail", &EngineOptions::batchTail, 0, 1, true, 0, nullptr},
    {"rerank", &EngineOptions::rerank, 0, 1, true, 0, nullptr},
    {"cluster_from", &EngineOptions::clusterFrom, 1024, 16384, false, kOptStopServer, nullptr},
    {"cluster_form", &EngineOptions::clusterForm, 0, 2, false, 0, nullptr},
    {"cluster_shape", &EngineOptions::clusterShape, 0, 2, false, 0, nullptr},
    {"long_row_form", &EngineOptions::longRowForm, 0, 1, true, 0, nullptr},
    {"top_exact", &EngineOptions::topExact, 0, 1, true, 0, nullptr},
    {"top_cache", &EngineOptions::topCache, 0, 256, false, 0, nullptr},
    {"rows_stage", &EngineOptions::rowsStage, 0, 1, true, 0, nullptr},
    {"train_chunk_steps", &EngineOptions::trainChunkSteps, 1, int64_t(1) << 28, false, 0, nullptr},
};
inline constexpr int64_t kOptionCount = (int64_t)(sizeof(kOptions) / sizeof(kOptions[0]));

inline const OptionSpec *FindOption(const char *name) {
  if (name)
    for (const OptionSpec &o : kOptions)
      if (std::strcmp(o.name, name) == 0) return &o;
  return nullptr;
}

// Whether `value` is one that SetOption stores for this option, and as what.
inline bool AcceptOption(const OptionSpec &o, int64_t &value) {
  if (o.flag) { value = value ? 1 : 0; return true; }
  return value >= o.lo && value <= o.hi;
}

// An integer variable of the environment within lo..hi.  Anything else is ignored, with a line on stderr if `report`.
inline bool EnvInteger(const char *name, int64_t lo, int64_t hi, int64_t &out, bool report = true) {
  const char *v = std::getenv(name);
  if (!v || !*v) return false;
  char *end = nullptr;
  const long long x = std::strtoll(v, &end, 10);
  if (end == v || *end != 0 || x < lo || x > hi) {
    if (report) std::fprintf(stderr, "PqaCore: ignoring %s=%s (expected an integer in %lld..%lld)\n", name, v, (long long)lo, (long long)hi);
    return false;
  }
  out = x;
  return true;
}
// PQA_SEED: the seed of the selector's generator (the reference's cannot be seeded).  Any int64.
inline bool SeedFromEnvironment(int64_t &seed, bool report) { return EnvInteger("PQA_SEED", INT64_MIN, INT64_MAX, seed, report); }

// The selector's generator: xorshift128+, the generator family of SRPlatform/Interface/SRFastRandom.h:60-72, its two words
// filled by SplitMix64.
struct SelectorRng {
  uint64_t s[2] = {0, 0};
  void Seed(uint64_t x) {
    for (uint64_t &word : s) {
      uint64_t z = (x += 0x9E3779B97F4A7C15ULL);
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
      word = z ^ (z >> 31);
    }
  }
  uint64_t Next() {
    uint64_t s1 = s[0];
    const uint64_t s0 = s[1];
    s[0] = s0;
    s1 ^= s1 << 23;
    s[1] = s1 ^ s0 ^ (s1 >> 18) ^ (s0 >> 5);
    return s[1] + s0;
  }
};

}  // namespace pqa
