/*
 * PqaHipExt.h -- additive exports of libPqaCore.so (MI355X build).  Nothing here exists in the reference; unchanged
 * wrappers never need it.  It exposes (a) the deterministic outputs of the hot path, which the reference hides
 * behind a random draw (PqaCore/CpuEngine.cpp:379), so that parity can be checked; (b) bulk KB transfer for tests and
 * benchmarks; (c) stream-ordered (no host sync) entry points and question-axis sharding for multi-GPU hosts.
 * Same conventions as PqaCInterop.h: void* returns are NULL or a PqaError*.
 */
#ifndef PQA_HIP_EXT_H
#define PQA_HIP_EXT_H

#include "PqaCInterop.h"

#pragma pack(push, 8)
typedef struct {
  int64_t _qFirst;   /* first GLOBAL question index held by this engine */
  int64_t _qTotal;   /* global number of questions (== _nQuestions of the definition when unsharded) */
  int32_t _device;   /* HIP device ordinal, -1 = current device */
  int32_t _reserved;
} CiHipShard;

typedef struct {     /* an entry of PqaEngine_ListTopQuestions: CiRatedTarget's layout, 16 bytes */
  int64_t _iQuestion; /* GLOBAL question index */
  double _priority;
} CiRatedQuestion;

typedef struct {     /* result of a stream-ordered selection; lives in device or pinned host memory */
  double _priority;
  int64_t _iQuestion; /* GLOBAL question index, -1 if no eligible question in this shard */
} CiHipSelection;

typedef struct {     /* a quiz's record of PqaEngine_QuizStatusBatch, 40 bytes */
  double _entropy;      /* -sum p log2 p over the candidates, in bits */
  double _mass;         /* sum p over the candidates */
  double _topProb;      /* the largest candidate probability, 0.0 without a candidate */
  int64_t _iTopTarget;  /* its target, the lowest id among equals; -1 without a candidate */
  int64_t _nCandidates; /* targets that are no gaps and hold p > 0 */
} CiHipQuizStatus;
#pragma pack(pop)

#ifdef __cplusplus
extern "C" {
#endif

/* Same as PqaEngineFactory_CreateCpuEngine (which creates the HIP engine too); explicit name for new callers. */
PQACORE_API void *PqaEngineFactory_CreateHipEngine(void *pvFactory, void **ppError, const CiEngineDefinition *pEngDef);
/* Same as PqaEngineFactory_LoadCpuEngine (which loads into the HIP engine too); explicit name for new callers. */
PQACORE_API void *PqaEngineFactory_LoadHipEngine(void *pvFactory, void **ppError, const char *filePath, uint64_t memPoolMaxBytes);
/* Engine over questions [_qFirst, _qFirst + pEngDef->_nQuestions) of a KB with _qTotal questions.  Question ids in
 * every call on such an engine are GLOBAL ids. */
PQACORE_API void *PqaEngineFactory_CreateHipEngineSharded(void *pvFactory, void **ppError,
                                                          const CiEngineDefinition *pEngDef, const CiHipShard *pShard);

/* ---- .kb files per shard and in either precision.  The byte layout is the reference's; a file's number type (its
 * PrecisionDefinition: Float or Double) and the engine's need not be the same: where they differ every row passes through a device
 * kernel on its way -- fp64 -> fp32 rounds to nearest even, as (float)x does, fp32 -> fp64 is exact -- instead of through fp64 host
 * arrays of the whole cube (PqaHip_GetKB / PqaHip_SetKB).
 *
 * precType: 0 = the file's, else TPqaPrecisionType Float (1) or Double (3); anything else is NotImplemented.
 * pShard NULL = the whole file (with PQA_DEVICES naming several devices: the one-process sharded engine, in that precision).
 * Otherwise the engine holds questions [_qFirst, _qFirst + nLocalQuestions) of the file on _device (-1: the current one); _qTotal must
 * be 0 or the file's question count (InsufficientEngineDimensions otherwise); a range that is not within the file's questions is
 * IndexOutOfRange, a negative count NegativeCount; pShard together with PQA_DEVICES is refused (WrongMode).  The shard reads its two
 * blocks of rows by seeking to them, the whole vB, the target gaps and the target and quiz id maps; the question gaps of its range
 * become its gap bits, and the file's question gap list and question id map become the shard's view of the whole question axis.
 * A header whose dimensions are no knowledge base's, or whose arrays the file is too short for, is FileOp before anything is
 * allocated.  A finite value that does not fit Float fails the load (FileOp, naming the array: _sA, _mD or _vB); no engine is
 * returned.  C++ exceptions do not cross these three calls: they come back as StdException / SRException. */
PQACORE_API void *PqaEngineFactory_LoadHipEngineAs(void *pvFactory, void **ppError, const char *filePath, uint8_t precType,
                                                   const CiHipShard *pShard, int64_t nLocalQuestions);
/* PqaEngine_SaveKB in a chosen precision (0 = the engine's own: the bytes PqaEngine_SaveKB writes).  The header is the one an
 * engine created in that precision writes (Float: mantissa 24, exponent 8; Double: 53, 11), the arrays are in that type.  One-device
 * engines and the one-process sharded engine; on a shard NotImplemented, as PqaEngine_SaveKB is. */
PQACORE_API void *PqaHip_SaveKBAs(void *pvEngine, const char *filePath, uint8_t precType);
/* A shard's part of a save, in place: the file is opened without being emptied (created if missing) and the shard writes its sA
 * block and its mD block at their offsets.  The shard that holds question 0 also writes the header -- with ITS count of questions
 * asked; every rank sees every Train --, vB and the trailer, and cuts the file behind the trailer.  The file is complete once every
 * shard's call has returned; the calls may run in any order or at once (they write disjoint ranges), ordering them against readers is the
 * caller's business (probqa_amd/dist.py: save_kb).  Every shard must name the same precType.  A shard loaded from a file writes that
 * trailer is the shard's view of the whole question axis -- the gap list and the id map every rank keeps: the file's as loaded, or
 * fresh ids for a created shard, with everything PqaHip_SetQuestionGaps and the maintenance calls have done to them since.
 * On a whole one-device engine the call is an equivalent of PqaHip_SaveKBAs (the engine is the only shard of its file); on the
 * one-process sharded engine it is NotImplemented. */
PQACORE_API void *PqaHip_SaveKBShard(void *pvEngine, const char *filePath, uint8_t precType);

/* ---- options: "select" (0 = sampled like the reference [default], 1 = argmax), "workers" (emulated CPU worker count
 * fixing the summation order of the prior updates, default 16), "eval_subtasks" (question subtasks of the sampled
 * selector, default 8*workers as PqaCore/CpuEngine.cpp:339), "eval_variant" (0 = auto), "bug_compat" (reproduce
 * PqaCore/CEUpdatePriorsSubtaskMul.cpp:53), "seed" (selector RNG seed), "use_graph" (argmax NextQuestion replays a per-quiz HIP graph
 * instead of launching the sweep), "top_cache" (how many of the new posterior's best
 * targets RecordAnswer's kernel lists at most ahead of the ListTopTargets call that follows it -- it lists as many as ListTopTargets
 * has been asked for lately; default 10, 0 = none), "server"
 * (argmax selections are served by a resident kernel instead of one launch each -- rows up to 1024 targets; default 0),
 * "server_idle_us" (that kernel leaves after this long without a request, default 500: what a device-wide synchronisation of the host waits at most -- PqaHip_Synchronize asks it to leave at once), "server_vram_mailbox" (requests
 * are written to host-visible device memory where the platform maps it, default 1; set before the first selection).
 * "host_sampled" (the sampled NextQuestion as one launch whose finisher hands the priority vector to the host, which runs the
 * reference's selector itself; default 1 -- 0: sweep + selector kernel), "fused_sampled" (the selector inside the sweep's launch;
 * default 0: measured slower),
 * "speculate" (StartQuiz / ResumeQuiz / RecordAnswer launch the sweep of the NextQuestion that normally follows them, which then only
 * waits for its result; same questions either way; default 1, also PQA_SPECULATE; read-only "spec_hits" / "spec_dropped" count the
 * speculative sweeps that were used / dropped),
 * "fuse_update" (RecordAnswer's posterior update runs inside the launch of that speculative sweep where its shape allows it -- rows
 * of up to 1024 targets -- instead of in a kernel of its own ahead of it; same bits; default 1; read-only "fused_updates"),
 * "combine" (concurrent client threads: their NextQuestion calls share batched sweeps, their RecordAnswer / StartQuiz /
 * ResumeQuiz / RecordQuizTarget calls share launches, and a call that finds the engine taken posts its operation to the thread inside instead
 * of queueing on the lock; default 1, also PQA_COMBINE; "combine_linger_us": how long a leader / a ListTopTargets waits for the
 * other clients' requests, default 20; read-only "combined_batches", "combined_requests", "combined_max_batch", "update_flushes",
 * "updates_flushed", "update_max_flush", "posted_ops", "posted_drains", "train_batches", "train_batch_calls",
 * "resume_batches", "resumes_batched"),
 * "long_row_form" (StartQuiz / RecordAnswer / ResumeQuiz over rows beyond 16384 targets as one workgroup per subtask of the reference's sum
 * plus a division launch; default 1), "post_always" (test hook: the posted form of the quiz-level calls even when the engine is free),
 * "eval_max_grid" (test hook: cap the workgroups of a sweep so that each streams many questions; 0 = no cap).
 * "batch_min" (PqaEngine_NextQuestionArgmaxBatch: batches of at least this many quizzes take the row-sharing sweep, which
 * reads the cube once per batch; default 0 = decided by how many waves the batch gives that sweep; Float engines always take it), "batch_tile" (targets per LDS tile of that sweep, 0 = default),
 * "batch_groups" (that sweep for batches of up to 128 quizzes: question groups side by side in a workgroup, so that the lanes a small
 * batch leaves over take further questions; 0 = as many as leave every CU a workgroup [default], else at most this many),
 * "batch_tail" (that sweep's last, partial round of question blocks as a second launch of a shape with fewer questions per group, where
 * exactly one full round precedes it; default 1),
 * "pole_fix" (every fp64 sweep watches, row by row, for a posterior element that holds nearly all -- or a quarter, while the answer
 * hardly moves the posterior -- of the row; such questions are listed and a kernel launched behind the sweep re-evaluates them in the
 * reference's own summation order -- SRAccumVectDbl256.h:40-46, :62-92 -- so that late quiz states stay within 1e-9 of the
 * reference's priorities on every kernel form; a resident sweep that finds such a row hands the quiz to the launched path; default 1,
 * also PQA_POLE_FIX), "top_exact" (ListTopTargets where probabilities tie among the listed targets or at the list's end: 1 [default] = the
 * reference's order among equals -- CEListTopTargetsAlgorithm::RunHeapifyBased's per-worker heaps and head heap reproduced on the device for
 * the emulated worker count --, 0 = by ascending target; read-only "top_exact_listings" counts the listings that took the heaps), "pole_gate" (where only the selected question leaves the engine -- NextQuestion with the argmax selector, one quiz -- that kernel
 * redoes only the listed questions whose priority can still be the maximum: per listed question the sweep hands over how close to 1 its
 * largest posterior element can be, a kernel ahead of the fix bounds how far the fix can move the priority, and questions whose upper bound
 * stays below the best lower bound keep the sweep's value; PqaEngine_EvalPriorities and the sampled selector always get every listed
 * question redone; default 1), "pole_lazy" (a synchronous single-quiz selection launches that kernel only when its sweep has listed something
 * -- one launch per selection of a fresh quiz instead of two; default 1; 0 = behind every sweep), "late_eager" (after this many
 * selections of a quiz in a row that needed the fix, RecordAnswer's speculative sweep has it launched right behind it again: it runs
 * while the client is elsewhere; default 3 -- long quizzes in late states +4 %, the learner loop unchanged), "pole_follow" (measurement hook: 0 = the watching sweep WITHOUT the launch behind it, for timing the sweep
 * kernel by itself in a quiz state that lists nothing; default 1),
 * "cluster_from" (rows of more than this many elements -- 1024..16384, default 10240: what the register shapes hold without spilling -- take the
 * cluster sweep, a question over a cluster of workgroups), "cluster_form" (that sweep: 0 = default, 1 = question by question, 2 = pass 1 a question
 * ahead of the exchange), "cluster_shape" (threads x 16-byte units per thread of the form that runs ahead: 0 = default, 1 = 512 x 1, 2 = 256 x 2;
 * two workgroups per CU both; 256 x 2 is built for questions of two to five answers, other answer counts take 512 x 1),
 * "combine_spin" (clients waiting for the engine spin first while they are fewer than the CPUs the process may use; default 1, 0 =
 * they always sleep), "batch_form" (the batched sweep's form: 0 = by the batch's size and the cube's shape [default], 1 = grid.y = quiz,
 * 2 = row-sharing, 3 = (quiz, chunk) lanes), "batch_qb" (questions per block of the row-sharing sweep, 0..4, 0 = default), "rerank"
 * (Float engines' batched argmax: the fp32 sweep's best 8 questions per quiz re-ranked in fp64, so the pick is the fp64 argmax of those 8
 * -- the fp64 argmax of all questions whenever that question is among them; default 1).
 * Described with the calls they belong to: "sampled_batch_host", "time_sweeps", "train_chunk_steps", "rows_stage".
 * The whole list -- name, accepted values, default, side effects, PQA_* variable -- is the table of probqa_amd/csrc/engine_options.h.
 * An option named a flag there takes any integer and stores 0 or 1; every other one refuses a value outside its range with
 * "Unknown option or value out of range: NAME" and keeps the value it had; an unknown name is refused the same way and reads -1.
 * "seed" is write-only and "eval_max_grid" is not readable either: both read -1.  For unchanged wrappers the environment presets
 * PQA_SELECT (sample | argmax), PQA_SERVER, PQA_BUG_COMPAT, PQA_SPECULATE, PQA_COMBINE, PQA_POLE_FIX, PQA_WORKERS and PQA_SEED when
 * an engine is created; a value that is refused there (a flag wants 0 or 1) is reported on stderr and ignored.
 * Read-only: "server_last_step_ns" (device-side duration of the newest finished step of the resident sweep: request in hand
 * to answer published, from the kernel's own 100 MHz clock; -1 if there is none), "precision" (TPqaPrecisionType of the engine: 1 = Float, 3 = Double), "server_active",
 * "ldT" and "capQ" (the allocation: elements between two rows of the cube, questions it has room for -- maintenance only ever grows
 * them), "device". */
PQACORE_API void *PqaHip_SetOption(void *pvEngine, const char *name, int64_t value);
PQACORE_API int64_t PqaHip_GetOption(void *pvEngine, const char *name);
PQACORE_API const char *PqaHip_EvalKernelName(void *pvEngine);

/* ---- bulk KB transfer: dense host arrays without padding, A[q][k][t], D[q][t], B[t] (local questions only) */
PQACORE_API void *PqaHip_SetKB(void *pvEngine, const double *pA, const double *pD, const double *pB);
PQACORE_API void *PqaHip_GetKB(void *pvEngine, double *pA, double *pD, double *pB);
/* Fill the device cube with the deterministic synthetic KB of probqa_amd/synth.py (no host transfer). */
PQACORE_API void *PqaHip_FillSynthetic(void *pvEngine, double nTrain, double noiseAmp, uint64_t seed);
/* Mark targets / (global) questions as gaps without going through maintenance mode (tests of gap handling). */
PQACORE_API void *PqaHip_SetTargetGaps(void *pvEngine, int64_t n, const int64_t *pTargets);
PQACORE_API void *PqaHip_SetQuestionGaps(void *pvEngine, int64_t n, const int64_t *pQuestions);

/* ---- deterministic outputs of the hot path */
/* priority[i] of local question i (0 for gap / asked), i < n == local question count. */
PQACORE_API void *PqaEngine_EvalPriorities(void *pvEngine, const int64_t iQuiz, double *pOut, const int64_t n);
/* NextQuestion with the argmax selector / with the reference's selector driven by the given 64-bit random number. */
PQACORE_API int64_t PqaEngine_NextQuestionArgmax(void *pvEngine, void **ppError, const int64_t iQuiz);
PQACORE_API int64_t PqaEngine_NextQuestionSampled(void *pvEngine, void **ppError, const int64_t iQuiz,
                                                  const uint64_t rnd);
/* NextQuestion (argmax selector) for nQuizzes <= 256 distinct quizzes with ONE launch: pQuestions[i] = the selected
 * question of pQuizzes[i], -1 if that quiz has no question left.  What a server with many quizzes in flight calls instead
 * of nQuizzes x PqaEngine_NextQuestion (reference PqaCore/CpuEngine.cpp:337-415 serves them one sweep at a time). */
PQACORE_API void *PqaEngine_NextQuestionArgmaxBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes,
                                                    int64_t *pQuestions);
/* The reference's own selector (PqaCore/CpuEngine.cpp:362-400: a question drawn with probability proportional to its priority) for
 * nQuizzes <= 256 distinct quizzes with ONE batched sweep and one selector launch behind it: pQuestions[i] is the question
 * PqaEngine_NextQuestionSampled(pQuizzes[i], pRnd[i]) selects, and it becomes that quiz's active question; -1 (and no error) for a
 * quiz with no question left.  A repeated or unknown quiz id is an error that names the entry and changes nothing.  The selector
 * reads the priorities on the device, where the sweep left them; option "sampled_batch_host" = 1 serves the same call with the
 * host's selector over the copied priorities instead (for comparison; default 0).  Read-only options: "sampled_batches" (calls that
 * selected), "sampled_batch_device_ns" (with "time_sweeps": the selector launches' time between events), "priority_host_bytes"
 * (bytes of priorities the batched sweeps have delivered to the host). */
PQACORE_API void *PqaEngine_NextQuestionSampledBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const uint64_t *pRnd,
                                                     int64_t *pQuestions);
/* What a server with many quizzes in flight calls instead of nQuizzes x PqaEngine_NextQuestion: the engine's "select" option
 * decides.  select = 1: PqaEngine_NextQuestionArgmaxBatch.  select = 0: one random number per quiz from the engine's generator, in
 * batch order, exactly as nQuizzes consecutive PqaEngine_NextQuestion calls would draw them (a refused call draws none), then
 * PqaEngine_NextQuestionSampledBatch. */
PQACORE_API void *PqaEngine_NextQuestionBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, int64_t *pQuestions);
/* RecordAnswer for nQuizzes quizzes (each with an active question) in one call and ONE launch -- every posterior bit-identical to
 * PqaEngine_RecordAnswer's (reference PqaCore/CERecordAnswerSubtaskMul.cpp:15-42 per quiz) -- and StartQuiz for nQuizzes new
 * quizzes likewise (pQuizzes receives their ids; all or none).  What a server with many quizzes in flight calls beside
 * PqaEngine_NextQuestionArgmaxBatch; concurrent PqaEngine_RecordAnswer calls of different client threads are gathered into the
 * same batched launch by the engine itself (option "combine"). */
PQACORE_API void *PqaEngine_RecordAnswerBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pAnswers);
PQACORE_API void *PqaEngine_StartQuizBatch(void *pvEngine, const int64_t nQuizzes, int64_t *pQuizzes);
/* ResumeQuiz for nQuizzes quizzes in one call and one launch per chunk.  Quiz i resumes from the pCounts[i] answered
 * questions starting at pAQs[sum(pCounts[0..i))]; pCounts[i] == 0 is a StartQuiz (BaseEngine.cpp:393-395).  Every posterior is
 * bit-identical to PqaEngine_ResumeQuiz's for the same list (CEUpdatePriorsSubtaskMul + NormalizePriors + CEDivTargPriors).
 * All or none: on any error (index out of range, I64Underflow of any quiz, out of memory) no quiz is created and the error
 * names the batch entry.  pQuizzes receives the ids, in the order consecutive PqaEngine_ResumeQuiz calls would assign them.
 * No speculative sweep is launched behind the batch.  Concurrent PqaEngine_ResumeQuiz calls of different client threads are
 * gathered into such a batch by the engine itself (option "combine"; counters "resume_batches", "resumes_batched"). */
PQACORE_API void *PqaEngine_ResumeQuizBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pCounts,
                                            const CiAnsweredQuestion *pAQs, int64_t *pQuizzes);
/* Train for nRecords records in one call: record i = the pCounts[i] answered questions starting at pAQs[sum(pCounts[0..i))],
 * its target pTargets[i] and amount pAmounts[i].  A, D and vB end bit-identical to nRecords consecutive PqaEngine_Train calls
 * in this order (reference PqaCore/CpuEngine.cpp:102-183, CETrainOperation.cpp:15-83); the asked-questions counter grows by
 * sum(pCounts).  All or none: every record is validated before any cell changes; the error names the batch entry.  pAQs may be
 * null when every count is 0.  One launch per chunk of at most "train_chunk_steps" steps (default 2^22); read-only counters
 * "train_bulk_calls", "train_bulk_records", "train_bulk_launches", "train_bulk_host_ns" (host preparation and launching) and
 * "train_bulk_device_ns" (the kernels, between events), summed over the engine's batches. */
PQACORE_API void *PqaEngine_TrainBatch(void *pvEngine, const int64_t nRecords, const int64_t *pCounts,
                                       const CiAnsweredQuestion *pAQs, const int64_t *pTargets, const double *pAmounts);
/* RecordQuizTarget for nQuizzes quizzes (ids may repeat) in one call: the same KB as consecutive PqaEngine_RecordQuizTarget
 * calls (BaseEngine.cpp:529-566, CpuEngine.cpp:442-466); the counter is not touched.  All or none likewise; same launches and
 * counters as PqaEngine_TrainBatch. */
PQACORE_API void *PqaEngine_RecordQuizTargetBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes,
                                                  const int64_t *pTargets, const double *pAmounts);
/* ListTopTargets for nQuizzes quizzes (any number; 256 per launch sequence) without copying a posterior to the host: pDest[i * maxCount + j],
 * j < pCounts[i], is the listing PqaEngine_ListTopTargets(pQuizzes[i], maxCount) returns -- descending probability, gaps and
 * probabilities <= 0 dropped (reference PqaCore/CEHeapifyPriorsSubtaskMake.cpp:42-52), equal probabilities in the order the reference's
 * per-worker heaps leave them (option "workers" = its thread count; option "top_exact" 0: by ascending target instead).
 * Rows of any length: 4096-target chunks list their own best maxCount on the device and merge there; what crosses to the host is
 * nQuizzes x maxCount records (the reference's GPU engine copies all nTargets posteriors per quiz: PqaCore/CudaEngine.cpp:251-289). */
PQACORE_API void *PqaEngine_ListTopTargetsBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t maxCount,
                                                CiRatedTarget *pDest, int64_t *pCounts);
/* The best next questions of a quiz, listed on the device: the quiz's questions that are neither asked nor gaps and whose priority is
 * > 0, by descending priority, ascending question index among equal priorities, at most maxCount of them.  Returns the number listed;
 * -1 and *ppError on failure.  The priorities are the ones PqaEngine_EvalPriorities returns for that quiz at that moment, bit for bit
 * (the same sweep, the pole fix behind it redoing every listed question): on a Double engine the first entry is the question
 * PqaEngine_NextQuestionArgmax selects whenever any priority is positive; a Float engine lists by its fp32 sweep's priorities, as its
 * single-quiz argmax selects by them (no fp64 re-rank).  Question ids are GLOBAL ids; an engine made by
 * PqaEngineFactory_CreateHipEngineSharded lists its own questions (probqa_amd/dist.py merges the ranks' lists), the one-process
 * sharded engine (PQA_DEVICES) lists on every shard at once and merges on the host.
 * No quiz state changes: the active question stays what it was, no counter moves; a client that takes a listed question follows with
 * PqaEngine_SetActiveQuestion and PqaEngine_RecordAnswer.  Towards the resident sweep (option "server"), the speculative sweep and the
 * pole list the call does what PqaEngine_EvalPriorities does.
 * maxCount <= 256: the listing kernels run on the engine's stream behind the sweep and write the records into host-coherent memory;
 * nothing of size nQuestions crosses to the host.  Beyond 256 the call is a bulk export, as long listings of targets are: the priority
 * vector is copied and its prefix taken on the host, in the same order.
 * maxCount == 0 lists nothing and is no error.  Errors: an unknown quiz and maintenance mode as PqaEngine_ListTopTargets answers them,
 * maxCount < 0 NegativeCount, pDest == NULL with maxCount > 0 NullArgument -- PqaEngine_ListTopTargetsBatch's codes.  C++ exceptions
 * do not cross the two calls (StdException / SRException). */
PQACORE_API int64_t PqaEngine_ListTopQuestions(void *pvEngine, void **ppError, const int64_t iQuiz, const int64_t maxCount,
                                               CiRatedQuestion *pDest);
/* The same for nQuizzes <= 256 distinct quizzes behind ONE batched sweep: pDest[i * maxCount + j], j < pCounts[i], is the listing of
 * pQuizzes[i] by the priorities PqaEngine_EvalPrioritiesBatch returns for the same batch, whichever form option "batch_form" and the
 * batch give that sweep (the listing reads the quizzes' own vectors or the quiz-minor matrix where the sweep left them; it forces no
 * form).  What crosses to the host is nQuizzes x maxCount records.  nQuizzes > 256, a repeated or an unknown quiz id are refused as
 * PqaEngine_EvalPrioritiesBatch refuses them, the error naming the entry, and nothing is written; negative counts and missing buffers
 * as PqaEngine_ListTopTargetsBatch. */
PQACORE_API void *PqaEngine_ListTopQuestionsBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t maxCount,
                                                  CiRatedQuestion *pDest, int64_t *pCounts);
/* The priority vectors of nQuizzes <= 256 distinct quizzes from ONE sweep that reads the cube once for the whole batch
 * (batch_kernels.hip): pOut[i * nLocalQuestions + q] = priority of local question q for pQuizzes[i], 0 for gap / asked
 * questions.  The deterministic output behind PqaEngine_NextQuestionArgmaxBatch's row-sharing form. */
/* This engine's (shard's) winners of a batch, without NextQuestion's bookkeeping: pOut[i] = {priority, GLOBAL question index or
 * -1} of pQuizzes[i].  A host that shards the question axis gathers these from the shards, picks per quiz (maximum priority,
 * lowest index on ties) and calls PqaEngine_SetActiveQuestion on every shard. */
PQACORE_API void *PqaHip_SelectArgmaxBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, CiHipSelection *pOut);
PQACORE_API void *PqaEngine_EvalPrioritiesBatch(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, double *pOut);
/* ---- The Among calls: evaluate and select over a LISTED set of questions per quiz (skipping a question, topics / locales / tenants
 * on one knowledge base, re-evaluating a short list between full sweeps).  "Among a list L" means: for this call only, every question
 * outside L counts as asked.  Quiz i's list is the pCounts[i] GLOBAL question ids starting at pQuestions[sum(pCounts[0..i))]; nQuizzes
 * <= 256 distinct quizzes.  One launch evaluates all (quiz, question) pairs of the call (among_kernels.hip: eval_listed_kernel), so the
 * cost follows the lists, not nQuestions: a Double engine's priorities are PqaEngine_EvalPriorities' to 1e-9 relative, late quiz states
 * included (the listed sweep watches for rows at the pole and the pole fix runs behind it, option "pole_fix"); a Float engine's are the
 * fp64 priorities on its fp32 cube rows (no fp32 sweep, no re-rank, no pole fix).
 *   A listed question that is a gap or was asked has priority 0 and is never picked; one that another process's shard holds is skipped
 *   on this shard (priority 0 here).  An empty list is no error: that quiz's pick is -1 and its state does not change.
 *   Argmax: maximum priority, lowest global id among equals; a NaN never wins.  Sampled: the reference's selector
 *   (PqaCore/CpuEngine.cpp:362-400) over the whole question axis with the skip bits gaps | asked | not listed; its fallback to the nearest
 *   free question (:403-406) runs over the same bits and never leaves the list.
 *   Errors: an id outside [0, nQuestions of the whole knowledge base) or repeated within one quiz's list is IndexOutOfRange naming the
 *   batch entry and the position; a negative count NegativeCount; unknown or repeated quizzes, nQuizzes > 256, missing buffers and
 *   maintenance mode as PqaEngine_EvalPrioritiesBatch / PqaEngine_NextQuestionSampledBatch answer them.  A refused call launches nothing,
 *   draws no random number and changes nothing.  The one-process sharded engine (PQA_DEVICES) answers NotImplemented.
 *   Nothing of size nQuestions crosses to the host: sum(pCounts) doubles for the evaluating call, the records for the selecting ones
 *   (read-only option "priority_host_bytes" counts them).  Read-only options "among_calls" / "among_pairs": the accepted calls and the
 *   pairs of theirs this engine holds.  No quiz's own speculative or resident state is touched: a PqaEngine_NextQuestion that follows
 *   returns what it would have returned without the call.
 *   When to use which (tools/among_bench.py, profiles/README.md): the listed sweep re-reads a question's rows from cache for its second pass
 *   where the full sweeps keep them on chip -- measured on an MI355X for batches of 64-256 quizzes, the full
 *   sweep (PqaEngine_NextQuestionArgmaxBatch) is the cheaper call from a list of about 7-8 % of nQuestions at 1000 x 5 x 1000 and on a Float
 *   engine at 10000 x 5 x 10000, and from about 16 % on a Double engine at 10000 x 5 x 10000 (one quiz there: 23 %; one quiz at 1000 x 5 x 1000:
 *   the single-quiz sweep is always cheaper).  With the whole axis listed the call is slower than the full sweep by 4-6 x (Double,
 *   10000 x 5 x 10000) to 13 x (1000 x 5 x 1000; Float engines).  256 quizzes x 16 questions: 0.4 ms and 1.5 ms at the two sizes.
 * pOut is parallel to pQuestions. */
PQACORE_API void *PqaEngine_EvalPrioritiesAmongBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                     const int64_t *pQuestions, double *pOut);
/* The best targets of nQuizzes quizzes WITHIN A LISTED SET of targets each -- a tenant's catalogue, what is in stock, a platform's
 * titles -- and how much of the posterior the set holds.  The lists are given once and the quizzes point at them: list l is
 * pListCounts[l] target ids from pTargets[sum(pListCounts[0..l))], in any order; quiz i takes list pListOf[i], or list i where pListOf
 * is NULL (then nLists == nQuizzes).  The reference has no such call.
 *  (a) Candidates: a target of the quiz's list that is no gap and whose posterior is > 0 -- PqaEngine_ListTopTargets' rule.
 *  (b) Order: probability descending, target id ascending among equal probabilities, whatever the list's order -- the order of the fast
 *      listing (option "top_exact" 0) and of PqaEngine_ListTopQuestions, NOT the reference's heap order among ties: its heaps are
 *      defined over the whole target axis, and no call of the reference lists within a set.
 *  (c) Counts: quiz i gets pCounts[i] = min(maxCount, candidates) records at pDest + i * maxCount.
 *  (d) Values: the probabilities are the posterior's own bits; nothing is renormalised.
 *  (e) Mass: pMass[i] (pMass may be NULL) is the sum of the candidates' probabilities in fp64; a client divides by it to renormalise.
 *  (f) Determinism: the mass is summed in a fixed order without atomics.  The same call gives the same bits, and a quiz's records and
 *      mass do not depend on what else is in the batch.
 *  (g) State: no quiz state changes.  Regular mode only; deferred answers are applied first, as in PqaEngine_ListTopTargetsBatch.
 *  (h) Batch shape: any number of quizzes (256 per launch sequence); a quiz may appear more than once (one quiz under several
 *      catalogues); a list may be empty (count 0, mass 0); a list no quiz points at is validated and otherwise ignored.
 *  (i) Refusals, all decided before anything is launched or written: negative nQuizzes, nLists, maxCount (NegativeCount) or list length
 *      (NegativeCount, "list="); a NULL buffer that is needed (NullArgument); pListOf == NULL with nLists != nQuizzes; pListOf[i] out
 *      of [0, nLists) ("entry="); an unknown quiz ("entry="); a target id out of [0, nTargets) or twice in one list (IndexOutOfRange,
 *      "list=", "position=", "targetId=").
 * The cost follows the lists, not nTargets: the ids are staged once per call (int32), every wave gathers 1024 entries of its quiz's
 * list and lists its own best, the existing merges do the rest; per quiz, maxCount records, a count and a mass cross to the host.  A
 * quiz whose min(maxCount, its list's length) exceeds 256 has the posteriors of its LIST gathered and is selected on the host in the
 * same order (b), its mass summed in the list's order -- still no copy of all nTargets posteriors.  Which of the two ways a quiz takes
 * depends on maxCount and its own list alone, which is what keeps (f).
 * Every shard of a sharded engine holds every quiz's whole posterior: the call works on a shard engine
 * (PqaEngineFactory_CreateHipEngineSharded) as on a whole engine, and the one-process sharded engine lets its first shard list. */
PQACORE_API void *PqaEngine_ListTopTargetsAmongBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pListOf,
                                                     int64_t nLists, const int64_t *pListCounts, const int64_t *pTargets, int64_t maxCount,
                                                     CiRatedTarget *pDest, int64_t *pCounts, double *pMass);
/* What each answer WOULD do to a quiz, before the user gives one: for nPairs (quiz pQuizzes[i], GLOBAL question pQuestions[i]) pairs, all
 * nAnswers would-be posteriors in one call, read-only.  Row r = i * nAnswers + k stands for "pair i answered with k".  The reference has
 * no such call.
 *  (a) Posterior: x_t = prior_t * (A[q][k][t] / D[q][t]) (0 at target gaps), total = the reference-order sum of x, p_t = x_t / total --
 *      RecordAnswer's operations in its order: bit for bit what PqaEngine_SetActiveQuestion(q) + PqaEngine_RecordAnswer(k) would leave
 *      in that quiz, on Double and Float engines, at every row length.
 *  (b) pLikelihood[r] (may be NULL) = total: the predictive probability of answer k.
 *  (c) pEntropy[r] (may be NULL) = -sum p_t log2 p_t over the p_t > 0, in bits: fp64, from the divided values, in a fixed order without
 *      atomics.  Against -math.fsum(p log2 p) it is within (nTargets + 16) 2^-52 max(1, H) bits.
 *  (d) Records: pCounts[r] = min(maxCount, candidates) records at pDest + r * maxCount; a candidate is a target that is no gap with
 *      p_t > 0; probability descending, target id ascending among equals -- the order of PqaEngine_ListTopTargetsAmongBatch and of the
 *      fast listing (option "top_exact" 0), not the reference's heap order; _prob carries the posterior's own bits.  pDest and pCounts
 *      may be NULL only when maxCount == 0.
 *  (e) A dead answer (total is 0 or not finite): likelihood = that total, entropy = a quiet NaN, count 0.
 *  (f) State: no quiz state changes -- posterior, active question, asked bits, answers, versions, speculative and resident state all stay;
 *      a NextQuestion that follows returns what it would have returned without the call.  Regular mode only; deferred answers are
 *      applied first, as in PqaEngine_ListTopTargetsBatch.
 *  (g) Batch shape: any number of pairs (256 rows per launch sequence); a quiz may appear in several pairs and a pair may repeat; an
 *      asked question is previewed like any other.  A row's outputs depend on its quiz, question and answer alone.
 *  (h) Refusals, all decided before anything is launched or written, in this order: negative nPairs or maxCount (NegativeCount);
 *      maxCount > 256 (IndexOutOfRange: a preview is a screenful, there is no bulk path); a needed buffer NULL (NullArgument); maintenance
 *      mode or shutdown, as PqaEngine_ListTopTargetsBatch answers them; an unknown quiz ("entry="); a question outside
 *      [0, nQuestions of the whole knowledge base) or a gap on the engine that holds it (IndexOutOfRange, "entry=", "questionId=").
 * One workgroup per row computes the posterior into engine scratch and reduces it to likelihood and entropy; the batched listing takes
 * the scratch rows; records, counts and two doubles per row cross to the host, nothing of size nTargets.
 * A shard engine (PqaEngineFactory_CreateHipEngineSharded) holds every posterior whole and answers for the pairs whose question it
 * holds; for the others it writes zeros (likelihood 0.0, entropy 0.0, count 0) -- there is no package: a host takes each pair from
 * the rank that holds its question (probqa_amd/dist.py: preview_answers_batch).  The one-process sharded engine (PQA_DEVICES) answers
 * NotImplemented.  Read-only options "preview_calls" / "preview_pairs": the accepted calls and the pairs this engine held; with
 * "time_sweeps", "preview_device_ns". */
PQACORE_API void *PqaEngine_PreviewAnswersBatch(void *pvEngine, int64_t nPairs, const int64_t *pQuizzes, const int64_t *pQuestions,
                                                int64_t maxCount, double *pLikelihood, double *pEntropy,
                                                CiRatedTarget *pDest, int64_t *pCounts);
/* The answers a quiz holds: returns their count and writes the first min(count, capacity) of them to pDest, in the order
 * PqaEngine_RecordQuizTarget would train them (the resumed ones, then the recorded ones), with GLOBAL question ids.  pDest == NULL with
 * capacity == 0 only counts.  Errors (the return is -1): an unknown quiz as PqaEngine_ListTopTargets answers it; a negative capacity
 * (NegativeCount); pDest NULL with capacity > 0 (NullArgument).  Whole engines, shard engines and the one-process sharded engine (which
 * hands its gathered answers to the shards first) answer alike: every engine records every answer of every quiz. */
PQACORE_API int64_t PqaHip_GetQuizAnswers(void *pvEngine, void **ppError, int64_t iQuiz, CiAnsweredQuestion *pDest, int64_t capacity);
/* A quiz with each of its answers LEFT OUT, looking back where PqaEngine_PreviewAnswersBatch looks ahead: row i stands for quiz
 * pQuizzes[i] as if its answer at position pPositions[i] (a position of PqaHip_GetQuizAnswers) had never been given.  Read-only; the
 * reference has no such call and no undo.
 *  (a) Posterior: bit for bit what PqaEngine_ResumeQuiz over the remaining answers, in their order, leaves on this engine under its
 *      current options "workers" and "bug_compat", on Double and Float engines at every row length -- the exponent-separated product
 *      chain, the exponent maximum and correction, the reference-order sum over `workers` subtasks, the division.  A quiz with one
 *      answer leaves PqaEngine_StartQuiz's posterior; a question answered more than once is a chain like any other.  The review reads
 *      the knowledge base as it is now, as ResumeQuiz does, and the quiz's recorded answers -- not the quiz's own posterior.
 *  (b) pLikelihood[i] (may be NULL) = the predictive probability, under that posterior, of the answer that was left out: the bits
 *      PqaEngine_PreviewAnswersBatch returns for (a twin quiz resumed from the remaining answers, the left-out question) at the
 *      left-out answer (the reference-order sum over max(1, workers - 1) subtasks).  A small value marks the answer the others
 *      contradict.
 *  (c) pEntropy[i] (may be NULL) = -sum p_t log2 p_t over the p_t > 0, in bits: fp64, from the divided values, in a fixed order without
 *      atomics.  Against -math.fsum(p log2 p) it is within (nTargets + 16) 2^-52 max(1, H) bits.
 *  (d) Records: pCounts[i] = min(maxCount, candidates) records at pDest + i * maxCount; a candidate is a target that is no gap with
 *      p_t > 0; probability descending, target id ascending among equals -- the order of PqaEngine_ListTopTargetsAmongBatch and of the
 *      fast listing (option "top_exact" 0), not the reference's heap order; _prob carries the posterior's own bits.  maxCount <= 256;
 *      pDest and pCounts may be NULL only when maxCount == 0.
 *  (e) A dead row -- the remaining answers would make PqaEngine_ResumeQuiz fail with I64Underflow, or their total is 0 or not finite:
 *      likelihood = a quiet NaN, entropy = a quiet NaN, count 0.  It is no error of the call.
 *  (f) State: nothing of any quiz changes -- posterior, asked bits, answers, active question, versions, speculative and resident state
 *      all stay; a NextQuestion that follows returns what it would have returned without the call.  Regular mode only.
 *  (g) Batch shape: any number of pairs; a quiz may appear under many positions and a pair may repeat.  A row's outputs depend on its
 *      quiz and position alone, not on the rest of the call or on where its chunks fall.
 *  (h) Refusals, all decided before anything is launched or written, in this order: negative nPairs or maxCount (NegativeCount);
 *      maxCount > 256 (IndexOutOfRange); a needed buffer NULL (NullArgument); maintenance mode or shutdown, as
 *      PqaEngine_PreviewAnswersBatch answers them; an unknown quiz ("entry="); a position outside [0, the quiz's answer count)
 *      (IndexOutOfRange, "entry=", "position=": a quiz without answers refuses every position); on a shard engine an answered question
 *      another shard holds whose rows the row needs -- a remaining one, or the left-out one when pLikelihood is given -- (NotImplemented,
 *      PqaEngine_ResumeQuiz's wording, pointing at PqaEngine_ReviewAnswersBatchFromRows).
 * Two launches and a listing per chunk (review_kernels.hip): the leave-one-out chains of a quiz share its answers' ratios, one division
 * per (answer, target), and their prefixes -- n divisions and about n^2 / 2 multiplications per target where n resumes take n (n - 1) of
 * each; a workgroup per row then normalises as ResumeQuiz does.  Rows go in chunks of at most 256, a quiz's rows together where they fit,
 * a chunk's scratch within 64 MiB; records, counts and two doubles per row cross to the host, nothing of size nTargets.
 * The one-process sharded engine (PQA_DEVICES) answers NotImplemented.  Read-only options "review_calls" / "review_rows": the accepted
 * calls and their pairs; with "time_sweeps", "review_device_ns"; "review_lds_answers": the most answers whose ratios stay in LDS. */
PQACORE_API void *PqaEngine_ReviewAnswersBatch(void *pvEngine, int64_t nPairs, const int64_t *pQuizzes, const int64_t *pPositions,
                                               int64_t maxCount, double *pLikelihood, double *pEntropy,
                                               CiRatedTarget *pDest, int64_t *pCounts);
/* ... on a shard that a process of its own drives: pair i's quiz has its n answers' row pairs in slots pRowFirst[i] .. pRowFirst[i] + n - 1
 * of the package pRows, in answer order; slot format and pitch are PqaHip_PackAnswerRows' (PqaHip_AnswerRowSlotBytes).  Slots of
 * questions this engine holds need not be filled and are not read; pRows may be NULL where no needed row is another engine's.  A
 * package in host memory is staged under option "rows_stage".  Pairs of one quiz name the same slots.  Everything else as above, with
 * pRowFirst NULL (NullArgument) and a negative slot (IndexOutOfRange, "entry=") among the refusals.  The posterior is replicated, so
 * every rank returns the whole engine's bits and nothing is merged (probqa_amd/dist.py: review_answers_batch). */
PQACORE_API void *PqaEngine_ReviewAnswersBatchFromRows(void *pvEngine, int64_t nPairs, const int64_t *pQuizzes, const int64_t *pPositions,
                                                       int64_t maxCount, double *pLikelihood, double *pEntropy,
                                                       CiRatedTarget *pDest, int64_t *pCounts, const void *pRows, const int64_t *pRowFirst);
/* Where a quiz stands NOW, where PqaEngine_PreviewAnswersBatch looks ahead and PqaEngine_ReviewAnswersBatch looks back: a handful of
 * numbers per quiz instead of its nTargets doubles (PqaHip_GetPriors) -- what a stopping rule needs ("one target holds 0.9", "95 % of the
 * mass sits in seven targets", "less than a bit is left") and the H_now of a question's information gain,
 * H_now - sum_k likelihood_k * H_k with PqaEngine_PreviewAnswersBatch's likelihood_k and H_k.  Read-only; the reference has no such call.
 * Per quiz i, over its posterior p as PqaHip_GetPriors would return it at that moment:
 *  (a) Candidates: a target that is no gap and has p_t > 0 -- PqaEngine_ListTopTargets' rule; a NaN is never one.  _nCandidates counts them.
 *  (b) _entropy = -sum p_t log2 p_t over the candidates, in bits: fp64, in a fixed order without atomics -- the order of
 *      PqaEngine_PreviewAnswersBatch's entropies, so the pEntropy[k] it returned for (quiz, q, k), followed by
 *      PqaEngine_SetActiveQuestion(q) + PqaEngine_RecordAnswer(k), is this value bit for bit, on Double and Float engines at every row
 *      length.  Against -math.fsum(p log2 p) it is within (nTargets + 16) 2^-52 max(1, H) bits.
 *  (c) _mass = sum p_t over the candidates, by the same partition and order; within (nTargets + 16) 2^-52 relative of math.fsum.
 *  (d) _topProb / _iTopTarget: the largest candidate probability and its target, the lowest id among equals -- entry 0 of
 *      PqaEngine_ListTopTargetsAmongBatch's order and of the fast listing (option "top_exact" 0); 0.0 and -1 without a candidate.
 *  (e) Levels, 0 <= nLevels <= 16, shared by the whole call: pLevelCounts[i * nLevels + j] = the number of candidates with
 *      p_t >= pLevels[j], pLevelMass[i * nLevels + j] = their sum in the order of (b).  A level <= 0 counts every candidate, +inf none; a
 *      NaN is refused.  Either level buffer may be NULL where the caller does not want it, both only when nLevels == 0.
 *  (f) State: nothing of any quiz changes -- posterior, asked bits, answers, active question, versions, speculative and resident state
 *      all stay; a NextQuestion that follows returns what it would have returned without the call.  Regular mode only; deferred answers
 *      are applied first, as in PqaEngine_ListTopTargetsBatch; a resident sweep is stopped, as PqaEngine_PreviewAnswersBatch stops it.
 *  (g) Batch shape: any number of quizzes, 256 per launch; a quiz may repeat.  A quiz's outputs depend on that quiz and the levels
 *      alone, never on the rest of the call.
 *  (h) Refusals, all decided before anything is launched or written, in this order: negative nQuizzes or nLevels (NegativeCount);
 *      nLevels > 16 (IndexOutOfRange); a needed buffer NULL (NullArgument); a NaN level (IndexOutOfRange, "level="); maintenance mode or
 *      shutdown, as PqaEngine_PreviewAnswersBatch answers them; an unknown quiz ("entry=", "quizId=").
 * One workgroup per quiz streams the posterior once (status_kernels.hip); 40 bytes and the level vectors per quiz cross to the host.
 * Every engine holds every posterior whole: a shard engine (PqaEngineFactory_CreateHipEngineSharded) answers like a whole engine, every
 * rank the same bits -- no package, no collective --, and the one-process sharded engine (PQA_DEVICES) lets its shard 0 answer.  Read-only
 * options "status_calls" / "status_quizzes" (and "rank_calls" / "rank_pairs" for the call below): the accepted calls and their entries;
 * with "time_sweeps", "status_device_ns" for both. */
PQACORE_API void *PqaEngine_QuizStatusBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes,
                                            int64_t nLevels, const double *pLevels,
                                            CiHipQuizStatus *pStatus, int64_t *pLevelCounts, double *pLevelMass);
/* Where named targets stand in their quizzes: pair i = (pQuizzes[i], pTargets[i]).  pProb[i] = the posterior's own bits at the target;
 * pRank[i] = the number of candidates that come before it in the order "probability descending, target id ascending among equals",
 * 0-based: where it is below maxCount, PqaEngine_ListTopTargetsAmongBatch and PqaEngine_ListTopTargetsBatch (option "top_exact" 0) list
 * the target at exactly that index.  A target that is a gap or whose probability is not > 0 gets rank -1; pProb is the stored value all
 * the same.  What a service asks when the user names the target (PqaEngine_RecordQuizTarget): reciprocal rank, hit@10.
 * Any number of pairs; a quiz under many targets; pairs may repeat; a pair's outputs depend on that pair alone.  The pairs of a quiz are
 * served 32 to a pass over its posterior.  State and refusals as above -- negative nPairs (NegativeCount), a buffer NULL (NullArgument),
 * the mode, an unknown quiz ("entry=", "quizId=") -- and then a target outside [0, nTargets) (IndexOutOfRange, "entry=", "targetId=").
 * Shard engines and the one-process sharded engine answer as for PqaEngine_QuizStatusBatch. */
PQACORE_API void *PqaEngine_RankTargetsBatch(void *pvEngine, int64_t nPairs, const int64_t *pQuizzes, const int64_t *pTargets,
                                             double *pProb, int64_t *pRank);
/* Targets that answer like a given one: "more like this" behind PqaEngine_ListTopTargets, and the duplicate hunt in front of
 * PqaEngine_RemoveTargets -- two targets no quiz can ever tell apart are two whose answer distributions agree on every question.
 * With p_qk(t) = A[q][k][t] / D[q][t]:
 *      BC_q(s, t) = sum_k sqrt(p_qk(s)) sqrt(p_qk(t))           the Bhattacharyya coefficient, in (0, 1], 1 iff equal
 *      sim(s, t)  = (sum over q not a gap of BC_q(s, t)) / nValidQuestions
 * nValidQuestions: the questions of the WHOLE knowledge base that are not gaps; 0 makes every sim 0.  The reference has no such call.
 *  (a) Arithmetic: fp64 throughout (a Float engine's elements are converted exactly); sqrt(A * (1 / D)), fma accumulation, a fixed
 *      summation order, no atomics.  Against math.fsum of sqrt(p_qk(s) p_qk(t)) a value is within (Q K + 16) 2^-52 relative.
 *  (b) Fixed: the value of (s, t) is a function of columns s and t of the cube alone -- not of the other sources of the call, the place
 *      of s in it, or where t falls.  A column t that is a bit-for-bit copy of column s has sim(s, t) == sim(s, s) in every bit.
 *  (c) Modes: regular AND maintenance mode (where an operator looks for duplicates); the calls read only the knowledge base and change
 *      neither it nor any quiz.  They take the engine as PqaEngine_TrainBatch does: a training enqueued earlier is ordered in front.
 *  (d) Refusals, all decided before anything is launched or written: negative nSources / maxCount (NegativeCount); a NULL buffer that is
 *      needed (NullArgument); a source id out of [0, nTargets) (IndexOutOfRange, "entry=", "targetId="); more than 256 sources on the
 *      pack / from-sums pair (IndexOutOfRange, "Batch size is out of range.", as PqaHip_PackAnswerPosteriors).
 *   PqaEngine_EvalTargetSimilarity        pOut[i * n + t] = sim(pSources[i], t), t == pSources[i] included; n must be nTargets.  0 where t
 *                                         is a gap; a row of zeros for a source that is a gap.  Any number of sources, ids may repeat.
 *   PqaEngine_ListSimilarTargetsBatch     source i's candidates are the targets t != pSources[i] that are no gaps and have sim > 0;
 *                                         pCounts[i] = min(maxCount, candidates) records at pDest + i * maxCount, sim descending, target
 *                                         id ascending among equal values (PqaEngine_ListTopQuestions' order); _prob carries the bits
 *                                         PqaEngine_EvalTargetSimilarity returns for the pair.  A gap source lists nothing; maxCount 0 is
 *                                         no error.  Up to 256 records a source the rows stay on the device and nSources x maxCount
 *                                         records come back; beyond that the rows are copied and the prefix is taken on the host.
 *   PqaHip_PackTargetSimilaritySums       a shard's part: stream-ordered, no host synchronisation.  nSources <= 256.  Slot i of the package
 *                                         at pDst (16-byte aligned, device-visible, pitch PqaHip_PosteriorSlotBytes) receives, for
 *                                         t < nTargets, the sum over the questions THIS engine holds that are not gaps of
 *                                         BC_q(pSources[i], t) -- 0 at gap targets, all 0 for a gap source -- and zeros behind.  Every
 *                                         slot is written whole by every rank; the ranks' packages are SUMMED.  pFlag / flagValue as
 *                                         PqaHip_PackAnswerRows.
 *   PqaEngine_ListSimilarTargetsFromSums  divides the summed package by nValidQuestions (IEEE division), drops the source and the gaps
 *                                         and lists as PqaEngine_ListSimilarTargetsBatch does.  A package in registered host memory is
 *                                         staged under option "rows_stage".
 * A whole engine's Eval and List ARE pack -> divide and pack -> list in one sequence, 256 sources at a time.  On an engine made by
 * PqaEngineFactory_CreateHipEngineSharded they answer NotImplemented and name the pair; the one-process sharded engine (PQA_DEVICES)
 * answers NotImplemented for all four.  Read-only counters: "similarity_calls", "similarity_sources", and with "time_sweeps"
 * "similarity_device_ns" (a whole engine's sweeps). */
PQACORE_API void *PqaEngine_EvalTargetSimilarity(void *pvEngine, int64_t nSources, const int64_t *pSources, double *pOut, int64_t n);
PQACORE_API void *PqaEngine_ListSimilarTargetsBatch(void *pvEngine, int64_t nSources, const int64_t *pSources, int64_t maxCount,
                                                    CiRatedTarget *pDest, int64_t *pCounts);
PQACORE_API void *PqaHip_PackTargetSimilaritySums(void *pvEngine, int64_t nSources, const int64_t *pSources, void *pDst, void *pFlag,
                                                  uint64_t flagValue);
PQACORE_API void *PqaEngine_ListSimilarTargetsFromSums(void *pvEngine, int64_t nSources, const int64_t *pSources, const void *pSums,
                                                       int64_t maxCount, CiRatedTarget *pDest, int64_t *pCounts);
/* Questions whose answers a given one predicts: the duplicate hunt in front of PqaEngine_RemoveQuestions, and for a client the
 * follow-ups the question just asked already implies -- near-duplicates, negations, rephrasings -- to dim, drop or hand to the Among
 * calls.  Sources and candidates are questions.  With w[t] = vB[t] for a target that is no gap (0 for a gap) and
 * p_qk(t) = A[q][k][t] * (1 / D[q][t]), for a source s and a question q, neither a gap:
 *      J[k][k'] = sum over t of (w[t] p_sk(t)) p_qk'(t)                   a K x K table, every term >= 0
 *      Z = sum J,  r[k] = sum_k' J[k][k'],  c[k'] = sum_k J[k][k']
 *      I(s, q)  = sum over J[k][k'] > 0 of (J[k][k'] / Z) log2(J[k][k'] Z / (r[k] c[k']))      bits; 0 if Z == 0
 * Draw a target from the knowledge base's prior and ask both questions: I(s, q) is the mutual information between the two answers --
 * how much of q's answer the answer to s already tells.  0 for independent questions; unchanged when a question's answers are
 * relabelled, so a negated question counts as redundant.  The table is normalised by its own total: neither sum vB == 1 nor
 * D == sum_k A is assumed.  I(s, s) is computed by the same formula.  The reference has no such call.
 *  (a) Arithmetic: fp64 throughout (a Float engine's elements are converted exactly); u = w * (A * (1 / D)), v = A * (1 / D), fma
 *      accumulation over the targets in a fixed order, no atomics; Z, r, c in index order, the sum in row-major order with the device's
 *      fp64 log2.  Against math.fsum per table entry and the formula in double precision a value is within
 *      (8 + K^2) (T + 16) 2^-52 bits ABSOLUTE (I is a difference of entropies and may be near 0).
 *  (b) Fixed: I(s, q) is a function of block s, block q, vB, the target gaps and nTargets alone -- not of the other sources of the
 *      call, the place of s in the call or in its tile, the tile's width, or where q falls in the grid or in a shard.  A question whose
 *      block is a bit-for-bit copy of the source's has I(s, q) == I(s, s) in every bit; the same call returns the same bits twice; and
 *      shards return the whole engine's bits (the summation over t does not depend on the split of the question axis).
 *  (c) Modes: regular AND maintenance mode; the calls read only the knowledge base and change neither it nor any quiz.  They take the
 *      engine as PqaEngine_TrainBatch does: a training enqueued earlier is ordered in front.
 *  (d) Refusals, all decided before anything is launched or written: negative nSources / maxCount (NegativeCount); a NULL buffer that is
 *      needed (NullArgument); a source id out of [0, nQuestions of the WHOLE knowledge base) (IndexOutOfRange, "entry=",
 *      "questionId="); more than 256 sources on the pack / from-weights calls (IndexOutOfRange, "Batch size is out of range."); a
 *      wrong n (IndexOutOfRange, as PqaEngine_EvalTargetSimilarity).  Source ids are GLOBAL on every call.
 *   PqaEngine_EvalQuestionRedundancy             pOut[i * n + q] = I(pSources[i], q), q == pSources[i] included; n must be nQuestions.  0
 *                                                where q is a gap; a row of zeros for a source that is a gap.  Any number of sources,
 *                                                ids may repeat.
 *   PqaEngine_ListRedundantQuestionsBatch        source i's candidates are the questions q != pSources[i] that are no gaps and have
 *                                                I > 0; pCounts[i] = min(maxCount, candidates) records at pDest + i * maxCount, I
 *                                                descending, question id ascending among equal values; _priority carries the bits
 *                                                PqaEngine_EvalQuestionRedundancy returns for the pair.  maxCount 0 is no error.  Up to
 *                                                256 records a source the rows stay on the device (the listing kernels of
 *                                                PqaEngine_ListTopQuestions) and nSources x maxCount records come back; beyond that
 *                                                the rows are copied and the prefix is taken on the host in the same order.
 *   PqaHip_QuestionWeightSlotBytes               nAnswers * RoundLdT(nTargets) * 8: a function of the dimensions, the same on every rank.
 *   PqaHip_PackQuestionWeights                   a shard's part: stream-ordered, no host synchronisation.  nSources <= 256.  For every
 *                                                source THIS engine holds, slot i of the package at pDst (16-byte aligned,
 *                                                device-visible) receives the K rows u_k[t] = w[t] p_sk(t): nTargets doubles each at
 *                                                the slot's pitch (RoundLdT(nTargets) doubles a row), 0 at gap targets, all 0 for a
 *                                                gap source, zeros behind the row.  Slots of sources other ranks hold are NOT touched:
 *                                                the ranks' zero-filled packages are SUMMED -- one writer per slot, x + 0 == x, so the
 *                                                bits are the owner's.  pFlag / flagValue as PqaHip_PackAnswerRows; an engine that
 *                                                holds none of the sources still publishes the flag.
 *   PqaEngine_EvalQuestionRedundancyFromWeights  the questions this engine holds against the package: n must be the LOCAL question
 *                                                count, column j is question q_first + j.  nSources <= 256.
 *   PqaEngine_ListRedundantQuestionsFromWeights  lists the questions this engine holds against the package, GLOBAL ids in the records;
 *                                                a host merges the ranks' lists (probqa_amd/dist.py: list_redundant_questions_batch).
 *                                                nSources <= 256.  A package in registered host memory is staged under "rows_stage".
 * A whole engine's Eval and List ARE pack -> evaluate and pack -> list in one sequence, 256 sources at a time.  On an engine made by
 * PqaEngineFactory_CreateHipEngineSharded they answer NotImplemented and name the from-weights pair; the one-process sharded engine
 * (PQA_DEVICES) answers NotImplemented for all of them and -1 for the size call.  Read-only counters: "redundancy_calls",
 * "redundancy_sources", and with "time_sweeps" "redundancy_device_ns" (a whole engine's pack, sweeps and listing kernels). */
PQACORE_API void *PqaEngine_EvalQuestionRedundancy(void *pvEngine, int64_t nSources, const int64_t *pSources, double *pOut, int64_t n);
PQACORE_API void *PqaEngine_ListRedundantQuestionsBatch(void *pvEngine, int64_t nSources, const int64_t *pSources, int64_t maxCount,
                                                        CiRatedQuestion *pDest, int64_t *pCounts);
PQACORE_API int64_t PqaHip_QuestionWeightSlotBytes(void *pvEngine);
PQACORE_API void *PqaHip_PackQuestionWeights(void *pvEngine, int64_t nSources, const int64_t *pSources, void *pDst, void *pFlag,
                                             uint64_t flagValue);
PQACORE_API void *PqaEngine_EvalQuestionRedundancyFromWeights(void *pvEngine, int64_t nSources, const int64_t *pSources,
                                                              const void *pWeights, double *pOut, int64_t n);
PQACORE_API void *PqaEngine_ListRedundantQuestionsFromWeights(void *pvEngine, int64_t nSources, const int64_t *pSources,
                                                              const void *pWeights, int64_t maxCount, CiRatedQuestion *pDest,
                                                              int64_t *pCounts);
/* Questions that tell listed targets apart: what an operator asks once PqaEngine_ListSimilarTargetsBatch has reported a confusable pair or
 * cluster -- no question separates them: duplicates for PqaEngine_RemoveTargets; a few do: the questions to train, or to hand to the Among
 * calls when a quiz is down to these candidates.  A GROUP is a list of n targets, 2 <= n <= 64; ids may repeat, a repeat counts twice.
 * pTargets holds the groups one after another, pGroupCounts[g] targets each.  For a question q that is no gap, with
 * p_k(j) = A[q][k][t_j] * (1 / D[q][t_j]) for member j:
 *      f(x) = x log2 x, f(0) = 0;    m_k = (sum over j of p_k(j)) * (1 / n)
 *      sep(G, q) = max(0, (1 / n) sum_j sum_k f(p_k(j)) - sum_k f(m_k))                                     bits
 * the Jensen-Shannon divergence of the members' answer distributions under equal weights, which is the mutual information between the
 * answer and which member it is: 0 when the members answer q alike, log2 n when no two of them share an answer, and for a pair 1 exactly
 * where the Bhattacharyya term of PqaEngine_EvalTargetSimilarity is 0.  The weights are equal on purpose: the value depends on the
 * group's columns of q's block alone -- not on vB, other targets or other questions.  0 where q is a gap; a group with a gap member gets a
 * row of zeros and lists nothing.  The reference has no such call.
 *  (a) Arithmetic: fp64 throughout (a Float engine's elements are converted exactly); per member sum_k f(p_k) with k ascending, the
 *      members added in a fixed tree over their places in the group, sum_k f(m_k) with k ascending, the device's fp64 log2, no atomics.
 *      Against math.fsum and math.log2 over the same p a value is within (16 + 8 n K) 2^-52 bits ABSOLUTE.
 *  (b) Fixed, bit for bit: a group's values depend on n, nAnswers and the listed order of its members only -- not on what else is in the
 *      call, where the group stands in it or how the call is chunked; a shard returns the whole engine's bits for its questions; a
 *      question block that is a bitwise copy of another gets the other's bits for every group.
 *  (c) Modes: regular AND maintenance mode; the calls read only the knowledge base and change neither it nor any quiz.  They take the
 *      engine as PqaEngine_TrainBatch does: a training enqueued earlier is ordered in front.
 *  (d) Refusals, all decided before anything is launched or written, in this order: negative nGroups / maxCount (NegativeCount); a NULL
 *      buffer that is needed (NullArgument); a group count outside [2, 64] (IndexOutOfRange, "entry=", "count="); a target outside
 *      [0, nTargets) (IndexOutOfRange, "entry=", "member=", "targetId="); a wrong n (IndexOutOfRange); a shut down engine
 *      (ObjectShutDown).
 *   PqaEngine_EvalTargetSeparation          pOut[g * n + j] = sep(G_g, q_first + j); n must be the engine's own question count (a whole
 *                                           engine: nQuestions).  Any number of groups: the host chunks at group boundaries.
 *   PqaEngine_ListSeparatingQuestionsBatch  group g's candidates are the engine's questions that are no gaps and have sep > 0;
 *                                           pCounts[g] = min(maxCount, candidates) records at pDest + g * maxCount, sep descending,
 *                                           question id ascending among equal values; GLOBAL ids; _priority carries the bits
 *                                           PqaEngine_EvalTargetSeparation returns.  maxCount 0 is no error.  Up to 256 records a group
 *                                           the rows stay on the device (the listing kernels of PqaEngine_ListTopQuestions); beyond that
 *                                           the rows are copied and the prefix is taken on the host in the same order.
 * Both calls work on a whole engine AND directly on an engine made by PqaEngineFactory_CreateHipEngineSharded, for the questions it
 * holds: a value needs nothing from another rank, so there is no package and no pack call; a host merges the ranks' lists
 * (probqa_amd/dist.py: list_separating_questions_batch).  The one-process sharded engine (PQA_DEVICES) keeps the interface's default and
 * answers NotImplemented, like the Among, similarity and redundancy families.  Read-only counters: "separation_calls",
 * "separation_groups", and with "time_sweeps" "separation_device_ns" (the staging copies, sweeps and listing kernels). */
PQACORE_API void *PqaEngine_EvalTargetSeparation(void *pvEngine, int64_t nGroups, const int64_t *pGroupCounts, const int64_t *pTargets,
                                                 double *pOut, int64_t n);
PQACORE_API void *PqaEngine_ListSeparatingQuestionsBatch(void *pvEngine, int64_t nGroups, const int64_t *pGroupCounts, const int64_t *pTargets,
                                                         int64_t maxCount, CiRatedQuestion *pDest, int64_t *pCounts);
/* What every question would tell a quiz: the information gain, in bits, of every question of the engine for each of many quizzes, from
 * one streaming pass over the cube per tile of quizzes (gain_kernels.hip).  With the quiz's posterior p (PqaHip_GetPriors, taken as 0 at
 * target gaps and where it is not > 0), r_k(t) = A[q][k][t] * (1 / D[q][t]) and f(x) = x log2 x (f(0) = 0), question q's joint table is
 * J[k][t] = p_t r_k(t), its answer totals W_k = sum_t J[k][t], Z = sum_k W_k, and
 *     gain(quiz, q) = max(0, (f(Z) - sum_k f(W_k) - sum_t p_t g_q(t)) / Z),   g_q(t) = f(sum_k r_k(t)) - sum_k f(r_k(t));
 * 0 if Z is not > 0 or not finite.  It is the mutual information between the answer to q and the target for a target drawn from the
 * posterior: the entropy of the answer under the posterior's mixture minus the posterior mean of each target's own answer entropy, 0 for
 * a question every candidate answers alike, at most log2 nAnswers.  The table is normalised by its own total: neither sum p == 1 nor
 * D == sum_k A is assumed (as in PqaEngine_EvalQuestionRedundancy); where both hold, the gain is _entropy of PqaEngine_QuizStatusBatch
 * minus sum_k likelihood_k * entropy_k of PqaEngine_PreviewAnswersBatch, up to rounding.  The reference has no such call.
 *  (a) Arithmetic: fp64 throughout (a Float engine's elements are converted exactly; posteriors are doubles on both engine types);
 *      r_k by the exact reciprocal, sum_k with k ascending, a lane's sums over its targets ascending, the lanes added in a fixed tree,
 *      the waves in wave order, Z and sum_k f(W_k) with k ascending; the device's fp64 log2; no atomics.  Against math.fsum and
 *      math.log2 over the table a value is within (nTargets + 16) (nAnswers + 8) 2^-52 bits ABSOLUTE.
 *  (b) Fixed, bit for bit: a value depends on the quiz's posterior, question q's block, the target gaps and nAnswers only -- not on the
 *      other quizzes of the call, the quiz's place in the call or in its tile, the tile's width, the chunking, or where q falls in the
 *      grid or in a shard.  A question block that is a bitwise copy of another gets the other's bits; a quiz listed twice gets the same
 *      row twice.
 *  (c) State: nothing of any quiz changes -- posterior, asked bits, answers, active question, versions, speculative and resident state;
 *      a PqaEngine_NextQuestion that follows returns what it would have returned without the call.  Regular mode only.  Deferred
 *      answers are applied first and a resident sweep is stopped, as for PqaEngine_QuizStatusBatch.
 *  (d) Refusals, all decided before anything is launched or written, in this order: negative nQuizzes / maxCount (NegativeCount); a
 *      NULL buffer that is needed (NullArgument); a wrong n (IndexOutOfRange); maintenance mode or shutdown, as
 *      PqaEngine_QuizStatusBatch answers them; an unknown quiz ("entry=", "quizId=").
 *   PqaEngine_EvalQuestionGainsBatch        pOut[i * n + j] = gain(pQuizzes[i], q_first + j); n must be the engine's own question count
 *                                           (a whole engine: nQuestions).  0 for a gap question; an asked question is evaluated like
 *                                           any other (what asking it again would gain); a quiz whose Z is 0 or not finite gets a row
 *                                           of zeros.  Any number of quizzes, in chunks of 256; a quiz may repeat.
 *   PqaEngine_ListInformativeQuestionsBatch quiz i's candidates are the engine's questions that are no gaps, not asked by that quiz, and
 *                                           have gain > 0; pCounts[i] = min(maxCount, candidates) records at pDest + i * maxCount, gain
 *                                           descending, question id ascending among equal values; GLOBAL ids; _priority carries the bits
 *                                           PqaEngine_EvalQuestionGainsBatch returns; entry 0 is the most informative question.
 *                                           maxCount 0 is no error.  Up to 256 records a quiz the rows stay on the device (the listing
 *                                           kernels of PqaEngine_ListTopQuestions, each quiz's own asked bitmap); beyond that the rows
 *                                           are copied and the prefix is taken on the host in the same order.
 * Both calls work on a whole engine AND directly on an engine made by PqaEngineFactory_CreateHipEngineSharded, for the questions it
 * holds: the posterior is replicated, so there is no package; a host merges the ranks' lists (probqa_amd/dist.py:
 * list_informative_questions_batch).  The one-process sharded engine (PQA_DEVICES) keeps the interface's default and answers
 * NotImplemented.  Read-only counters: "gain_calls", "gain_quizzes", and with "time_sweeps" "gain_device_ns" (sweeps and listing
 * kernels). */
PQACORE_API void *PqaEngine_EvalQuestionGainsBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, double *pOut, int64_t n);
PQACORE_API void *PqaEngine_ListInformativeQuestionsBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, int64_t maxCount,
                                                          CiRatedQuestion *pDest, int64_t *pCounts);
/* Question pages: what every question would tell a quiz ONCE the answers to a set of questions are known, and a page of questions filled
 * greedily by that number -- for clients that put several questions on one screen, where the best m questions by
 * PqaEngine_ListInformativeQuestionsBatch are typically near-duplicates of each other (page_kernels.hip).  The conditional gain is
 *     CG(q | S) = I(A_q ; T | A_S)   bits;
 * by the chain rule the conditional gains of a page add up to the page's joint information I(A_page ; T).  pGiven holds the quizzes'
 * given sets one after another, GLOBAL question ids in listed order, pGivenCounts[i] the length of quiz i's; both may be NULL: every
 * set is empty.  The reference has no such call.
 *  (a) Definition.  p: the quiz's posterior (PqaHip_GetPriors), taken as 0 at target gaps and where it is not > 0.
 *      r_k^q(t) = A[q][k][t] * (1 / D[q][t]), the gain sweep's own product, 0 at gap targets.  For S = (q_1 .. q_j), BRANCH
 *      b = ((k_1 nAnswers + k_2) nAnswers + ...) + k_j is the row w_b(t) = (((p_t r_k1^q1(t)) r_k2^q2(t)) ...), each product rounded and
 *      stored as a double; its mass m_b is the sum of the STORED values -- a lane's 16-byte pieces ascending, the lanes added in a fixed
 *      tree, the waves in wave order --; M = sum_b m_b with b ascending; and
 *          CG(q | S) = sum_b (m_b / M) gain(w_b, q),   b ascending, one fma chain,
 *      gain(w_b, q) being exactly the value PqaEngine_EvalQuestionGainsBatch's sweep produces for a posterior w_b (it is normalised by
 *      its own table, so the rows are NOT normalised).  A branch whose m_b is not > 0 contributes nothing; M not > 0 or not finite: a
 *      row of zeros.  With S empty there is one branch and m / M == 1.0 exactly: the row is PqaEngine_EvalQuestionGainsBatch's bit for
 *      bit.  Against math.fsum and math.log2 a value is within
 *      ((nTargets + 16) (nAnswers + 8) + (2 (nTargets + 16) + B + 2) log2 nAnswers) 2^-52 bits ABSOLUTE, B = nAnswers^|S|.
 *  (b) Fixed, bit for bit: a value depends on the quiz's posterior, the blocks of S and of q, the listed ORDER of S (another order agrees
 *      to rounding), the target gaps and nAnswers only -- not on the other quizzes of the call, the quiz's place in it, tiles or
 *      chunking.  A duplicate id in S is a chain like any other.
 *  (c) State: nothing of any quiz changes; regular mode only; deferred answers are applied first and a resident sweep is stopped, as for
 *      PqaEngine_EvalQuestionGainsBatch.
 *  (d) Limits, refused before any launch: the largest branch count of a step -- nAnswers^|S_i| for Eval,
 *      nAnswers^(|S_i| + pageSize - 1) for a page -- must be at most 256 (one chunk of the gain sweep), and a quiz's branch rows must fit
 *      64 MiB of scratch: IndexOutOfRange with "entry=" and "branches=".
 *  (e) Refusals, all decided before anything is launched or written, in this order: negative nQuizzes / pageSize / a negative given
 *      count (NegativeCount); a NULL buffer that is needed (NullArgument; pGiven may be NULL only with pGivenCounts NULL or all counts
 *      0); a wrong n (IndexOutOfRange); maintenance mode or shutdown, as PqaEngine_EvalQuestionGainsBatch answers them; an unknown quiz
 *      ("entry=", "quizId="); a given question outside the knowledge base, or a gap ("entry=", "questionId="); the limits of (d).
 *   PqaEngine_EvalConditionalGainsBatch  pOut[i * n + j] = CG(q_first + j | S_i); n must be the engine's own question count.  0 for a gap
 *                                        question; asked questions and the members of S are evaluated like any other.
 *   PqaEngine_ListQuestionPageBatch      the page starts from S_i; each step takes the question with the largest CG > 0 among those that
 *                                        are no gaps, not asked by the quiz and not in the set so far (the lowest id among equals),
 *                                        appends it to the set and repeats, until pageSize questions are taken or no candidate is
 *                                        left.  pCounts[i] records at pDest + i * pageSize in pick order: _iQuestion the GLOBAL id,
 *                                        _priority the bits PqaEngine_EvalConditionalGainsBatch returns for that question given the
 *                                        prefix before it.  Entry 0 of a page with S empty is entry 0 of
 *                                        PqaEngine_ListInformativeQuestionsBatch.  pageSize 0 is no error.  The picks are made on the
 *                                        device and a page's steps are enqueued back to back: the host waits once per chunk of quizzes.
 * These two calls are for whole engines.  The branch rows need the given questions' blocks, which live on one rank: an engine made by
 * PqaEngineFactory_CreateHipEngineSharded and the one-process sharded engine (PQA_DEVICES) answer them NotImplemented; shards that
 * separate processes drive use the block-package forms below.  Read-only counters: "page_calls", "page_quizzes", and with
 * "time_sweeps" "page_device_ns" and, of it, "page_head_ns" (the roots and the given sets' expansions: what runs before the first sweep). */
PQACORE_API void *PqaEngine_EvalConditionalGainsBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts,
                                                      const int64_t *pGiven, double *pOut, int64_t n);
PQACORE_API void *PqaEngine_ListQuestionPageBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts,
                                                  const int64_t *pGiven, int64_t pageSize, CiRatedQuestion *pDest, int64_t *pCounts);
/* Question pages across shards that separate processes drive.  The branch rows are functions of the quiz's posterior, which every shard
 * holds whole, and of the blocks of the set's questions, which their owners hold: handed those blocks as a BLOCK PACKAGE
 * (PqaHip_QuestionBlockSlotBytes a slot, the layout of PqaHip_PackQuestionBlocks), a shard builds the rows bit for bit as the owner would,
 * sweeps ITS questions with the unchanged gain sweep and returns the whole engine's bits for them.
 *   PqaHip_PackGivenBlocks      PqaHip_PackQuestionBlocks in REGULAR mode: GLOBAL ids; slot i receives the block where this engine holds
 *                               question i, other slots are untouched; stream-ordered, no host wait; pFlag / flagValue as
 *                               PqaHip_PackAnswerRows; everything is checked before any launch.  Deferred answers and a resident sweep are
 *                               handled as PqaEngine_EvalQuestionGainsBatch handles them.  A gap question -- every shard knows the whole
 *                               axis' gaps -- is IndexOutOfRange naming "questionId=".  Counted by "pack_calls" / "pack_bytes".
 *   PqaEngine_EvalConditionalGainsBatchFromBlocks
 *                               PqaEngine_EvalConditionalGainsBatch in everything -- (a) to (e), the chunking, n = the engine's OWN
 *                               question count, pOut[i * n + j] = CG(q_first + j | S_i) -- except where a given question's block comes
 *                               from: this engine's own cube where it holds the question, otherwise the slot of pBlocks whose entry in
 *                               pBlockQuestions[0 .. nBlocks) names it (GLOBAL ids, distinct; a slot may serve many quizzes and
 *                               positions).  Slots of questions the engine holds itself need not be filled and are not read.  Further
 *                               refusals, decided before any launch and after the plain call's own: a negative nBlocks (NegativeCount)
 *                               and NULL pBlockQuestions with nBlocks > 0 (NullArgument), with the argument checks; then slotBytes other
 *                               than PqaHip_QuestionBlockSlotBytes (IndexOutOfRange; not looked at when nBlocks is 0 and pBlocks NULL); a
 *                               given question this engine does not hold and the package does not name (IndexOutOfRange, "entry=" and
 *                               "questionId="); pBlocks NULL while such a question exists (NullArgument).  pBlocks: device-visible
 *                               memory, 16-byte aligned, valid until the call returns; a package in registered host memory is staged to
 *                               the device first under option "rows_stage" (the needed slots only).  A whole engine accepts nBlocks 0 and
 *                               pBlocks NULL and returns the plain call's bits.
 *   PqaHip_SelectPageStepFromBlocks
 *                               ONE step of a page for this engine's questions: per quiz {CG, GLOBAL id} of the question with the
 *                               largest CG(q | S_i) > 0 among the engine's own questions that are no gaps, not asked by the quiz and not
 *                               members of S_i, the lowest id among equals; {0, -1} without a candidate.  _priority carries exactly the
 *                               bits the Eval form returns for that question.  It is the first step of PqaEngine_ListQuestionPageBatch's
 *                               chunk: roots, the given levels' expansions, the gain sweep, the combine with the exclusion bitmap, the
 *                               listing of one record; the host waits once per chunk.  Limit: nAnswers^|S_i| <= 256 and the scratch, as
 *                               for Eval.  The same further refusals.  A host merges the ranks' records (the largest CG, the lowest id
 *                               among equals), appends the pick to the sets and calls again: probqa_amd/dist.py list_question_page_batch.
 * The one-process sharded engine answers all three NotImplemented.  "page_calls", "page_quizzes", "page_device_ns" count them too. */
PQACORE_API void *PqaHip_PackGivenBlocks(void *pvEngine, int64_t nQuestions, const int64_t *pQuestions, void *pDst, void *pFlag, uint64_t flagValue);
PQACORE_API void *PqaEngine_EvalConditionalGainsBatchFromBlocks(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts,
                                                                const int64_t *pGiven, int64_t nBlocks, const int64_t *pBlockQuestions,
                                                                const void *pBlocks, int64_t slotBytes, double *pOut, int64_t n);
PQACORE_API void *PqaHip_SelectPageStepFromBlocks(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pGivenCounts,
                                                  const int64_t *pGiven, int64_t nBlocks, const int64_t *pBlockQuestions, const void *pBlocks,
                                                  int64_t slotBytes, CiHipSelection *pOut);
/* This engine's (shard's) winner per quiz among its list, {priority, GLOBAL question id or -1}, without NextQuestion's bookkeeping: a
 * process-per-GPU host merges the shards' records (probqa_amd/dist.py: select_among_batch) and calls PqaEngine_SetActiveQuestion. */
PQACORE_API void *PqaHip_SelectArgmaxAmongBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                const int64_t *pQuestions, CiHipSelection *pOut);
/* The three selecting forms do PqaEngine_NextQuestion's bookkeeping: the active question, and one question asked per quiz that got one.
 * pPicked[i]: the GLOBAL id, or -1.  PqaEngine_NextQuestionAmongBatch obeys option "select": with select = 0 it draws one number per
 * quiz from the engine's generator in batch order, after the whole call has been validated (as PqaEngine_NextQuestionBatch). */
PQACORE_API void *PqaEngine_NextQuestionArgmaxAmongBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                         const int64_t *pQuestions, int64_t *pPicked);
PQACORE_API void *PqaEngine_NextQuestionSampledAmongBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                          const int64_t *pQuestions, const uint64_t *pRnd, int64_t *pPicked);
PQACORE_API void *PqaEngine_NextQuestionAmongBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                   const int64_t *pQuestions, int64_t *pPicked);
/* pOut[i] = the device's Log2Hot(pIn[i]) (host buffers): the function the sweep applies to every posterior element
 * (replaces SRVectMath::Log2Hot, reference SRPlatform/Interface/SRVectMath.h:87-135), exposed so that it can be held to
 * the reference's own SRVectMathTest.Log2Hot criteria (SRPlatformTests/SRVectMathTest.cpp:45-103). */
PQACORE_API void *PqaHip_Log2Hot(void *pvEngine, const double *pIn, double *pOut, const int64_t n);
/* Current target probabilities of a quiz (n == nTargets). */
PQACORE_API void *PqaHip_GetPriors(void *pvEngine, const int64_t iQuiz, double *pOut, const int64_t n);

/* ---- stream-ordered entry points (no host synchronisation inside) */
PQACORE_API void *PqaHip_GetStream(void *pvEngine);                 /* hipStream_t */
PQACORE_API void *PqaHip_SetStream(void *pvEngine, void *hipStream); /* run on the caller's stream, NULL = own */
PQACORE_API void *PqaHip_Synchronize(void *pvEngine);
/* Everything the engine has put on the device has finished, and its resident sweep kernel -- if one is serving the selections
   (option "server") -- STAYS, idle: the bracket of a timed region of synchronous calls (PqaHip_Synchronize sends the kernel away,
   for a caller about to synchronise the whole device). */
PQACORE_API void *PqaHip_Quiesce(void *pvEngine);
/* Enqueue sweep + local argmax; the 16-byte CiHipSelection is written to pOut (device or pinned host pointer). */
PQACORE_API void *PqaHip_EnqueueSelectArgmax(void *pvEngine, const int64_t iQuiz, void *pOut);
/* ---- exchange of the shards' winners through host memory shared by the ranks of a node (probqa_amd/dist.py).
 * The 16-byte message per rank is latency-bound: the sweep's finisher writes {priority, GLOBAL index} to pOut and then
 * flagValue to pFlag -- device-visible addresses of registered host memory -- and every rank's host picks the winner as
 * soon as all flags carry the step's value.  No collective launch, no copy, no stream synchronisation. */
PQACORE_API void *PqaHip_EnqueueSelectArgmaxFlag(void *pvEngine, const int64_t iQuiz, void *pOut, void *pFlag,
                                                 const uint64_t flagValue);
/* ... or through ONE RCCL collective on the engine's stream, for a process-per-GPU host that owns a communicator (pNcclComm: its
 * ncclComm_t; world: its size): the shards' 16-byte winners are all-gathered and every rank returns the same exact pick (max
 * priority, lowest GLOBAL index on ties, -1 if none).  librccl.so is loaded at the first call; libPqaCore.so does not link it.
 * (probqa_amd/dist.py does the same through torch.distributed, where the communicator is PyTorch's.) */
PQACORE_API void *PqaHip_SelectArgmaxRccl(void *pvEngine, const int64_t iQuiz, void *pNcclComm, const int64_t world, double *pPriority,
                                          int64_t *pIndex);
PQACORE_API void *PqaHip_HostRegister(void *pHost, const int64_t nBytes, void **ppDevice);
PQACORE_API void *PqaHip_HostUnregister(void *pHost);
/* Slots of strideBytes each, starting with {double priority; int64 index; uint64 flag}: wait until all `world` flags
 * equal flagValue, then the exact global pick (max priority, lowest index on ties, NaN never wins, -1 if none). */
PQACORE_API void *PqaHip_PickWhenAll(const void *pSlots, const int64_t world, const int64_t strideBytes,
                                     const uint64_t flagValue, const double timeoutSec, double *pPriority, int64_t *pIndex);
/* The two calls above as one step: this shard's selection goes to slot `rank` (pSlotsDev = the device-visible address of
 * pSlots), then the pick over all `world` slots. */
PQACORE_API void *PqaHip_SelectThroughSlots(void *pvEngine, const int64_t iQuiz, const void *pSlots, void *pSlotsDev,
                                            const int64_t rank, const int64_t world, const int64_t strideBytes,
                                            const uint64_t flagValue, const double timeoutSec, double *pPriority,
                                            int64_t *pIndex);
/* Enqueue only the sweep (dominant kernel), for kernel timing. */
PQACORE_API void *PqaHip_EnqueueEval(void *pvEngine, const int64_t iQuiz);
/* Device pointer of the quiz's prior vector (ldT doubles, *pLdT receives ldT) for collectives between shards.  The engine
 * updates it in stream order (PqaEngine_RecordAnswer returns once its kernel is enqueued): read it on the engine's stream
 * (PqaHip_GetStream / PqaHip_SetStream) or after PqaHip_Synchronize. */
PQACORE_API void *PqaHip_GetPriorDevicePtr(void *pvEngine, const int64_t iQuiz, void **ppDev, int64_t *pLdT);
/* RecordAnswer on a shard that does not own the active question: bookkeeping only; the owner's prior is expected to be
 * broadcast into PqaHip_GetPriorDevicePtr's buffer by the caller. */
PQACORE_API void *PqaHip_RecordAnswerRemote(void *pvEngine, const int64_t iQuiz, const int64_t iAnswer);
/* ---- ResumeQuiz on shards that separate processes drive (PqaEngineFactory_CreateHipEngineSharded, one per GPU): the two rows
 * of every answered question reach the ranks that do not hold it as a ROW PACKAGE.  A package for n answered questions is n
 * slots of PqaHip_AnswerRowSlotBytes bytes (2 * ldT elements of the engine's own type, 8 bytes for Double engines and 4 for
 * Float; a multiple of 16): slot i = sA[q_i][k_i][0..ldT) followed by mD[q_i][0..ldT), exactly as they lie in the owner's cube,
 * padding included.  A package is a snapshot: it is valid while no rank trains between packing and resuming. */
PQACORE_API int64_t PqaHip_AnswerRowSlotBytes(void *pvEngine);
/* Stream-ordered on the engine's stream, no host synchronisation: for every i < nAnswered whose question THIS engine holds,
 * its two rows are copied into slot i of pDst -- any device-visible address, 16-byte aligned: device memory, or registered host
 * memory (PqaHip_HostRegister), as for PqaHip_EnqueueSelectArgmaxFlag.  Other slots are not touched, so several shards fill one
 * (zero-initialised) buffer.  Question ids are GLOBAL; an id out of [0, nQuestions of the whole KB) or an answer out of
 * [0, nAnswers) is IndexOutOfRange, and nothing is launched.  pFlag != NULL: flagValue is stored there once every row is visible
 * system-wide (also when this engine holds none of the questions); a reader in another process may poll it.  One launch for
 * all rows, a workgroup per 16 KB of a row; a training enqueued before the call is ordered in front of it by the stream. */
PQACORE_API void *PqaHip_PackAnswerRows(void *pvEngine, const int64_t nAnswered, const CiAnsweredQuestion *pAQs, void *pDst,
                                        void *pFlag, const uint64_t flagValue);
/* PqaEngine_ResumeQuiz / PqaEngine_ResumeQuizBatch in everything -- validation, the asked bits of the LOCAL questions,
 * I64Underflow, all or none for the batch, the ids, no speculative sweep behind the batch -- except where the rows come from:
 * those of answered question i are read from slot i of pRows when this engine does not hold the question, from its own cube when
 * it does (such slots may be left unfilled).  For the batch the slots count through all its answered questions, in entry order.
 * pRows: device-visible memory, valid until the call returns; both calls synchronise.  A package in registered host memory is
 * copied to the device first (option "rows_stage", default 1; 0 = read in place).  Concurrent calls take the engine one after the
 * other.  PqaEngine_ResumeQuiz itself keeps answering NotImplemented for a question another process's shard holds. */
PQACORE_API int64_t PqaEngine_ResumeQuizFromRows(void *pvEngine, void **ppError, const int64_t nAnswered,
                                                 const CiAnsweredQuestion *pAQs, const void *pRows);
PQACORE_API void *PqaEngine_ResumeQuizBatchFromRows(void *pvEngine, const int64_t nQuizzes, const int64_t *pCounts,
                                                    const CiAnsweredQuestion *pAQs, const void *pRows, int64_t *pQuizzes);
/* A PAGE of answers per quiz in one launch: the way back of PqaEngine_ListQuestionPageBatch.  Quiz pQuizzes[i] receives the pCounts[i]
 * answers that start at pAQs[sum(pCounts[0..i))], in that order, with GLOBAL question ids; pLikelihood (may be NULL) runs parallel to
 * pAQs.  Where a client today calls PqaEngine_SetActiveQuestion + PqaEngine_RecordAnswer once per answer -- one launch and one pass of
 * the posterior through memory each -- one workgroup per quiz keeps the posterior on chip and walks the page.
 *  (a) Posterior: bit for bit what SetActiveQuestion(q_j) + RecordAnswer(a_j), j = 0 .. count - 1, leave -- per answer the element
 *      product, the reference-order sum over max(1, workers - 1) subtasks, the division, by the update kernels' own device code -- on
 *      Double and Float engines, at every row length, under the engine's current option "workers"; the NaNs a dead answer (a total of
 *      0) produces included, as the update kernels leave them (at a target gap too: 0 / NaN; the update fused into a speculative sweep,
 *      option "fuse_update", writes 0.0 there instead -- the one element in which RecordAnswer's own two routes differ).
 *  (b) Bookkeeping, as the calls would do it: the asked bits are set -- a question that is repeated within the page or was asked before
 *      is recorded again --, the answers are appended in order (PqaHip_GetQuizAnswers), the active question becomes -1, the last use
 *      is touched.
 *  (c) A quiz with pCounts[i] == 0 is not changed at all: its active question stays.
 *  (d) pLikelihood[j] = the total of step j, the predictive probability of the answer that was given: the bits
 *      PqaEngine_PreviewAnswersBatch returns for the quiz in its state just before that step, at (q_j, a_j).
 *  (e) All or none.  Refusals, all decided before any quiz changes and before anything is launched, in this order: negative nQuizzes or
 *      a negative count (NegativeCount, "entry="); a needed buffer NULL (NullArgument); maintenance mode or shutdown, as
 *      PqaEngine_RecordAnswerBatch answers them; a count above 4096 (IndexOutOfRange, "entry="; a fixed limit: a chunk's pointer table
 *      stays within 16 MiB); an unknown quiz ("entry=", "quizId="); a quiz that appears twice in the call (IndexOutOfRange, "entry=");
 *      a question outside [0, nQuestions of the whole knowledge base) or a gap (IndexOutOfRange, "entry=", "position=", "questionId=":
 *      PqaEngine_PreviewAnswersBatch's code for a gap); an answer outside [0, nAnswers) (IndexOutOfRange, "entry=", "position=").
 *  (f) A shard engine that meets a question another shard holds answers NotImplemented from the plain call, in PqaEngine_ResumeQuiz's
 *      wording; the FromRows form reads such a question's rows from slot j of a row package (PqaHip_PackAnswerRows over the
 *      flattened pages; this engine's own slots may be left unfilled), as PqaEngine_ResumeQuizBatchFromRows does; pRows is valid
 *      until the call returns, so a call that reads the package synchronises before it does.  Every shard knows
 *      the gaps of the whole question axis, so the FromRows form refuses the same calls on every rank (probqa_amd/dist.py:
 *      record_answer_page_batch -- one exchange per page).
 *  (g) Engine state: deferred answers are applied first; a resident sweep is quiesced as PqaEngine_RecordAnswer does it; a speculative
 *      sweep that belongs to one of the quizzes is dropped and no new one is launched (as PqaEngine_ResumeQuizBatch); a NextQuestion that
 *      follows returns what it returns after the consecutive calls.
 *  (h) The kernel lists the last posterior's best targets ahead of PqaEngine_ListTopTargets, as PqaEngine_RecordAnswerBatch's kernel
 *      does (option "top_cache"): the listing that follows returns the records it returns after the consecutive calls.
 *  (i) Any number of quizzes, 256 per launch: per chunk one pinned block of tables, one copy, one launch; the likelihoods are copied
 *      back behind it and the stream is synchronised once per chunk only when pLikelihood is given -- without it nothing waits for the
 *      device, as in PqaEngine_RecordAnswerBatch.  Rows that fit 64 KB of LDS beside the sum's scratch (about 8000 targets) stay on chip
 *      across the page; longer ones are updated in place in memory, still in the one launch.
 *  (j) Read-only options "record_page_calls", "page_answers", "page_launches": the accepted calls, their answers and their launches;
 *      with "time_sweeps", "record_page_device_ns".  ("page_calls" and "page_device_ns" count the question pages.)
 * The one-process sharded engine (PQA_DEVICES) validates the whole call and then serves it position by position through its gathered
 * answers -- the same bits, no kernel of its own, no speed claimed -- and answers NotImplemented when pLikelihood is given; its FromRows
 * form ignores the package. */
PQACORE_API void *PqaEngine_RecordAnswerPageBatch(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                  const CiAnsweredQuestion *pAQs, double *pLikelihood);
PQACORE_API void *PqaEngine_RecordAnswerPageBatchFromRows(void *pvEngine, int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pCounts,
                                                          const CiAnsweredQuestion *pAQs, double *pLikelihood, const void *pRows);

/* ---- The sampled selector (PqaEngine_NextQuestionSampled, the reference's PqaCore/CpuEngine.cpp:362-400) on shards that separate
 * processes drive.  The selector splits the GLOBAL question axis into eval_subtasks subtasks (CalcSplit) and runs one Kahan chain
 * per subtask in question order; a shard's range does not end on subtask bounds, and a Kahan chain cannot be cut and re-joined bit
 * for bit from two totals -- it can be continued by whoever sees the earlier questions' priorities and skip bits.  So every rank
 * contributes, per quiz, a SELECTION PART (probqa_amd/csrc/sampled_part.h), with (quot, rem, nS) the CalcSplit of q_total over
 * eval_subtasks (8 x workers if unset), L = quot + (rem > 0) and W = ceil(L / 64):
 *   header    int64 qFirst, int64 nLocal (the shard's range), int64 nS, uint64 seq (the pack's sequence number on its engine)
 *   total     nS doubles: the Kahan total of subtask s where s lies whole inside the shard, 0 elsewhere
 *   2 pieces  each L doubles, then W 64-bit words: the priorities, in question order, and the gap | asked bits (bit j of the words:
 *             question j of the piece) of the shard's questions of ONE subtask that its bounds cut -- the one cut at the lower bound
 *             first, then the one cut at the upper bound; both bounds inside one subtask make one piece.  Which pieces a part holds
 *             follows from its header.  Doubles behind a piece's questions, and an unused piece, are not written.
 * rounded up to 16 bytes: a function of q_total and eval_subtasks alone, the same on every rank whatever its range.  Nothing of the
 * size of the question axis crosses between ranks.  The sequence, run by probqa_amd/dist.py (next_question_sampled_batch); a whole
 * engine is a world of one:
 *   PqaHip_SampledPartBytes      the size of one part.
 *   PqaHip_PackSampledParts      stream-ordered, no host synchronisation.  nQuizzes <= 256 distinct quizzes, refused as
 *                                PqaEngine_EvalPrioritiesBatch refuses them.  Runs the batched sweep that call would run (whichever
 *                                form option batch_form gives, the pole fix behind it) and ONE launch that writes part i to
 *                                pDst + i * partBytes.  pDst, pFlag, flagValue as PqaHip_PackAnswerRows.  The run lengths of the
 *                                shard's whole subtasks stay in engine scratch, stamped with the header's sequence number.
 *   (all-gather the parts: world x nQuizzes of them, rank-major)
 *   PqaHip_SampledPickFromParts  pParts: the gathered parts, device-visible.  ONE launch: per quiz every whole subtask's total from
 *                                the rank whose range contains it, every cut subtask's by continuing one Kahan chain through the
 *                                ranks' pieces in rank order, then the selector's own finish -- the Kahan grand totals in subtask
 *                                order, selRunLen = total * (double)rnd / 18446744073709551615.0, the upper_bound, the n - 1 clamp,
 *                                the second upper_bound: the operations of the whole engine's selector on the same values, so the
 *                                same bits.  pOut[i] = {grand total, the GLOBAL pick}; -1 in place of the pick where the chosen
 *                                subtask lies whole on ANOTHER rank (that rank reports it; a cut subtask's pick is reported by every
 *                                rank).  pRnd must be the same on every rank.  WrongMode if the part of `rank` does not carry the
 *                                sequence number of this engine's latest pack -- or that pack was for another batch, or a quiz of
 *                                it has recorded an answer since -- or if the headers' ranges do not tile [0, q_total).  No
 *                                bookkeeping, no change of quiz state; world <= 64.  The parts are a snapshot of the cube, as a row
 *                                package is: no rank may train between pack and pick.
 *   (all-gather the picks; per quiz the one value that is not -1)
 *   PqaEngine_TakeSampledPicks   host only.  pPicks[i]: the agreed GLOBAL pick.  A pick that is a gap or was asked falls back to
 *                                the reference's FindNearestQuestion over the WHOLE question axis -- every rank keeps the axis'
 *                                gap list and a quiz's answered questions, other ranks' among them, so every rank arrives at the
 *                                same question; then the quiz's active question is set and one question asked is counted per
 *                                quiz, on every rank.  pQuestions[i] = -1, and no error, for a quiz with no question left.
 * Timed only with the shards side by side on one device (tools/sampled_ranks_bench.py, profiles/README.md), not over a process group. */
PQACORE_API int64_t PqaHip_SampledPartBytes(void *pvEngine);
PQACORE_API void *PqaHip_PackSampledParts(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, void *pDst, void *pFlag,
                                          const uint64_t flagValue);
PQACORE_API void *PqaHip_SampledPickFromParts(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const uint64_t *pRnd,
                                              const void *pParts, const int64_t rank, const int64_t world, CiHipSelection *pOut);
PQACORE_API void *PqaEngine_TakeSampledPicks(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pPicks,
                                             int64_t *pQuestions);

/* ---- RecordAnswer for many quizzes on shards that separate processes drive.  Only the rank that holds a quiz's active question can
 * compute the new posterior (it needs the question's two rows); the others only need to store it.  So the posteriors travel as a
 * POSTERIOR PACKAGE: slot i = quiz i's new posterior as nTargets doubles at a pitch of RoundLdT(nTargets) doubles (RoundLdT: up to a
 * 128-byte line), zeros behind them.  Posteriors are fp64 in Float and Double engines alike, and the pitch is a function of nTargets
 * alone -- the same on every rank, whatever the pitch of its allocation.  The pack changes no quiz: every rank validates the whole
 * batch first, the ranks exchange one status word, and only then does anybody record -- a refusal on any rank leaves every rank
 * untouched.  The sequence, run by probqa_amd/dist.py (record_answer_batch); a whole engine is a world of one:
 *   PqaHip_PosteriorSlotBytes    RoundLdT(nTargets) * 8.
 *   PqaHip_PackAnswerPosteriors  stream-ordered, no host synchronisation, CHANGES NO QUIZ STATE.  nQuizzes <= 256 distinct quizzes,
 *                                regular mode.  Every entry is validated before anything is launched, and an error names its batch
 *                                entry: a known quiz; an active question that is valid and no gap (PqaEngine_RecordAnswer's checks
 *                                and codes); an answer in [0, nAnswers).  Deferred updates are launched first.  For every entry
 *                                whose active question THIS engine holds, the quiz's posterior is copied to engine scratch and the
 *                                update kernels of PqaEngine_RecordAnswerBatch run on the copy in place (rows of more than 16384
 *                                targets: the long-row launches), so the bits are PqaEngine_RecordAnswer's; then ONE launch, a
 *                                workgroup per 16 KB of a slot, writes slot i of pDst.  Slots of other ranks' questions are not
 *                                touched, so several shards fill one zero-filled buffer (or the ranks sum theirs: every slot has
 *                                one writer, the values are finite, x + 0 == x).  pDst, pFlag, flagValue as PqaHip_PackAnswerRows;
 *                                the flag is also published by an engine that holds none of the questions.  The engine remembers
 *                                the pack: the quizzes, the answers, and every quiz's posterior version and active question.
 *   (all-reduce(SUM) the packages, or fill one buffer; one status word: nobody goes on if a rank's pack was refused)
 *   PqaEngine_RecordAnswerBatchFromPosteriors
 *                                synchronises.  WrongMode, and nothing has changed, if the batch is not the one of this engine's
 *                                latest PqaHip_PackAnswerPosteriors, or a quiz of it has changed its posterior or its active
 *                                question since.  Otherwise every entry gets PqaEngine_RecordAnswer's bookkeeping -- the answer
 *                                joins the quiz with the GLOBAL question id, no active question, on the holder the question counts
 *                                as asked -- and ONE launch stores the nTargets doubles of slot i as quiz i's posterior (elements
 *                                behind them stay) and sets the holder's bit in the quiz's device bitmap.  pPosteriors: device-
 *                                visible, valid until the call returns; a package in registered host memory is copied to the
 *                                device first under option "rows_stage".  No speculative sweep behind the batch, no best targets
 *                                listed ahead: PqaEngine_ListTopTargets lists on demand and returns the same records.  Concurrent
 *                                calls take the engine one after the other.
 * A posterior depends on the cube: no rank may train between the pack and the consuming call.  PqaEngine_RecordAnswer on the holder,
 * PqaHip_RecordAnswerRemote elsewhere and the caller's own copy of PqaHip_GetPriorDevicePtr's buffer stay as the single-quiz form.
 * Read-only options "posterior_packs", "posteriors_packed" (entries this engine held), "posteriors_taken".  The one-process sharded
 * engine (PQA_DEVICES) answers NotImplemented (-1 for the size): PqaEngine_RecordAnswerBatch records over its shards. */
PQACORE_API int64_t PqaHip_PosteriorSlotBytes(void *pvEngine);
PQACORE_API void *PqaHip_PackAnswerPosteriors(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes, const int64_t *pAnswers,
                                              void *pDst, void *pFlag, const uint64_t flagValue);
PQACORE_API void *PqaEngine_RecordAnswerBatchFromPosteriors(void *pvEngine, const int64_t nQuizzes, const int64_t *pQuizzes,
                                                            const int64_t *pAnswers, const void *pPosteriors);

/* ---- Maintenance on shards that separate processes drive.  PqaEngine_AddQsTs, PqaEngine_RemoveQuestions and PqaEngine_RemoveTargets
 * are COLLECTIVE AND REPLICATED on such shards: every rank makes the same call with the same arguments (as every rank sees every
 * PqaEngine_Train), in maintenance mode.  Each shard keeps the bookkeeping of the whole question axis -- the gap list in the
 * reference's order, the permanent ids, the question count (option "q_total", read-only, beside "q_first") -- and applies the data
 * changes to the questions it holds: the ids a call returns are GLOBAL and the same on every rank.  A removed question is flagged by
 * its holder; a reused question id is re-initialised by its holder; APPENDED questions go to the shard whose range ends at the
 * question count (its local count and capacity grow, the others only raise q_total), so the ranges are no longer an even split
 * afterwards; added target columns are filled by every shard over its own questions.  PqaEngine_QuestionPermFromComp / CompFromPerm
 * answer over GLOBAL compact ids.  Nothing travels between the ranks, and a failing call changes nothing on the rank it fails on.
 *
 * PqaEngine_Compact moves data between ranks and is refused on a shard (NotImplemented); the collective form is:
 *   PqaHip_CompactPlan          host only, changes nothing: the dimensions after the compaction and the whole-question moves of the
 *                               plan as *pnMoves pairs {dst, src} of GLOBAL ids (released with CiReleaseCompaction) -- the same on
 *                               every rank -- and whether THIS shard would be left without a question.  The ranks vote: if any would,
 *                               nobody compacts (a shard keeps [q_first, min(q_first + its count, new question count)); there is no
 *                               re-split -- rebalancing is a save followed by a load at another split).
 *   PqaHip_QuestionBlockSlotBytes   (nAnswers + 1) * RoundLdT(nTargets) * element size, RoundLdT: up to a 128-byte line.  A function
 *                               of the dimensions and the precision alone: every rank computes the same value, whatever the pitch
 *                               of its allocation.
 *   PqaHip_PackQuestionBlocks   stream-ordered, no host synchronisation, one launch: for every i whose (GLOBAL) question this engine
 *                               holds, slot i of pDst receives the question's nAnswers sA rows and its mD row, nTargets elements each
 *                               at the slot's pitch, zeros behind them.  Other slots are untouched, so the ranks fill one zero-filled
 *                               buffer (or sum theirs).  pDst, pFlag, flagValue as PqaHip_PackAnswerRows; ids out of [0, q_total) are
 *                               IndexOutOfRange and nothing is launched.  Maintenance mode.  The questions are the plan's sources.
 *   PqaEngine_CompactFromBlocks PqaEngine_Compact in everything except where a moved question comes from: this engine's own cube
 *                               where it holds src (such slots may be left unfilled), otherwise slot i of pBlocks for move i.  The
 *                               outputs are the global maps, the same on every rank.  slotBytes must be
 *                               PqaHip_QuestionBlockSlotBytes (IndexOutOfRange otherwise).  emptiedRank: the outcome of the ranks'
 *                               vote, -1 = nobody; any other value refuses the call with InsufficientEngineDimensions naming that
 *                               rank -- the same text on every rank -- as does a shard that would itself be left empty; nothing has
 *                               changed then.  A whole engine accepts pBlocks == NULL and does what PqaEngine_Compact does.
 * probqa_amd/dist.py (compact) runs the sequence over a process group.  Nothing of this has been timed on a GPU. */
PQACORE_API void *PqaHip_CompactPlan(void *pvEngine, int64_t *pnQuestions, int64_t *pnTargets, int64_t *pnMoves, int64_t const **const ppMoves,
                                     uint8_t *pWouldBeEmpty);
PQACORE_API int64_t PqaHip_QuestionBlockSlotBytes(void *pvEngine);
PQACORE_API void *PqaHip_PackQuestionBlocks(void *pvEngine, const int64_t nQuestions, const int64_t *pQuestions, void *pDst, void *pFlag,
                                            const uint64_t flagValue);
PQACORE_API void *PqaEngine_CompactFromBlocks(void *pvEngine, const void *pBlocks, const int64_t slotBytes, const int64_t emptiedRank,
                                              int64_t *pnQuestions, int64_t const **const ppOldQuestions, int64_t *pnTargets,
                                              int64_t const **const ppOldTargets);

/* Host bookkeeping of the engine that needs no device, driven by a small script so that it is testable where there is no GPU.
   what = "id_ledger": pIn is a sequence of operations on one fresh compact<->permanent id map (reference behaviour:
   PqaCore/PermanentIdManager.cpp), each {op, a, b}: 0 permanent id of slot a; 1 slot of permanent id a; 2 raise the issue floor
   to a; 3 vacate slot a; 4 reissue slot a; 5 extend to a slots; 6 rename permanent a to b; 7 repack to a slots, the b = a source
   slots following inline; 8 write to a temporary file, read back into a second map, continue on that one; 9 the number of slots that hold an id.  One result per
   operation into pOut (ids, or 0 / 1 for the boolean ones).
   what = "let_go": pIn = {now, maxCount, maxAgeSec, n, then n x {quiz id, last usage}}; pOut receives the count and then the ids
   ClearOldQuizzes would release, in release order (reference behaviour: PqaCore/BaseEngine.cpp:814-873).
   The maintenance plans and the shards' pick both engines share (lists travel as {n, then n words}, doubles as their bit patterns):
   what = "add_plan": pIn = {Q, T, question gaps, target gaps, the questions' init amounts, the targets'}; pOut = {gaps reused for
   questions, for targets, new Q, new T, question ids, target ids, question amounts, target amounts} (PqaCore/CpuEngine.cpp:468-575).
   what = "compact_plan": pIn = {Q, T, question gaps, target gaps}; pOut = {old question of every new one, old target of every new
   one, the question moves as dst, src pairs in the order they are made} (PqaCore/CpuEngine.cpp:577-658).
   what = "shard_compact": pIn = {the shards' upper bounds, Q, T, question gaps, target gaps}; pOut = {1 if a shard would be left without
   a question, the bounds clipped to the new question count, the question moves as {dst, src, dst's shard, src's shard}}.
   what = "check_removal": pIn = {limit, gaps, ids to remove}; pOut = {position of the first id that is out of range, a gap or
   repeated, or -1; the error code the call returns}.
   what = "better_pick": pIn = {priority, index} per shard; pOut = {priority, index} of the winner (maximum priority, lowest index
   on ties, a NaN counts as -infinity, a negative index is no candidate; {0, -1} if there is none).
   what = "merge_top": pIn = {maxCount, nLists, then per list n and n x {priority bits, index}}; pOut = {n, then n x {priority bits,
   index}}: the best maxCount of the shards' PqaEngine_ListTopQuestions lists under the listings' order (descending priority, ascending
   index among equal priorities; a priority that is not > 0 -- a NaN among them -- or a negative index is no candidate).
   what = "sampled_part": pIn = {Q, nSub, qFirst, n}: a shard [qFirst, qFirst + n) of Q questions under nSub subtasks; pOut = {the
   bytes of a selection part, the first subtask that lies whole in the shard, how many do, piece 0's subtask (-1: none) and its
   length, piece 1's subtask and length} (probqa_amd/csrc/sampled_part.h).
   Returns the number of results written, or -1 for a malformed script / too small an output. */
PQACORE_API int64_t PqaHip_HostLogicProbe(const char *what, const int64_t *pIn, const int64_t nIn, int64_t *pOut, const int64_t nOut);

#ifdef __cplusplus
}
#endif
#endif
