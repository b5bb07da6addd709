"""Question-axis sharding of one knowledge base over the GPUs of a node (one process per GPU).

The reference has no multi-device path (PqaCore/BaseCudaEngine.cpp:15 hard-wires device 0;
PqaCore/PqaEngineBaseFactory.cpp:85-91 `CreateGridEngine` is a stub).  The path shards naturally: the priority of a
question depends only on its own sA/mD rows plus the small replicated prior vector
(PqaCore/CEEvalQsSubtaskConsider.cpp:53-215), so every rank sweeps its contiguous question range
(SRPoolRunner::CalcSplit, SRPlatform/Interface/SRPoolRunner.h:96-110) and ONE tiny collective picks the global winner:
an all-gather of 16-byte (priority, global index) records over RCCL/xGMI followed by a local pick (exact, lowest
index on ties).  The message is 16 B per GPU, so the collective is latency-bound; ring bandwidth is irrelevant.
RecordAnswer runs on the rank that owns the answered question and the new prior vector (8*ldT bytes) is broadcast.

`torch.distributed` is plumbing only: backend "nccl" is RCCL on ROCm, "gloo" is used by the CPU tests, where the
local selection comes from a caller-supplied function instead of the HIP engine.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import torch
import torch.distributed as dist


def shard_bounds(n_questions: int, world_size: int) -> List[int]:
    """End bound of each rank's contiguous question range; the reference's CalcSplit arithmetic."""
    quot, rem = divmod(n_questions, world_size)
    bounds, nxt = [], 0
    for r in range(world_size):
        nxt += quot + (1 if r < rem else 0)
        bounds.append(nxt)
    return bounds


def shard_range(n_questions: int, world_size: int, rank: int) -> Tuple[int, int]:
    b = shard_bounds(n_questions, world_size)
    return (0 if rank == 0 else b[rank - 1]), b[rank]


def pick_global(records) -> Tuple[float, int]:
    """records: [world, 2] float64 rows (priority, index-as-bits), a CPU tensor or numpy array.  Returns (priority,
    global question) of the maximum priority, lowest index on ties, -1 if no shard had an eligible question.  NaN never
    wins.  Plain Python over <= 8 records: this sits on the latency path of every selection."""
    arr = records.numpy() if isinstance(records, torch.Tensor) else records
    pris = arr[:, 0].tolist()
    idxs = arr[:, 1].copy().view("<i8").tolist()
    best_p, best_i = float("nan"), -1
    for p, i in zip(pris, idxs):
        if i < 0:
            continue
        if p != p:
            p = float("-inf")
        if best_i < 0 or p > best_p or (p == best_p and i < best_i):
            best_p, best_i = p, i
    return best_p, best_i


def pick_batch(all_winners) -> List[int]:
    """all_winners: [world, B, 2] float64 (priority, GLOBAL question index as a float, -1 = none), the ranks' per-quiz winners of
    one batched sweep (PqaHip_SelectArgmaxBatch), gathered.  Returns the B global picks: maximum priority, lowest index on ties,
    NaN never wins, -1 where no shard had an eligible question."""
    arr = all_winners.cpu().numpy() if isinstance(all_winners, torch.Tensor) else all_winners
    world, n_quizzes = arr.shape[0], arr.shape[1]
    picks = []
    for b in range(n_quizzes):
        best, best_p = -1, 0.0
        for r in range(world):
            p, qi = float(arr[r, b, 0]), int(arr[r, b, 1])
            if qi < 0:
                continue
            if p != p:
                p = float("-inf")
            if best < 0 or p > best_p or (p == best_p and qi < best):
                best, best_p = qi, p
        picks.append(best)
    return picks


def select_batch(local_winners: torch.Tensor, group: Optional[dist.ProcessGroup] = None) -> List[int]:
    """One batched selection over the shards: local_winners [B, 2] of this rank (device tensor under RCCL, CPU tensor under
    gloo) -> one all-gather of 16 B x B per rank -> the same B picks on every rank."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1:
        return pick_batch(local_winners.unsqueeze(0))
    parts = [torch.empty_like(local_winners) for _ in range(world)]
    dist.all_gather(parts, local_winners.contiguous(), group=group)   # (the list form: RCCL and gloo both have it)
    return pick_batch(torch.stack(parts))


def select_among_batch(engine, quizzes, lists, group: Optional[dist.ProcessGroup] = None, device: Optional[torch.device] = None) -> List[int]:
    """The argmax AMONG LISTS over the shards (PqaHip_SelectArgmaxAmongBatch): every rank calls with the same quizzes and the same
    lists of GLOBAL question ids; each shard evaluates the listed questions it holds and reports its winner per quiz, then the
    gather and pick of select_batch -> the same picks on every rank (-1: no eligible question in the list).  The active questions
    are NOT set: the caller follows with PqaEngine_SetActiveQuestion on every rank.  device: where the collective's tensors live
    (the group's device under RCCL; None: the CPU, as under gloo)."""
    local = torch.from_numpy(engine.select_argmax_among_batch(quizzes, lists))
    if device is not None:
        local = local.to(device)
    return select_batch(local, group)


# ---- the process group as one collective sees it ----------------------------------------------------------------------------
# The only place that knows about backends.  A collective's tensors live on the device exactly when the group's backend is "nccl" (RCCL);
# under gloo a device payload makes the detour through the host.  The ranks stay in step only because every rank issues the same
# sequence of collectives, a rank whose engine refused a step included: the helpers below never skip one.


class _Ranks:
    """Built from (group, device, rank, world) at the top of a public collective.  `world` and `rank` are the caller's, or the
    group's where the public function takes none; `device` is the caller's, or the current one where it gives none."""

    def __init__(self, group, device: Optional[torch.device] = None, rank: Optional[int] = None, world: Optional[int] = None):
        self.group, self._device = group, device
        size = dist.get_world_size(group) if dist.is_initialized() else 1
        self.multi = size > 1
        self.world = size if world is None else world
        self.rank = rank
        self.on_dev = self.multi and dist.get_backend(group) == "nccl"

    @property
    def device(self) -> torch.device:
        if self._device is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    def gather(self, t: torch.Tensor) -> torch.Tensor:
        """ONE all_gather of t: the ranks' tensors stacked rank-major, on t's device."""
        if not self.multi:
            return t.unsqueeze(0)
        wire = (t.to(self.device) if self.on_dev else t.cpu()).contiguous()
        parts = [torch.empty_like(wire) for _ in range(self.world)]
        dist.all_gather(parts, wire, group=self.group)   # (the list form: RCCL and gloo both have it)
        out = torch.stack(parts).to(t.device)
        if out.is_cuda:
            torch.cuda.current_stream(out.device).synchronize()
        return out

    def sum_(self, t: torch.Tensor) -> torch.Tensor:
        """ONE all_reduce(SUM) of t, in place."""
        if self.multi:
            if t.is_cuda and not self.on_dev:               # gloo: through the host
                host = t.cpu()
                dist.all_reduce(host, op=dist.ReduceOp.SUM, group=self.group)
                t.copy_(host)
            else:
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
            if t.is_cuda:
                torch.cuda.current_stream(t.device).synchronize()
        return t

    def min_word(self, value: int) -> int:
        """ONE all_reduce(MIN) of one int64."""
        if not self.multi:
            return value
        word = torch.tensor([value], dtype=torch.int64, device=self.device if self.on_dev else "cpu")
        dist.all_reduce(word, op=dist.ReduceOp.MIN, group=self.group)
        return int(word.item())

    def global_rank(self, r: int) -> int:
        return dist.get_global_rank(self.group, r) if self.group is not None else r

    def fail(self, first: int, error: Optional[str]) -> None:
        """Every rank raises the text of rank `first`, which that rank broadcasts."""
        from . import interop

        text = [error if self.rank == first else None]
        if self.multi:
            dist.broadcast_object_list(text, src=self.global_rank(first), group=self.group, device=self.device if self.on_dev else None)
        raise interop.PqaException("rank %d: %s" % (first, text[0]))

    def settle(self, error: Optional[str], undo: Optional[Callable[[], None]] = None, name_alone: bool = False) -> None:
        """One status word between the ranks: all succeeded, or every rank calls `undo` and raises the same PqaException (the
        first failing rank's).  Without a group of several ranks the text is the engine's own, unless `name_alone`."""
        from . import interop

        if error is not None and not self.multi and not name_alone:
            raise interop.PqaException(error)
        first = self.min_word(self.rank if error is not None else self.world)
        if first >= self.world:
            return
        if undo is not None:
            undo()
        self.fail(first, error)


def _summed_package(ranks: _Ranks, engine, pkg: torch.Tensor, pack: Callable[[int], None]) -> Optional[str]:
    """The owners pack into the zero-filled `pkg`, ONE all_reduce(SUM) combines the ranks' packages in place.  -> this rank's error
    text or None: a rank whose pack is refused still takes part in the collective, so that the ranks stay in step; the status word
    that follows fails the call everywhere."""
    from . import interop

    if pkg.is_cuda:
        torch.cuda.current_stream(pkg.device).synchronize()   # the zeros are there before the engine's stream writes among them
    error = None
    try:
        pack(pkg.data_ptr())
    except interop.PqaException as e:
        error = str(e)
    engine.synchronize()                                      # ... and the rows before the collective's stream (or the host) reads them
    ranks.sum_(pkg)
    return error


# ---- ListTopQuestions over the shards ---------------------------------------------------------------------------------------
# On a shard (PqaEngineFactory_CreateHipEngineSharded) PqaEngine_ListTopQuestions lists the shard's own questions with GLOBAL ids.  The
# best max_count of the whole question axis are among the shards' best max_count each: the ranks all-gather their records -- 16 bytes
# each, max_count per quiz -- and every rank merges them under the listing's own order.


def merge_top_questions(lists, max_count: int) -> List[Tuple[int, float]]:
    """The best max_count (question, priority) of several listings: descending priority, ascending question among equal priorities.
    A priority that is not > 0 (a NaN among them) or a negative question is no candidate.  Plain Python, no torch."""
    cand = [(int(q), float(p)) for lst in lists for q, p in lst if p > 0 and q >= 0]
    cand.sort(key=lambda r: (-r[1], r[0]))
    return cand[:max(int(max_count), 0)]


def _gather_top(local: List[List[Tuple[int, float]]], max_count: int, group, device: Optional[torch.device]) -> List[List[Tuple[int, float]]]:
    ranks = _Ranks(group, device)
    if not ranks.multi or max_count <= 0:
        return [merge_top_questions([lst], max_count) for lst in local]
    # one [quizzes, max_count, 2] tensor of 8-byte words per rank: the question (-1: no record) and the priority's bits
    words = torch.full((len(local), max_count, 2), -1, dtype=torch.int64)
    for i, lst in enumerate(local):
        if lst:
            words[i, :len(lst), 0] = torch.tensor([q for q, _ in lst], dtype=torch.int64)
            words[i, :len(lst), 1] = torch.tensor([p for _, p in lst], dtype=torch.float64).view(torch.int64)
    parts = ranks.gather(words)
    merged = []
    for i in range(len(local)):
        lists = []
        for p in parts:
            qs = p[i, :, 0].tolist()
            ps = p[i, :, 1].contiguous().view(torch.float64).tolist()
            lists.append([(q, pr) for q, pr in zip(qs, ps) if q >= 0])
        merged.append(merge_top_questions(lists, max_count))
    return merged


def list_top_questions(engine, quiz: int, max_count: int, group: Optional[dist.ProcessGroup] = None,
                       device: Optional[torch.device] = None) -> List[Tuple[int, float]]:
    """The quiz's best max_count questions over the shards of all ranks: a collective every rank calls alike; every rank returns the
    same list of (GLOBAL question, priority).  Under an NCCL (RCCL) group the records travel on the device, under gloo through the host."""
    return _gather_top([engine.list_top_questions(quiz, max_count)], max_count, group, device)[0]


def list_top_questions_batch(engine, quizzes, max_count: int, group: Optional[dist.ProcessGroup] = None,
                             device: Optional[torch.device] = None) -> List[List[Tuple[int, float]]]:
    """list_top_questions for up to 256 quizzes behind one batched sweep per rank and ONE all-gather."""
    return _gather_top(engine.list_top_questions_batch(list(quizzes), max_count), max_count, group, device)


class ShardedSelector:
    """Global next-question selection over question shards.

    local_select(out) must ENQUEUE (stream-ordered, no host sync needed) the local sweep + argmax and write the
    16-byte record (float64 priority, int64 GLOBAL index or -1) into `out`, a 2-element float64 tensor on the
    collective's device.  With the HIP engine this is `PqaHip_EnqueueSelectArgmax(engine, quiz, out.data_ptr())`.
    """

    def __init__(self, local_select: Callable[[torch.Tensor], None], device: torch.device,
                 group: Optional[dist.ProcessGroup] = None):
        self.local_select = local_select
        self.device = device
        self.group = group
        self.world = _Ranks(group, device).world
        self.local = torch.zeros(2, dtype=torch.float64, device=device)
        self.gathered = torch.zeros(self.world, 2, dtype=torch.float64, device=device)
        on_gpu = device.type == "cuda"
        # the gathered records land here: pinned, so the D2H copy is a single async DMA followed by one stream wait
        self.host = torch.zeros(self.world, 2, dtype=torch.float64, pin_memory=on_gpu)
        self._host_np = self.host.numpy()

    def enqueue(self) -> torch.Tensor:
        """Sweep + local argmax + all-gather, all stream-ordered; returns the [world,2] device tensor."""
        self.local_select(self.local)
        if self.world == 1:
            self.gathered[0].copy_(self.local)
        else:
            dist.all_gather_into_tensor(self.gathered.view(-1), self.local, group=self.group)
        return self.gathered

    def select(self) -> Tuple[float, int]:
        recs = self.enqueue()
        if recs.device.type == "cuda":
            self.host.copy_(recs, non_blocking=True)
            torch.cuda.current_stream(recs.device).synchronize()
            return pick_global(self._host_np)
        return pick_global(recs)


class _ShmSegment:
    """One /dev/shm file, mapped: `host` is its address, `dev` the address the GPU sees it at (PqaHip_HostRegister) if `register`,
    `bytes` a numpy byte view.  Creating means truncate and zero-fill; the creator is the owner, whose close removes the file."""

    def __init__(self, path: str, size: int, create: bool, register: bool):
        import ctypes
        import mmap
        import os

        import numpy as np

        from . import interop

        self.path, self._owner = path, create
        fd = os.open(path, (os.O_CREAT | os.O_TRUNC | os.O_RDWR) if create else os.O_RDWR, 0o600)
        try:
            if create:
                os.ftruncate(fd, size)
            elif os.fstat(fd).st_size < size:
                raise ValueError("%s is smaller than the %d bytes the exchange needs" % (path, size))
            self._map = mmap.mmap(fd, size)
        finally:
            os.close(fd)
        self.host = ctypes.addressof(ctypes.c_char.from_buffer(self._map))
        self.bytes = np.frombuffer(self._map, dtype=np.uint8)
        self._unregister = interop.host_unregister if register else None
        self.dev = interop.host_register(self.host, size) if register else None

    def close(self, unlink: bool = True) -> None:
        """The user drops its own views of `bytes` first.  Safe to call twice."""
        import os

        if self._map is None:
            return
        if self._unregister is not None:
            self._unregister(self.host)
        self.bytes = None
        try:
            self._map.close()
        except BufferError:
            pass
        self._map = None
        if unlink and self._owner:
            try:
                os.unlink(self.path)
            except OSError:
                pass


def _next_half(exchange) -> int:
    """The next step of a selector or an exchange, and which of its two halves that step uses: they alternate by step parity."""
    exchange.step += 1
    return exchange.step & 1


def _spin_until(read: Callable[[int], int], want, world: int, timeout_s: float, what: str) -> List[int]:
    """Wait until read(r) is one of `want` for every rank r in turn, `timeout_s` for all of them together.  -> what was read."""
    import time

    t0 = time.perf_counter()
    seen = []
    for r in range(world):
        while True:
            v = int(read(r))
            if v in want:
                break
            if time.perf_counter() - t0 > timeout_s:
                raise TimeoutError(what % r)
        seen.append(v)
    return seen


class ShmSelector:
    """Global next-question selection over question shards, the ranks' 16-byte records exchanged through a host
    shared-memory segment instead of a collective.

    Why: the message is 16 bytes per rank, so the exchange is pure latency.  An RCCL all-gather costs a kernel launch, the
    collective's own protocol, a D2H copy and a stream synchronisation per selection (~9 us even with ONE rank, measured;
    more with eight) on top of a ~15 us sweep.  Here the sweep's finisher writes {priority, GLOBAL index} and then a
    step number straight into rank r's 64-byte slot of a /dev/shm segment that every rank has mapped and registered with
    its GPU (PqaHip_HostRegister), and every rank's host spins on the `world` step numbers (PqaHip_PickWhenAll) and
    picks: no launch besides the sweep, no copy, no synchronisation.  Two slot sets alternate by step parity, so a fast
    rank's step s+1 never overwrites what a slow rank still reads for step s (a rank cannot finish s+1 before every
    rank has published s+1, which each does only after it is done with s).
    torch.distributed is not involved on the data path; it stays the control plane (rendezvous, barriers, timing).
    """

    SLOT = 64

    def __init__(self, engine, quiz: int, rank: int, world: int, name: str, create: Optional[bool] = None):
        self.engine, self.quiz, self.rank, self.world = engine, quiz, rank, world
        self.path = "/dev/shm/pqa_select_%s" % name
        # (zero-filled by its creator: step 0 is never used)
        self._seg = _ShmSegment(self.path, 2 * world * self.SLOT, rank == 0 if create is None else create, register=True)
        self._host, self._dev = self._seg.host, self._seg.dev
        self.step = 0

    def select(self) -> Tuple[float, int]:
        self.step += 1
        half = (self.step & 1) * self.world * self.SLOT
        # (one call into the library: enqueue with this rank's slot as the destination, then the pick over all slots)
        return self.engine.select_through_slots(self.quiz, self._host + half, self._dev + half, self.rank, self.world, self.SLOT,
                                                self.step)

    def close(self) -> None:
        self._seg.close()


class ShmBatchExchange:
    """The ranks' per-quiz winners of one BATCHED sweep (PqaHip_SelectArgmaxBatch: [B, 2] = priority, GLOBAL index) exchanged
    through a host shared-memory segment: the records are on the host already when the batched call returns, so the exchange is
    16 B x B of stores per rank and a spin on `world` step numbers -- no collective launch, no H2D / D2H copy.  Two slot sets
    alternate by step parity (as ShmSelector).  x86 keeps stores in order: the records are written before the step number."""

    def __init__(self, n_quizzes: int, rank: int, world: int, name: str, create: Optional[bool] = None):
        self.B, self.rank, self.world = n_quizzes, rank, world
        self.stride = 16 * n_quizzes + 64               # records, then the step number on its own line
        self.path = "/dev/shm/pqa_batch_%s" % name
        self._seg = _ShmSegment(self.path, 2 * world * self.stride, rank == 0 if create is None else create, register=False)
        self._bytes = self._seg.bytes
        self.step = 0

    def _slot(self, half: int, r: int):
        import numpy as np

        off = (half * self.world + r) * self.stride
        recs = self._bytes[off:off + 16 * self.B].view(np.float64).reshape(self.B, 2)
        flag = self._bytes[off + 16 * self.B:off + 16 * self.B + 8].view(np.uint64)
        return recs, flag

    def exchange(self, local_winners, timeout_s: float = 600.0) -> List[int]:
        """local_winners: numpy [B, 2] of this rank -> the B global picks, the same on every rank."""
        import numpy as np

        half = _next_half(self)
        recs, flag = self._slot(half, self.rank)
        recs[:] = local_winners
        flag[0] = self.step
        slots = [self._slot(half, r) for r in range(self.world)]
        _spin_until(lambda r: slots[r][1][0], (self.step,), self.world, timeout_s, "rank %%d never published step %d" % self.step)
        return pick_batch(np.stack([rr for rr, _ in slots]))

    def close(self) -> None:
        self._bytes = None
        self._seg.close()


def broadcast_prior(prior: torch.Tensor, owner_rank: int, group: Optional[dist.ProcessGroup] = None) -> None:
    """After RecordAnswer on the owner of the answered question: replicate the new prior vector."""
    if _Ranks(group, prior.device).multi:
        dist.broadcast(prior, src=owner_rank, group=group)


def owner_of(question: int, n_questions: int, world_size: int) -> int:
    for r, b in enumerate(shard_bounds(n_questions, world_size)):
        if question < b:
            return r
    raise IndexError(question)


def _question_of(answered) -> int:
    q = getattr(answered, "i_question", None)
    return int(answered[0]) if q is None else int(q)


def row_owners(answered, n_questions: int, world: int) -> List[int]:
    """The rank that holds the two rows of each answered question (AnsweredQuestion objects or (question, answer) pairs, GLOBAL
    ids): `owner_of` over `shard_bounds`.  IndexError for an id outside [0, n_questions)."""
    import bisect

    bounds = shard_bounds(n_questions, world)
    owners = []
    for a in answered:
        q = _question_of(a)
        if q < 0 or q >= n_questions:
            raise IndexError(q)
        owners.append(bisect.bisect_right(bounds, q))
    return owners


# ---- ResumeQuiz in the process-per-GPU form ------------------------------------------------------------------------------
# A quiz is resumed from the rows of its answered questions (PqaCore/CECreateQuizOperation.cpp:55-83), and those lie on whichever
# rank holds the question.  The owners copy them into a ROW PACKAGE (PqaHip_PackAnswerRows: slot i = the sA and the mD row of
# answered question i, as they lie in the owner's cube), the ranks combine their packages, and every rank resumes from the
# combined one (PqaEngine_ResumeQuizFromRows).  A package is a snapshot of the cube: it is valid only while no rank trains
# between pack and resume.  The helpers below run both back to back and promise nothing beyond that.


def _package(engine, n_slots: int, device: torch.device) -> torch.Tensor:
    """A zero-filled package of n_slots slots in the engine's element type: [n_slots, 2 * ldT]."""
    slot = engine.answer_row_slot_bytes()
    ld = engine.get_option("ldT")
    elem = slot // (2 * ld)
    if elem not in (4, 8) or 2 * ld * elem != slot:
        raise ValueError("unexpected slot size %d for rows of %d elements" % (slot, ld))
    return torch.zeros(max(n_slots, 1), 2 * ld, dtype=torch.float64 if elem == 8 else torch.float32, device=device)


def resume_quiz(engine, answered, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                device: Optional[torch.device] = None) -> int:
    """ResumeQuiz on the shards of `world` ranks: a collective every rank calls with the same list of AnsweredQuestion (GLOBAL
    question ids).  Returns the quiz id, the same on every rank whose engines have created and released the same quizzes.

    Each rank packs the rows it holds into a zero-filled torch tensor on its device, the packages are combined by ONE
    all_reduce(SUM) in the engine's element type -- exact, and a move of bits: every slot is written by exactly one rank, every
    count and every padding element of the cube is finite (0 behind the sA rows, 1 behind the mD rows), and x + 0 == x -- and
    every rank resumes from the combined package.  Under an NCCL (RCCL) group the tensors stay on the device, under gloo they go
    through the host.  All or none: if any rank fails, the others release their quiz and all raise the first failure.
    The package is a snapshot of the cube: no rank may train between the pack and the resume inside this call."""
    from . import interop

    ranks = _Ranks(group, device, rank, world)
    answered = list(answered)
    quiz = -1
    pkg = _package(engine, len(answered), ranks.device)
    error = _summed_package(ranks, engine, pkg, lambda ptr: engine.pack_answer_rows(answered, ptr))
    if error is None:
        try:
            quiz = engine.resume_quiz_from_rows(answered, pkg.data_ptr())
        except interop.PqaException as e:
            error = str(e)
    ranks.settle(error, lambda: error is None and engine.release_quiz(quiz))
    return quiz


def resume_quiz_batch(engine, lists, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                      device: Optional[torch.device] = None) -> List[int]:
    """resume_quiz for many lists at once (PqaEngine_ResumeQuizBatchFromRows): one package whose slots count through all the
    lists' answered questions, one all_reduce, one batched resume per rank; all or none over the ranks as over the entries."""
    from . import interop

    ranks = _Ranks(group, device, rank, world)
    lists = [list(l) for l in lists]
    flat = [aq for l in lists for aq in l]
    quizzes = []
    pkg = _package(engine, len(flat), ranks.device)
    error = _summed_package(ranks, engine, pkg, lambda ptr: engine.pack_answer_rows(flat, ptr))
    if error is None:
        try:
            quizzes = engine.resume_quiz_batch_from_rows(lists, pkg.data_ptr())
        except interop.PqaException as e:
            error = str(e)
    ranks.settle(error, lambda: [engine.release_quiz(q) for q in quizzes])   # (no quizzes where this rank is one that failed)
    return quizzes


# ---- the sampled selector in the process-per-GPU form ----------------------------------------------------------------------
# The reference's selector (PqaEngine_NextQuestionSampled) splits the GLOBAL question axis into subtasks and runs one Kahan chain per
# subtask; a shard holds a stretch of the axis.  Every rank packs a SELECTION PART per quiz (PqaHip_PackSampledParts: the totals of the
# subtasks that lie whole inside its range, the raw priorities of the at most two its bounds cut), the parts are all-gathered, every
# rank picks from all of them (PqaHip_SampledPickFromParts: a cut subtask's chain is continued through the ranks' pieces in rank
# order, so every rank arrives at the whole engine's bits), the picks are all-gathered -- 8 bytes per quiz and rank; a rank reports -1
# where the chosen subtask lies whole on another rank -- and every rank takes the one pick that is not -1
# (PqaEngine_TakeSampledPicks).  Nothing of the size of the question axis crosses between ranks.  Over a
# process group nothing here has been timed (tools/sampled_ranks_bench.py times the engine calls with the shards on one device).


def broadcast_rnds(rnds, group: Optional[dist.ProcessGroup] = None) -> List[int]:
    """The selector's random numbers (one unsigned 64-bit number per quiz) as rank 0 has them, on every rank."""
    rnds = [int(r) for r in rnds]
    ranks = _Ranks(group)
    if not ranks.multi:
        return rnds
    words = torch.tensor([r - (1 << 64) if r >= (1 << 63) else r for r in rnds], dtype=torch.int64)   # (the bits, as signed words)
    if ranks.on_dev:
        words = words.to(ranks.device)
    dist.broadcast(words, src=ranks.global_rank(0), group=group)
    return [w + (1 << 64) if w < 0 else w for w in words.cpu().tolist()]


def merge_sampled_picks(picks) -> List[int]:
    """picks: [world][n] GLOBAL picks of the ranks, -1 where a rank leaves the pick to the rank that holds the chosen subtask.  Per
    quiz the one value that is not -1; ValueError if two ranks report different ones, or none reports any.  Plain Python."""
    merged = []
    for i in range(len(picks[0])):
        seen = sorted({int(p[i]) for p in picks if int(p[i]) >= 0})
        if len(seen) != 1:
            raise ValueError("batch entry %d: the ranks report %s" % (i, "no pick" if not seen else "different picks %s" % seen))
        merged.append(seen[0])
    return merged


def next_question_sampled_batch(engine, quizzes, rnds, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                                device: Optional[torch.device] = None) -> List[int]:
    """PqaEngine_NextQuestionSampledBatch on the shards of `world` ranks: a collective every rank calls with the same quizzes and
    the same random numbers (broadcast_rnds).  Returns the questions, the same on every rank: what the whole engine would select,
    -1 for a quiz with no question left.  Under an NCCL (RCCL) group the parts and the picks travel on the device, under gloo
    through the host.  A rank whose engine refuses a step still takes part in both all-gathers, so that the ranks stay in step;
    the status word that follows fails the call everywhere, and no quiz's active question has changed then."""
    from . import interop

    ranks = _Ranks(group, device, rank, world)
    quizzes, rnds = list(quizzes), [int(r) for r in rnds]
    n = len(quizzes)
    words = max(engine.sampled_part_bytes(), 16) // 8
    mine = torch.empty(max(n, 1), words, dtype=torch.int64, device=ranks.device)
    error = None
    try:
        engine.pack_sampled_parts(quizzes, mine.data_ptr())
    except interop.PqaException as e:
        error = str(e)
    engine.synchronize()                                   # the parts before the collective's stream (or the host) reads them
    parts = ranks.gather(mine)
    local = torch.full((n + 1,), -1, dtype=torch.int64)       # the picks, then this rank's status: 0 = no step was refused
    if error is None:
        try:
            picked = engine.sampled_pick_from_parts(quizzes, rnds, parts.data_ptr(), rank, world)
            local[:n] = torch.from_numpy(picked[:, 1].astype("int64"))
        except interop.PqaException as e:
            error = str(e)
    local[n] = 0 if error is None else 1
    words = ranks.gather(local).tolist()
    questions = []
    if all(w[n] == 0 for w in words):                         # (else nobody takes anything: the status word below says who failed)
        try:
            questions = engine.take_sampled_picks(quizzes, merge_sampled_picks([w[:n] for w in words]) if n else [])
        except (interop.PqaException, ValueError) as e:       # (disagreeing picks are the same finding on every rank)
            error = str(e)
    ranks.settle(error)
    return questions


def next_question_sampled(engine, quiz: int, rnd: int, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                          device: Optional[torch.device] = None) -> int:
    """PqaEngine_NextQuestionSampled likewise, for one quiz; QuestionsExhausted if it has no question left."""
    from . import interop

    question = next_question_sampled_batch(engine, [quiz], [rnd], rank, world, group, device)[0]
    if question < 0:
        raise interop.PqaException("[Engine has run out of questions] message=[Found no unasked question that is not in a gap.] [nullptr]")   # (QuestionsExhausted, as the engine words it)
    return question


# ---- RecordAnswer in the process-per-GPU form --------------------------------------------------------------------------------
# Only the rank that holds a quiz's active question can compute the new posterior (it needs the question's two rows); the others
# only need to store it.  The holders pack the posteriors into a POSTERIOR PACKAGE (PqaHip_PackAnswerPosteriors: slot i = quiz i's
# new posterior, T doubles at a pitch that depends on T alone, zeros behind them) WITHOUT changing any quiz, the ranks sum their
# packages and exchange one status word, and only then every rank records from the combined package
# (PqaEngine_RecordAnswerBatchFromPosteriors).  The sum moves bits: every slot is written by exactly one rank -- the holder of the
# quiz's active question -- into a zero-filled buffer, a posterior's elements and the zeros behind them are finite, and
# x + 0 == x.  (-0.0 + 0.0 is +0.0, and a posterior holds no -0.0: its elements are products and quotients of non-negative numbers.)
# A posterior depends on the cube: no rank may train between the pack and the recording inside the call.  The single-quiz,
# caller-driven form -- RecordAnswer on the holder, RecordAnswerRemote elsewhere, broadcast_prior -- stays.  Over a process group
# nothing here has been timed (tools/record_ranks_bench.py times the engine calls with the shards on one device).


def record_answer_batch(engine, quizzes, answers, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                        device: Optional[torch.device] = None) -> None:
    """PqaEngine_RecordAnswerBatch on the shards of `world` ranks: a collective every rank calls with the same quizzes -- each
    with an active question, the same on every rank -- and the same answers, at most 256.  All or none over the ranks as over the
    entries: the pack validates the whole batch and changes nothing, a rank whose pack is refused still takes part in the
    all-reduce, and after the status word that follows NOBODY records if any rank's pack was refused -- every rank raises the
    first failing rank's text, and no quiz has changed anywhere.  A second status word covers the recording itself.  Under an
    NCCL (RCCL) group the package stays on the device, under gloo it goes through the host."""
    from . import interop

    ranks = _Ranks(group, device, rank, world)
    quizzes, answers = [int(q) for q in quizzes], [int(a) for a in answers]
    pitch = engine.posterior_slot_bytes() // 8
    pkg = torch.zeros(max(len(quizzes), 1), pitch, dtype=torch.float64, device=ranks.device)
    error = _summed_package(ranks, engine, pkg, lambda ptr: engine.pack_answer_posteriors(quizzes, answers, ptr))
    ranks.settle(error)
    try:
        engine.record_answer_batch_from_posteriors(quizzes, answers, pkg.data_ptr())
    except interop.PqaException as e:
        error = str(e)
    ranks.settle(error)


def record_answer(engine, quiz: int, answer: int, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                  device: Optional[torch.device] = None) -> None:
    """PqaEngine_RecordAnswer likewise: the batch of one."""
    record_answer_batch(engine, [quiz], [answer], rank, world, group, device)


def record_answer_page_batch(engine, quizzes, pages, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                             device: Optional[torch.device] = None, likelihoods: bool = False):
    """PqaEngine_RecordAnswerPageBatch on the shards of `world` ranks: a collective every rank calls with the same quizzes and the
    same pages (lists of AnsweredQuestion, GLOBAL question ids).  The row package of resume_quiz_batch -- pack_answer_rows over the
    flattened pages, ONE all_reduce -- and one recording per rank (PqaEngine_RecordAnswerPageBatchFromRows): one exchange per
    page, where record_answer_batch per position costs a posterior package each.  A status word comes before the recording: if any
    rank's pack or look-up of the quizzes is refused nobody records, and every rank raises the first failing rank's text.  The recording validates the whole
    call before it changes anything, identically on every rank (every rank knows the gaps of the whole question axis); a second
    status word covers it.  Returns None, or with `likelihoods` each quiz's list of its steps' totals, the same on every rank.  The
    package is a snapshot of the cube: no rank may train between the pack and the recording inside this call."""
    from . import interop

    ranks = _Ranks(group, device, rank, world)
    quizzes, pages = [int(q) for q in quizzes], [list(p) for p in pages]
    flat = [aq for p in pages for aq in p]
    pkg = _package(engine, len(flat), ranks.device)

    def validate_and_pack(ptr):
        for i, q in enumerate(quizzes):                       # what may differ between the ranks: the mode, the quiz registry
            try:
                engine.get_active_question_id(q)
            except interop.PqaException as e:
                raise interop.PqaException("entry=%d quizId=%d: %s" % (i, q, e))
        engine.pack_answer_rows(flat, ptr)

    error = _summed_package(ranks, engine, pkg, validate_and_pack)
    ranks.settle(error)
    result = None
    try:
        result = engine.record_answer_page_batch_from_rows(quizzes, pages, pkg.data_ptr(), likelihoods)
    except interop.PqaException as e:
        error = str(e)
    ranks.settle(error)
    return result


def record_answer_page(engine, quiz: int, page, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                       device: Optional[torch.device] = None, likelihoods: bool = False):
    """record_answer_page_batch for one quiz: None, or the list of its steps' likelihoods."""
    result = record_answer_page_batch(engine, [quiz], [page], rank, world, group, device, likelihoods)
    return result[0] if likelihoods else None


def _list_from_summed_packages(engine, ranks: _Ranks, sources, pitch: int, pack, list_from, finish=None) -> list:
    """The source listings' exchange, 256 sources at a time: a zero-filled package of `pitch` doubles a source, pack(chunk, address)
    and the all-reduce (_summed_package), the status word, list_from(chunk, address), the status word; finish (optional): what turns a
    chunk's local listings into the call's (a collective of its own)."""
    from . import interop

    sources = [int(s) for s in sources]
    out = []
    for first in range(0, len(sources), 256):
        chunk = sources[first:first + 256]
        pkg = torch.zeros(len(chunk), pitch, dtype=torch.float64, device=ranks.device)
        error = _summed_package(ranks, engine, pkg, lambda ptr: pack(chunk, ptr))
        ranks.settle(error)
        listed = None
        try:
            listed = list_from(chunk, pkg.data_ptr())
        except interop.PqaException as e:
            error = str(e)
        ranks.settle(error)
        out.extend(finish(listed) if finish else listed)
    return out


# ---- targets that answer like a given one, over the shards ------------------------------------------------------------------------
# The similarity of a source and a target is a sum over the questions: every rank packs the sums over ITS questions into a
# zero-filled package (PqaHip_PackTargetSimilaritySums; every slot is written whole by every rank), ONE all_reduce(SUM) adds them,
# and every rank divides, drops the source and the gaps and lists from the same summed package -- the same records everywhere.
# The calls read only the knowledge base: no rank may train or maintain between the pack and the listing inside the call.


def list_similar_targets_batch(engine, sources, max_count: int, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                               device: Optional[torch.device] = None):
    """PqaEngine_ListSimilarTargetsBatch on the shards of `world` ranks: a collective every rank calls with the same sources and
    max_count; any number of sources, 256 per exchange.  All or none as record_answer_batch is: a rank whose pack is refused still
    takes part in the all-reduce, and after the status word every rank raises the first failing rank's text.  Under an NCCL
    (RCCL) group the package stays on the device, under gloo it goes through the host."""
    return _list_from_summed_packages(engine, _Ranks(group, device, rank, world), sources, engine.posterior_slot_bytes() // 8, engine.pack_target_similarity_sums,
                                      lambda chunk, ptr: engine.list_similar_targets_from_sums(chunk, ptr, max_count))


# ---- questions whose answers a given one predicts, over the shards -----------------------------------------------------------------
# The table of a (source, question) pair contracts over the targets, which every rank holds whole: what a rank lacks is the SOURCE's
# block.  The owner of a source packs its weighted answer rows into a zero-filled package (PqaHip_PackQuestionWeights: one writer per
# slot), ONE all_reduce(SUM) hands every rank every source's rows -- x + 0 == x, the owner's bits --, every rank lists its own
# questions against them, and the ranks' lists are all-gathered and merged as list_top_questions merges.


def list_redundant_questions_batch(engine, sources, max_count: int, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                                   device: Optional[torch.device] = None) -> List[List[Tuple[int, float]]]:
    """PqaEngine_ListRedundantQuestionsBatch on the shards of `world` ranks: a collective every rank calls with the same sources
    (GLOBAL ids) and max_count; any number of sources, 256 per exchange.  Every rank returns the same (question, bits) records.  All
    or none as list_similar_targets_batch is: a rank whose pack is refused still takes part in the all-reduce, and after the status
    word every rank raises the first failing rank's text."""
    return _list_from_summed_packages(engine, _Ranks(group, device, rank, world), sources, engine.question_weight_slot_bytes() // 8, engine.pack_question_weights,
                                      lambda chunk, ptr: engine.list_redundant_questions_from_weights(chunk, ptr, max_count),
                                      lambda listed: _gather_top(listed, max_count, group, device))


# ---- questions that tell listed targets apart, over the shards ---------------------------------------------------------------------
# The separation of a group at a question needs the group's columns of that question's block and nothing else, and every rank holds its
# questions' blocks whole: there is no package and nothing to sum.  Every rank lists its own questions, one status word keeps the ranks
# in step, and the lists are all-gathered and merged as list_top_questions merges.


def list_separating_questions_batch(engine, groups, max_count: int, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                                    device: Optional[torch.device] = None) -> List[List[Tuple[int, float]]]:
    """PqaEngine_ListSeparatingQuestionsBatch on the shards of `world` ranks: a collective every rank calls with the same groups of
    targets and max_count; any number of groups.  Every rank returns the same (GLOBAL question, bits) records.  All or none: a rank
    whose call is refused still takes part in the status word, after which every rank raises the first failing rank's text."""
    from . import interop

    ranks = _Ranks(group, device, rank, world)
    groups = [[int(t) for t in g] for g in groups]
    error, listed = None, None
    try:
        listed = engine.list_separating_questions_batch(groups, max_count)
    except interop.PqaException as e:
        error = str(e)
    ranks.settle(error)
    return _gather_top(listed, max_count, group, device)


# ---- what every question would tell a quiz, over the shards -------------------------------------------------------------------------
# The gain of a question for a quiz needs the quiz's posterior, which every rank holds whole, and that question's block, which its
# owner holds whole: there is no package and nothing to sum.  Every rank lists its own questions under the quiz's asked bits, one status
# word keeps the ranks in step, and the lists are all-gathered and merged as list_top_questions merges.


def list_informative_questions_batch(engine, quizzes, max_count: int, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                                     device: Optional[torch.device] = None) -> List[List[Tuple[int, float]]]:
    """PqaEngine_ListInformativeQuestionsBatch on the shards of `world` ranks: a collective every rank calls with the same quizzes and
    max_count; any number of quizzes.  Every rank returns the same (GLOBAL question, bits) records; entry 0 is the most informative
    question of the whole knowledge base.  All or none: a rank whose call is refused still takes part in the status word, after which
    every rank raises the first failing rank's text."""
    from . import interop

    ranks = _Ranks(group, device, rank, world)
    error, listed = None, None
    try:
        listed = engine.list_informative_questions_batch([int(z) for z in quizzes], max_count)
    except interop.PqaException as e:
        error = str(e)
    ranks.settle(error)
    return _gather_top(listed, max_count, group, device)


# ---- question pages over the shards ----------------------------------------------------------------------------------------------
# CG(q | S) needs the branch rows of S -- functions of the quiz's posterior, which every rank holds whole, and of the blocks of S's
# questions, which their owners hold.  The owners pack those blocks into a zero-filled BLOCK PACKAGE (PqaHip_PackGivenBlocks: one writer
# per slot), ONE all_reduce(SUM) hands every rank every block -- x + 0 == x, the owner's bits --, and every rank builds the same rows and
# sweeps its own questions (the FromBlocks calls).  A page is a loop of such steps over a package that grows by the picks: only the
# picked question's block crosses between two steps.  Each step rebuilds the branch rows from the root: the call is stateless and every
# value is by construction the Eval form's bits.  Over a process group with a device per rank nothing here has been timed
# (tools/question_page_ranks_bench.py times the engine calls with the shards on one device).


def _distinct(sets, known=()) -> List[int]:
    """The questions of the sets that are not in `known`, each once, in order of first appearance."""
    seen, out = set(known), []
    for s in sets:
        for q in s:
            if q not in seen:
                seen.add(q)
                out.append(q)
    return out


def _block_package(engine, n_slots: int, device: torch.device) -> torch.Tensor:
    """A zero-filled block package of n_slots slots in the engine's element type."""
    elem = 4 if engine.get_option("precision") == 1 else 8
    return torch.zeros(max(n_slots, 1), engine.question_block_slot_bytes() // elem, dtype=torch.float32 if elem == 4 else torch.float64, device=device)


def _given_sets(quizzes, given) -> Tuple[List[int], List[List[int]]]:
    quizzes = [int(z) for z in quizzes]
    sets = [[] for _ in quizzes] if given is None else [[int(q) for q in s] for s in given]
    if len(sets) != len(quizzes):
        raise ValueError("one given set per quiz")
    return quizzes, sets


def eval_conditional_gains_batch(engine, quizzes, given, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                                 device: Optional[torch.device] = None):
    """PqaEngine_EvalConditionalGainsBatch on the shards of `world` ranks: a collective every rank calls with the same quizzes and
    given sets (GLOBAL ids).  Returns THIS rank's columns, [n, local questions]: the ranks' arrays side by side are the whole
    engine's bits.  The package's slots are the distinct given questions in order of first appearance.  All or none: a rank whose
    pack or evaluation is refused still takes part in the all-reduce and the status words, after which every rank raises the first
    failing rank's text.  The package is a snapshot of the cube: no rank may train between the pack and the evaluation."""
    from . import interop

    ranks = _Ranks(group, device, rank, world)
    quizzes, sets = _given_sets(quizzes, given)
    slots = _distinct(sets)
    pkg = _block_package(engine, len(slots), ranks.device)
    error = _summed_package(ranks, engine, pkg, lambda ptr: engine.pack_given_blocks(slots, ptr))
    ranks.settle(error)
    out = None
    try:
        out = engine.eval_conditional_gains_batch_from_blocks(quizzes, sets, slots, pkg.data_ptr())
    except interop.PqaException as e:
        error = str(e)
    ranks.settle(error)
    return out


def merge_page_step(records_per_rank) -> List[Tuple[int, float]]:
    """records_per_rank: [world][n] records (bits, GLOBAL question or -1), the ranks' PqaHip_SelectPageStepFromBlocks results of one
    step.  Per quiz the pick (question, bits): the largest bits > 0, the lowest question among equals; (-1, 0.0) without a candidate
    (a NaN is none).  Plain Python, no collective."""
    arr = records_per_rank.cpu().numpy() if isinstance(records_per_rank, torch.Tensor) else records_per_rank
    n = len(arr[0]) if len(arr) else 0
    picks = []
    for i in range(n):
        best_q, best = -1, 0.0
        for part in arr:
            bits, q = float(part[i][0]), int(part[i][1])
            if q < 0 or not bits > 0:
                continue
            if best_q < 0 or bits > best or (bits == best and q < best_q):
                best_q, best = q, bits
        picks.append((best_q, best))
    return picks


def list_question_page_batch(engine, quizzes, page_size: int, given, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                             device: Optional[torch.device] = None) -> List[List[Tuple[int, float]]]:
    """PqaEngine_ListQuestionPageBatch on the shards of `world` ranks: a collective every rank calls with the same quizzes, page size
    and given sets.  Every rank returns the same (GLOBAL question, bits) records in pick order, the whole engine's.  Per step: the
    owners pack the questions the package does not hold yet (the first step the given ones, later the picks: fresh quizzes all pick
    the same first question, which crosses once), ONE all_reduce over those slots and a status word, one
    PqaHip_SelectPageStepFromBlocks per rank and a status word, ONE all-gather of 16 bytes a quiz, and merge_page_step.  A quiz without a pick is finished and leaves the later
    steps.  nAnswers^(|given| + page_size - 1) <= 256 is checked before the first step: every rank raises the same text.  All or
    none per step as eval_conditional_gains_batch."""
    from . import interop

    ranks = _Ranks(group, device, rank, world)
    quizzes, sets = _given_sets(quizzes, given)
    page_size = int(page_size)
    if page_size < 0:
        raise interop.PqaException("[The count is negative] count=%d |pageSize| must be non-negative." % page_size)
    k = engine.copy_dims().n_answers
    for i, s in enumerate(sets):
        if k ** (len(s) + max(page_size, 1) - 1) > 256:
            raise interop.PqaException("[Index is out of range] entry=%d branches=>256 A quiz's answer combinations must be at most 256." % i)
    pages = [[] for _ in quizzes]
    active = list(range(len(quizzes)))
    slots: List[int] = []
    # every slot the call can need: the distinct given questions, and a pick per quiz and step but the last
    pkg = _block_package(engine, len(_distinct(sets)) + len(quizzes) * max(page_size - 1, 0), ranks.device)
    for _ in range(page_size):
        if not active:
            break
        new = _distinct([sets[i] for i in active], slots)
        if new:   # (the same on every rank: the sets are)
            ranks.settle(_summed_package(ranks, engine, pkg[len(slots):len(slots) + len(new)], lambda ptr: engine.pack_given_blocks(new, ptr)))
            slots.extend(new)
        error, records = None, None
        try:
            records = engine.select_page_step_from_blocks([quizzes[i] for i in active], [sets[i] for i in active], slots, pkg.data_ptr())
        except interop.PqaException as e:
            error = str(e)
        ranks.settle(error)
        merged = merge_page_step(ranks.gather(torch.as_tensor(records, dtype=torch.float64)))
        still = []
        for i, (q, bits) in zip(active, merged):
            if q >= 0:
                pages[i].append((q, bits))
                sets[i].append(q)
                still.append(i)
        active = still
    return pages


def list_question_page(engine, quiz: int, page_size: int, given, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                       device: Optional[torch.device] = None) -> List[Tuple[int, float]]:
    """list_question_page_batch for one quiz."""
    return list_question_page_batch(engine, [quiz], page_size, [list(given or ())], rank, world, group, device)[0]


# ---- .kb files in the process-per-GPU form ---------------------------------------------------------------------------------
# Every rank loads its own window of one file (PqaEngineFactory_LoadHipEngineAs: a seek to its two blocks of rows) and writes it back in
# place (PqaHip_SaveKBShard); the rank that holds question 0 writes everything that is not a row.  The ranks write disjoint byte ranges
# of one file, so the only ordering a save needs is: the file is emptied before the first part lands, and nobody reads it before the
# last one has.  Deployments without a process group order the calls themselves: empty (or remove) the file, let every rank call
# engine.save_kb_shard(path) in any order, and take the file once all have returned.


def load_shard(factory, path: str, rank: int, world: int, precision=None, device: int = -1):
    """This rank's shard of the .kb file `path`: questions shard_range(Q, world, rank) of the file's Q, in `precision` (None: the
    file's).  No collective: every rank reads the 40-byte header and its own rows."""
    from . import interop

    _, dims, _ = interop.read_kb_header(path)
    first, limit = shard_range(dims.n_questions, world, rank)
    return factory.load_hip_engine(path, precision, q_first=first, n_local=limit - first, q_total=dims.n_questions, device=device)


def save_kb(engine, path: str, rank: int, world: int, group: Optional[dist.ProcessGroup] = None, precision=None) -> None:
    """SaveKB of the shards of `world` ranks into ONE file: a collective every rank calls with the same path and precision.  The
    rank that holds question 0 creates or empties the file; a barrier; every rank writes its part; one status word.  All or none:
    if any rank failed, the rank that holds question 0 removes the file and every rank raises the first failure."""
    import os

    from . import interop

    ranks = _Ranks(group, None, rank, world)
    creator = engine.get_option("q_first") == 0
    error = None
    if creator:
        try:
            open(path, "wb").close()
        except OSError as e:
            error = "cannot create %s: %s" % (path, e)
    if ranks.multi:
        dist.barrier(group=group)
    if error is None:
        try:
            engine.save_kb_shard(path, precision)
        except interop.PqaException as e:
            error = str(e)

    def remove():
        if creator:
            try:
                os.remove(path)
            except OSError:
                pass

    ranks.settle(error, remove, name_alone=True)


# ---- changing the KB in the process-per-GPU form -----------------------------------------------------------------------------------
# Maintenance on shards that separate processes drive is COLLECTIVE AND REPLICATED (include/PqaHipExt.h): every rank makes the same
# call with the same arguments, each shard keeps the bookkeeping of the whole question axis and changes the rows it holds.  Appended
# questions go to the shard whose range ends at the question count, and a compaction clips the ranges to the new count -- so once
# maintenance has run, the ranges are no longer shard_bounds' even split: a host loop asks gather_bounds once after every maintenance
# call that changes the question count and uses owner_in, not shard_bounds / owner_of / row_owners.  (Rebalancing is save_kb followed by
# load_shard.)  Only compact moves data between ranks.  Nothing here has been timed on a GPU.


def gather_bounds(engine, group: Optional[dist.ProcessGroup] = None) -> List[int]:
    """End bound of each rank's question range as the engines hold them now: an all_gather of (q_first, local question count)."""
    mine = [engine.get_option("q_first"), engine.get_option("local_questions")]
    return [int(p[0]) + int(p[1]) for p in _Ranks(group).gather(torch.tensor(mine, dtype=torch.int64))]


def owner_in(bounds: List[int], question: int) -> int:
    """The rank whose range holds the question, under bounds as gather_bounds returns them.  IndexError outside [0, bounds[-1])."""
    import bisect

    if question < 0 or question >= bounds[-1]:
        raise IndexError(question)
    return bisect.bisect_right(bounds, question)


# ---- what each answer would do to a quiz, over the shards ---------------------------------------------------------------------------
# Every rank holds every posterior whole, and a would-be posterior needs nothing but the previewed question's rows: the rank that holds
# the question answers for the pair, the others leave zeros.  There is no package and nothing to sum: one status word, one all-gather
# of the ranks' results, and every rank takes each pair from its owner.


def preview_answers_batch(engine, pairs, max_count: int, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                          device: Optional[torch.device] = None) -> list:
    """PqaEngine_PreviewAnswersBatch on the shards of `world` ranks: a collective every rank calls with the same (quiz, GLOBAL question)
    pairs and max_count.  Every rank returns the same lists of interop.AnswerPreview, K per pair.  All or none: a rank whose call is
    refused still takes part in the status word, after which every rank raises the first failing rank's text."""
    from . import interop

    ranks = _Ranks(group, device, rank, world)
    pairs = [(int(a), int(b)) for a, b in pairs]
    error, mine = None, None
    try:
        mine = engine.preview_answers_batch(pairs, max_count)
    except interop.PqaException as e:
        error = str(e)
    ranks.settle(error)
    if not ranks.multi:
        return mine
    bounds = gather_bounds(engine, group)
    # one [rows, 3 + 2 max_count] tensor of 8-byte words per rank: likelihood and entropy bits, the count, then (target, probability bits)
    flat = [p for previews in mine for p in previews]
    words = torch.zeros((max(len(flat), 1), 3 + 2 * max_count), dtype=torch.int64)
    if flat:
        words[:len(flat), 0] = torch.tensor([p.likelihood for p in flat], dtype=torch.float64).view(torch.int64)
        words[:len(flat), 1] = torch.tensor([p.entropy for p in flat], dtype=torch.float64).view(torch.int64)
    for r, p in enumerate(flat):
        words[r, 2] = len(p.targets)
        if p.targets:
            words[r, 3:3 + 2 * len(p.targets):2] = torch.tensor([t.i_target for t in p.targets], dtype=torch.int64)
            words[r, 4:4 + 2 * len(p.targets):2] = torch.tensor([t.prob for t in p.targets], dtype=torch.float64).view(torch.int64)
    parts = ranks.gather(words)
    k = len(mine[0]) if mine else 0

    def previews_of(part, i):
        out = []
        for r in range(i * k, (i + 1) * k):
            row = part[r]
            n = int(row[2])
            vals = row[:2].contiguous().view(torch.float64).tolist()
            ids = row[3:3 + 2 * n:2].tolist()
            probs = row[4:4 + 2 * n:2].contiguous().view(torch.float64).tolist()
            out.append(interop.AnswerPreview(vals[0], vals[1], [interop.RatedTarget(t, pr) for t, pr in zip(ids, probs)]))
        return out

    return [previews_of(parts[owner_in(bounds, q)], i) for i, (_, q) in enumerate(pairs)]


# ---- a quiz with each of its answers left out, over the shards ---------------------------------------------------------------------
# The review resumes from the rows of the quiz's answered questions, and those lie on whichever rank holds the question: the exchange is
# resume_quiz_batch's -- one package whose slots count through the distinct quizzes' answers, packed by the owners and summed -- and
# every rank reviews from the combined package.  The posterior is replicated: every rank computes the whole engine's bits, nothing is merged.


def review_answers_batch(engine, pairs, max_count: int, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                         device: Optional[torch.device] = None) -> list:
    """PqaEngine_ReviewAnswersBatchFromRows on the shards of `world` ranks: a collective every rank calls with the same (quiz, position)
    pairs and max_count.  Every rank returns the same list of interop.AnswerPreview, one per pair.  All or none: a rank whose call is
    refused still takes part in the exchange and the status words (one behind the reading of the answers, one behind the review),
    after which every rank raises the first failing rank's text.  The package is a snapshot of the cube: no rank may train between the pack and the review inside this call."""
    from . import interop

    ranks = _Ranks(group, device, rank, world)
    pairs = [(int(a), int(b)) for a, b in pairs]
    error, out = None, []
    first_of, flat = {}, []
    try:
        for quiz, _ in pairs:   # (the answers are the same on every rank: every engine records every answer)
            if quiz not in first_of:
                first_of[quiz] = len(flat)
                flat.extend(engine.get_quiz_answers(quiz))
    except interop.PqaException as e:
        error = str(e)
    ranks.settle(error)   # (before the exchange: the ranks' packages must be of one size)
    pkg = _package(engine, len(flat), ranks.device)
    error = _summed_package(ranks, engine, pkg, lambda ptr: engine.pack_answer_rows(flat, ptr))
    if error is None:
        try:
            out = engine.review_answers_batch_from_rows(pairs, max_count, pkg.data_ptr(), [first_of[quiz] for quiz, _ in pairs])
        except interop.PqaException as e:
            error = str(e)
    ranks.settle(error)
    return out


def _replicated(call, rank: int, world: int, group, device: Optional[torch.device]):
    """One replicated maintenance call and a status word: if any rank failed, every rank raises the first failure.  (The calls
    validate against state every rank holds alike, so they fail on all ranks or on none; what can fail on one rank alone is its
    device's memory, and that rank's engine is unchanged then.)"""
    from . import interop

    result, error = None, None
    try:
        result = call()
    except interop.PqaException as e:
        error = str(e)
    _Ranks(group, device, rank, world).settle(error)
    return result


def remove_questions(engine, question_ids, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                     device: Optional[torch.device] = None) -> None:
    """RemoveQuestions (GLOBAL ids) on the shards of `world` ranks: a collective every rank calls with the same ids."""
    _replicated(lambda: engine.remove_questions(list(question_ids)), rank, world, group, device)


def remove_targets(engine, target_ids, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
                   device: Optional[torch.device] = None) -> None:
    """RemoveTargets on the shards of `world` ranks: a collective every rank calls with the same ids."""
    _replicated(lambda: engine.remove_targets(list(target_ids)), rank, world, group, device)


def add_qs_ts(engine, add_questions, add_targets, rank: int, world: int, group: Optional[dist.ProcessGroup] = None,
              device: Optional[torch.device] = None) -> None:
    """AddQsTs on the shards of `world` ranks: a collective every rank calls with the same parameters; their i_question / i_target
    receive the GLOBAL ids, the same on every rank.  Appended questions land on the last rank: see gather_bounds."""
    _replicated(lambda: engine.add_qs_ts(add_questions, add_targets), rank, world, group, device)


def compact(engine, rank: int, world: int, group: Optional[dist.ProcessGroup] = None, device: Optional[torch.device] = None):
    """Compact on the shards of `world` ranks: a collective every rank calls.  Returns (old_q, old_t), the global maps, the same on
    every rank.

    Every rank plans (host only); one all_reduce(MIN) votes on errors and on whether any shard would be left without a question --
    then every rank raises the same InsufficientEngineDimensions and nothing has changed; the owners pack the questions that move
    into a zero-filled tensor on the device; ONE all_reduce(SUM) in the engine's element type combines the packages -- exact, and a
    move of bits, for the reason resume_quiz's is: every slot is written by exactly one rank and x + 0 == x --, under gloo through
    the host; every rank compacts from the combined package; one status word.  A shard keeps the part of its range below the new
    question count: see gather_bounds."""
    from . import interop

    ranks = _Ranks(group, device, rank, world)
    plan, error = None, None
    try:
        plan = engine.compact_plan()
    except interop.PqaException as e:
        error = str(e)
    # the vote: 2 * rank for an error, 2 * rank + 1 for a shard that would be emptied, 2 * world for neither
    vote = ranks.min_word(2 * rank if error is not None else 2 * rank + 1 if plan[3] else 2 * world)
    if vote < 2 * world:
        first = vote // 2
        if vote % 2:
            engine.compact_from_blocks(0, 0, first)      # (refused, with the text every rank gets: nothing has changed)
            raise AssertionError("a compaction that empties rank %d was not refused" % first)
        ranks.fail(first, error)
    moves = plan[2]
    slot = engine.question_block_slot_bytes()
    pkg = None
    if moves:
        elem = 4 if engine.get_option("precision") == 1 else 8
        pkg = torch.zeros(len(moves), slot // elem, dtype=torch.float32 if elem == 4 else torch.float64, device=ranks.device)
        error = _summed_package(ranks, engine, pkg, lambda ptr: engine.pack_question_blocks([src for _, src in moves], ptr))
    result = None
    if error is None:
        try:
            result = engine.compact_from_blocks(pkg.data_ptr() if pkg is not None else 0, slot if pkg is not None else 0, -1)
        except interop.PqaException as e:
            error = str(e)
    ranks.settle(error)
    return result


class ShmRowExchange:
    """resume_quiz / resume_quiz_batch without a process group, for the shared-memory deployments that use ShmSelector: the
    package lives in ONE /dev/shm segment every rank has mapped and registered with its GPU.  The owners pack straight into it
    with the flag form of PqaHip_PackAnswerRows, every rank waits (bounded) for all `world` flags to carry the step number and
    resumes from the segment's device-visible address; a status word per rank, written by the host, then makes the call all or
    none as the collective is.  Two halves alternate by step parity, as ShmSelector's slot sets do.  The segment (`size_for`
    bytes, zero-filled) is created by the caller before the ranks open it.  No rank may train between pack and resume."""

    LINE = 64

    @classmethod
    def size_for(cls, world: int, slot_bytes: int, max_slots: int) -> int:
        return 2 * (2 * world * cls.LINE + max_slots * slot_bytes)

    def __init__(self, rank: int, world: int, name: str, slot_bytes: int, max_slots: int):
        import numpy as np

        from . import interop

        self.rank, self.world, self.slot_bytes, self.max_slots = rank, world, slot_bytes, max_slots
        self.path = "/dev/shm/pqa_rows_%s" % name
        self._half = 2 * world * self.LINE + max_slots * slot_bytes
        self._seg = _ShmSegment(self.path, self.size_for(world, slot_bytes, max_slots), create=False, register=True)
        self._dev = self._seg.dev
        self._words = self._seg.bytes.view(np.uint64)
        self._interop = interop
        self.step = 0

    def _word(self, half: int, kind: int, r: int) -> int:
        """Index (in 8-byte words) of rank r's flag (kind 0) or status (kind 1) of a half."""
        return (half * self._half + (kind * self.world + r) * self.LINE) // 8

    def _wait(self, half: int, kind: int, timeout_s: float):
        """Every rank's flag (the step) or status (twice the step, plus 1 for a failure) of this step, as read."""
        want = (2 * self.step, 2 * self.step + 1) if kind else (self.step,)
        return _spin_until(lambda r: self._words[self._word(half, kind, r)], want, self.world, timeout_s,
                           "rank %%d never published %s %d" % ("status" if kind else "rows of step", self.step))

    def _run(self, engine, flat, resume, release, timeout_s: float):
        if len(flat) > self.max_slots:
            raise ValueError("%d answered questions, the segment holds %d" % (len(flat), self.max_slots))
        half = _next_half(self)
        rows = half * self._half + 2 * self.world * self.LINE
        result, error = None, None
        try:
            engine.pack_answer_rows(flat, self._dev + rows, self._dev + 8 * self._word(half, 0, self.rank), self.step)
        except self._interop.PqaException as e:   # (the others must not wait for rows that never come: the status fails the call)
            error = str(e)
            self._words[self._word(half, 0, self.rank)] = self.step
        self._wait(half, 0, timeout_s)
        if error is None:
            try:
                result = resume(self._dev + rows)
            except self._interop.PqaException as e:
                error = str(e)
        self._words[self._word(half, 1, self.rank)] = 2 * self.step + (1 if error is not None else 0)
        status = self._wait(half, 1, timeout_s)
        failed = [r for r in range(self.world) if status[r] & 1]
        if failed:
            if error is None:
                release(result)
            raise self._interop.PqaException("ResumeQuiz failed on rank%s %s%s" % ("s" if len(failed) > 1 else "", ", ".join(map(str, failed)),
                                                                              "" if error is None else ": " + error))
        return result

    def resume_quiz(self, engine, answered, timeout_s: float = 30.0) -> int:
        answered = list(answered)
        return self._run(engine, answered, lambda rows: engine.resume_quiz_from_rows(answered, rows), engine.release_quiz, timeout_s)

    def resume_quiz_batch(self, engine, lists, timeout_s: float = 30.0) -> List[int]:
        lists = [list(l) for l in lists]

        def release(quizzes):
            for q in quizzes:
                engine.release_quiz(q)

        return self._run(engine, [aq for l in lists for aq in l], lambda rows: engine.resume_quiz_batch_from_rows(lists, rows), release,
                         timeout_s)

    def close(self) -> None:
        self._words = None
        self._seg.close()


def tensor_from_device_ptr(ptr: int, n_doubles: int, device: torch.device) -> torch.Tensor:
    """Wrap engine-owned device memory (e.g. a quiz's prior vector) as a torch tensor without copying."""

    class _Holder:
        pass

    h = _Holder()
    h.__cuda_array_interface__ = {"shape": (n_doubles,), "typestr": "<f8", "data": (ptr, False), "version": 3}
    return torch.as_tensor(h, device=device)
