"""What a greedy page of questions costs over separately created shards (a tool, not a test).  One process, the shards side by side on
ONE device and called one after another, no collective: separate processes on separate devices would run the shards' steps side by
side, so the slowest shard is what a process group would wait for per page, and the exchange -- one all-reduce of the new slots, two
status words and one all-gather of 16 bytes a quiz per step -- is NOT in any number here.  Per shape, shard count and page size, after a
warm-up that also holds the shards' pages to the whole engine's record for record, round by round, min / median / max:
  (whole)   PqaEngine_ListQuestionPageBatch on the whole engine;
  (shard r) the sum over the page's steps of PqaHip_SelectPageStepFromBlocks on shard r, the host's wait included;
  (pack)    the sum over the steps of PqaHip_PackGivenBlocks on every shard and the wait for it;
and, from one more round under option "time_sweeps", the share of the shards' device time that runs before the first sweep of a step
(the roots and the expansions that rebuild the branch rows: "page_head_ns" of "page_device_ns").
Shapes: 1000x5x1000 in 2 and 8 shards, 10000x5x10000 in 8 (questions x answers x targets), 64 quizzes resumed from 1 .. 5 answers each, pages of 2 / 3.
Prints one JSON line per shape, shard count and page size, then the table.
usage: question_page_ranks_bench.py [--quick] [rounds=5]      --quick: one small shape, 40x5x1300 in 2 and 3 shards, 8 quizzes"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probqa_amd import dist as pdist
from probqa_amd import interop

AQ = interop.AnsweredQuestion
factory = interop.PqaEngineFactory()


def engine(first, limit, Q, K, T):
    e = factory.create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=0.1), first, Q, 0)
    e.fill_synthetic(8.0, 0.5, 7)
    return e


def resume_on_shards(shards, seqs, live):
    """the whole engine's quizzes `live` on every (fresh) shard: the shards resume from a row package, as dist.resume_quiz_batch does"""
    flat = [aq for s in seqs for aq in s]
    slot = shards[0].answer_row_slot_bytes()
    pkg = torch.zeros(max(len(flat), 1), slot // 8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for sh in shards:
        sh.pack_answer_rows(flat, pkg.data_ptr())
    for sh in shards:
        sh.synchronize()
    for sh in shards:
        assert sh.resume_quiz_batch_from_rows(seqs, pkg.data_ptr()) == live


def shard_page(shards, quizzes, page_size, slot_doubles, clock):
    """dist.list_question_page_batch's loop without a process group; clock[r] += shard r's steps, clock[-1] += the packs"""
    sets, pages, active, slots = [[] for _ in quizzes], [[] for _ in quizzes], list(range(len(quizzes))), []
    pkg = torch.zeros(max(len(quizzes) * max(page_size - 1, 0), 1), slot_doubles, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(page_size):
        if not active:
            break
        new = pdist._distinct([sets[i] for i in active], slots)
        if new:
            t0 = time.perf_counter()
            for sh in shards:
                sh.pack_given_blocks(new, pkg[len(slots):].data_ptr())
            for sh in shards:
                sh.synchronize()
            clock[-1] += time.perf_counter() - t0
            slots.extend(new)
        records = []
        for r, sh in enumerate(shards):
            t0 = time.perf_counter()
            records.append(sh.select_page_step_from_blocks([quizzes[i] for i in active], [sets[i] for i in active], slots, pkg.data_ptr()))
            clock[r] += time.perf_counter() - t0
        still = []
        for i, (q, bits) in zip(active, pdist.merge_page_step(records)):
            if q >= 0:
                pages[i].append((q, bits))
                sets[i].append(q)
                still.append(i)
        active = still
    return pages


def spread(ts):
    return {"ms_min": round(min(ts) * 1e3, 4), "ms_median": round(statistics.median(ts) * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4)}


def run(Q, K, T, worlds, n_quizzes, sizes, rounds, rows):
    shape = "%dx%dx%d" % (Q, K, T)
    whole = engine(0, Q, Q, K, T)
    rng = np.random.default_rng(3)
    seqs = [[AQ(int(q), int(rng.integers(K))) for q in rng.permutation(Q)[:1 + j % 5]] for j in range(n_quizzes)]
    quizzes = whole.resume_quiz_batch(seqs)
    for world in worlds:
        shards = [engine(*pdist.shard_range(Q, world, r), Q, K, T) for r in range(world)]
        resume_on_shards(shards, seqs, quizzes)
        slot_doubles = whole.question_block_slot_bytes() // 8
        for size in sizes:
            want = whole.list_question_page_batch(quizzes, size)                               # warm-up, and the check
            got = shard_page(shards, quizzes, size, slot_doubles, [0.0] * (world + 1))
            assert [[(q, np.float64(b).tobytes()) for q, b in p] for p in got] == [[(q, np.float64(b).tobytes()) for q, b in p] for p in want], (shape, world, size)
            t_whole, t_shard, t_pack = [], [[] for _ in shards], []
            for _ in range(rounds):
                t0 = time.perf_counter()
                whole.list_question_page_batch(quizzes, size)
                t_whole.append(time.perf_counter() - t0)
                clock = [0.0] * (world + 1)
                shard_page(shards, quizzes, size, slot_doubles, clock)
                for r in range(world):
                    t_shard[r].append(clock[r])
                t_pack.append(clock[-1])
            for sh in shards:
                sh.set_option("time_sweeps", 1)
            ns0 = [(sh.get_option("page_device_ns"), sh.get_option("page_head_ns")) for sh in shards]
            shard_page(shards, quizzes, size, slot_doubles, [0.0] * (world + 1))
            device = [sh.get_option("page_device_ns") - a for sh, (a, _) in zip(shards, ns0)]
            head = [sh.get_option("page_head_ns") - b for sh, (_, b) in zip(shards, ns0)]
            for sh in shards:
                sh.set_option("time_sweeps", 0)
            medians = [statistics.median(ts) for ts in t_shard]
            slowest = max(range(world), key=lambda r: medians[r])
            out = {"shape": shape, "shards": world, "quizzes": n_quizzes, "page_size": size, "rounds": rounds, "pages_agree": True,
                   "whole": spread(t_whole), "shard_steps": [spread(ts) for ts in t_shard], "slowest_shard": slowest, "slowest": spread(t_shard[slowest]),
                   "shards_summed_ms_median": round(sum(medians) * 1e3, 4), "pack": spread(t_pack),
                   "head_share": [round(h / d, 4) if d > 0 else None for h, d in zip(head, device)]}
            out["whole_over_slowest"] = round(statistics.median(t_whole) / medians[slowest], 2)
            print(json.dumps(out), flush=True)
            fmt = lambda s: "%.3f (%.3f .. %.3f)" % (s["ms_median"], s["ms_min"], s["ms_max"])
            rows.append("| %s | %d | %d | %d | %s | %s | %.3f | %s | %.2f | %s |" % (
                shape, world, n_quizzes, size, fmt(out["whole"]), fmt(out["slowest"]), out["shards_summed_ms_median"], fmt(out["pack"]), out["whole_over_slowest"],
                "%.1f %%" % (100 * max(x for x in out["head_share"] if x is not None)) if any(x is not None for x in out["head_share"]) else "-"))
        for sh in shards:
            sh.close()
    whole.close()


def main():
    args = [a for a in sys.argv[1:] if a != "--quick"]
    quick = len(args) != len(sys.argv) - 1
    rounds = int(args[0]) if args else 5
    rows = []
    plan = [(40, 5, 1300, (2, 3), 8, (2, 3))] if quick else [(1000, 5, 1000, (2, 8), 64, (2, 3)), (10000, 5, 10000, (8,), 64, (2, 3))]
    for Q, K, T, worlds, n, sizes in plan:
        run(Q, K, T, worlds, n, sizes, rounds, rows)
    print("| shape | shards | quizzes | page | whole engine ms median (min .. max) | slowest shard's steps ms | all shards' steps summed ms | packs ms | whole / slowest | "
          "largest share before the sweep |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(r)


if __name__ == "__main__":
    main()
