"""Maintenance over shards in separate processes (probqa_amd/dist.py: add_qs_ts, remove_questions, remove_targets, compact,
gather_bounds).  Spawned processes share the one GPU of the test box under gloo, as tests/test_gpu_resume_ranks_procs.py starts them;
each holds its range of the questions of the script `compact_across_granule` (tests/maintenance_cases.py) and must end with its slice
of the arrays of the numpy model.  At three ranks the compaction would leave the last one without a question: every rank must raise
the same refusal and keep what it had.  Every wait is bounded: the collectives time out, and the parent takes the results with a time
limit."""
import numpy as np
import pytest

import maintenance_cases as mc
import ranks_common as rc

pytestmark = pytest.mark.gpu

SCRIPT = "compact_across_granule"


def _rank_main(rank, world, port):
    import torch
    import torch.distributed as dist

    from probqa_amd import dist as pdist
    from probqa_amd import interop

    (K, Q, T), seed, steps = mc.array_scripts(False)[SCRIPT]
    model = mc.synthetic_model(K, Q, T, seed, False)
    first, limit = pdist.shard_range(Q, world, rank)
    eng = interop.PqaEngineFactory().create_hip_engine(interop.EngineDefinition(K, limit - first, T, init_amount=mc.INIT), first, Q, 0)
    eng.set_kb(model.A[first:limit], model.D[first:limit], model.B)
    torch.cuda.set_device(0)
    rc.init_group("gloo", rank, world, port)
    eng.start_maintenance(False)
    res = {"bounds": [pdist.gather_bounds(eng)], "returned": [], "error": None}
    try:
        for step in steps:
            if step[0] == "remove_q":
                pdist.remove_questions(eng, step[1], rank, world)
            elif step[0] == "remove_t":
                pdist.remove_targets(eng, step[1], rank, world)
            elif step[0] == "add":
                aq = [interop.AddQuestionParam(a) for a in step[1]]
                at = [interop.AddTargetParam(a) for a in step[2]]
                pdist.add_qs_ts(eng, aq, at, rank, world)
                res["returned"].append(([p.i_question for p in aq], [p.i_target for p in at]))
            else:
                res["returned"].append(pdist.compact(eng, rank, world))
            if step[0] in ("add", "compact"):
                res["bounds"].append(pdist.gather_bounds(eng))
    except interop.PqaException as e:
        res["error"] = str(e)
    res["dims"] = tuple(eng.get_option(o) for o in ("q_first", "local_questions", "q_total"))
    res["plan"] = eng.compact_plan()[:3]
    res["kb"] = eng.get_kb(res["dims"][1])
    eng.finish_maintenance()
    dist.destroy_process_group()
    eng.close()
    return res


def _run_ranks(world):
    return rc.run_ranks(_rank_main, world, (world, rc.free_port()))


def _model(n_steps):
    (K, Q, T), seed, steps = mc.array_scripts(False)[SCRIPT]
    model = mc.synthetic_model(K, Q, T, seed, False)
    returned = [model.apply(step) for step in steps[:n_steps]]
    return model, [r for r in returned if r is not None]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_two_processes_run_the_script_over_gloo(factory):
    got = _run_ranks(2)
    model, returned = _model(5)
    lt = model.live_t()
    for r in range(2):
        res = got[r]
        assert res["error"] is None, res["error"]
        assert res["bounds"] == [[5, 9], [5, 6], [5, 8], [5, 11]], res["bounds"]
        assert [tuple(map(list, x)) for x in res["returned"]] == [tuple(map(list, x)) for x in returned]      # the model's ids and maps, on every rank
        first, limit = (0, 5) if r == 0 else (5, 11)
        assert res["dims"] == (first, limit - first, 11)
        A, D, B = res["kb"]
        assert _same_bits(A[:, :, lt], model.A[first:limit][:, :, lt]) and _same_bits(D[:, lt], model.D[first:limit][:, lt]) and _same_bits(B[lt], model.B[lt])


def test_three_processes_refuse_the_compaction_alike(factory):
    got = _run_ranks(3)
    model, _ = _model(2)                      # the two removals ran, the compaction did not
    lt = model.live_t()
    texts = {got[r]["error"] for r in range(3)}
    assert len(texts) == 1 and None not in texts, texts
    assert "Insufficient engine dimensions" in got[0]["error"] and "rank=2" in got[0]["error"], texts
    for r in range(3):
        res = got[r]
        assert res["bounds"] == [[3, 6, 9]] and res["dims"] == (3 * r, 3, 9) and res["returned"] == []
        assert res["plan"] == (6, 14, [(0, 7), (4, 6)])            # the gaps are as they were
        A, D, B = res["kb"]
        lq = [q - 3 * r for q in model.live_q() if 3 * r <= q < 3 * r + 3]
        assert _same_bits(A[lq][:, :, lt], model.A[3 * r:3 * r + 3][lq][:, :, lt]) and _same_bits(D[lq][:, lt], model.D[3 * r:3 * r + 3][lq][:, lt])
        assert _same_bits(B[lt], model.B[lt])
