"""The numpy model of the maintenance operations (tests/kb_model.py) and the cases built on it (tests/maintenance_cases.py), without a
device: the model's ids are the engine's own planner's (kb_plan.h through the host-logic probe), its arrays are those the existing
device test works out by hand, the scripts reach the allocations they are meant to reach, and every serving case's quiz states give the
oracle an unambiguous best question and unambiguous sampled picks -- so tests/test_gpu_maintenance.py has no check to skip."""
import numpy as np
import pytest

import maintenance_cases as mc
from kb_model import KBModel, random_step, round_ldt
from probqa_amd import synth
from test_host_logic import add_plan, compact_plan


def run_random_script(seed, f32, check):
    rng, (K, Q, T), kb_seed = mc.random_script_start(seed)
    model = mc.synthetic_model(K, Q, T, kb_seed, f32)
    for _ in range(mc.RANDOM_STEPS):
        step = random_step(model, rng)
        check(model, step)
    return model


@pytest.mark.parametrize("seed", range(mc.N_RANDOM_SCRIPTS))
def test_model_ids_are_the_planners_over_random_scripts(seed):
    ops = set()

    def check(model, step):
        Q, T, qg, tg = model.Q, model.T, list(model.q_gaps), list(model.t_gaps)
        ld_t, cap_q = model.ld_t, model.cap_q
        got = model.apply(step)
        ops.add(step[0])
        if step[0] == "add":
            plan = add_plan(Q, T, qg, tg, step[1], step[2])
            assert got == (plan["q_ids"], plan["t_ids"])
            assert (model.Q, model.T) == (plan["new_q"], plan["new_t"])
            assert model.q_gaps == qg[:len(qg) - plan["n_q_reuse"]] and model.t_gaps == tg[:len(tg) - plan["n_t_reuse"]]
        elif step[0] == "compact":
            old_q, old_t, _ = compact_plan(Q, T, qg, tg)
            assert got == (old_q, old_t)
            assert (model.Q, model.T) == (len(old_q), len(old_t)) and not model.q_gaps and not model.t_gaps
        # the allocation only grows, and holds the dimensions
        assert model.ld_t == max(ld_t, round_ldt(model.T)) and model.cap_q == max(cap_q, model.Q)
        assert 1 <= model.Q <= 40 and 2 <= model.T <= 80 and len(model.live_q()) >= 1 and len(model.live_t()) >= 2
        assert not np.isnan(model.A).any() and not np.isnan(model.D).any() and not np.isnan(model.B).any()   # every cell an operation makes is defined

    run_random_script(seed, False, check)
    assert "add" in ops


def test_random_scripts_cover_every_operation_and_a_reallocation():
    ops, regrown = set(), 0
    for seed in range(mc.N_RANDOM_SCRIPTS):
        def check(model, step):
            nonlocal regrown
            before = (model.ld_t, model.cap_q)
            model.apply(step)
            ops.add(step[0])
            regrown += before != (model.ld_t, model.cap_q)
        run_random_script(seed, False, check)
    assert ops == {"remove_q", "remove_t", "add", "compact"} and regrown >= 5


@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
def test_model_reproduces_the_fixed_sequence_of_the_device_test(f32):
    """tests/test_gpu_kb.py::test_add_remove_compact_against_numpy_model: its calls, its expected ids and its hand-made expected arrays."""
    K, Q, T = 4, 12, 19
    r = (lambda x: float(np.float32(x))) if f32 else (lambda x: x)
    A, D, B = synth.synthetic_kb(K, Q, T, 0.1, 8.0, 0.5, 9)
    if f32:
        A, D, B = (x.astype(np.float32).astype(np.float64) for x in (A, D, B))
    model = KBModel(A, D, B, f32=f32)
    model.remove_questions([2, 9])
    model.remove_targets([0, 5, 18])
    assert model.add([0.5, 0.25, 2.0], [0.3, 0.7]) == ([9, 2, 12], [18, 5])
    A = np.concatenate([A, np.zeros((1, K, T))], axis=0)
    D = np.concatenate([D, np.zeros((1, T))], axis=0)
    for t, amount in ((18, 0.3), (5, 0.7)):
        A[:, :, t], D[:, t], B[t] = r(amount * amount), r(amount * amount * K), r(amount)
    for q, amount in ((9, 0.5), (2, 0.25), (12, 2.0)):
        A[q], D[q] = r(amount * amount), r(amount * amount * K)
    assert (model.Q, model.T) == (13, 19) and model.t_gaps == [0] and model.q_gaps == []
    assert np.array_equal(model.A, A) and np.array_equal(model.D, D) and np.array_equal(model.B, B)   # (gap column 0 untouched on both sides)
    model.remove_questions([3, 11])
    old_q, old_t = model.compact()
    assert len(old_q) == 11 and sorted(old_q) == [q for q in range(13) if q not in (3, 11)] and old_q[3] == 12 and old_q[:3] == [0, 1, 2]
    assert len(old_t) == 18 and old_t[0] == 18 and old_t[1:] == list(range(1, 18))
    assert np.array_equal(model.A, A[old_q][:, :, old_t]) and np.array_equal(model.D, D[old_q][:, old_t]) and np.array_equal(model.B, B[old_t])
    assert (model.ld_t, model.cap_q) == (32, 13)


@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
def test_array_scripts_reach_the_allocations_they_are_for(f32):
    seen = {}
    for name, ((K, Q, T), seed, steps) in mc.array_scripts(f32).items():
        model = mc.synthetic_model(K, Q, T, seed, f32)
        trail = [(model.Q, model.T, model.ld_t, model.cap_q)]
        for step in steps:
            model.apply(step)
            trail.append((model.Q, model.T, model.ld_t, model.cap_q))
        seen[name] = trail
    g = 32 if f32 else 16
    t0, t1 = (30, 35) if f32 else (13, 19)
    assert seen["grow_t"] == [(5, t0, g, 5), (5, t1, 2 * g, 5)]                      # across a granule, the capacity stays
    assert seen["grow_t_and_q"] == [(5, t0, g, 5), (7, t1, 2 * g, 7)]
    assert seen["grow_q"] == [(5, t0, g, 5), (8, t0, g, 8)]
    assert seen["grow_t_inside_granule"] == [(5, 17, 32, 5), (5, 20, 32, 5)]         # no reallocation
    assert seen["more_additions_than_gaps"][-1][:2] == (10, 23)                     # 3 gaps + 2 new questions, 2 gaps + 2 new targets
    ld40 = round_ldt(40, f32)                                                        # 48 fp64 elements, 64 fp32 elements
    assert seen["compact_across_granule"][3:] == [(6, 14, ld40, 9), (8, 18, ld40, 9), (11, 78, round_ldt(78, f32), 11)]
    assert ld40 > round_ldt(14, f32)                                                 # the compacted cube keeps a pitch a fresh one would not have


@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("case", mc.SERVING_CASES, ids=lambda c: c.name)
def test_serving_cases_leave_the_oracle_no_ambiguity(case, f32):
    """The margins tests/test_gpu_maintenance.py asserts again on the device's own arrays, here on the model's: in each of the three quiz
    states the oracle's top-2 margin exceeds ten times the priorities' bar, and no sampled draw falls near a boundary."""
    model = case.model(f32)
    for step in case.steps:
        model.apply(step)
    fresh = mc.untrained_questions(model)
    assert len(fresh) == (3 if "grow" in case.name else 2) and not mc.untrained_questions(case.model(f32))      # the added questions, and only they
    records = mc.post_training(model)
    mc.train_model(model, records)
    assert {q for q, _, _, _ in records} == set(fresh) and not mc.untrained_questions(model)
    assert model.T == case.T1 and model.Q == case.Q + (2 if "grow" in case.name else 1) and model.cap_q == case.Q + 2
    assert len(model.q_gaps) == 1 and len(model.t_gaps) == 2
    assert model.ld_t == round_ldt(max(case.T0, case.T1), f32) and (model.ld_t > round_ldt(model.T, f32)) == ("compact" in case.name)
    states, asked = mc.serving_states(model, mc.ANSWERS)
    assert len(states) == 3 and len({q for q, _ in asked}) == 2
    for s in states:
        assert s.margin > 10 * mc.PRIORITY_RTOL and s.argmax_clearance > 0 and s.sampled_clearance > 0
    print(case.name, "float" if f32 else "double", "top-2 margins %s, least %.3g" % (["%.3g" % s.margin for s in states], min(s.margin for s in states)))
