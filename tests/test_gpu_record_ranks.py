"""RecordAnswer for many quizzes across separately created shards on a real MI355X (PqaHip_PosteriorSlotBytes,
PqaHip_PackAnswerPosteriors, PqaEngine_RecordAnswerBatchFromPosteriors).  One process: the shards of one synthetic KB sit side by
side on the one device as create_hip_engine(def, q_first, Q, 0) engines, one whole engine holds the same KB, and the CPU oracle
records the same answers.  Every shard packs into ONE zero-filled torch tensor (what the all-reduce delivers), every shard consumes
it; posteriors are compared for equality.  The shapes are the smallest that reach each edge of the two kernels and of the update
forms: an odd T (a partial 16-byte unit), a Float engine (its ldT differs from the slot's pitch), one full 16 KB chunk plus one
element, and rows beyond 16384 targets (the long-row update, ten chunks, the last one partial)."""
import ctypes
import mmap

import numpy as np
import pytest
import torch

import orclib
from probqa_amd import dist as pdist
from probqa_amd import interop
from test_gpu_resume_ranks import WORKERS, Shape, aq_list

pytestmark = pytest.mark.gpu

SHAPES = {s.name: s for s in [
    Shape("gaps37x5x101", 5, 37, 101, tgaps=(3, 17, 100)),          # odd T: a partial unit, pitch 112
    Shape("ragged90x4x700", 4, 90, 700),                            # pitch 704
    Shape("float120x5x1000", 5, 120, 1000, f32=True),               # the engine's ldT is 1024, the slot's pitch 1008
    Shape("chunk40x3x2049", 3, 40, 2049),                           # one full 16 KB chunk plus one element
    Shape("long64x5x20000", 5, 64, 20000, tgaps=(5, 19999)),        # the long-row update form; ten chunks, the last partial
]}
PITCH = {"gaps37x5x101": 112, "ragged90x4x700": 704, "float120x5x1000": 1008, "chunk40x3x2049": 2064, "long64x5x20000": 20000}
N_QUIZZES, ROUNDS = 12, 3


def plan(shape, world):
    """questions[round][quiz]: quiz i's question of round r lies on rank (i + r) % world, so that every rank holds one of a
    round's questions, none holds all of them, and no quiz meets a question twice."""
    bounds = pdist.shard_bounds(shape.Q, world)
    firsts = [0] + bounds[:-1]
    rounds = []
    for r in range(ROUNDS):
        qs = []
        for i in range(N_QUIZZES):
            k = (i + r) % world
            qs.append(firsts[k] + (i // world + 4 * r) % (bounds[k] - firsts[k]))
        rounds.append(qs)
    return rounds


def check_plan(rounds, shape, world):
    bounds = pdist.shard_bounds(shape.Q, world)
    for qs in rounds:
        owners = [pdist.owner_in(bounds, q) for q in qs]
        assert set(owners) == set(range(world)), owners             # every rank holds at least one of the round's questions
        if world > 1:
            assert all(owners.count(r) < len(qs) for r in range(world)), owners     # ... and none holds all of them
    for i in range(N_QUIZZES):
        assert len({qs[i] for qs in rounds}) == ROUNDS, i           # an unasked question every round


def answers_of(shape, r):
    return [(i + r) % shape.K for i in range(N_QUIZZES)]


def package(eng, n, name=None):
    slot = eng.posterior_slot_bytes()
    assert slot % 128 == 0 and (name is None or slot == 8 * PITCH[name]), slot
    pkg = torch.zeros(max(n, 1), slot // 8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return pkg


def pack_and_consume(shards, quizzes, answers, name=None):
    pkg = package(shards[0], len(quizzes), name)
    for sh in shards:
        sh.pack_answer_posteriors(quizzes, answers, pkg.data_ptr())
    for sh in shards:
        sh.synchronize()
    for sh in shards:
        sh.record_answer_batch_from_posteriors(quizzes, answers, pkg.data_ptr())
    return pkg


_oracles = {}


def oracle_posteriors(shape, whole, rounds):
    """[quiz][round] -> the oracle's posterior; one oracle KB per shape, shared by the worlds."""
    if shape.name not in _oracles:
        orc = orclib.Oracle(shape.K, shape.Q, shape.T, 0.1)
        orc.set_kb(*whole.get_kb())
        orc.set_target_gaps(list(shape.tgaps))
        _oracles[shape.name] = orc
    orc = _oracles[shape.name]
    out = []
    for i in range(N_QUIZZES):
        orc.start_quiz(WORKERS)
        per = []
        for r, qs in enumerate(rounds):
            orc.record_answer(qs[i], answers_of(shape, r)[i], WORKERS - 1)
            per.append(orc.priors())
        out.append(per)
    return out


def listing(eng, quiz, n=3):
    return [(t.i_target, t.prob) for t in eng.list_top_targets(quiz, n)]


def close_all(engines):
    for e in engines:
        e.close()


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_three_rounds_bit_for_bit(name, world, factory):
    shape = SHAPES[name]
    rounds = plan(shape, world)
    check_plan(rounds, shape, world)
    whole, shards = shape.world(factory, world)
    engines = [whole] + shards
    want_orc = None if shape.f32 else oracle_posteriors(shape, whole, rounds)      # (the suite holds Float engines to each other)
    quizzes = whole.start_quiz_batch(N_QUIZZES)
    for sh in shards:
        assert sh.start_quiz_batch(N_QUIZZES) == quizzes
    bounds = pdist.shard_bounds(shape.Q, world)
    for r, qs in enumerate(rounds):
        answers = answers_of(shape, r)
        for e in engines:
            for quiz, q in zip(quizzes, qs):
                e.set_active_question(quiz, q)
        whole.record_answer_batch(quizzes, answers)
        packs0 = [sh.get_option("posterior_packs") for sh in shards]
        owned0 = [sh.get_option("posteriors_packed") for sh in shards]
        taken0 = [sh.get_option("posteriors_taken") for sh in shards]
        pack_and_consume(shards, quizzes, answers, name)
        for k, sh in enumerate(shards):                             # the counters move as documented
            assert sh.get_option("posterior_packs") - packs0[k] == 1
            assert sh.get_option("posteriors_packed") - owned0[k] == sum(pdist.owner_in(bounds, q) == k for q in qs)
            assert sh.get_option("posteriors_taken") - taken0[k] == N_QUIZZES
        for i, quiz in enumerate(quizzes):
            want = whole.get_priors(quiz)
            if want_orc is not None:
                assert np.array_equal(want, want_orc[i][r]), f"whole engine vs oracle: quiz {i}, round {r}"
            for k, sh in enumerate(shards):
                got = sh.get_priors(quiz)
                assert np.array_equal(got, want), f"shard {k} of {world}: quiz {i}, round {r}: {np.abs(got - want).max():g}"
    # the sweep on the new posteriors, and the device's asked bits: exactly 0 at every asked question this shard holds
    pri_w = whole.eval_priorities_batch(quizzes)
    firsts = [0] + bounds[:-1]
    for k, sh in enumerate(shards):
        pri = sh.eval_priorities_batch(quizzes, bounds[k] - firsts[k])
        ref = pri_w[:, firsts[k]:bounds[k]]
        rel = np.abs(pri - ref) / np.maximum(np.abs(ref), 1e-300)
        print("shard %d of %d: largest relative priority difference %g" % (k, world, rel.max()))
        assert rel.max() < 1e-9, (k, rel.max())
        for i in range(N_QUIZZES):
            for qs in rounds:
                if firsts[k] <= qs[i] < bounds[k]:
                    assert pri[i, qs[i] - firsts[k]] == 0 and pri_w[i, qs[i]] == 0, (k, i, qs[i])
        assert ((pri == 0) == (ref == 0)).all(), k
    for e in engines:
        assert [e.get_active_question_id(q) for q in quizzes] == [-1] * N_QUIZZES
    # ListTopTargets after a consume: listed on demand, record for record the whole engine's
    for quiz in quizzes[:3]:
        want = listing(whole, quiz)
        for sh in shards:
            assert listing(sh, quiz) == want
    # the resumed twin of a quiz, on every shard, from a row package over the recorded answers (GLOBAL question ids); resumed as
    # the formulas say, not as the reference's ResumeQuiz reads vB (option bug_compat), so that it is the posterior of the answers
    for e in engines:
        e.set_option("bug_compat", 0)
    for i in (0, N_QUIZZES - 1):
        history = [(qs[i], answers_of(shape, r)[i]) for r, qs in enumerate(rounds)]
        slot = shards[0].answer_row_slot_bytes()
        rows = torch.zeros(len(history), slot // 8, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for sh in shards:
            sh.pack_answer_rows(aq_list(history), rows.data_ptr())
        for sh in shards:
            sh.synchronize()
        twin_w = whole.get_priors(whole.resume_quiz(aq_list(history)))
        for k, sh in enumerate(shards):
            twin = sh.get_priors(sh.resume_quiz_from_rows(aq_list(history), rows.data_ptr()))
            assert np.array_equal(twin, twin_w), (k, i)
            # resumed and recorded step by step: the same posterior up to the roundings of the two orders of operations -- under
            # 20 roundings per element and two Kahan sums on either path, 40 x 2^-53 = 5e-15; a wrong question or answer moves it by O(1)
            stepwise = sh.get_priors(quizzes[i])
            print("shard %d, quiz %d: resumed against recorded, largest relative difference %g" % (k, i, (np.abs(stepwise - twin) / np.maximum(twin, 1e-300)).max()))
            np.testing.assert_allclose(stepwise, twin, rtol=1e-12, atol=0)
    close_all(engines)


def test_recorded_answers_carry_global_question_ids(factory):
    """RecordQuizTarget trains from the quiz's own answers and keeps the steps of the questions its engine holds: after three
    rounds through packages every shard's part of the cube is the whole engine's."""
    shape, world = SHAPES["gaps37x5x101"], 3
    rounds = plan(shape, world)
    whole, shards = shape.world(factory, world)
    quizzes = whole.start_quiz_batch(N_QUIZZES)
    for sh in shards:
        sh.start_quiz_batch(N_QUIZZES)
    for r, qs in enumerate(rounds):
        for e in [whole] + shards:
            for quiz, q in zip(quizzes, qs):
                e.set_active_question(quiz, q)
        whole.record_answer_batch(quizzes, answers_of(shape, r))
        pack_and_consume(shards, quizzes, answers_of(shape, r))
    for e in [whole] + shards:
        e.record_quiz_target(quizzes[5], 40, 2.5)
    A, D, B = whole.get_kb()
    for k, sh in enumerate(shards):
        first, limit = pdist.shard_range(shape.Q, world, k)
        a, d, b = sh.get_kb(limit - first)
        assert np.array_equal(a, A[first:limit]) and np.array_equal(d, D[first:limit]) and np.array_equal(b, B), k
    close_all([whole] + shards)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_pack_changes_nothing(name, factory):
    shape, world = SHAPES[name], 3
    rounds = plan(shape, world)
    shards = [shape.engine(factory, *pdist.shard_range(shape.Q, world, r)) for r in range(world)]
    quizzes = shards[0].start_quiz_batch(N_QUIZZES)
    bounds = pdist.shard_bounds(shape.Q, world)
    answers = answers_of(shape, 0)
    for k, sh in enumerate(shards):
        if k > 0:
            assert sh.start_quiz_batch(N_QUIZZES) == quizzes
        for quiz, q in zip(quizzes, rounds[0]):
            sh.set_active_question(quiz, q)
        before = [sh.get_priors(q) for q in quizzes]
        lists = [listing(sh, q) for q in quizzes[:4]]
        first_pkg = package(sh, N_QUIZZES, name)
        sh.pack_answer_posteriors(quizzes, answers, first_pkg.data_ptr())
        sh.synchronize()
        assert [sh.get_active_question_id(q) for q in quizzes] == rounds[0]
        for q, want in zip(quizzes, before):
            assert np.array_equal(sh.get_priors(q), want), (k, q)
        assert [listing(sh, q) for q in quizzes[:4]] == lists
        again = package(sh, N_QUIZZES, name)
        sh.pack_answer_posteriors(quizzes, answers, again.data_ptr())
        sh.synchronize()
        got, second = first_pkg.cpu().numpy(), again.cpu().numpy()
        assert got.tobytes() == second.tobytes(), k                  # identical bytes, the zeros behind T among them
        for i, q in enumerate(rounds[0]):
            if pdist.owner_in(bounds, q) == k:
                assert got[i, :shape.T].sum() > 0.99 and not got[i, shape.T:].any(), (k, i)
            else:
                assert not got[i].any(), (k, i)                      # a slot of a question the shard does not hold stays zero
    close_all(shards)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_world_of_one(name, factory):
    shape = SHAPES[name]
    rounds = plan(shape, 1)
    check_plan(rounds, shape, 1)
    whole, twin = shape.engine(factory, 0, shape.Q), shape.engine(factory, 0, shape.Q)
    quizzes = whole.start_quiz_batch(N_QUIZZES)
    assert twin.start_quiz_batch(N_QUIZZES) == quizzes
    for r, qs in enumerate(rounds):
        for e in (whole, twin):
            for quiz, q in zip(quizzes, qs):
                e.set_active_question(quiz, q)
        twin.record_answer_batch(quizzes, answers_of(shape, r))
        pack_and_consume([whole], quizzes, answers_of(shape, r), name)
        for quiz in quizzes:
            assert np.array_equal(whole.get_priors(quiz), twin.get_priors(quiz)), (r, quiz)
    close_all([whole, twin])


def test_refusals_change_nothing_and_name_the_entry(factory):
    shape, world = SHAPES["gaps37x5x101"], 3
    rounds = plan(shape, world)
    shards = [shape.engine(factory, *pdist.shard_range(shape.Q, world, r)) for r in range(world)]
    answers = answers_of(shape, 0)
    for sh in shards:
        quizzes = sh.start_quiz_batch(N_QUIZZES)
        for quiz, q in zip(quizzes, rounds[0]):
            sh.set_active_question(quiz, q)
        sh.set_active_question(quizzes[7], -1)
        state = lambda: ([sh.get_active_question_id(q) for q in quizzes], [sh.get_priors(q).tobytes() for q in quizzes],   # noqa: E731
                         sh.get_option("posterior_packs"), sh.get_option("posteriors_taken"))
        before = state()
        pkg = package(sh, N_QUIZZES)
        with pytest.raises(interop.PqaException, match="Batch entry 7: .*doesn't have an active question"):
            sh.pack_answer_posteriors(quizzes, answers, pkg.data_ptr())
        sh.set_active_question(quizzes[7], shape.Q + 3)
        with pytest.raises(interop.PqaException, match="Batch entry 7: .*invalid active question"):
            sh.pack_answer_posteriors(quizzes, answers, pkg.data_ptr())
        sh.set_active_question(quizzes[7], -1)
        good, good_answers = quizzes[:7], answers[:7]
        with pytest.raises(interop.PqaException, match="Batch entry 4: .*appears twice"):
            sh.pack_answer_posteriors(good[:4] + [good[1]], good_answers[:5], pkg.data_ptr())
        with pytest.raises(interop.PqaException, match="Batch entry 2: .*Answer index"):
            sh.pack_answer_posteriors(good, good_answers[:2] + [shape.K] + good_answers[3:], pkg.data_ptr())
        with pytest.raises(interop.PqaException, match="Batch entry 3: "):
            sh.pack_answer_posteriors(good[:3] + [9999], good_answers[:4], pkg.data_ptr())
        with pytest.raises(interop.PqaException, match="Batch size is out of range"):
            sh.pack_answer_posteriors(list(range(257)), [0] * 257, pkg.data_ptr())
        with pytest.raises(interop.PqaException, match="packed no posteriors"):          # consume without a pack
            sh.record_answer_batch_from_posteriors(good, good_answers, pkg.data_ptr())
        sh.synchronize()
        assert not pkg.any().item()                                  # nothing was launched by any refused pack
        assert state() == before
        # consume with another batch than the packed one
        sh.pack_answer_posteriors(good, good_answers, pkg.data_ptr())
        with pytest.raises(interop.PqaException, match="WrongMode|another batch"):
            sh.record_answer_batch_from_posteriors(good[:6], good_answers[:6], pkg.data_ptr())
        other = [(a + 1) % shape.K for a in good_answers]
        with pytest.raises(interop.PqaException, match="another batch"):
            sh.record_answer_batch_from_posteriors(good, other, pkg.data_ptr())
        # ... and after one quiz of the batch took a SetActiveQuestion to another question in between
        sh.set_active_question(good[2], rounds[1][2])
        with pytest.raises(interop.PqaException, match="active question since"):
            sh.record_answer_batch_from_posteriors(good, good_answers, pkg.data_ptr())
        sh.set_active_question(good[2], rounds[0][2])
        sh.record_answer_batch_from_posteriors(good, good_answers, pkg.data_ptr())          # its question put back: every quiz is as the pack saw it
        assert [sh.get_active_question_id(q) for q in good] == [-1] * 7
        with pytest.raises(interop.PqaException, match="packed no posteriors"):          # a pack is consumed once
            sh.record_answer_batch_from_posteriors(good, good_answers, pkg.data_ptr())
    close_all(shards)


def test_consume_after_the_quiz_moved_on(factory):
    shape = SHAPES["gaps37x5x101"]
    eng = shape.engine(factory, 0, shape.Q)
    quiz = eng.start_quiz()
    pkg = package(eng, 1)
    with pytest.raises(interop.PqaException) as info:
        eng.record_answer_batch_from_posteriors([quiz], [0], pkg.data_ptr())
    assert "Can't record from these posteriors" in str(info.value)
    eng.set_active_question(quiz, 4)
    eng.pack_answer_posteriors([quiz], [1], pkg.data_ptr())
    assert eng.record_answer(quiz, 1) is None                        # the quiz moves on by itself: its posterior has changed since
    eng.set_active_question(quiz, 4)
    with pytest.raises(interop.PqaException, match="changed its posterior"):
        eng.record_answer_batch_from_posteriors([quiz], [1], pkg.data_ptr())
    eng.close()


@pytest.mark.parametrize("name", ["gaps37x5x101", "float120x5x1000", "long64x5x20000"])
def test_flag_form_and_registered_host_package(name, factory):
    shape, world = SHAPES[name], 3
    rounds = plan(shape, world)
    whole, shards = shape.world(factory, world)
    engines = [whole] + shards
    quizzes = whole.start_quiz_batch(N_QUIZZES)
    answers = answers_of(shape, 0)
    for e in engines:
        if e is not whole:
            assert e.start_quiz_batch(N_QUIZZES) == quizzes
        for quiz, q in zip(quizzes, rounds[0]):
            e.set_active_question(quiz, q)
    slot = shards[0].posterior_slot_bytes()
    size = N_QUIZZES * slot + 64
    seg = mmap.mmap(-1, size)
    address = ctypes.addressof(ctypes.c_char.from_buffer(seg))
    dev = interop.host_register(address, size)
    try:
        for k, sh in enumerate(shards):
            device_pkg = package(sh, N_QUIZZES, name)
            sh.pack_answer_posteriors(quizzes, answers, device_pkg.data_ptr())
            seg[:size] = bytes(size)
            sh.pack_answer_posteriors(quizzes, answers, dev, dev + N_QUIZZES * slot, 41 + k)
            sh.synchronize()
            assert int(np.frombuffer(seg, dtype=np.uint64, count=1, offset=N_QUIZZES * slot)[0]) == 41 + k
            assert bytes(seg[:N_QUIZZES * slot]) == device_pkg.cpu().numpy().tobytes(), k
        # the flag alone: a shard that holds none of the batch's questions still publishes it, and writes nothing else
        bounds = pdist.shard_bounds(shape.Q, world)
        foreign = [i for i, q in enumerate(rounds[0]) if pdist.owner_in(bounds, q) != 0]
        seg[:size] = bytes(size)
        shards[0].pack_answer_posteriors([quizzes[i] for i in foreign], [answers[i] for i in foreign], dev, dev + N_QUIZZES * slot, 7)
        shards[0].synchronize()
        assert int(np.frombuffer(seg, dtype=np.uint64, count=1, offset=N_QUIZZES * slot)[0]) == 7
        assert bytes(seg[:N_QUIZZES * slot]) == bytes(N_QUIZZES * slot)
        # every shard into the host package, every shard consumes it: staged to the device first, or read in place
        seg[:size] = bytes(size)
        for sh in shards:
            sh.pack_answer_posteriors(quizzes, answers, dev)
        for sh in shards:
            sh.synchronize()
        whole.record_answer_batch(quizzes, answers)
        for k, sh in enumerate(shards):
            sh.set_option("rows_stage", k % 2)
            staged0 = sh.get_option("rows_staged")
            sh.record_answer_batch_from_posteriors(quizzes, answers, dev)
            assert sh.get_option("rows_staged") - staged0 == k % 2
            for quiz in quizzes:
                assert np.array_equal(sh.get_priors(quiz), whole.get_priors(quiz)), (k, quiz)
    finally:
        close_all(engines)
        interop.host_unregister(address)


def test_one_process_sharded_engine_refuses(factory, monkeypatch):
    monkeypatch.setenv("PQA_DEVICES", "0,0")        # (two shards side by side on the one device, as the tools make theirs)
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(5, 37, 101, init_amount=0.1))
    assert err is None and eng.get_option("shards") == 2
    quiz = eng.start_quiz()
    assert eng.posterior_slot_bytes() == -1
    for call in (lambda: eng.pack_answer_posteriors([quiz], [0], 16), lambda: eng.record_answer_batch_from_posteriors([quiz], [0], 16)):
        with pytest.raises(interop.PqaException, match="Posterior packages are for shards"):
            call()
    eng.close()
