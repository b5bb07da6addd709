"""The buffers the batched listings share -- device scratch that only grows, pinned result lines, the staged package -- driven on
purpose: ONE engine serves a sequence of requests that grows, shrinks and grows again, across the 256-source chunk and the 256-record
switch between the device's listing and the host's prefix.  Every listing is held, record for record and bit for bit, to the listing
of the vector the engine itself returns in the same state (value descending, id ascending, the source, the gaps and what is not > 0
left out: listing_of_row); no tolerance is involved, the vectors' own accuracy is other tests' subject.
(K, Q, T) = (3, 40, 70): a row's tail lies off the 16-double pitch."""
import ctypes
import mmap

import numpy as np
import pytest

from probqa_amd import interop
from test_gpu_similar_targets import listing_of_row, make_engine, records

pytestmark = pytest.mark.gpu

K, Q, T = 3, 40, 70
TGAPS, QGAPS = (5, 69), (11,)
VALID_T = [t for t in range(T) if t not in TGAPS]
VALID_Q = [q for q in range(Q) if q not in QGAPS]
STEPS = [(1, 1), (5, 7), (257, 3), (2, 256), (3, 257), (1, 1), (257, 256)]   # (sources, max_count)
N_QUIZZES = 256


def cycled(ids, n):
    return [ids[i % len(ids)] for i in range(n)]


def listing(row, max_count):
    return listing_of_row(row, -1, max_count)   # (no source to leave out)


def play(eng, n):
    """n quizzes after 0..4 answers each"""
    rng = np.random.default_rng(3)
    AQ = interop.AnsweredQuestion
    return eng.resume_quiz_batch([[AQ(int(q), int(rng.integers(K))) for q in rng.permutation(VALID_Q)[:j % 5]] for j in range(n)])


def test_grow_shrink_grow(factory):
    eng = make_engine(factory, K, Q, T, TGAPS, QGAPS)
    quizzes = play(eng, N_QUIZZES)
    among = [VALID_T[::7][:9], VALID_T]
    assert len(among[0]) == 9
    for step, (n, max_count) in enumerate(STEPS):
        at = (step, n, max_count)
        # ---- sources
        src = cycled(VALID_T, n)
        rows = eng.eval_target_similarity(src)
        got = eng.list_similar_targets_batch(src, max_count)
        assert [records(x) for x in got] == [listing_of_row(rows[i], s, max_count) for i, s in enumerate(src)], at
        src = cycled(VALID_Q, n)
        rows = eng.eval_question_redundancy(src)
        got = eng.list_redundant_questions_batch(src, max_count)
        assert got == [listing_of_row(rows[i], s, max_count) for i, s in enumerate(src)], at
        # ---- quizzes
        ids = quizzes[:min(n, N_QUIZZES)]
        priors = [eng.get_priors(quiz) for quiz in ids]
        for exact in (1, 0):   # (no two targets of a posterior tie here: the reference's order among equals is the id's)
            eng.set_option("top_exact", exact)
            got = eng.list_top_targets_batch(ids, max_count)
            assert [records(x) for x in got] == [listing(p, max_count) for p in priors], (at, exact)
        pri = eng.eval_priorities_batch(ids)   # (the batched sweep's values: what the batched listing lists)
        got = eng.list_top_questions_batch(ids, max_count)
        assert got == [listing(pri[i], max_count) for i in range(len(ids))], at
        for k, ts in enumerate(among):
            got, mass = eng.list_top_targets_among_batch(ids, [ts], max_count, list_of=[0] * len(ids))
            assert len(mass) == len(ids)
            for i, p in enumerate(priors):
                sub = np.zeros(T)
                sub[ts] = p[ts]
                assert records(got[i]) == listing(sub, max_count), (at, k, i)
    eng.close()


def test_staged_host_packages(factory):
    """The from-package calls with the package in registered host memory under option rows_stage: one staging per call, the same
    records."""
    eng = make_engine(factory, K, Q, T, TGAPS, QGAPS)
    eng.set_option("rows_stage", 1)
    sim_slot, red_slot = eng.posterior_slot_bytes(), eng.question_weight_slot_bytes()
    assert sim_slot == 80 * 8 and red_slot == K * 80 * 8
    seg = mmap.mmap(-1, (256 * red_slot + 4095) // 4096 * 4096)
    address = ctypes.addressof(ctypes.c_char.from_buffer(seg))
    dev = interop.host_register(address, len(seg))
    families = [
        (VALID_T, eng.eval_target_similarity, eng.pack_target_similarity_sums, eng.list_similar_targets_from_sums, lambda x: [records(r) for r in x]),
        (VALID_Q, eng.eval_question_redundancy, eng.pack_question_weights, eng.list_redundant_questions_from_weights, lambda x: x),
    ]
    try:
        for step in (1, 2, 1):
            n, max_count = STEPS[step]
            for valid, evaluate, pack, list_from, plain in families:
                src = cycled(valid, n)
                rows = evaluate(src)
                for first in range(0, n, 256):
                    chunk = src[first:first + 256]
                    ctypes.memset(address, 0, len(seg))   # (a question-weight package is summed into: zero-filled)
                    pack(chunk, dev)
                    eng.synchronize()
                    staged0 = eng.get_option("rows_staged")
                    got = plain(list_from(chunk, dev, max_count))
                    assert eng.get_option("rows_staged") == staged0 + 1, (step, first)
                    assert got == [listing_of_row(rows[first + i], s, max_count) for i, s in enumerate(chunk)], (step, first)
    finally:
        eng.close()
        interop.host_unregister(address)
