""".kb files per shard and in either precision, on the device: a file of one number type loaded into an engine of the other (the
rows pass through convert_rows_kernel), saved in the other, loaded as shards -- a seek to each shard's two blocks -- and saved shard
by shard in place.  Nothing here has a tolerance: every comparison is bit for bit against numpy's rounding (astype(float32) rounds to
nearest even, as the kernel's conversion does) or byte for byte against the engine's own SaveKB.

The shapes are chosen for the dense side's alignment and the row forms, not for size: T = 2 and 3 (rows shorter than one quad), 67 and
101 (odd: every other dense row starts 8 bytes off a 16-byte line, the fp32 ones 4 or 12), 1025 (one element past a quad boundary), 4096
(aligned throughout), 16387 (just past the long-row boundary, three tail elements)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ranks_common as rc
from probqa_amd import dist as pdist
from probqa_amd import interop

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = interop.PrecisionType
# Q x K x T.  The smallest row is T = 2: no engine, here or in the reference (PqaEngineBaseFactory.cpp:29-42), exists with fewer than two
# targets, so a 3 x 2 x 1 knowledge base can be neither created nor loaded -- test_one_target_is_no_knowledge_base holds that instead.
SHAPES = [(3, 2, 2), (5, 3, 3), (50, 4, 67), (37, 5, 101), (8, 5, 1025), (16, 5, 4096), (3, 2, 16387)]
GAPS = {(37, 5, 101): ([4, 36, 17], [0, 100, 33])}
F32 = dict(prec_type=P.FLOAT, prec_exponent=8, prec_mantissa=24)


def arrays(Q, K, T, seed=5):
    """seeded non-integers, so that rounding to fp32 shows; a tie that rounds down, one that rounds up, and a value that is
    subnormal in fp32, at both ends of a row and wherever T leaves room in between"""
    rng = np.random.default_rng(seed + 1000 * Q + T)
    A = rng.uniform(0.01, 9.0, size=(Q, K, T))
    D = A.sum(axis=1) * rng.uniform(0.9, 1.1, size=(Q, T))
    B = rng.uniform(0.5, 7.0, size=T)
    special = [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1e-40, 7.0 + 2.0 ** -22, 3e-39]
    flat = A.reshape(-1)
    for i, v in enumerate(special):
        flat[(i * 7919) % flat.size] = abs(v)
        D.reshape(-1)[(i * 104729 + 1) % D.size] = abs(v) + 2.0
    A[-1, -1, -1] = 1.0 + 2.0 ** -24
    A[0, 0, 0] = 1.0 + 3 * 2.0 ** -24
    B[-1] = 1.0 + 3 * 2.0 ** -24
    return A, D, B


def rounded(x):
    return x.astype(np.float32).astype(np.float64)


def make_engine(factory, Q, K, T, f32, kb, gaps=None):
    eng = factory.create_hip_engine(interop.EngineDefinition(K, Q, T, init_amount=0.1, **(F32 if f32 else {})), 0, Q, 0)
    eng.set_kb(*kb)
    if gaps:
        eng.set_question_gaps(gaps[0])
        eng.set_target_gaps(gaps[1])
    return eng


_files = {}


@pytest.fixture(scope="module")
def kb_file(factory, tmp_path_factory):
    """the .kb file of a shape in one precision, written once by an engine of that precision and shared: (path, A, D, B as the file holds them)"""
    def get(shape, f32):
        key = (shape, f32)
        if key not in _files:
            Q, K, T = shape
            A, D, B = arrays(Q, K, T)
            if f32:
                A, D, B = rounded(A), rounded(D), rounded(B)
            eng = make_engine(factory, Q, K, T, f32, (A, D, B), GAPS.get(shape))
            path = str(tmp_path_factory.mktemp("kb") / ("%dx%dx%d_%s.kb" % (Q, K, T, "f32" if f32 else "f64")))
            eng.save_kb(path, False)
            eng.close()
            _files[key] = (path, A, D, B)
        return _files[key]
    return get


def packed_rows(eng, Q, K):
    """every question / answer's slot of a row package, as bytes: the two rows WITH the cube's padding"""
    import torch

    pairs = [interop.AnsweredQuestion(q, k) for q in range(Q) for k in range(K)]
    buf = torch.zeros(len(pairs) * eng.answer_row_slot_bytes(), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.pack_answer_rows(pairs, buf.data_ptr())
    eng.synchronize()
    return buf.cpu().numpy().tobytes()


def serve(eng, Q, K, gaps):
    """a quiz with one answer: its priorities and its pick"""
    quiz = eng.start_quiz()
    q0 = next(q for q in range(Q) if not gaps or q not in gaps[0])
    eng.set_active_question(quiz, q0)
    eng.record_answer(quiz, K - 1)
    return eng.eval_priorities(quiz), eng.next_question_argmax(quiz)


def same_engine(a, b, Q, K, gaps):
    for x, y in zip(a.get_kb(), b.get_kb()):
        assert np.array_equal(x, y)
    assert packed_rows(a, Q, K) == packed_rows(b, Q, K)            # the slot carries the padding: it was not written
    (pa, sa), (pb, sb) = serve(a, Q, K, gaps), serve(b, Q, K, gaps)
    assert np.array_equal(pa, pb, equal_nan=True) and sa == sb


def test_one_target_is_no_knowledge_base(factory, tmp_path):
    """3 x 2 x 1: refused at creation (Insufficient engine dimensions) and, as a file, at the header"""
    import struct

    eng, err = factory.create_cpu_engine(interop.EngineDefinition(2, 3, 1))
    assert eng is None and "Insufficient engine dimensions" in err.to_string(True)
    path = str(tmp_path / "3x2x1.kb")
    open(path, "wb").write(struct.pack("<QqqqQ", 3 | (53 << 4) | (11 << 32), 2, 3, 1, 0) + b"\0" * 8 * (3 * 3 + 1) + b"\0" * 80)
    for prec in (None, P.FLOAT):
        with pytest.raises(interop.PqaException, match="File operation failed"):
            factory.load_hip_engine(path, prec)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_double_file_into_float_engine(factory, kb_file, shape):
    Q, K, T = shape
    path, A, D, B = kb_file(shape, False)
    eng = factory.load_hip_engine(path, P.FLOAT)
    assert eng.get_option("precision") == P.FLOAT.value
    gA, gD, gB = eng.get_kb()
    assert np.array_equal(gA, rounded(A)) and np.array_equal(gD, rounded(D)) and np.array_equal(gB, rounded(B))
    assert not np.array_equal(gA, A)                               # (the rounding shows)
    twin = make_engine(factory, Q, K, T, True, (A, D, B), GAPS.get(shape))
    same_engine(eng, twin, Q, K, GAPS.get(shape))
    eng.close(); twin.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_float_file_into_double_engine(factory, kb_file, shape):
    Q, K, T = shape
    path, A, D, B = kb_file(shape, True)
    eng = factory.load_hip_engine(path, P.DOUBLE)
    assert eng.get_option("precision") == P.DOUBLE.value
    gA, gD, gB = eng.get_kb()
    assert np.array_equal(gA, A) and np.array_equal(gD, D) and np.array_equal(gB, B)      # the widening is exact
    twin = make_engine(factory, Q, K, T, False, (A, D, B), GAPS.get(shape))
    same_engine(eng, twin, Q, K, GAPS.get(shape))
    eng.close(); twin.close()


@pytest.mark.parametrize("shape", [(5, 3, 3), (37, 5, 101), (3, 2, 16387)], ids=lambda s: "%dx%dx%d" % s)
def test_save_in_the_other_precision(factory, kb_file, tmp_path, shape):
    Q, K, T = shape
    path64, A, D, B = kb_file(shape, False)
    path32 = kb_file(shape, True)[0]
    rows = Q * (K + 1) * T + T
    # a Float engine saved as Double: the header and size of a Double file, and today's loader reads the widened values
    ef = factory.load_hip_engine(path32)
    assert ef.get_option("precision") == P.FLOAT.value
    as64 = str(tmp_path / "as64.kb")
    ef.save_kb_as(as64, P.DOUBLE)
    assert open(as64, "rb").read(40)[:8] == open(path64, "rb").read(8)
    assert os.path.getsize(as64) - os.path.getsize(path32) == 4 * rows and os.path.getsize(as64) == os.path.getsize(path64)
    back, err = factory.load_cpu_engine(as64)
    assert err is None and back.get_option("precision") == P.DOUBLE.value
    for x, y in zip(back.get_kb(), (rounded(A), rounded(D), rounded(B))):
        assert np.array_equal(x, y)
    # the engine's own precision: the bytes SaveKB writes
    own, plain = str(tmp_path / "own.kb"), str(tmp_path / "plain.kb")
    ef.save_kb_as(own, P.FLOAT)
    ef.save_kb(plain, False)
    assert open(own, "rb").read() == open(plain, "rb").read() == open(path32, "rb").read()
    ef.save_kb_as(own, None)
    assert open(own, "rb").read() == open(plain, "rb").read()
    # Double -> saved as Float -> loaded as Double -> saved as Float: the same bytes the second time
    ed = factory.load_hip_engine(path64)
    first, second = str(tmp_path / "first.kb"), str(tmp_path / "second.kb")
    ed.save_kb_as(first, P.FLOAT)
    again = factory.load_hip_engine(first, P.DOUBLE)
    again.save_kb_as(second, P.FLOAT)
    assert open(first, "rb").read() == open(second, "rb").read() == open(path32, "rb").read()
    for e in (ef, back, ed, again):
        e.close()


def load_shards(factory, path, world, precision=None):
    return [pdist.load_shard(factory, path, r, world, precision, device=0) for r in range(world)]


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("shape,prec", [((50, 4, 67), P.FLOAT), ((37, 5, 101), None), ((16, 5, 4096), P.FLOAT)], ids=["50x4x67-as-f32", "37x5x101-gaps", "16x5x4096-as-f32"])
def test_shards_of_one_file(factory, kb_file, shape, prec, world):
    Q, K, T = shape
    path = kb_file(shape, False)[0]
    whole = factory.load_hip_engine(path, prec)
    wA, wD, wB = whole.get_kb()
    quiz = whole.start_quiz()
    wpri = whole.eval_priorities(quiz)
    shards = load_shards(factory, path, world, prec)
    winners = []
    for r, sh in enumerate(shards):
        first, limit = pdist.shard_range(Q, world, r)
        assert (sh.get_option("q_first"), sh.get_option("local_questions"), sh.copy_dims().n_questions) == (first, limit - first, Q)
        sA, sD, sB = sh.get_kb(limit - first)
        assert np.array_equal(sA, wA[first:limit]) and np.array_equal(sD, wD[first:limit]) and np.array_equal(sB, wB)
        sq = sh.start_quiz()
        assert np.array_equal(sh.eval_priorities(sq, limit - first), wpri[first:limit], equal_nan=True)   # gaps included
        winners.append(sh.select_argmax_batch([sq]))
    assert pdist.pick_batch(np.stack(winners)) == pdist.pick_batch(np.stack([whole.select_argmax_batch([quiz])]))
    assert pdist.pick_batch(np.stack(winners)) == [whole.next_question_argmax(quiz)]
    for e in shards + [whole]:
        e.close()


@pytest.fixture(scope="module")
def edited_file(factory, tmp_path_factory):
    """a file whose gap lists and id ledgers are not trivial: questions and targets removed, added, compacted, removed again"""
    Q, K, T = 24, 5, 67
    eng = make_engine(factory, Q, K, T, False, arrays(Q, K, T, seed=9))
    eng.start_maintenance(True)
    eng.remove_questions([3, 17])
    eng.remove_targets([5])
    eng.add_qs_ts([interop.AddQuestionParam(0.3) for _ in range(4)], [interop.AddTargetParam(0.2) for _ in range(3)])
    eng.remove_questions([7, 20, 25])
    eng.compact()
    eng.remove_questions([2, 9, 20])
    eng.remove_targets([11, 68])
    eng.finish_maintenance()
    path = str(tmp_path_factory.mktemp("kb") / "edited.kb")
    eng.save_kb(path, False)
    dims = eng.copy_dims()
    eng.close()
    return path, dims


def training(dims):
    aq = interop.AnsweredQuestion
    q = dims.n_questions
    return [([aq(0, 1), aq(q - 1, 0), aq(5, 2)], 3, 1.5), ([aq(q // 2, 4), aq(q // 2, 4)], 8, 0.75), ([aq(1, 0), aq(q - 2, 3), aq(1, 2), aq(6, 1)], 3, 2.25)]


@pytest.mark.parametrize("world", [3, 8])
@pytest.mark.parametrize("load_as,save_as", [(None, None), (P.FLOAT, P.DOUBLE), (P.FLOAT, None)], ids=["f64", "f32-saved-f64", "f32"])
def test_shard_saves_in_place(factory, edited_file, tmp_path, world, load_as, save_as):
    path, dims = edited_file
    whole = factory.load_hip_engine(path, load_as)
    whole.train_batch(training(dims))
    want = str(tmp_path / "whole.kb")
    if save_as is None:
        whole.save_kb(want, False)
    else:
        whole.save_kb_as(want, save_as)
    shards = load_shards(factory, path, world, load_as)
    got = str(tmp_path / "shards.kb")
    open(got, "wb").write(b"\xee" * (os.path.getsize(want) + 4096))     # a stale, longer file: every byte is written or cut
    for sh in reversed(shards):                                          # (any order)
        sh.train_batch(training(dims))
        sh.save_kb_shard(got, save_as)
    assert open(got, "rb").read() == open(want, "rb").read()
    for e in shards + [whole]:
        e.close()


def test_refusals(factory, kb_file, tmp_path):
    shape = (37, 5, 101)
    Q, K, T = shape
    path = kb_file(shape, False)[0]

    def refused(**kw):
        with pytest.raises(interop.PqaException) as e:
            factory.load_hip_engine(kw.pop("path", path), kw.pop("precision", None), **kw)
        return str(e.value)

    assert "Index is out of range" in refused(q_first=30, n_local=8, device=0)           # a range beyond the file's Q
    assert "Index is out of range" in refused(q_first=37, n_local=1, device=0)
    assert "Insufficient engine dimensions" in refused(q_first=0, n_local=8, q_total=36, device=0)
    assert "The count is negative" in refused(q_first=0, n_local=-2, device=0)
    assert "Not implemented" in refused(precision=P.DOUBLE_PAIR)
    cut = str(tmp_path / "cut.kb")
    raw = open(path, "rb").read()
    open(cut, "wb").write(raw[:40 + Q * K * T * 8 + 11 * T * 8 + 4])                    # cut inside the mD block
    assert "shorter than the arrays" in refused(path=cut)
    assert "shorter than the arrays" in refused(path=cut, q_first=0, n_local=4, device=0)
    # a finite value that does not fit fp32: the load fails and says which array
    for name, offset in (("_sA", 40 + 8 * (2 * K * T + 70)), ("_mD", 40 + 8 * (Q * K * T + 36 * T + 100)), ("_vB", 40 + 8 * (Q * (K + 1) * T + 1))):
        big = str(tmp_path / ("big%s.kb" % name))
        data = bytearray(raw)
        data[offset:offset + 8] = np.float64(-1e300 if name == "_mD" else 1e300).tobytes()
        open(big, "wb").write(bytes(data))
        text = refused(path=big, precision=P.FLOAT)
        assert "array=" + name in text and "values=1" in text, text
        ok = factory.load_hip_engine(big)                                                # ... while the file's own precision takes it
        ok.close()
        if name == "_sA":   # the shard that holds the value fails, another one loads
            assert "array=_sA" in refused(path=big, precision=P.FLOAT, q_first=0, n_local=8, device=0)
            factory.load_hip_engine(big, P.FLOAT, q_first=8, n_local=8, device=0).close()
    # save_kb_as is for whole engines (as save_kb is); save_kb_shard on a whole engine is an equivalent of save_kb_as
    shard = factory.load_hip_engine(path, None, q_first=8, n_local=8, device=0)
    out = str(tmp_path / "out.kb")
    for call in (lambda: shard.save_kb_as(out, P.DOUBLE), lambda: shard.save_kb(out, False)):
        with pytest.raises(interop.PqaException, match="Not implemented"):
            call()
    assert not os.path.exists(out)
    with pytest.raises(interop.PqaException, match="Not implemented"):
        shard.save_kb_shard(out, P.FLOAT_PAIR)
    assert not os.path.exists(out)
    whole = factory.load_hip_engine(path)
    with pytest.raises(interop.PqaException, match="Not implemented"):
        whole.save_kb_as(out, P.ARBITRARY)
    assert not os.path.exists(out)
    whole.save_kb_shard(out)
    assert open(out, "rb").read() == raw
    # the engines are what they were, and the device is idle: they still serve
    quiz = shard.start_quiz()
    assert shard.select_argmax_batch([quiz]).shape[0] == 1
    assert whole.next_question_argmax(whole.start_quiz()) >= 0
    whole.synchronize(); shard.synchronize()
    whole.close(); shard.close()


_SHARDED_CHILD = r"""
import json, sys
from probqa_amd import interop
P = interop.PrecisionType
path, out = sys.argv[1], sys.argv[2]
f = interop.PqaEngineFactory()
eng = f.load_hip_engine(path, P.FLOAT)
assert eng.get_option("shards") == 2 and eng.get_option("precision") != P.DOUBLE.value
quiz = eng.start_quiz()
eng.set_active_question(quiz, 0)
eng.record_answer(quiz, 1)
picks = [eng.next_question_argmax(quiz)]
eng.record_answer(quiz, 0)
picks.append(eng.next_question_argmax(quiz))
eng.save_kb_as(out, P.DOUBLE)
try:
    eng.save_kb_shard(out + ".x")
    refused = False
except interop.PqaException:
    refused = True
print(json.dumps({"picks": picks, "refused": refused}))
"""


def test_one_process_sharded_engine(factory, kb_file, tmp_path):
    shape = (50, 4, 67)
    path = kb_file(shape, False)[0]
    single = factory.load_hip_engine(path, P.FLOAT)
    quiz = single.start_quiz()
    single.set_active_question(quiz, 0)
    single.record_answer(quiz, 1)
    picks = [single.next_question_argmax(quiz)]
    single.record_answer(quiz, 0)
    picks.append(single.next_question_argmax(quiz))
    want = str(tmp_path / "single.kb")
    single.save_kb_as(want, P.DOUBLE)
    got = str(tmp_path / "sharded.kb")
    env = dict(os.environ, PQA_DEVICES="0,0", PQA_SELECT="argmax", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _SHARDED_CHILD, path, got], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["picks"] == picks and res["refused"]
    assert open(got, "rb").read() == open(want, "rb").read()
    # a shard together with PQA_DEVICES is refused
    code = ("from probqa_amd import interop\n"
            "try:\n    interop.PqaEngineFactory().load_hip_engine(%r, None, q_first=0, n_local=8, device=0)\n    print('LOADED')\n"
            "except interop.PqaException as e:\n    print('REFUSED', e)\n" % path)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, text=True)
    assert "REFUSED" in r.stdout and "LOADED" not in r.stdout, r.stdout[-2000:]
    single.close()


def _rank_main(rank, world, port, path, out_path, records):
    import torch.distributed as dist

    rc.init_group("gloo", rank, world, port)
    aq = interop.AnsweredQuestion
    eng = pdist.load_shard(interop.PqaEngineFactory(), path, rank, world, P.FLOAT, device=0)
    eng.train_batch([([aq(q, a) for q, a in pairs], t, amount) for pairs, t, amount in records])
    pdist.save_kb(eng, out_path, rank, world, precision=P.DOUBLE)
    dist.barrier()
    eng.close()
    dist.destroy_process_group()
    return {"ok": True}


def test_two_processes_over_gloo(factory, edited_file, tmp_path):
    path, dims = edited_file
    records = [([(a.i_question, a.i_answer) for a in aqs], t, amount) for aqs, t, amount in training(dims)]
    whole = factory.load_hip_engine(path, P.FLOAT)
    whole.train_batch(training(dims))
    want = str(tmp_path / "whole.kb")
    whole.save_kb_as(want, P.DOUBLE)
    whole.close()
    got = str(tmp_path / "ranks.kb")
    results = rc.run_ranks(_rank_main, 2, (2, rc.free_port(), path, got, records), timeout_s=240)
    assert results == {0: {"ok": True}, 1: {"ok": True}}, results
    assert open(got, "rb").read() == open(want, "rb").read()


def test_kb_convert_bench_tool(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kb_convert_bench.py"), "64", "5", "1001", "1", str(tmp_path)], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    row = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    for leg in ("a_load_same", "a_save_same", "b_load_convert", "b_save_convert", "c_getkb_setkb", "d_eight_shard_loads"):
        assert row["gbps"][leg]["median"] > 0, row
    assert row["file_bytes"] == 40 + 8 * (64 * 6 * 1001 + 1001) + 8 * 2 + 3 * 16 + 8 * (64 + 1001)
