"""How a selection reaches the waiting host: the sweep's finisher (csrc/eval_kernels.hip: fused_select) reduces the workgroups'
records with a DPP / permlane butterfly (wave_best) and publishes the winner without a release fence -- the engine's own
selections as one packed, self-tagged 16-byte record (csrc/select_record.h; a record per path: launched, graph-replayed,
resident), outside readers' as write-through stores with the flag behind their acknowledgement (csrc/pqa_device.h:
host_publish).  None of it may change a pick, a priority or what a caller of the C ABI gets when nothing is left, and no call
may ever be handed the previous call's answer.

The values of the parent commit (what "nothing left" returns; the sampled selector's picks) are recorded by
    python tests/test_gpu_publish.py record tests/golden/publish/parent.json
run on a GPU from a tree of that commit."""
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":          # the recorder: the package of the tree it is started in, the helpers beside this file
    sys.path[:0] = [os.getcwd(), os.path.dirname(os.path.abspath(__file__))]

import cases
from probqa_amd import interop

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "publish", "parent.json")
# what a selection with nothing left returned at the parent commit, through every path: the reference's error, no question id
NOTHING_LEFT = "error: [Engine has run out of questions] message=[Found no unasked question that is not in a gap.] [nullptr]"
CUBES = [(1, 2, 2), (5, 5, 130), (7, 5, 1000)]      # (Q, K, T)
SAMPLED_RNDS = [0, 1, 0x123456789ABCDEF, 0x7FFFFFFFFFFFFFFF, 0x8000000000000000, 0xC0FFEE0DDBA11, 0xFEDCBA9876543210, 0xFFFFFFFFFFFFFFFF]


def make(factory, Q, K, T, seed=31, tie=False):
    """An argmax engine over a synthetic cube; tie: a second question gets the rows of the best one -- two equal best questions."""
    case = cases.Case("publish", K, Q, T, seed=seed)
    A, D, B = case.kb()
    eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T, init_amount=case.init))
    assert err is None and eng is not None, err
    eng.set_option("workers", cases.WORKERS)
    eng.set_option("select", 1)
    eng.set_kb(A, D, B)
    if tie:
        quiz = eng.start_quiz()
        best = int(np.argmax(eng.eval_priorities(quiz)))
        eng.release_quiz(quiz)
        twin = (best + 2) % Q
        A, D = A.copy(), D.copy()
        A[twin], D[twin] = A[best], D[best]
        eng.set_kb(A, D, B)
    return eng


def expected_pick(eng, quiz, asked=()):
    pri = eng.eval_priorities(quiz).copy()
    pri[list(asked)] = -np.inf
    want = int(np.argmax(pri))          # (the first of equal maxima: the lowest index)
    return want, pri


@pytest.mark.parametrize("grid", [0, 1, 2, 3])
@pytest.mark.parametrize("cube", CUBES + ["tie"], ids=lambda c: c if isinstance(c, str) else "%dx%dx%d" % c)
def test_finisher_shapes(factory, cube, grid):
    """A lone finisher (one workgroup), every workgroup striding over several questions, the finisher holding the most: the
    question and the priority delivered are the argmax of EvalPriorities for the same quiz, the lowest index among equals."""
    import torch

    tie = cube == "tie"
    Q, K, T = (5, 5, 130) if tie else cube
    eng = make(factory, Q, K, T, tie=tie)
    try:
        eng.set_option("eval_max_grid", grid)
        quiz = eng.start_quiz()
        want, pri = expected_pick(eng, quiz)
        if tie:
            twins = np.flatnonzero(pri == pri[want])
            print("tie: questions", twins.tolist(), "priority", pri[want])
            assert len(twins) == 2 and want == twins[0]
        got = eng.next_question_argmax(quiz)
        print("grid", grid, "cube", cube, "pick", got, "expected", want)
        assert got == want
        # ... and the record itself (priority and index), through the entry point that hands out both
        buf = torch.zeros(4, dtype=torch.int64).pin_memory()
        eng.enqueue_select_argmax_flag(quiz, buf.data_ptr(), buf.data_ptr() + 16, 77)
        eng.synchronize()
        assert int(buf[2]) == 77
        assert int(buf[1]) == want
        assert buf[:1].numpy().view(np.float64)[0] == pri[want]
    finally:
        eng.close()


def via(eng, path, quiz):
    eng.set_option("server", 1 if path == "resident" else 0)
    eng.set_option("use_graph", 1 if path == "graph" else 0)
    return eng.next_question(quiz)


@pytest.mark.parametrize("mode", ["resident", "graph", "switching"])
def test_no_stale_answer(factory, mode):
    """Two quizzes of one engine whose winners differ by one recorded answer, asked in turn 2000 times: every call gets its own
    quiz's pick -- a record or a flag left by the call before (or by another path) never passes for this call's."""
    eng = make(factory, 48, 4, 300, seed=130)
    try:
        qa = eng.start_quiz()
        want_a, _ = expected_pick(eng, qa)
        qb = eng.resume_quiz([interop.AnsweredQuestion(want_a, 2)])
        want_b, _ = expected_pick(eng, qb, asked=[want_a])
        assert want_a != want_b
        paths = ("launch", "graph", "resident")
        wrong = []
        for i in range(2000):
            path = paths[(i // 50) % 3] if mode == "switching" else mode
            quiz, want = ((qa, want_a), (qb, want_b))[i & 1]
            got = via(eng, path, quiz)
            if got != want:
                wrong.append((i, path, got, want))
        assert not wrong, wrong[:10]
    finally:
        eng.close()


def nothing_left(factory):
    """Every question asked or a gap, then a selection through each path: what the caller gets (a question id or the error text)."""
    eng = make(factory, 5, 5, 130)
    out = {}
    try:
        eng.set_question_gaps([1, 3])
        quiz = eng.resume_quiz([interop.AnsweredQuestion(0, 1), interop.AnsweredQuestion(2, 4), interop.AnsweredQuestion(4, 0)])
        for path in ("launch", "graph", "resident"):
            try:
                out[path] = via(eng, path, quiz)
            except interop.PqaException as e:
                out[path] = "error: %s" % e
    finally:
        eng.close()
    return out


def sampled_picks(factory, host_sampled):
    """The reference's sampled selector (select = 0) on the 5 x 5 x 130 cube: three picks of a quiz per random number."""
    eng = make(factory, 5, 5, 130)
    picks = []
    try:
        eng.set_option("select", 0)
        eng.set_option("host_sampled", host_sampled)
        for n, rnd in enumerate(SAMPLED_RNDS):
            quiz = eng.start_quiz()
            for step in range(3):
                q = eng.next_question_sampled(quiz, (rnd + step * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
                picks.append(q)
                eng.record_answer(quiz, (q + n + step) % 5)
            eng.release_quiz(quiz)
    finally:
        eng.close()
    return picks


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_nothing_left_returns_what_it_did(factory):
    """Every question asked or a gap: the finisher's "nothing left" reaches the caller as it did at the parent commit."""
    got = nothing_left(factory)
    print(got)
    assert got == {"launch": NOTHING_LEFT, "graph": NOTHING_LEFT, "resident": NOTHING_LEFT}
    assert got == golden()["nothing_left"]


@pytest.mark.parametrize("host_sampled", [1, 0])
def test_sampled_selector_picks(factory, host_sampled):
    got = sampled_picks(factory, host_sampled)
    print(got)
    assert got == golden()["sampled_picks"][str(host_sampled)]


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "record":
        raise SystemExit(__doc__)
    f = interop.PqaEngineFactory()
    rec = {"nothing_left": nothing_left(f), "sampled_picks": {str(h): sampled_picks(f, h) for h in (1, 0)}}
    with open(sys.argv[2], "w") as out:
        json.dump(rec, out, indent=1)
        out.write("\n")
    print(json.dumps(rec))
