"""The cases of tests/test_gpu_deep.py qualify, shown on the oracle alone: their posteriors do walk through the subnormal range and end
mostly at 0 with one element near 1, the oracle's priorities stay usable there, and enough of the landmark steps have a decided argmax
that the GPU test's selection comparisons are not skipped.  Conditions, not measurements."""
import numpy as np
import pytest

import cases
import deep_cases as dc

CASES = [(name, False) for name in dc.TABLE if name != "d17000r"] + [("d1000", True)]       # (True: on the cube rounded to fp32, a Float engine's)


@pytest.mark.parametrize("name,f32", CASES, ids=["%s%s" % (n, "_f32" if f else "") for n, f in CASES])
def test_case_qualifies(name, f32):
    case = dc.get(name)
    K, Q, T, depth = dc.TABLE[name][:4]
    assert (case.K, case.Q, case.T, len(case.answers)) == (K, Q, T, depth)
    assert case.hidden == T // 2 + 17 and case.q_offset == min(max(case.hidden - Q // 2, 0), T - Q)
    assert case.answers[0][0] == case.hidden - case.q_offset and len({q for q, _ in case.answers}) == depth
    tr = dc.trace(case, f32)
    marks = dc.landmarks(case, f32)
    assert len(marks) <= 12 and marks[0] == 0 and marks[-1] == depth and 40 in marks
    assert tr.first_sub is not None and tr.first_zero is not None and tr.first_sub - 1 in marks and tr.first_zero in marks
    assert max(tr.nsub[s] for s in marks) >= 4, "some landmark step has 4 subnormal elements"
    assert 4 * max(tr.nsub) >= T, "some step has a quarter of the row subnormal at once"
    assert 3 * tr.nzero[-1] >= T, "a third of the row is exactly 0 at the last step"
    assert tr.posts[-1].max() > 0.99
    assert set(marks) <= set(dc.compared_steps(case, f32))
    refs = dc.reference(case, marks, f32)
    decided = 0
    for s in marks:
        opri = refs[s].opri
        assert np.isfinite(opri).all() and (opri >= 0).all() and (opri != 0).sum() >= 10, (name, s)
        assert (opri != 0).sum() == Q - s           # (asked questions, and only they, have priority 0)
        decided += int(refs[s].margin > 1e-8)
    assert 2 * decided >= len(marks), (name, decided, len(marks))
    orc = dc.make_oracle(case, f32)
    for bug in (False, True):
        assert orc.resume_quiz(case.answers, cases.WORKERS, bug) == 0
        nsub, nzero = dc.counts(orc.priors(), case)
        assert nsub >= 1 and 3 * nzero >= T, (name, bug, nsub, nzero)
    orc.close()
    print(name, "landmarks", marks, "first subnormal", tr.first_sub, "first zero", tr.first_zero, "most subnormals", max(tr.nsub),
          "zeros at the end", tr.nzero[-1], "decided", decided)


@pytest.mark.parametrize("name", dc.FLUSHED)
def test_resumed_rows_reach_the_flush(name):
    """The ResumeQuiz legs that are to exercise NormalizePriors' flush do: at the full script a third of the row lies below the threshold,
    some of it within 60 binades, and the oracle resumes it."""
    case = dc.get(name)
    flushed, near = dc.flush_counts(case, len(case.answers))
    assert 3 * flushed >= case.T and near >= 1, (name, flushed, near)
    assert dc.flush_counts(case, 40) == (0, 0)
    orc = case.make_oracle()
    for bug in (False, True):
        assert orc.resume_quiz(case.answers, cases.WORKERS, bug) == 0
        nsub, nzero = dc.counts(orc.priors(), case)
        assert nzero >= flushed and orc.priors().max() > 0.99, (name, bug, nsub, nzero)
    orc.close()
    print(name, "flushed", flushed, "within 60 binades of the threshold", near)
