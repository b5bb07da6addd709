"""Pages of answers across separately created shards on a real MI355X (PqaEngine_RecordAnswerPageBatchFromRows), and on the
one-process sharded engine.  One process: the shards of one synthetic KB sit side by side on the one device as
create_hip_engine(def, q_first, Q, 0) engines and one whole engine holds the same KB.  Every owner packs the flattened pages' rows
into one zero-filled torch tensor, every shard records from it; posteriors, answers and likelihoods are compared for equality."""
import numpy as np
import pytest

from probqa_amd import dist as pdist
from probqa_amd import interop
from test_gpu_resume_ranks import Shape, aq_list, pack_all

pytestmark = pytest.mark.gpu

SHAPES = {s.name: s for s in [
    Shape("gaps37x5x101", 5, 37, 101, tgaps=(3, 17, 100)),          # the 256-thread form, an odd T
    Shape("float120x5x1000", 5, 120, 1000, f32=True),               # package slots in the cube's own element type
    Shape("long64x5x20000", 5, 64, 20000, tgaps=(5, 19999)),        # rows beyond 16384 targets: the posterior in memory
]}
LENGTHS = (0, 1, 2, 4, 7, 12)


def pages_for(shape, world):
    """A page per length; consecutive answers of a page lie a shard's width apart, so every page of two or more crosses the bounds."""
    stride = shape.Q // world + 1
    pages = [[((5 * i + j * stride) % shape.Q, (i + j) % shape.K) for j in range(n)] for i, n in enumerate(LENGTHS)]
    for p in pages:
        if world > 1 and len(p) >= 2:
            assert len(set(pdist.row_owners(p, shape.Q, world))) >= 2, p
    assert {o for p in pages for o in pdist.row_owners(p, shape.Q, world)} == set(range(world))
    return pages


def answers_of(eng, quiz):
    return [(a.i_question, a.i_answer) for a in eng.get_quiz_answers(quiz)]


def bits(rows):
    return [np.asarray(r, dtype=np.float64).tobytes() for r in rows]


def close_all(engines):
    for e in engines:
        e.close()


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shards_record_the_whole_engines_bits(name, world, factory):
    shape = SHAPES[name]
    pages = pages_for(shape, world)
    whole, shards = shape.world(factory, world)
    quizzes = whole.start_quiz_batch(len(pages))
    for sh in shards:
        assert sh.start_quiz_batch(len(pages)) == quizzes
    for e in [whole] + shards:
        e.set_active_question(quizzes[0], 9)                        # the quiz with the empty page
    lists = [aq_list(p) for p in pages]
    want = whole.record_answer_page_batch(quizzes, lists, likelihoods=True)
    flat = [aq for p in pages for aq in p]
    pkg = pack_all(shards, flat)
    for k, sh in enumerate(shards):
        launches0 = sh.get_option("page_launches")
        # (a world of one holds every question: the package is not read, and may be absent)
        got = sh.record_answer_page_batch_from_rows(quizzes, lists, 0 if world == 1 else pkg.data_ptr(), likelihoods=True)
        assert bits(got) == bits(want), k
        assert sh.get_option("page_launches") == launches0 + 1
        first, limit = pdist.shard_range(shape.Q, world, k)
        for quiz, page in zip(quizzes, pages):
            assert np.array_equal(sh.get_priors(quiz), whole.get_priors(quiz)), (k, len(page))
            assert answers_of(sh, quiz) == page == answers_of(whole, quiz)
            assert sh.get_active_question_id(quiz) == (-1 if page else 9)
            # the device's asked bits: a priority of exactly 0 at every question of the page this shard holds
            mine = sh.eval_priorities(quiz, limit - first)
            assert all(mine[q - first] == 0.0 for q, _ in page if first <= q < limit), (k, len(page))
            assert (mine == 0.0).sum() <= len(page), (k, len(page))
    # the call without likelihoods, one more page for every quiz: the same bits again
    more = [[((q + 3) % shape.Q, (a + 1) % shape.K) for q, a in p[:3]] for p in pages]
    whole.record_answer_page_batch(quizzes, [aq_list(p) for p in more])
    pkg = pack_all(shards, [aq for p in more for aq in p])
    for k, sh in enumerate(shards):
        assert sh.record_answer_page_batch_from_rows(quizzes, [aq_list(p) for p in more], pkg.data_ptr()) is None
        for quiz in quizzes:
            assert np.array_equal(sh.get_priors(quiz), whole.get_priors(quiz)), k
            assert [(t.i_target, t.prob) for t in sh.list_top_targets(quiz, 5)] == [(t.i_target, t.prob) for t in whole.list_top_targets(quiz, 5)]
    close_all([whole] + shards)


def test_refusals_on_shards(factory):
    shape, world = SHAPES["gaps37x5x101"], 3
    whole, shards = shape.world(factory, world)
    gap = pdist.shard_range(shape.Q, world, 2)[0] + 1                 # a question rank 2 holds
    for e in [whole] + shards:
        e.set_question_gaps([gap])
    quizzes = [sh.start_quiz_batch(2) for sh in shards][0]
    foreign = pdist.shard_range(shape.Q, world, 1)[0]
    own = pdist.shard_range(shape.Q, world, 0)[0]

    def state(sh):
        return [(sh.get_priors(z).tobytes(), answers_of(sh, z), sh.get_active_question_id(z)) for z in quizzes] + [sh.get_option("page_answers")]

    before = [state(sh) for sh in shards]
    # the plain call on a shard that meets another shard's question: ResumeQuiz's wording, pointing at the FromRows form
    with pytest.raises(interop.PqaException, match=r"Not implemented.*belongs to another shard.*RecordAnswerPageBatchFromRows"):
        shards[0].record_answer_page_batch(quizzes, [aq_list([(own, 1)]), aq_list([(own, 0), (foreign, 2)])])
    # a gap on another rank: the same refusal on every rank
    pages = [[(own, 1)], [(foreign, 2), (gap, 0)]]
    pkg = pack_all(shards, [aq for p in pages for aq in p])
    texts = []
    for sh in shards:
        with pytest.raises(interop.PqaException) as e:
            sh.record_answer_page_batch_from_rows(quizzes, [aq_list(p) for p in pages], pkg.data_ptr())
        texts.append(str(e.value))
    assert len(set(texts)) == 1 and "entry=1" in texts[0] and "position=1" in texts[0] and "questionId=%d" % gap in texts[0] and "gap" in texts[0], texts
    # a foreign question without a package
    with pytest.raises(interop.PqaException, match="Expected non-null argument"):
        shards[0].record_answer_page_batch_from_rows(quizzes, [aq_list([(own, 1)]), aq_list([(foreign, 2)])], 0)
    assert [state(sh) for sh in shards] == before
    close_all([whole] + shards)


def test_one_process_sharded_engine(factory, monkeypatch):
    shape = SHAPES["gaps37x5x101"]
    whole = shape.engine(factory, 0, shape.Q)
    monkeypatch.setenv("PQA_DEVICES", "0,0")        # two shards side by side on the one device
    eng, err = factory.create_cpu_engine(shape.definition(shape.Q))
    assert err is None and eng.get_option("shards") == 2
    eng.fill_synthetic(8.0, 0.5, shape.seed)
    eng.set_target_gaps(list(shape.tgaps))
    eng.set_option("workers", 16)
    pages = pages_for(shape, 2)
    quizzes = whole.start_quiz_batch(len(pages))
    assert eng.start_quiz_batch(len(pages)) == quizzes
    eng.set_active_question(quizzes[0], 9)
    lists = [aq_list(p) for p in pages]
    with pytest.raises(interop.PqaException, match=r"Not implemented.*likelihoods"):
        eng.record_answer_page_batch(quizzes, lists, likelihoods=True)
    with pytest.raises(interop.PqaException, match="Index is out of range.*entry=5.*position=1"):
        eng.record_answer_page_batch(quizzes, lists[:5] + [aq_list([(0, 0), (shape.Q, 0)])])
    for quiz in quizzes:
        assert answers_of(eng, quiz) == []                          # the refusals changed nothing
    whole.record_answer_page_batch(quizzes, lists)
    assert eng.record_answer_page_batch(quizzes[:3], lists[:3]) is None
    assert eng.record_answer_page_batch_from_rows(quizzes[3:], lists[3:], 0) is None     # (the package is ignored there)
    for quiz, page in zip(quizzes, pages):
        assert np.array_equal(eng.get_priors(quiz), whole.get_priors(quiz)), len(page)
        assert answers_of(eng, quiz) == page
        assert eng.get_active_question_id(quiz) == (-1 if page else 9)
    close_all([whole, eng])
