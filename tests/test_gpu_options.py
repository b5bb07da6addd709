"""The contract of PqaHip_SetOption / PqaHip_GetOption and of the PQA_* variables, on an engine and on a sharded engine of two
shards on one device: defaults, accepted and refused values, what a refused value leaves behind, the names nobody knows, the
options that do not fit the table (engine_options.h).  The rows come from tests/test_host_logic.py, where they are held against
the table itself.  The contract does not depend on the cube's size: 4 questions x 2 answers x 8 targets."""
import pytest

from probqa_amd import interop
from test_host_logic import OPTIONS

pytestmark = pytest.mark.gpu

K, Q, T = 2, 4, 8
ENV = ["PQA_SERVER", "PQA_BUG_COMPAT", "PQA_SPECULATE", "PQA_COMBINE", "PQA_POLE_FIX", "PQA_WORKERS", "PQA_SEED", "PQA_SELECT"]
REFUSED = "Unknown option or value out of range"
KINDS = ["whole", "sharded"]


@pytest.fixture
def make(factory, monkeypatch):
    """make(kind, **env): a fresh engine created with nothing of PQA_* in the environment but `env`."""
    made = []

    def create(kind, **env):
        for name in ENV + ["PQA_DEVICES"]:
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        if kind == "sharded":
            monkeypatch.setenv("PQA_DEVICES", "0,0")          # as tests/test_gpu_sharded.py: two shards on one device
        eng, err = factory.create_cpu_engine(interop.EngineDefinition(K, Q, T))
        assert err is None and eng is not None, err
        assert eng.get_option("shards") == (2 if kind == "sharded" else -1)
        made.append(eng)
        return eng

    yield create
    for eng in made:
        eng.close()


def reads(name, value, workers=16):
    """what GetOption answers while the option holds `value`"""
    if name == "eval_max_grid":
        return -1
    if name == "eval_subtasks" and value == 0:
        return 8 * workers
    return value


def refused(eng, name, value):
    with pytest.raises(interop.PqaException, match=REFUSED):
        eng.set_option(name, value)


@pytest.mark.parametrize("kind", KINDS)
def test_defaults_ranges_flags_and_names(kind, make):
    eng = make(kind)
    for name, lo, hi, default, flag, effects, has_env in OPTIONS:
        assert eng.get_option(name) == reads(name, default), name
    assert eng.get_option("eval_max_grid") == -1 and eng.get_option("eval_subtasks") == 128
    for name, lo, hi, default, flag, effects, has_env in OPTIONS:
        if flag:
            for value, stored in ((7, 1), (0, 0), (-1, 1), (0, 0), (1, 1)):
                eng.set_option(name, value)
                assert eng.get_option(name) == stored, (name, value)
        else:
            for value in (lo, hi):
                eng.set_option(name, value)
                assert eng.get_option(name) == reads(name, value), (name, value)
            refused(eng, name, lo - 1)
            assert eng.get_option(name) == reads(name, hi), name          # ... and the value stays as it was
            if name != "eval_variant":                                    # (no upper bound)
                refused(eng, name, hi + 1)
                assert eng.get_option(name) == reads(name, hi), name
        eng.set_option(name, default)
        assert eng.get_option(name) == reads(name, default), name
    refused(eng, "select", 2)
    assert eng.get_option("select") == 0
    refused(eng, "combine_linger_us", 10001)
    assert eng.get_option("combine_linger_us") == 20
    eng.set_option("workers", 5)
    assert eng.get_option("eval_subtasks") == 40
    # names: one nobody knows, a counter, the write-only seed
    refused(eng, "no_such_option", 1)
    assert eng.get_option("no_such_option") == -1
    refused(eng, "posted_ops", 1)
    assert eng.get_option("posted_ops") >= 0
    eng.set_option("seed", 1)
    assert eng.get_option("seed") == -1


@pytest.mark.parametrize("kind", KINDS)
def test_server_vram_mailbox_is_refused_once_the_resident_sweep_has_started(kind, make):
    eng = make(kind)
    eng.set_option("server_vram_mailbox", 0)
    eng.set_option("server_vram_mailbox", 1)
    eng.set_option("server", 1)
    first = eng.next_question_argmax(eng.start_quiz())
    assert 0 <= first < Q
    if kind == "whole":
        refused(eng, "server_vram_mailbox", 0)
        assert eng.get_option("server_vram_mailbox") in (0, 1)            # the live state: where the request line is
    else:
        # A sharded engine's selections are launched while pole_fix is on (HipEngine::EnqueueSelectArgmaxFlag), so its shards
        # have no resident sweep yet and the option is still theirs to set.
        eng.set_option("server_vram_mailbox", 0)
        assert eng.get_option("server_vram_mailbox") == 0
    eng.set_option("server", 0)
    assert eng.get_option("server") == 0
    assert eng.next_question_argmax(eng.start_quiz()) == first            # the engine still selects: a fresh quiz again


@pytest.mark.parametrize("kind", KINDS)
def test_seed_fixes_the_sampled_selections(kind, make):
    drawn = []
    for _ in range(2):
        eng = make(kind)
        assert eng.get_option("select") == 0
        eng.set_option("seed", 12345)
        drawn.append([eng.next_question(eng.start_quiz()) for _ in range(8)])
        assert all(0 <= q < Q for q in drawn[-1])
    assert drawn[0] == drawn[1]


@pytest.mark.parametrize("kind", KINDS)
def test_environment_presets(kind, make):
    eng = make(kind, PQA_WORKERS="7", PQA_COMBINE="0", PQA_SELECT="argmax")
    # (a sharded engine answers "combine" for its own combining, which only SetOption reaches: its shards took PQA_COMBINE)
    assert (eng.get_option("workers"), eng.get_option("combine"), eng.get_option("select")) == (7, 0 if kind == "whole" else 1, 1)
    eng = make(kind, PQA_WORKERS="0")                                     # out of range: reported on stderr and ignored
    assert eng.get_option("workers") == 16
