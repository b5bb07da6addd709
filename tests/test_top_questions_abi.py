"""No-GPU checks that PqaEngine_ListTopQuestions / PqaEngine_ListTopQuestionsBatch are part of the boundary -- declared in
include/PqaHipExt.h, bound in probqa_amd/interop.py with their Python methods, exported by the built libPqaCore.so -- and that the two
merges of the shards' lists (PqaHip_HostLogicProbe "merge_top" for the one-process sharded engine, dist.merge_top_questions for the
process-per-GPU form) agree with a numpy sort by (-priority, index)."""
import ctypes
import re
import struct

import numpy as np
import pytest

import abi_common as abi
from probqa_amd import interop

NAMES = {"PqaEngine_ListTopQuestions": 5, "PqaEngine_ListTopQuestionsBatch": 6}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_declares_top_questions(name):
    args = [a.strip() for a in abi.header_params(name, r"(?:int64_t|void\s*\*)").split(",")]
    assert len(args) == NAMES[name], args
    assert any("CiRatedQuestion" in a for a in args), args
    s = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*CiRatedQuestion\s*;", abi.header_text())
    assert s and re.search(r"int64_t\s+_iQuestion\s*;.*double\s+_priority\s*;", s.group(1), re.S), "CiRatedQuestion {int64_t _iQuestion; double _priority;}"


@pytest.mark.parametrize("name", sorted(NAMES))
def test_binding_carries_top_questions(name):
    _, argtypes = abi.bound_as(name)
    assert len(argtypes) == NAMES[name]


def test_structure_and_python_methods():
    assert ctypes.sizeof(interop.CiRatedQuestion) == 16
    assert interop.CiRatedQuestion.iQuestion.offset == 0 and interop.CiRatedQuestion.priority.offset == 8
    for m in ("list_top_questions", "list_top_questions_batch"):
        assert callable(getattr(interop.PqaEngine, m, None)), m


def test_library_exports_top_questions(factory):
    for name in NAMES:
        assert name in abi.exported_symbols()
        assert getattr(interop.load_library(), name) is not None


def bits(p):
    return struct.unpack("<q", struct.pack("<d", p))[0]


def probe_merge(lists, max_count):
    words = [max_count, len(lists)]
    for lst in lists:
        words.append(len(lst))
        for q, p in lst:
            words += [bits(p), q]
    n_out = 1 + 2 * sum(len(l) for l in lists)
    inp = (ctypes.c_int64 * len(words))(*words)
    out = (ctypes.c_int64 * n_out)()
    n = interop.load_library().PqaHip_HostLogicProbe(b"merge_top", inp, len(words), out, n_out)
    assert n >= 1 and n == 1 + 2 * out[0], n
    return [(out[2 + 2 * k], struct.unpack("<d", struct.pack("<q", out[1 + 2 * k]))[0]) for k in range(out[0])]


def numpy_merge(lists, max_count):
    rec = [(q, p) for lst in lists for q, p in lst]
    if not rec:
        return []
    q = np.array([r[0] for r in rec], dtype=np.int64)
    p = np.array([r[1] for r in rec], dtype=np.float64)
    keep = p > 0   # (False for a NaN)
    q, p = q[keep], p[keep]
    order = np.lexsort((q, -p))[:max_count]
    return [(int(q[i]), float(p[i])) for i in order]


def random_list_sets(n_sets, seed):
    """Shards' listings as the engines make them: disjoint ascending index ranges, each list sorted by (-priority, index).  Priorities
    come from a handful of values, so equal ones meet across and within lists; some lists are empty; every fifth set has fewer
    candidates than max_count; every seventh carries a NaN record."""
    rng = np.random.default_rng(seed)
    values = [0.5, 0.25, 0.25 + 2.0**-54, 1e-300, 3.0, 0.125]
    for s in range(n_sets):
        n_lists = int(rng.integers(1, 6))
        max_count = int(rng.integers(1, 12))
        lists, base = [], 0
        for _ in range(n_lists):
            span = int(rng.integers(1, 40))
            n = 0 if rng.random() < 0.2 else int(rng.integers(1, min(span, max_count) + 1))
            if s % 5 == 0:
                n = min(n, 1)
            qs = sorted(rng.choice(span, n, replace=False).tolist())
            lst = [(base + int(q), values[int(rng.integers(0, len(values)))] if rng.random() < 0.7 else float(rng.random())) for q in qs]
            lst.sort(key=lambda r: (-r[1], r[0]))
            lists.append(lst)
            base += span
        if s % 7 == 0:
            lists[int(rng.integers(0, n_lists))].append((base, float("nan")))
        yield lists, max_count


def test_merges_agree_with_numpy_sort():
    from probqa_amd import dist

    seen_tie = seen_short = seen_empty = seen_nan = 0
    for lists, max_count in random_list_sets(200, 20251):
        want = numpy_merge(lists, max_count)
        assert probe_merge(lists, max_count) == want, (lists, max_count)
        assert dist.merge_top_questions(lists, max_count) == want, (lists, max_count)
        assert all(p == p for _, p in want)
        flat = [r for l in lists for r in l if r[1] == r[1]]
        seen_tie += len({p for _, p in flat}) < len(flat)
        seen_short += len(flat) < max_count
        seen_empty += any(len(l) == 0 for l in lists)
        seen_nan += any(p != p for l in lists for _, p in l)
    assert seen_tie > 20 and seen_short > 20 and seen_empty > 20 and seen_nan > 20


def test_merge_of_one_list_is_its_prefix():
    from probqa_amd import dist

    lst = [(7, 0.9), (3, 0.5), (4, 0.5), (1, 0.1)]
    for n in (0, 1, 3, 4, 9):
        assert dist.merge_top_questions([lst], n) == lst[:n]
        assert probe_merge([lst], n) == lst[:n]
    assert probe_merge([], 5) == [] and dist.merge_top_questions([], 5) == []
