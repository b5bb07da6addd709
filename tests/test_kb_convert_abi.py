"""No-GPU checks of .kb files per shard and in either precision: the three exports are declared in include/PqaHipExt.h, bound in
probqa_amd/interop.py with the same argument types and exported by the built libPqaCore.so; the file offsets of a shard's two blocks
(kb_plan.h: KbLayout, through PqaHip_HostLogicProbe) agree with a Python model of the layout; and the bookkeeping of dist.load_shard /
dist.save_kb runs over gloo on the CPU against a stub engine that records what it is asked to do."""
import ctypes
import os
import re
import struct
import sys

import numpy as np
import pytest
import torch.distributed as dist

import abi_common as abi
import ranks_common as rc
from probqa_amd import dist as pdist
from probqa_amd import interop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _pvp, _u8, _i64, _str = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint8, ctypes.c_int64, ctypes.c_char_p
# name -> (C parameter types as the header spells them, ctypes argument types, Python method and its owner)
EXPORTS = {
    "PqaEngineFactory_LoadHipEngineAs": (["void *", "void **", "const char *", "uint8_t", "const CiHipShard *", "int64_t"],
                                         [_vp, _pvp, _str, _u8, ctypes.POINTER(interop.CiHipShard), _i64], (interop.PqaEngineFactory, "load_hip_engine")),
    "PqaHip_SaveKBAs": (["void *", "const char *", "uint8_t"], [_vp, _str, _u8], (interop.PqaEngine, "save_kb_as")),
    "PqaHip_SaveKBShard": (["void *", "const char *", "uint8_t"], [_vp, _str, _u8], (interop.PqaEngine, "save_kb_shard")),
}


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_header_declares_what_the_binding_declares(name):
    params = [re.sub(r"\s*\w+$", "", " ".join(a.split())).replace(" *", " *").strip() for a in abi.header_params(name, r"void\s*\*").split(",")]
    assert params == EXPORTS[name][0], params
    res, argtypes = abi.bound_as(name)
    assert res is _vp and argtypes == EXPORTS[name][1]
    owner, method = EXPORTS[name][2]
    assert callable(getattr(owner, method, None))


def test_library_exports(factory):
    assert set(EXPORTS) <= abi.exported_symbols(), set(EXPORTS) - abi.exported_symbols()
    lib = interop.load_library()
    for name in EXPORTS:
        assert getattr(lib, name).argtypes == EXPORTS[name][1]


def test_null_handles_answer_with_errors(factory):
    """the null-handle conventions of the other exports: an error object, no crash, no engine"""
    lib = interop.load_library()
    for fn in (lib.PqaHip_SaveKBAs, lib.PqaHip_SaveKBShard):
        err = fn(None, b"/nonexistent/x.kb", 0)
        assert err
        assert "Expected non-null argument" in interop.PqaError(err).to_string(True)
    c_err = ctypes.c_void_p()
    assert not lib.PqaEngineFactory_LoadHipEngineAs(None, ctypes.byref(c_err), b"x", 0, None, 0)
    assert "Expected non-null argument" in interop.PqaError(c_err.value).to_string(True)


def test_load_refusals_that_need_no_device(factory, tmp_path):
    """what is decided before anything is allocated comes back as a PqaError: a missing file, a header of absurd dimensions, arrays
    the file is too short for, a number type no engine has, an unsupported precType"""
    def load(path, prec=None, **kw):
        with pytest.raises(interop.PqaException) as e:
            factory.load_hip_engine(str(path), prec, **kw)
        return str(e.value)

    assert "Cannot open file" in load(tmp_path / "absent.kb")
    double = 3 | (53 << 4) | (11 << 32)
    absurd = tmp_path / "absurd.kb"
    absurd.write_bytes(struct.pack("<QqqqQ", double, 5, 1 << 61, 1 << 61, 0) + b"\0" * 64)
    assert "File operation failed" in load(absurd)
    huge = tmp_path / "huge.kb"
    huge.write_bytes(struct.pack("<QqqqQ", double, 5, 1 << 30, 1 << 20, 0) + b"\0" * 64)   # 48 PB of arrays in a 104-byte file
    assert "shorter than the arrays" in load(huge)
    negative = tmp_path / "negative.kb"
    negative.write_bytes(struct.pack("<QqqqQ", double, 5, -4, 100, 0) + b"\0" * 64)
    assert "File operation failed" in load(negative)
    pair = tmp_path / "pair.kb"
    pair.write_bytes(struct.pack("<QqqqQ", 4, 2, 1, 2, 0) + b"\0" * 1024)                   # DoublePair
    assert "Not implemented" in load(pair)
    small = tmp_path / "small.kb"
    small.write_bytes(struct.pack("<QqqqQ", double, 2, 1, 2, 0) + b"\0" * 1024)
    assert "Not implemented" in load(small, 2)                                                # FloatPair asked for
    assert interop.read_kb_header(str(small))[1].n_questions == 1


# ---- the file offsets of a shard's two blocks ------------------------------------------------------------------------------------
def model_layout(K, Q, T, elem, q_first, n_local):
    """hip_engine_kb.cpp's layout comment, spelled out: header 40 | sA [Q][K][T] | mD [Q][T] | vB [T] | trailer"""
    row = T * elem
    sa, md = 40, 40 + Q * K * row
    vb = md + Q * row
    return [sa + q_first * K * row, n_local * K * row, md + q_first * row, n_local * row, vb, vb + row]


def probe_layout(K, Q, T, elem, q_first, n_local):
    lib = interop.load_library()
    src = (ctypes.c_int64 * 6)(K, Q, T, elem, q_first, n_local)
    out = (ctypes.c_int64 * 8)()
    assert lib.PqaHip_HostLogicProbe(b"kb_layout", src, 6, out, 8) == 8
    return list(out)


@pytest.mark.parametrize("elem", [4, 8])
@pytest.mark.parametrize("K,Q,T", [(2, 3, 1), (3, 5, 3), (4, 50, 67), (5, 37, 101), (5, 8, 1025), (5, 16, 4096), (2, 3, 16387),
                                   (5, 4000, 10000), (5, 10_000_000, 1_000_000)])
def test_shard_blocks_lie_where_the_layout_says(factory, K, Q, T, elem):
    for world in (1, 2, 3, 8):
        if Q < world:
            continue
        end = 40
        for rank in range(world):
            first, limit = pdist.shard_range(Q, world, rank)
            got = probe_layout(K, Q, T, elem, first, limit - first)
            assert got[:2] == [1, 1] and got[2:] == model_layout(K, Q, T, elem, first, limit - first)
            assert got[2] == end                 # the shards' sA blocks follow each other ...
            end = got[2] + got[3]
        assert end == model_layout(K, Q, T, elem, 0, Q)[2]   # ... and end where the mD rows begin


def test_windows_and_dimensions_that_are_refused(factory):
    assert probe_layout(5, 10, 7, 8, 4, 6)[:2] == [1, 1]
    for q_first, n_local in ((4, 7), (10, 1), (-1, 2), (0, 0), (0, -3), (11, 1), (2**62, 2**62)):
        assert probe_layout(5, 10, 7, 8, q_first, n_local)[:3] == [1, 0, -1], (q_first, n_local)
    for K, Q, T, elem in ((5, 10, 7, 2), (0, 10, 7, 8), (5, 0, 7, 8), (5, 10, -7, 8), (5, 2**40, 2**40, 8), (2**31, 2**31, 2, 8)):
        assert probe_layout(K, Q, T, elem, 0, 1)[0] == 0, (K, Q, T, elem)


# ---- dist.load_shard / dist.save_kb over gloo, against a stub engine ----------------------------------------------------------
Q_FILE = 11


class StubFactory:
    def __init__(self):
        self.calls = []

    def load_hip_engine(self, path, precision=None, q_first=0, n_local=None, q_total=None, device=-1):
        self.calls.append((precision, q_first, n_local, q_total, device))
        return StubEngine(q_first, n_local)


class StubEngine:
    """writes its rank's bytes at its offset of the file, in place; `fail` makes the save raise"""

    def __init__(self, q_first, n_local, fail=False):
        self.q_first, self.n_local, self.fail, self.saves = q_first, n_local, fail, []

    def get_option(self, name):
        assert name == "q_first"
        return self.q_first

    def save_kb_shard(self, path, precision=None):
        self.saves.append((precision, os.path.exists(path), os.path.getsize(path) if os.path.exists(path) else -1))
        if self.fail:
            raise interop.PqaException("[FileOp] stub failure")
        fd = os.open(path, os.O_RDWR | os.O_CREAT)
        try:
            os.pwrite(fd, bytes([65 + self.q_first]) * self.n_local, self.q_first)
        finally:
            os.close(fd)


def _worker(rank, world, port, folder, ret):
    sys.path.insert(0, ROOT)
    rc.init_group("gloo", rank, world, port)
    out = {}
    src = os.path.join(folder, "src.kb")
    fac = StubFactory()
    eng = pdist.load_shard(fac, src, rank, world, precision=interop.PrecisionType.FLOAT, device=0)
    out["load"] = fac.calls
    # all succeed: a stale, longer file is emptied by the rank that holds question 0 before any part lands
    good = os.path.join(folder, "good.kb")
    pdist.save_kb(eng, good, rank, world, precision=interop.PrecisionType.DOUBLE)
    out["saves"] = eng.saves
    dist.barrier()
    out["good"] = open(good, "rb").read()
    # one rank fails: every rank raises the same text, the file is gone
    for failing in (0, world - 1):
        path = os.path.join(folder, "bad%d.kb" % failing)
        bad = StubEngine(eng.q_first, eng.n_local, fail=(rank == failing))
        try:
            pdist.save_kb(bad, path, rank, world)
            out["raised%d" % failing] = None
        except interop.PqaException as e:
            out["raised%d" % failing] = str(e)
        dist.barrier()
        out["left%d" % failing] = os.path.exists(path)
    ret[rank] = out
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_load_shard_and_save_kb_bookkeeping_over_gloo(tmp_path, world):
    (tmp_path / "src.kb").write_bytes(struct.pack("<QqqqQ", 3 | (53 << 4) | (11 << 32), 5, Q_FILE, 7, 0))
    (tmp_path / "good.kb").write_bytes(b"stale" * 100)
    ret = rc.run_gloo(_worker, world, str(tmp_path))
    want = b""
    for r in range(world):
        first, limit = pdist.shard_range(Q_FILE, world, r)
        want += bytes([65 + first]) * (limit - first)
        assert ret[r]["load"] == [(interop.PrecisionType.FLOAT, first, limit - first, Q_FILE, 0)]   # the ranges equal shard_range
        # every part is written after the creator -- the rank that holds question 0 -- has emptied the file: nobody meets the stale bytes
        (prec, existed, size), = ret[r]["saves"]
        assert prec == interop.PrecisionType.DOUBLE and existed and size < 500, ret[r]["saves"]
        assert ret[r]["good"] == want if r == world - 1 else True
        for failing in (0, world - 1):
            text = ret[r]["raised%d" % failing]
            assert text is not None and "rank %d" % failing in text and "stub failure" in text, ret[r]
            assert text == ret[0]["raised%d" % failing]
            assert ret[r]["left%d" % failing] is False      # all or none: the file is removed
    assert ret[0]["good"] == want and len(want) == Q_FILE


def test_save_kb_without_a_process_group(tmp_path):
    eng = StubEngine(0, Q_FILE)
    path = str(tmp_path / "one.kb")
    pdist.save_kb(eng, path, 0, 1)
    assert open(path, "rb").read() == b"A" * Q_FILE
    with pytest.raises(interop.PqaException, match="stub failure"):
        pdist.save_kb(StubEngine(0, Q_FILE, fail=True), path, 0, 1)
    assert not os.path.exists(path)
