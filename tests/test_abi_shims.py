"""The C boundary on its own, no GPU: probqa_amd/csrc/c_abi_shims.h -- the exception barrier, the three null-handle conventions and
the factory helper -- driven by tests/abi_shims_check.cpp with lambdas in place of engines, built with g++ as it is and again
under AddressSanitizer and UndefinedBehaviorSanitizer (a CPU build, run as a process of its own); and a reading of c_abi.cpp:
every exported entry is one call of a shim, or is listed here with the reason why not."""
import os
import re
import subprocess

import pytest

from abi_common import declared_functions
from probqa_amd import interop

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "probqa_amd", "csrc")
SOURCE = os.path.join(HERE, "abi_shims_check.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module")
def checks(tmp_path_factory):
    out = tmp_path_factory.mktemp("abi_shims")
    exes = {}
    for name, flags in BUILDS.items():
        exe = str(out / ("abi_shims_check_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, SOURCE])
        exes[name] = exe
    return exes


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_shims_and_barrier(checks, build):
    """Each shim and the factory helper: a null handle, success, an error returned, std::bad_alloc and std::runtime_error thrown
    (StdException with what=[...]), throw 7 (SRException); the value or pointer returned, *ppError set or left null, a null ppError
    tolerated, every error object released (the sanitizer's build also counts what was not).  The logging shim's lines are read
    here: one for the null handle, one naming what() for each exception."""
    res = subprocess.run([checks[build]], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
    assert re.fullmatch(r"ok \d+\n", res.stdout), res.stdout
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
    assert res.stderr.splitlines() == [
        "PqaCore: Nullptr is passed in place of IPqaEngine.",
        "PqaCore: A C++ exception was caught at the C interface. what=[std::bad_alloc]",
        "PqaCore: A C++ exception was caught at the C interface. what=[boom]",
        "PqaCore: An unknown exception was caught at the C interface. ",
        "PqaCore: A C++ exception was caught at the C interface. what=[name]",
    ], res.stderr


# ---- c_abi.cpp, read --------------------------------------------------------------------------------------------------------------
SHIMS = {"ErrorOf": r"\bErrorOf\(pvEngine, ", "ValueOf": r"\bValueOf<\w+>\(pvEngine, ppError, ", "LoggedOf": r"\bLoggedOf<[\w \*]+>\(pvEngine, ",
         "EngineOf": r"\b(?:Create|Load)Engine\(pvFactory, ppError, "}   # (the two factory helpers, each one call of EngineOf)
# No engine handle, but they allocate: the barrier alone, with what an exception makes them answer.
BARRIER_ONLY = {
    "PqaHip_PickWhenAll": "the error object",
    "PqaHip_HostRegister": "the error object",
    "PqaError_ToString": "a null string",
    "Logger_Init": "0 and the exception's text",
    "PqaHip_HostLogicProbe": "-1",
}
# Nothing in them can throw.
BARE = {
    "CiDebugBreak": "empty",
    "CiReleaseString": "delete[] of a string this library made",
    "CiGetPqaEngineFactory": "the address of a global",
    "CiReleasePqaError": "delete of an error object: strings' destructors",
    "CiReleasePqaEngine": "destructors, and a lookup in the side tables that inserts nothing",
    "CiReleaseCompaction": "free()",
    "PqaHip_HostUnregister": "one HIP call",
}


def exported_definitions():
    """name -> (signature, body) of every PQACORE_API definition in c_abi.cpp: up to the closing brace in column 0, or the
    line's end for a definition on one line."""
    text = open(os.path.join(CSRC, "c_abi.cpp")).read()
    defs = {}
    for m in re.finditer(r"^PQACORE_API\s+[\w\s\*]+?\b(\w+)\s*\(", text, re.M):
        line_end = text.index("\n", m.start())
        opening = text.index("{", m.start())
        if text[opening:line_end].rstrip().endswith("}"):
            end = line_end
        else:
            end = text.index("\n}\n", m.start()) + 2
        assert m.group(1) not in defs, m.group(1)
        defs[m.group(1)] = (text[m.start():opening], text[opening:end])
    return text, defs


def test_every_entry_is_one_call_of_a_shim():
    text, defs = exported_definitions()
    declared = set(interop.REFERENCE_EXPORTS) | set(interop.HIP_EXPORTS)
    for header in ("PqaCInterop.h", "PqaHipExt.h"):
        declared |= set(declared_functions(header))
    assert set(defs) == declared, sorted(set(defs) ^ declared)
    assert len(BARE) == 7 and len(BARRIER_ONLY) == 5 and not set(BARE) & set(BARRIER_ONLY)
    assert set(BARE) | set(BARRIER_ONLY) <= set(defs)
    for name, (signature, body) in defs.items():
        found = [(shim, call) for shim, pattern in SHIMS.items() for call in re.findall(pattern, body)]
        calls = [shim for shim, _ in found]
        if name in BARE:
            assert not calls and "Guarded" not in body, (name, BARE[name])
        elif name in BARRIER_ONLY:
            assert not calls and len(re.findall(r"\bGuarded(?:Value<[\w \*]+>)?\(", body)) >= 1, (name, BARRIER_ONLY[name])
            assert "pvEngine" not in signature and "pvFactory" not in signature, name
        else:
            assert len(calls) == 1, (name, calls)
            assert ("pvFactory" in signature) == (calls[0] == "EngineOf"), (name, calls)
            assert ("ppError" in signature) == (calls[0] in ("ValueOf", "EngineOf")), (name, calls)
            # ... and nothing beside it: the body is `return <shim>(...);`, with at most a static_assert in front
            stripped = re.sub(r"^\{\s*(static_assert\(.*\);\s*)?", "", body)
            assert stripped.startswith("return " + found[0][1]) and re.search(r"\}?\);\s*\}$", body), name
    # the macros are gone, the cast lives in the shims header alone, and the barrier is the one place that catches
    assert "ENGINE_OR_" not in text
    for helper in ("CreateEngine", "LoadEngine"):
        body = re.search(r"^void \*%s\(void \*pvFactory, void \*\*ppError, .*?^\}$" % helper, text, re.M | re.S).group(0)
        assert len(re.findall(r"\bEngineOf\(pvFactory, ppError, ", body)) == 1, helper
    assert len(re.findall(r"\bEngineOf\(", text)) == 2
    for fname in os.listdir(CSRC):
        if fname != "c_abi_shims.h" and fname.endswith((".cpp", ".h", ".hip")):
            assert "static_cast<pqa::IEngine" not in open(os.path.join(CSRC, fname)).read(), fname
    assert not re.search(r"\b(try|catch)\b", text)
    shims = open(os.path.join(CSRC, "c_abi_shims.h")).read()
    assert len(re.findall(r"\btry\b", shims)) == 1 and len(re.findall(r"\bcatch\b", shims)) == 2
