"""What the *_abi.py tests share: the declarations of the headers under include/, the symbols the built libPqaCore.so exports and
the ctypes binding of probqa_amd/interop.py.  The tables of names, counts and types stay with the tests."""
import os
import re
import subprocess

from probqa_amd import interop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text(header="PqaHipExt.h"):
    return open(os.path.join(ROOT, "include", header)).read()


def declared_functions(header):
    """The names of all functions the header declares PQACORE_API."""
    return re.findall(r"PQACORE_API\s+[\w\s\*]+?\b(\w+)\s*\(", header_text(header))


def header_params(name, returns=r"\w+\s*\*?"):
    """The parameter list, as text, of the declaration of `name` in include/PqaHipExt.h (`returns`: a pattern its return type must match)."""
    m = re.search(r"PQACORE_API\s+" + returns + r"\s*" + name + r"\s*\(([^)]*)\)", header_text())
    assert m, "PqaHipExt.h does not declare " + name
    return m.group(1)


def exported_symbols():
    """The functions the built library defines and exports."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", interop.LIB_PATH], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def bound_as(name):
    """(restype, argtypes) of the ctypes binding."""
    assert name in interop.HIP_EXPORTS, name
    return interop.HIP_EXPORTS[name]
