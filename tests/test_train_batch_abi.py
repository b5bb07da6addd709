"""No-GPU checks that PqaEngine_TrainBatch and PqaEngine_RecordQuizTargetBatch are part of the boundary: declared in
include/PqaHipExt.h, bound in probqa_amd/interop.py with their Python methods, and exported by the built libPqaCore.so."""
import pytest

import abi_common as abi
from probqa_amd import interop

NAMES = {"PqaEngine_TrainBatch": 6, "PqaEngine_RecordQuizTargetBatch": 5}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_declares_train_batch(name):
    args = [a.strip() for a in abi.header_params(name, r"void\s*\*").split(",")]
    assert len(args) == NAMES[name], args
    if name == "PqaEngine_TrainBatch":
        assert "CiAnsweredQuestion" in args[3] and "double" in args[5], args
    else:
        assert "double" in args[4], args


@pytest.mark.parametrize("name", sorted(NAMES))
def test_binding_carries_train_batch(name):
    _, argtypes = abi.bound_as(name)
    assert len(argtypes) == NAMES[name]


def test_python_methods_present():
    for m in ("train_batch", "train_batch_arrays", "record_quiz_target_batch"):
        assert callable(getattr(interop.PqaEngine, m, None)), m


def test_library_exports_train_batch(factory):
    for name in NAMES:
        assert name in abi.exported_symbols()
        assert getattr(interop.load_library(), name) is not None
