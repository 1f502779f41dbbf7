"""A whole epoch of HIP training steps straight from example records (bb_trainer_epoch, training.HipTrainer.epoch_records), the
part that needs no GPU: the entry point is declared, exported and bound, it refuses no trainer at all before any device call,
the binding turns that answer into ValueError, and the front end has the switch.  tests/test_gpu_trainer_epoch.py holds the
epoch to the per-batch loop on the GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

from blackbird_amd import Blackbird, _lib
from blackbird_amd.training import HipTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "blackbird_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"int\s+bb_trainer_epoch\s*\(([^)]*)\)\s*;", code)
    assert decl, "include/blackbird_hip.h does not declare bb_trainer_epoch"
    names = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert names == ["t", "n_records", "records", "n_batches", "batch", "order", "sym", "noise", "lr", "loss_out", "bad_out", "stream"]
    assert "bb_trainer_epoch" in _lib.EXPORTS and hasattr(_lib.lib(), "bb_trainer_epoch")
    assert len(_lib.lib().bb_trainer_epoch.argtypes) == 12 and _lib.lib().bb_trainer_epoch.argtypes[8] is C.c_double


def test_no_trainer_is_an_argument_error():
    L = _lib.lib()
    assert L.bb_trainer_epoch(None, 0, None, 0, 1, None, None, None, 0.01, None, None, None) == _lib.ERR_ARG
    assert L.bb_trainer_epoch(None, 4, None, 2, 2, None, None, None, 0.01, None, None, None) == _lib.ERR_ARG
    assert "trainer" in _lib.last_error()
    with pytest.raises(ValueError, match="trainer"):
        _lib.trainer_epoch(None, 4, 0, 2, 2, lr=0.01)


def test_front_end_has_the_call_and_the_switch():
    args = list(inspect.signature(HipTrainer.epoch_records).parameters)
    assert args == ["self", "examples", "order", "batchSize", "learningRate", "sym", "noise"]
    p = inspect.signature(Blackbird.TrainWithDeviceExamples).parameters
    assert [p[k].default for k in ("augment", "merge", "fused")] == [False, False, False]   # every extension is on request
