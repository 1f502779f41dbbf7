"""One-launch self-play of the rollout evaluator (bb_selfplay_rollouts) where no GPU is needed: the entry point in the header, in
the library and in the binding, its argument checks, and that nothing here pretends to run without a device."""
import ctypes as C
import os
import re

import pytest

from blackbird_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "blackbird_hip.h")


def test_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+bb_selfplay_rollouts\s*\(\s*bb_engine\s*\*\s*e\s*,\s*int\s+on\s*\)\s*;", code)
    assert "bb_selfplay_rollouts" in _lib.EXPORTS
    fn = _lib.lib().bb_selfplay_rollouts          # (AttributeError: the library does not export it)
    assert list(fn.argtypes) == [C.c_void_p, C.c_int] and fn.restype is C.c_int
    assert callable(_lib.Engine.selfplay_rollouts)


def test_mode_six_is_documented_in_the_header():
    text = open(HEADER).read()
    comment = text[:text.index("int bb_selfplay_mode(")].rsplit("/*", 1)[1]
    assert re.search(r"\b6\b", comment) and "bb_selfplay_rollouts" in comment


@pytest.mark.parametrize("on", [0, 1, 2, -1])
def test_null_engine_is_an_argument_error(on):
    assert _lib.lib().bb_selfplay_rollouts(None, on) == _lib.ERR_ARG
    assert b"bb_selfplay_rollouts" in _lib.lib().bb_last_error()


def test_a_value_other_than_0_or_1_is_refused_before_the_engine_is_touched():
    """`on` is checked without reading the engine: a handle that is never dereferenced stands in for one (no GPU here)."""
    blob = C.create_string_buffer(1 << 16)
    assert _lib.lib().bb_selfplay_rollouts(C.addressof(blob), 2) == _lib.ERR_ARG
    assert blob.raw == bytes(1 << 16)


def test_engine_creation_still_fails_loudly_without_a_gpu():
    """No CPU fall-back came with the new structure: without a device bb_create answers with an error, not with an engine."""
    kw = dict(n_slots=4, sims_per_move=8, evaluator=_lib.EVAL_ROLLOUT)
    if _lib.lib().bb_device_count() > 0:          # (a GPU is present: the same call gives an engine, in lock-step until asked)
        eng = _lib.Engine(_lib.GAME_CONNECT4, **kw)
        assert eng.selfplay_mode() == 0
        eng.close()
        return
    with pytest.raises(_lib.BlackbirdHipError, match="no HIP device"):
        _lib.Engine(_lib.GAME_CONNECT4, **kw)
