"""The one-launch search (BB_LAUNCH_WAVE) where no GPU is needed: its entry point in the header, the library and the binding;
the front end's switch; argument checks."""
import ctypes as C
import os
import re

import pytest

from blackbird_amd import _lib
from blackbird_amd.DynamicMCTS import DynamicMCTS
from blackbird_amd.MCTS import MCTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structure_entry_point_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "blackbird_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+bb_run_sims_structure\s*\(\s*bb_engine\s*\*\s*e\s*,\s*int32_t\s*\*\s*out\s*\)\s*;", code)
    m = re.search(r"#define\s+BB_LAUNCH_WAVE\s+(\d+)", code)
    assert m and int(m.group(1)) == _lib.LAUNCH_WAVE == 3
    assert "bb_run_sims_structure" in _lib.EXPORTS
    L = _lib.lib()
    assert L.bb_run_sims_structure.argtypes == [C.c_void_p, C.POINTER(C.c_int32)] and L.bb_run_sims_structure.restype is C.c_int
    assert hasattr(_lib.Engine, "run_sims_structure")


def test_null_arguments_are_refused():
    L = _lib.lib()
    out = C.c_int32(-7)
    assert L.bb_run_sims_structure(None, C.byref(out)) == _lib.ERR_ARG
    assert L.bb_run_sims_structure(None, None) == _lib.ERR_ARG
    assert out.value == -7 and _lib.last_error()


def test_search_launch_values():
    assert MCTS.SearchLaunch == "lockstep"
    m = DynamicMCTS(explorationRate=0.85, playLimit=4)
    assert m._search_launch() == _lib.LAUNCH_AUTO   # the default leaves bb_config.launch alone
    m.SearchLaunch = "wave"
    assert m._search_launch() == _lib.LAUNCH_WAVE
    m.SearchLaunch = "nonsense"
    with pytest.raises(ValueError, match="SearchLaunch"):
        m._make_engine(_lib.GAME_CONNECT4, 1, 4)
    assert MCTS.SearchLaunch == "lockstep"
