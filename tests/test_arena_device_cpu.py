"""The arena on the device (bb_arena_*, arena.TestModelsBatched(loop=...)), the part that needs no GPU:

  * the BB_ERR_ARG answers of the six entry points that come before any device call.  Without a GPU no engine exists, so the
    arguments here are null pointers, and for `a == b` one non-null handle that the check must refuse before it looks inside
    (the header documents that order: null, a == b, log_plies, then the engines' configurations);
  * the Python choice of loop, which is made before any engine is."""
import ctypes as C

import numpy as np
import pytest

from blackbird_amd import _lib, arena
from blackbird_amd import Connect4
from blackbird_amd.DynamicMCTS import DynamicMCTS
from blackbird_amd.FixedMCTS import FixedMCTS
from blackbird_amd.MCTS import MCTS
from blackbird_amd.RandomMCTS import RandomMCTS


def test_arena_entry_points_refuse_null_arguments():
    L = _lib.lib()
    out = C.c_void_p()
    alive = C.c_int(-7)
    first = np.ones(4, dtype=np.uint8)
    assert L.bb_arena_create(None, None, 8, C.byref(out)) == _lib.ERR_ARG
    assert "null" in _lib.last_error()
    assert out.value is None
    assert L.bb_arena_begin(None, 4, _lib.ptr(first), None, 0.0) == _lib.ERR_ARG
    assert L.bb_arena_step(None, 1) == _lib.ERR_ARG
    assert L.bb_arena_status(None, C.byref(alive)) == _lib.ERR_ARG
    assert alive.value == -7
    assert L.bb_arena_fetch(None, None, None, None, None) == _lib.ERR_ARG
    assert L.bb_arena_destroy(None) == _lib.OK


def test_arena_create_refuses_one_engine_on_both_sides_before_reading_it():
    """a == b is answered from the two pointer values alone; so is a missing `out`."""
    L = _lib.lib()
    keep = np.zeros(64, dtype=np.uint8)          # any address: the check may not look behind it
    handle = C.c_void_p(keep.ctypes.data)
    out = C.c_void_p()
    assert L.bb_arena_create(handle, handle, 8, C.byref(out)) == _lib.ERR_ARG
    assert "two engines" in _lib.last_error()
    assert L.bb_arena_create(handle, None, 8, C.byref(out)) == _lib.ERR_ARG
    assert L.bb_arena_create(None, handle, 8, C.byref(out)) == _lib.ERR_ARG
    assert L.bb_arena_create(handle, handle, 8, None) == _lib.ERR_ARG
    assert out.value is None and not keep.any()


def test_python_wrapper_maps_the_refusals_to_value_error():
    class _NoEngine:
        h = None
    with pytest.raises(ValueError):
        _lib.Arena(_NoEngine(), _NoEngine(), log_plies=4)


class _Player(DynamicMCTS):
    def __init__(self, **kw):
        DynamicMCTS.__init__(self, explorationRate=0.85, **kw)
        self.Game = Connect4.BoardState


def test_default_loop_is_host():
    assert MCTS.ArenaLoop == 'host'
    assert _Player(playLimit=8).ArenaLoop == 'host'
    a, b = _Player(playLimit=8), _Player(playLimit=8)
    assert arena._choose_loop(a, b, None, None, None) == 'host'
    assert arena._choose_loop(a, b, None, None, 'device') == 'device'
    a.ArenaLoop = 'device'
    assert arena._choose_loop(a, b, None, None, None) == 'device'
    assert arena._choose_loop(a, b, None, None, 'host') == 'host'
    with pytest.raises(ValueError, match="'host' or 'device'"):
        arena._choose_loop(a, b, None, None, 'gpu')


@pytest.mark.parametrize("case", ["random", "time_only", "uniforms"])
def test_explicit_device_loop_names_what_it_cannot_play(case):
    a = _Player(playLimit=8)
    kw = {}
    if case == "random":
        b, word = RandomMCTS(), "RandomMCTS"
    elif case == "time_only":
        b, word = FixedMCTS(maxDepth=3, explorationRate=0.85, timeLimit=0.05), "TimeLimit"
        b.Game = a.Game
    else:
        b, word = _Player(playLimit=8), "uniforms"
        kw["uniforms"] = np.random.RandomState(0).random_sample
    with pytest.raises(ValueError, match=word):        # raised before any engine is made: no GPU needed
        arena.TestModelsBatched(a, b, 0, 4, loop='device', **kw)
    if case == "time_only":                            # with a playLimit for the call the budget is simulations again
        assert arena._choose_loop(a, b, 8, None, 'device') == 'device'


def test_device_preference_falls_back_to_host_for_a_random_side():
    a = _Player(playLimit=8)
    a.ArenaLoop = 'device'
    arena.last_loop = None
    try:
        arena.TestModelsBatched(a, RandomMCTS(), 0, 2, first=[True, False])
    except _lib.BlackbirdHipError:
        assert _lib.lib().bb_device_count() == 0       # no GPU: the engines cannot be made -- the loop was chosen before
    assert arena.last_loop == 'host'


def test_start_states_need_the_device_loop():
    a, b = _Player(playLimit=8), _Player(playLimit=8)
    with pytest.raises(ValueError, match="device loop"):
        arena.TestModelsBatched(a, b, 0, 1, startStates=[Connect4.BoardState()])
    with pytest.raises(ValueError, match="one state per game"):
        arena.TestModelsBatched(a, b, 0, 2, loop='device', startStates=[Connect4.BoardState()])
