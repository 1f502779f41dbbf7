"""The one-launch search of the rollout evaluator (bb_search_rollouts, MCTS.SearchRollouts) where no GPU is needed: the entry
point in the header, in the library and in the binding, and the front end calling the setter on exactly the engines it is for."""
import ctypes as C
import os
import re

import pytest

from blackbird_amd import Blackbird, Connect4, DragonChess, TicTacToe, _lib
from blackbird_amd.DynamicMCTS import DynamicMCTS
from blackbird_amd.FixedMCTS import FixedMCTS
from blackbird_amd.MCTS import MCTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "blackbird_hip.h")
GAMES = {"c4": Connect4.BoardState, "ttt": TicTacToe.BoardState, "dc": DragonChess.BoardState}
NET_CFG = {"blocks": 2, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": {"optimizer": "adam"}}


def test_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+bb_search_rollouts\s*\(\s*bb_engine\s*\*\s*e\s*,\s*int\s+on\s*\)\s*;", code)
    assert "bb_search_rollouts" in _lib.EXPORTS
    fn = _lib.lib().bb_search_rollouts          # (AttributeError: the library does not export it)
    assert list(fn.argtypes) == [C.c_void_p, C.c_int] and fn.restype is C.c_int


@pytest.mark.parametrize("on", [0, 1, 2])
def test_null_engine_is_an_argument_error(on):
    assert _lib.lib().bb_search_rollouts(None, on) == _lib.ERR_ARG


def test_attribute_defaults_to_off():
    assert MCTS.SearchRollouts is False and FixedMCTS.SearchRollouts is False and Blackbird.Model.SearchRollouts is False


@pytest.fixture
def engines(monkeypatch):
    """Every _lib.Engine(...) the front end creates, as a stand-in that records its arguments and the setter's calls (nothing
    is created: no GPU here)."""
    made = []

    class Fake(object):
        def __init__(self, game, **kw):
            self.game, self.kw, self.rollouts = game, kw, []
            self.info = _lib.game_info(game)
            made.append(self)

        def search_rollouts(self, on=True):
            self.rollouts.append(on)

        def load_weights(self, flat):
            pass

    monkeypatch.setattr(_lib, "Engine", Fake)
    return made


def _searchers():
    return {"fixed": FixedMCTS(maxDepth=10, explorationRate=0.85, playLimit=16),
            "dynamic": DynamicMCTS(explorationRate=0.85, playLimit=16)}


@pytest.mark.parametrize("launch", ["lockstep", "wave"])
@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("kind", ["fixed", "dynamic"])
@pytest.mark.parametrize("key", list(GAMES))
def test_setter_is_called_exactly_for_wave_rollout_engines(monkeypatch, engines, key, kind, on, launch):
    monkeypatch.setattr(MCTS, "SearchLaunch", launch)
    monkeypatch.setattr(MCTS, "SearchRollouts", on)
    m = _searchers()[kind]
    cls = GAMES[key]
    m._ensure_engine(cls())                                   # what FindMove / MoveRoot / ResetRoot / Children search with
    m._make_engine(cls.GAME_ID, 4, 16, node_capacity=1088)    # the arena's engines: one slot per game (arena._Searcher)
    assert len(engines) == 2
    for e in engines:
        assert e.kw["evaluator"] == _lib.EVAL_ROLLOUT
        assert e.kw["launch"] == (_lib.LAUNCH_WAVE if launch == "wave" else _lib.LAUNCH_AUTO)
        assert e.rollouts == ([True] if on and launch == "wave" else []), (key, kind, on, launch, e.rollouts)


@pytest.mark.parametrize("on", [False, True])
def test_setter_is_never_called_for_a_model(tmp_path, monkeypatch, engines, on):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(MCTS, "SearchLaunch", "wave")
    monkeypatch.setattr(MCTS, "SearchRollouts", on)
    m = Blackbird.Model(Connect4.BoardState, "m", {"explorationRate": 0.85, "playLimit": 16}, NET_CFG)
    m._ensure_engine(Connect4.BoardState())
    m._make_engine(_lib.GAME_CONNECT4, 4, 16, node_capacity=1088)
    assert len(engines) == 2
    assert all(e.kw["evaluator"] == _lib.EVAL_NET and e.kw["launch"] == _lib.LAUNCH_WAVE and e.rollouts == [] for e in engines)


def test_setter_is_not_called_for_another_evaluator(monkeypatch, engines):
    class HashSearch(DynamicMCTS):
        _EVALUATOR = _lib.EVAL_HASH

    monkeypatch.setattr(MCTS, "SearchLaunch", "wave")
    monkeypatch.setattr(MCTS, "SearchRollouts", True)
    HashSearch(explorationRate=0.85, playLimit=16)._ensure_engine(Connect4.BoardState())
    assert len(engines) == 1 and engines[0].rollouts == []


@pytest.mark.parametrize("launch", ["lockstep", "wave"])
@pytest.mark.parametrize("bad", [1, 0, "wave", None])
def test_a_value_that_is_no_bool_is_refused(tmp_path, monkeypatch, engines, bad, launch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(MCTS, "SearchLaunch", launch)
    monkeypatch.setattr(MCTS, "SearchRollouts", bad)
    for m in _searchers().values():
        with pytest.raises(ValueError, match="SearchRollouts"):
            m._ensure_engine(Connect4.BoardState())
    model = Blackbird.Model(Connect4.BoardState, "m", {"explorationRate": 0.85, "playLimit": 16}, NET_CFG)
    with pytest.raises(ValueError, match="SearchRollouts"):
        model._make_engine(_lib.GAME_CONNECT4, 4, 16)
    assert engines == []
