"""The evaluation cache of the one-launch search (bb_config.search_cache, MCTS.SearchEvalCache) where no GPU is needed: the
field in the header and in the binding, and the front end handing the option to the engines it creates for the search API."""
import inspect
import os
import re

import pytest

from blackbird_amd import Blackbird, Connect4, DragonChess, _lib
from blackbird_amd.DynamicMCTS import DynamicMCTS
from blackbird_amd.MCTS import MCTS
from tests.model_cases import Recorded, engine_args  # noqa: F401  (engine_args: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "blackbird_hip.h")
GAMES = {"c4": (Connect4.BoardState, _lib.GAME_CONNECT4), "dc": (DragonChess.BoardState, _lib.GAME_DRAGONCHESS)}


def test_header_and_binding_end_with_search_cache():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*bb_config\s*;", code).group(1)
    fields = re.findall(r"\b(\w+)\s*[;,]", body)
    assert fields[-2:] == ["track_ancestors", "search_cache"], fields[-4:]
    assert re.search(r"int32_t\s+search_cache\s*;", body)
    names = [n for n, _t in _lib.Config._fields_]
    assert names[-2:] == ["track_ancestors", "search_cache"]
    assert set(fields) == set(names)                      # (every member of the struct is bound: the layouts agree)


def test_engine_takes_search_cache_off_by_default():
    p = inspect.signature(_lib.Engine.__init__).parameters
    assert "search_cache" in p and p["search_cache"].default is False


def test_attribute_defaults_to_off():
    assert MCTS.SearchEvalCache is False and MCTS.SearchLaunch == "lockstep"


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("key", list(GAMES))
def test_searcher_passes_the_option_on(monkeypatch, engine_args, key, on):
    cls, gid = GAMES[key]
    monkeypatch.setattr(MCTS, "SearchLaunch", "wave")
    monkeypatch.setattr(MCTS, "SearchEvalCache", on)
    m = DynamicMCTS(explorationRate=0.85, playLimit=16)
    with pytest.raises(Recorded):
        m._ensure_engine(cls())                              # what FindMove / MoveRoot / ResetRoot search with
    assert engine_args["game"] == gid and engine_args["launch"] == _lib.LAUNCH_WAVE
    assert (engine_args.get("search_cache") is True) == on
    assert on or "search_cache" not in engine_args


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("key", list(GAMES))
def test_model_passes_the_option_on(tmp_path, monkeypatch, engine_args, key, on):
    cls, gid = GAMES[key]
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(MCTS, "SearchLaunch", "wave")
    monkeypatch.setattr(MCTS, "SearchEvalCache", on)
    cfg = {"blocks": 2, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": {"optimizer": "adam"}}
    m = Blackbird.Model(cls, "m", {"explorationRate": 0.85, "playLimit": 16}, cfg)
    with pytest.raises(Recorded):
        m._ensure_engine(cls())
    assert engine_args["evaluator"] == _lib.EVAL_NET and (engine_args.get("search_cache") is True) == on
    engine_args.clear()
    with pytest.raises(Recorded):                           # the arena's engines: one slot per game (arena._Searcher)
        m._make_engine(gid, 4, 16, node_capacity=1088)
    assert engine_args["n_slots"] == 4 and engine_args["launch"] == _lib.LAUNCH_WAVE
    assert (engine_args.get("search_cache") is True) == on
    engine_args.clear()
    monkeypatch.setattr(_lib, "fit_slots", lambda *a, **k: (4, 0))
    with pytest.raises(Recorded):                           # self-play engines are not concerned
        m._selfplay_engine(4)
    assert engine_args["launch"] == _lib.LAUNCH_AUTO and not engine_args.get("search_cache")


@pytest.mark.parametrize("bad", [1, 0, "wave", None])
def test_a_value_that_is_no_bool_is_refused(tmp_path, monkeypatch, engine_args, bad):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(MCTS, "SearchLaunch", "wave")
    monkeypatch.setattr(MCTS, "SearchEvalCache", bad)
    m = DynamicMCTS(explorationRate=0.85, playLimit=16)
    with pytest.raises(ValueError, match="SearchEvalCache"):
        m._ensure_engine(Connect4.BoardState())
    cfg = {"blocks": 2, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": {"optimizer": "adam"}}
    model = Blackbird.Model(Connect4.BoardState, "m", {"explorationRate": 0.85, "playLimit": 16}, cfg)
    with pytest.raises(ValueError, match="SearchEvalCache"):
        model._make_engine(_lib.GAME_CONNECT4, 4, 16)
