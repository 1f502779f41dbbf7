"""DragonChess under the one-launch search (BB_LAUNCH_WAVE) where no GPU is needed: the header says so, no entry point was
added for it, and the front end hands the launch to the engines it creates for the wide game."""
import os
import re

import pytest

from blackbird_amd import Blackbird, DragonChess, _lib
from blackbird_amd.DynamicMCTS import DynamicMCTS
from blackbird_amd.MCTS import MCTS
from tests.model_cases import Recorded, engine_args  # noqa: F401  (engine_args: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "blackbird_hip.h")


def test_header_names_dragonchess_under_launch_wave():
    text = open(HEADER).read()
    m = re.search(r"#define\s+BB_LAUNCH_WAVE\s+3\s*/\*(.*?)\*/", text, flags=re.S)
    assert m and "DragonChess" in m.group(1) and "bb_run_sims_structure" in m.group(1)


def test_no_new_entry_point():
    """The wide game searches through bb_run_sims / bb_run_sims_masked / bb_run_sims_structure like the others: every bb_*
    function the header declares is one the binding already lists, and the other way round."""
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(bb_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.EXPORTS)
    assert not any("wave" in name for name in declared)
    L = _lib.lib()
    assert all(hasattr(L, name) for name in declared)


@pytest.mark.parametrize("launch, want", [("wave", _lib.LAUNCH_WAVE), ("lockstep", _lib.LAUNCH_AUTO)])
def test_dragonchess_searcher_passes_the_launch_on(monkeypatch, engine_args, launch, want):
    monkeypatch.setattr(MCTS, "SearchLaunch", launch)
    m = DynamicMCTS(explorationRate=0.85, playLimit=16)
    with pytest.raises(Recorded):
        m._ensure_engine(DragonChess.BoardState())          # what FindMove / MoveRoot / ResetRoot search with
    assert engine_args["game"] == _lib.GAME_DRAGONCHESS and engine_args["launch"] == want
    assert engine_args["track_ancestors"] is True and engine_args["n_slots"] == 1


@pytest.mark.parametrize("launch, want", [("wave", _lib.LAUNCH_WAVE), ("lockstep", _lib.LAUNCH_AUTO)])
def test_dragonchess_model_passes_the_launch_on(tmp_path, monkeypatch, engine_args, launch, want):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(MCTS, "SearchLaunch", launch)
    cfg = {"blocks": 2, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": {"optimizer": "adam"}}
    m = Blackbird.Model(DragonChess.BoardState, "dc", {"explorationRate": 0.85, "playLimit": 16}, cfg)
    with pytest.raises(Recorded):
        m._ensure_engine(DragonChess.BoardState())
    assert engine_args["game"] == _lib.GAME_DRAGONCHESS and engine_args["launch"] == want
    assert engine_args["evaluator"] == _lib.EVAL_NET and engine_args["noise_on"] is True
    engine_args.clear()
    with pytest.raises(Recorded):                           # the arena's engines: one slot per game (arena._Searcher)
        m._make_engine(_lib.GAME_DRAGONCHESS, 4, 16, node_capacity=1088)
    assert engine_args["launch"] == want and engine_args["n_slots"] == 4
