"""-m gpu: the batched arena (blackbird_amd/arena.py) against the serial TestModels mirror
(Blackbird.py:177-216 semantics: FindMove on my turns, MoveRoot by both sides after every move)."""
import random

import numpy as np
import pytest

from blackbird_amd import Blackbird, Connect4, TicTacToe
from blackbird_amd.RandomMCTS import RandomMCTS
from blackbird_amd.arena import TestModelsBatched

from tests import model_cases as M

pytestmark = pytest.mark.gpu


def _model(game, name, tmp_seed, play_limit, eps=0.0):
    return M.model(game, name, seed=tmp_seed, play_limit=play_limit, eps=eps, blocks=2)


def _serial(model1, model2, temp, first):
    """TestModels with the coin flips replaced by `first` (same loop as Blackbird.TestModels)."""
    out = []
    for f in first:
        model1ToMove = bool(f)
        model1Player = 1 if model1ToMove else 2
        model1.DropRoot()
        model2.DropRoot()
        state = model1.Game()
        winner = None
        while winner is None:
            (state, *_) = (model1 if model1ToMove else model2).FindMove(state, temp)
            model1.MoveRoot(state)
            model2.MoveRoot(state)
            model1ToMove = not model1ToMove
            winner = state.Winner()
        out.append(1 if winner == model1Player else (0 if winner == 0 else -1))
    return np.array(out)


@pytest.mark.parametrize("game", [Connect4.BoardState, TicTacToe.BoardState])
def test_batched_arena_equals_serial_when_deterministic(tmp_path, monkeypatch, game):
    """temp = 0 and epsilon = 0: no random number is consumed, so every game must end exactly as in the serial loop."""
    monkeypatch.chdir(tmp_path)
    m1, m2 = _model(game, "a", 1, 24), _model(game, "b", 2, 24)
    first = np.array([True, False, True, True, False, False, True, False])
    serial = _serial(m1, m2, 0, first)
    batched = TestModelsBatched(m1, m2, 0, len(first), first=first)
    assert np.array_equal(serial, batched)
    assert set(np.unique(batched)) <= {-1, 0, 1}


def test_batched_arena_against_random_player_and_coin(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    m1 = _model(Connect4.BoardState, "a", 3, 48, eps=0.3)
    rnd = RandomMCTS()
    random.seed(7)
    np.random.seed(7)
    res = TestModelsBatched(m1, rnd, 0.5, 64)
    assert res.shape == (64,) and set(np.unique(res)) <= {-1, 0, 1}
    assert (res == 1).sum() > (res == -1).sum()  # 48 simulations per move beat uniformly random moves
    with pytest.raises(ValueError):
        TestModelsBatched(m1, rnd, 0.5, 0)


# ---- against the oracle ------------------------------------------------------------------------
from blackbird_amd import _lib  # noqa: E402
from blackbird_amd.DynamicMCTS import DynamicMCTS  # noqa: E402
from blackbird_amd.FixedMCTS import FixedMCTS  # noqa: E402
from tests import arena_cases as AC  # noqa: E402


class _HashPlayer(DynamicMCTS):
    """DynamicMCTS on the deterministic validation evaluator (same integer hash in the oracle): results must be exact."""
    _EVALUATOR = _lib.EVAL_HASH

    def __init__(self, game, salt, **kw):
        DynamicMCTS.__init__(self, **kw)
        self.Game, self.salt = game, salt

    def _make_engine(self, game_id, n_slots, sims, **kw):
        return _lib.Engine(game_id, n_slots=n_slots, sims_per_move=max(int(sims), 1), mcts_kind=self._KIND,
                           evaluator=_lib.EVAL_HASH, hash_salt=self.salt, c_puct=float(self.ExplorationRate), seed=77, **kw)


class _RolloutFixed(FixedMCTS):
    """TestGood's opponent (Blackbird.py:164): FixedMCTS with random rollouts, here with a play limit and a fixed seed."""

    def __init__(self, game, **kw):
        FixedMCTS.__init__(self, **kw)
        self.Game = game

    def _make_engine(self, game_id, n_slots, sims, **kw):
        return _lib.Engine(game_id, n_slots=n_slots, sims_per_move=max(int(sims), 1), mcts_kind=self._KIND,
                           max_depth=self._max_depth(), evaluator=_lib.EVAL_ROLLOUT, c_puct=float(self.ExplorationRate),
                           seed=77, **kw)


@pytest.mark.parametrize("key,temp", [("c4", 0), ("ttt", 0), ("c4", 1.0), ("ttt_rollout", 0), ("c4_rollout", 0), ("c4", 0.1),
                                      ("ttt", 0.1)])
def test_batched_arena_equals_two_searcher_oracle(orc, key, temp):
    """TestModelsBatched against the oracle's own two-searcher game loop, game by game: hash-evaluator DynamicMCTS with
    different salts / exploration rates on the two sides (exact), at temp 0 (PUCT argmax move), temp 1 (sampled moves, same
    uniforms) and the exploitation temperature 0.1 of every evaluation game (N ** 10 through pow; tests/test_sample_temp_cpu.py
    holds every draw of these two cases 2^-40 away from the boundaries of its cdf, so the comparison stays exact); and
    DynamicMCTS against the rollout FixedMCTS that TestGood uses, on TicTacToe and on Connect4."""
    game = TicTacToe.BoardState if key.startswith("ttt") else Connect4.BoardState
    og = 1 if key.startswith("ttt") else 0
    first, sims = AC.FIRST, AC.SIMS
    p1 = _HashPlayer(game, 11, explorationRate=0.85, playLimit=sims[0])
    cfg1, cfg2 = AC.hash_cfgs(orc, og)
    if key.endswith("_rollout"):
        p2 = _RolloutFixed(game, maxDepth=10, explorationRate=0.85, playLimit=sims[1])
        cfg2 = orc.make_cfg(og, kind=orc.FIXED, max_depth=10, evaluator=orc.EVAL_ROLLOUT, c_puct=0.85, seed=77)
    else:
        p2 = _HashPlayer(game, 22, explorationRate=1.3, playLimit=sims[1])
    rng_a, rng_b = np.random.RandomState(AC.UNIFORM_SEED), np.random.RandomState(AC.UNIFORM_SEED)
    got = TestModelsBatched(p1, p2, temp, len(first), first=first, uniforms=rng_a.random_sample)
    want = AC.oracle_arena(orc, og, (cfg1, cfg2), sims, first, temp, rng_b.random_sample)
    assert np.array_equal(got, want), (got, want)


def test_test_models_and_tally_go_through_the_arena(tmp_path, monkeypatch):
    """Blackbird.TestModels plays one game and returns its result; TestRandom logs every game (Blackbird.py:84-111)."""
    monkeypatch.chdir(tmp_path)
    m1 = _model(TicTacToe.BoardState, "a", 3, 24)
    random.seed(3)
    np.random.seed(3)
    assert Blackbird.TestModels(m1, RandomMCTS(), 0.5, 5) in (-1, 0, 1)
    stats = Blackbird.TestRandom(m1, 0.5, 7)
    assert sum(stats.values()) == 7
    rows = m1.Conn.Cursor.execute("SELECT COUNT(*) FROM TrainingStatisticsFact;").fetchone()[0]
    assert rows == 7
    # a time-limited searcher (TestGood's FixedMCTS(timeLimit=...)) searches until its budget is spent, every move
    good = FixedMCTS(maxDepth=10, explorationRate=0.85, timeLimit=0.05)
    good.Game = m1.Game
    res = TestModelsBatched(m1, good, 0.5, 4)
    assert res.shape == (4,) and set(np.unique(res)) <= {-1, 0, 1}
    m1.Conn.Close()
