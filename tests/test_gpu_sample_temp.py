"""-m gpu: move choice at temperatures other than 1, in every structure that chooses a move.

The reference plays self-play at temp 1 and EVERY evaluation game at temp 0.1 (FindMove's own default); until this file the suite
reached choose_move<G> / dc_choose_move on the GPU at temp 1 almost only, which takes the `1 / temp == 1.0` shortcut and never
calls pow.  The yardstick is the oracle, pinned to the reference's numpy expression in tests/test_sample_temp_cpu.py, which also
shows that every draw compared here keeps a relative distance of 2^-40 from the boundaries of its cdf -- far more than two pow
implementations can differ by -- so every comparison is exact.

1. bb_sample_moves on Connect4 and TicTacToe roots (initial, full column / taken cells, one legal move), lock-step and one-launch
   search, over temps {0.1, 0.3, 0.5, 0.7, 2.0, 50.0}, mid-interval and boundary draws, and the keyed draw (u = None).
2. Self-play at temp 0.1, 0.5 and 0 (the PUCT-argmax move, which consumes no draw): lock-step against the oracle for all three
   games; queue kernel, rounds, DragonChess one-wave kernel and the rollout wave kernels byte-identical to lock-step.
3. N ** (1 / temp) overflowing: BB_ERR_NAN / ValueError / a parked slot instead of the last child."""
import ctypes as C

import numpy as np
import pytest

from blackbird_amd import _lib
from tests import arena_cases as AC
from tests import temp_cases as T
from tests import model_cases as M
from tests import selfplay_cases as SS

pytestmark = pytest.mark.gpu
C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
OG = SS.OG


def _sample_engine(orc, game, launch):
    """The SAMPLE engine of tests/temp_cases.py on the roots the oracle searched, after its 48 simulations."""
    og, S = OG[game], T.SAMPLE
    rows = T.sample_oracle(orc, og)
    packed = []
    for st, _o in rows:
        board, player, prev = T.root_arrays(orc, og, st)
        packed.append(_lib.pack_grid(game, board[None], [player], [prev]))
    eng = _lib.Engine(game, n_slots=S["n_slots"], sims_per_move=S["sims"], evaluator=_lib.EVAL_HASH, hash_salt=S["salt"],
                      salt_per_game=True, seed=S["seed"], launch=launch)
    assert eng.run_sims_structure() == launch
    eng.set_roots(np.concatenate(packed), game_ids=np.arange(S["n_slots"]))
    eng.run_sims(S["sims"])
    return eng, rows


# ---- 1. bb_sample_moves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch", [_lib.LAUNCH_LOCKSTEP, _lib.LAUNCH_WAVE], ids=["lockstep", "wave"])
@pytest.mark.parametrize("game", [C4, TTT], ids=["c4", "ttt"])
def test_sample_moves_follow_the_oracle_at_every_temperature(orc, game, launch):
    og, A, n = OG[game], _lib.game_info(game).A, T.SAMPLE["n_slots"]
    eng, rows = _sample_engine(orc, game, launch)
    out = eng.sample_moves(1.0, np.full(n, 0.5))
    for s, (_st, o) in enumerate(rows):        # the roots are the oracle's: as test_find_move_golden compares them
        assert np.array_equal(out["child_plays"][s, :A].astype(np.float64), o["plays"]), (s, out["child_plays"][s], o["plays"])
        n32 = out["child_plays"][s, :A].astype(np.float32)
        wr = np.where(n32 > 0, out["child_value"][s, :A] / np.maximum(n32, 1), 0).astype(np.float64)
        assert np.array_equal(wr, o["winrates"]), s
        assert out["root_plays"][s] == o["root_plays"] and float(out["root_winrate"][s]) == o["winrate"], s
        assert out["action"][s] == o["action"], s
    compared = 0
    for temp in T.TEMPS:
        per_slot = [T.draws(o["plays"], temp) for _st, o in rows]   # (a slot whose visited children are all next to a share
        for j in range(max(len(d) for d in per_slot)):              # under 2^-30 at this temp has none: it sits the temp out)
            u = np.array([d[j][2] if j < len(d) else 0.5 for d in per_slot])
            got = eng.sample_moves(temp, u)["action"]
            for s, (_st, o) in enumerate(rows):
                if j < len(per_slot[s]):
                    want = orc.sample_action(o["plays"], temp, float(u[s]))
                    assert want >= 0 and got[s] == want, (temp, s, per_slot[s][j], got[s], want, o["plays"])
                    compared += 1
                else:
                    assert got[s] >= 0, (temp, s)
    assert compared >= T.SAMPLE_MIN_DRAWS
    # u = None: the engine draws from (seed, game id, ply 0), and so does the oracle's find_move for u < 0
    got = eng.sample_moves(0.1, None)["action"]
    for s, (st, _o) in enumerate(rows):
        cfg = orc.make_cfg(og, evaluator=orc.EVAL_HASH, salt=T.SAMPLE["salt"] + s, seed=T.SAMPLE["seed"])
        assert got[s] == orc.Search(cfg, s).find_move(st, 0.1, T.SAMPLE["sims"], u=-1.0, ply=0)["action"], s
    assert eng.counters()["overflow"] == 0
    eng.close()


# ---- 2. self-play --------------------------------------------------------------------------------------------------------------------
def _lockstep_engine(game, seed=None):
    L = T.LOCKSTEP
    eng = _lib.Engine(game, n_slots=L["n_slots"], sims_per_move=L["sims"], evaluator=_lib.EVAL_HASH, hash_salt=L["salt"],
                      salt_per_game=True, seed=L["seed"] if seed is None else seed, max_games=L["n_games"],
                      first_game_id=L["first_id"], launch=_lib.LAUNCH_LOCKSTEP, max_plies=T.DC_MAX_PLIES if game == DC else None)
    assert eng.selfplay_mode() == 0 and eng.max_plies == T.lockstep_max_plies(OG[game])
    return eng


@pytest.mark.parametrize("temp", T.SELFPLAY_TEMPS)
@pytest.mark.parametrize("game", [C4, TTT, DC], ids=["c4", "ttt", "dc"])
def test_lockstep_hash_selfplay_vs_oracle(orc, game, temp):
    """7 games on 3 slots, 24 simulations; at temp 0 the move is the PUCT argmax and no draw is consumed, so an engine with
    another seed plays the same games.  The oracle's games come from SC.oracle_selfplay_from, the loop over Search.find_move that
    also records each move's plays and draw (draw_margins needs them); tests/test_sample_temp_cpu.py pins that loop to
    orc.selfplay_game at temps 0.1, 0.5 and 0, game by game."""
    L = T.LOCKSTEP
    eng = _lockstep_engine(game)
    out = SS.play_from_starts(eng, L["n_games"], temp=temp)
    eng.close()
    games = T.lockstep_games(orc, OG[game], temp)
    for k, o in enumerate(games):
        SS.assert_game_is_the_oracles(game, out, k, o, L["first_id"])
    assert out["cnt"]["sims"] == sum(o["stats"].sims for o in games) and out["cnt"]["examples"] == len(out["rec"])
    if temp == 0:
        other = _lockstep_engine(game, seed=L["seed"] + 1)
        SS.assert_same_runs(out, SS.play_from_starts(other, L["n_games"], temp=0.0), "another seed")
        other.close()


@pytest.mark.parametrize("temp", T.SELFPLAY_TEMPS)
@pytest.mark.parametrize("game,n_slots,n_games,sims", [(C4, 19, 24, 24), (TTT, 16, 21, 24)], ids=["c4", "ttt"])
def test_dense_launch_structures_are_byte_identical(game, n_slots, n_games, sims, temp):
    """1-block network, prior noise on: queue kernel (mode 3), rounds (mode 1), lock-step (mode 0)."""
    runs, modes = {}, {}
    for name, launch in (("queue", _lib.LAUNCH_AUTO), ("rounds", _lib.LAUNCH_ROUNDS), ("lockstep", _lib.LAUNCH_LOCKSTEP)):
        eng, _flat = SS.net_engine(game, n_slots, n_games, sims, 1, launch=launch, seed=5, first_id=0)
        modes[name] = eng.selfplay_mode()
        runs[name] = SS.play_from_starts(eng, n_games, step=2, temp=temp)
        eng.close()
    assert modes == {"queue": 3, "rounds": 1, "lockstep": 0}
    for other in ("rounds", "lockstep"):
        SS.assert_same_runs(runs["queue"], runs[other], (other, temp))


@pytest.mark.parametrize("temp", T.SELFPLAY_TEMPS)
def test_dc_one_wave_kernel_is_lockstep(temp):
    n_slots, n_games, sims = 5, 9, 12
    runs, modes = {}, {}
    for name, launch in (("wave", _lib.LAUNCH_AUTO), ("lockstep", _lib.LAUNCH_LOCKSTEP)):
        eng, _flat = SS.net_engine(DC, n_slots, n_games, sims, 1, launch=launch, seed=7, first_id=0, max_plies=5)
        modes[name] = eng.selfplay_mode()
        runs[name] = SS.play_from_starts(eng, n_games, temp=temp)
        eng.close()
    assert modes == {"wave": 5, "lockstep": 0}
    SS.assert_same_runs(runs["wave"], runs["lockstep"], ("dc", temp))


@pytest.mark.parametrize("temp", T.SELFPLAY_TEMPS)
@pytest.mark.parametrize("game", [C4, TTT, DC], ids=["c4", "ttt", "dc"])
@pytest.mark.parametrize("fixed", [True, False], ids=["fixed3", "dynamic"])
def test_rollout_wave_selfplay_is_lockstep(game, fixed, temp):
    """The one-launch rollout self-play (mode 6), FixedMCTS(maxDepth 3) and DynamicMCTS, against its lock-step run."""
    n_slots, n_games, sims = 5, 9, 12
    runs = {}
    for wave in (True, False):
        eng = _lib.Engine(game, n_slots=n_slots, sims_per_move=sims, mcts_kind=_lib.MCTS_FIXED if fixed else _lib.MCTS_DYNAMIC,
                          max_depth=3, evaluator=_lib.EVAL_ROLLOUT, seed=31, max_games=n_games, first_game_id=1000,
                          max_plies=5 if game == DC else None)
        eng.selfplay_rollouts(wave)
        assert eng.selfplay_mode() == (6 if wave else 0)
        runs[wave] = SS.play_from_starts(eng, n_games, temp=temp)
        eng.close()
    SS.assert_same_runs(runs[True], runs[False], (game, fixed, temp))
    assert {k: runs[True]["cnt"][k] for k in SS.COUNTERS} == {k: runs[False]["cnt"][k] for k in SS.COUNTERS}


# ---- 3. N ** (1 / temp) overflows ---------------------------------------------------------------------------------------------------
def test_sample_moves_refuses_an_overflowing_temperature_connect4(orc):
    """48 simulations: 47 or 48 visits over at most 7 children give some child >= 7, and 7 ** 500 = inf.  inf / inf is NaN in the
    reference and np.random.choice raises; the engine answers BB_ERR_NAN per slot (not the last child: column 6, legal or not)
    and FindMove raises ValueError.  (Engine.sample_moves itself does not raise: bb_sample_moves reports per slot, which
    tests/test_gpu_mcts.py::test_error_mapping holds; the ValueError is the front end's, MCTS.FindMove.)"""
    from blackbird_amd import Connect4
    n = T.SAMPLE["n_slots"]
    eng, rows = _sample_engine(orc, C4, _lib.LAUNCH_LOCKSTEP)
    for u in (np.full(n, 0.5), np.zeros(n), None):
        out = eng.sample_moves(T.OVERFLOW_TEMP, u)
        assert (out["action"] == _lib.ERR_NAN).all(), out["action"]
        for s, (_st, o) in enumerate(rows):     # the statistics are reported all the same
            assert np.array_equal(out["child_plays"][s, :7].astype(np.float64), o["plays"]) and o["plays"].max() >= 7
            assert orc.sample_action(o["plays"], T.OVERFLOW_TEMP, 0.5) == -3
    assert (eng.sample_moves(50.0, np.full(n, 0.5))["action"] >= 0).all()     # the tree is untouched, a sane temp still samples
    eng.close()
    player = AC.HashPlayer(Connect4.BoardState, 11, playLimit=48)
    with pytest.raises(ValueError, match="NaN"):
        player.FindMove(Connect4.BoardState(), T.OVERFLOW_TEMP)
    nxt, _wr, _p = player.FindMove(Connect4.BoardState(), 50.0)                # (the same root, 48 more simulations)
    assert nxt.Winner() is None


def test_sample_moves_refuses_an_overflowing_temperature_dragonchess(orc):
    from blackbird_amd import DragonChess
    n, S = T.SAMPLE["n_slots"], T.SAMPLE
    eng = _lib.Engine(DC, n_slots=n, sims_per_move=S["sims"], evaluator=_lib.EVAL_HASH, hash_salt=S["salt"], salt_per_game=True,
                      seed=S["seed"])
    eng.set_roots(np.repeat(_lib.game_initial(DC), n, axis=0), game_ids=np.arange(n))
    eng.run_sims(S["sims"])
    for u in (np.full(n, 0.5), None):
        out = eng.sample_moves(T.OVERFLOW_TEMP, u)
        assert (out["action"] == _lib.ERR_NAN).all(), out["action"]
        assert (out["child_plays"].max(axis=1) >= 7).all() and (out["root_plays"] == S["sims"]).all()
    o = orc.Search(orc.make_cfg(orc.DC, evaluator=orc.EVAL_HASH, salt=S["salt"], seed=S["seed"])).find_move(
        orc.new_state(orc.DC), 1.0, S["sims"], u=0.5)
    k = int((out["child_action"][0] >= 0).sum())
    assert np.array_equal(out["child_plays"][0, :k].astype(np.float64), o["plays"][out["child_action"][0, :k]])
    ok = eng.sample_moves(50.0, np.full(n, 0.5))
    assert (ok["action"] >= 0).all() and ok["action"][0] == orc.sample_action(o["plays"], 50.0, 0.5)
    eng.close()
    player = AC.HashPlayer(DragonChess.BoardState, 11, playLimit=48)
    with pytest.raises(ValueError, match="NaN"):
        player.FindMove(DragonChess.BoardState(), T.OVERFLOW_TEMP)


def test_lockstep_selfplay_parks_its_slots_at_an_overflowing_temperature(orc):
    """Where the reference's GenerateTrainingSamples stops with ValueError the slot stops too: no move, no record, one count in
    the error counter per slot, and nothing more happens to it."""
    L = T.LOCKSTEP
    eng = _lib.Engine(C4, n_slots=L["n_slots"], sims_per_move=48, evaluator=_lib.EVAL_HASH, hash_salt=L["salt"], salt_per_game=True,
                      seed=L["seed"], max_games=L["n_games"], first_game_id=L["first_id"], launch=_lib.LAUNCH_LOCKSTEP)
    assert eng.selfplay_mode() == 0
    eng.reset_counters()
    eng.selfplay_begin(L["n_games"], T.OVERFLOW_TEMP)
    seen = []
    for steps in (1, 2):
        eng.selfplay_step(steps)
        assert eng.selfplay_done() == (False, 0)
        cnt = eng.counters()
        assert cnt["games_finished"] == 0 and cnt["overflow"] == L["n_slots"], cnt
        assert cnt["examples"] == 0 and cnt["plies"] == 0 and cnt["sims"] > 0, cnt
        assert not eng.selfplay_headers().any()
        seen.append(cnt)
    assert seen[0] == seen[1]                       # a parked slot searches no further
    eng.close()
    with pytest.raises(RuntimeError, match="rc=-3"):
        orc.selfplay_game(T.lockstep_cfg(orc, 0, 0), L["first_id"], T.OVERFLOW_TEMP, 48, 42)


def test_generate_training_samples_raises_at_an_overflowing_temperature(tmp_path, monkeypatch):
    from blackbird_amd import Blackbird, Connect4
    monkeypatch.chdir(tmp_path)
    np.random.seed(11)
    m = Blackbird.Model(Connect4.BoardState, "hot", {"explorationRate": 0.85, "playLimit": 48}, M.net_config(blocks=1, eps=0.3))
    np.random.seed(21)
    with pytest.raises(ValueError, match="NaN"):
        Blackbird.GenerateTrainingSamples(m, 3, T.OVERFLOW_TEMP)
    assert len(m.Conn.GetGames(m.Name, m.Version)) == 0
    Blackbird.GenerateTrainingSamples(m, 3, 50.0)        # a near-uniform choice over the visited children; the engine recovers
    assert len(m.Conn.GetGames(m.Name, m.Version)) >= 3 * 8
    m._batch_engine.close()
    m.Conn.Close()


def test_arena_reports_nan_for_every_game_at_an_overflowing_temperature():
    from blackbird_amd import Connect4
    players = (AC.HashPlayer(Connect4.BoardState, 11, playLimit=48), AC.HashPlayer(Connect4.BoardState, 22, c_puct=1.3, playLimit=48))
    ea, eb = AC.searcher_engines(players, 5)
    ar = _lib.Arena(ea, eb, log_plies=4)
    try:
        ar.begin([True, False, True, True, False], T.OVERFLOW_TEMP)
        ar.step(1)
        alive = C.c_int(-1)
        assert _lib.lib().bb_arena_status(ar.h, C.byref(alive)) == _lib.ERR_NAN and "action -4" in _lib.last_error()
        assert alive.value == 0                       # every game stopped ...
        with pytest.raises(ValueError, match="NaN"):
            ar.status()
        out = ar.fetch()
        assert not out["plies"].any() and (out["moves"] == -1).all() and not out["result"].any()   # ... without a move
        assert np.array_equal(out["states"], np.repeat(_lib.game_initial(C4), 5, axis=0))
    finally:
        ar.close()
        ea.close()
        eb.close()
