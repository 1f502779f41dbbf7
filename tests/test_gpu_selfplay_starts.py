"""-m gpu: self-play from caller-given start positions (bb_selfplay_set_starts, GenerateTrainingSamples(startStates=...)).

Game k of a run starts from starts[k % n] in EVERY launch structure: lock-step, asynchronous rounds, the persistent Connect4 /
TicTacToe queue kernel (mode 3), the DragonChess one-wave kernel (mode 5) and the one-launch rollout self-play (mode 6).  The
yardstick is tests/selfplay_cases.py::oracle_selfplay_from, which tests/test_selfplay_starts_cpu.py pins to the committed oracle.

Start sets are fixed action lists applied to the initial position (no random boards).  Every run uses a table whose length
neither divides the number of games nor equals the number of slots, and more games than slots: the modulo wraps, and both the
begin sites and the refill site of every structure run.  All comparisons are exact."""
import numpy as np
import pytest

from blackbird_amd import _lib
from tests import dc_wide_cases as WC
from tests import model_cases as M
from tests import selfplay_cases as SP
from tests.selfplay_cases import ALPHA, COUNTERS, EPS, OG, assert_first_records_are, assert_games_are_the_oracles, starts_of

pytestmark = pytest.mark.gpu
C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
# ---- 1. against the oracle: lock-step, hash evaluator ----------------------------------------------------------------------------
@pytest.mark.parametrize("game", [C4, TTT, DC])
def test_lockstep_hash_selfplay_from_starts_vs_oracle(orc, game):
    """7 games on 3 slots over 4 starts: games 4..6 wrap the table, games 3..6 start in a refilled slot."""
    n_games, n_slots, sims, salt, seed, first_id = 7, 3, 16, 4242, 99, 1000
    starts = starts_of(game)
    eng = _lib.Engine(game, n_slots=n_slots, sims_per_move=sims, evaluator=_lib.EVAL_HASH, hash_salt=salt, salt_per_game=True,
                      seed=seed, max_games=n_games, first_game_id=first_id, launch=_lib.LAUNCH_LOCKSTEP,
                      max_plies=6 if game == DC else None)
    assert eng.selfplay_mode() == 0
    out = SP.play_from_starts(eng, n_games, starts)
    assert_first_records_are(game, out, starts, first_id)
    total = assert_games_are_the_oracles(
        orc, game, out, starts, lambda k: orc.make_cfg(OG[game], evaluator=orc.EVAL_HASH, salt=salt + k, seed=seed), first_id, sims,
        eng.max_plies)
    assert out["cnt"]["sims"] == total and out["cnt"]["examples"] == len(out["rec"])
    eng.close()


# ---- 2. against the oracle: the queue kernel, network and prior noise ------------------------------------------------------------
def test_queue_kernel_with_prior_noise_from_starts_vs_oracle(orc):
    """TicTacToe, 21 slots (one 16-game workgroup + 5: ragged), 30 games over 4 starts; the oracle's keyed callback gets the
    priors the engine's network waves drew for (game id, node serial): tests/test_gpu_noise_parity.py."""
    game, n_slots, n_games, sims, seed, first_id = TTT, 21, 30, 16, 17, 500
    gi = _lib.game_info(game)
    starts = starts_of(game)
    eng, flat = SP.net_engine(game, n_slots, n_games, sims, 1, seed=seed, first_id=first_id)
    assert eng.selfplay_mode() == 3
    out = SP.play_from_starts(eng, n_games, starts, step=2)
    max_plies = eng.max_plies
    eng.close()
    assert_first_records_are(game, out, starts, first_id)
    ev = _lib.Engine(game, n_slots=4, sims_per_move=2, evaluator=_lib.EVAL_NET, seed=seed, alpha=ALPHA, epsilon=EPS)
    ev.load_weights(flat)
    calls = {"with_policy": 0}

    def getpolicy(_ctx, stp, gid, serial, vp, pp):
        v, _l, p = ev.net_eval_keyed([gid], [serial], planes=orc.encode(OG[game], stp.contents))
        vp[0] = float(v[0])
        if pp:
            calls["with_policy"] += 1
            for a in range(gi.A):
                pp[a] = float(p[0, a])

    cfg = orc.make_cfg(OG[game], evaluator=orc.EVAL_CALLBACK_KEYED, seed=seed, cb2=orc.EVAL_CB2(getpolicy))
    total = assert_games_are_the_oracles(orc, game, out, starts, lambda k: cfg, first_id, sims, max_plies)
    assert out["cnt"]["sims"] == total and calls["with_policy"] > 0
    ev.close()


# ---- 3. the launch structures give the same bytes from starts --------------------------------------------------------------------
@pytest.mark.parametrize("game,n_slots,n_games,sims", [(C4, 19, 30, 24), (TTT, 16, 24, 24)])
def test_dense_launch_structures_from_starts_are_byte_identical(game, n_slots, n_games, sims):
    starts = starts_of(game)
    runs, modes = {}, {}
    for name, launch in (("queue", _lib.LAUNCH_AUTO), ("rounds", _lib.LAUNCH_ROUNDS), ("lockstep", _lib.LAUNCH_LOCKSTEP)):
        eng, _flat = SP.net_engine(game, n_slots, n_games, sims, 1, launch=launch, seed=5, first_id=0)
        modes[name] = eng.selfplay_mode()
        runs[name] = SP.play_from_starts(eng, n_games, starts, step=2)
        eng.close()
    assert modes == {"queue": 3, "rounds": 1, "lockstep": 0}
    assert_first_records_are(game, runs["queue"], starts)
    for other in ("rounds", "lockstep"):
        SP.assert_same_runs(runs["queue"], runs[other], other)


def test_dc_one_wave_kernel_from_starts_is_lockstep():
    game, n_slots, n_games, sims = DC, 5, 9, 12
    starts = starts_of(game)
    runs, modes = {}, {}
    for name, launch in (("wave", _lib.LAUNCH_AUTO), ("lockstep", _lib.LAUNCH_LOCKSTEP)):
        eng, _flat = SP.net_engine(game, n_slots, n_games, sims, 1, launch=launch, seed=7, first_id=0, max_plies=5)
        modes[name] = eng.selfplay_mode()
        runs[name] = SP.play_from_starts(eng, n_games, starts)
        eng.close()
    assert modes == {"wave": 5, "lockstep": 0}
    assert_first_records_are(game, runs["wave"], starts)
    SP.assert_same_runs(runs["wave"], runs["lockstep"], "dc")


@pytest.mark.parametrize("game", [C4, TTT, DC])
@pytest.mark.parametrize("fixed", [True, False], ids=["fixed3", "dynamic"])
def test_rollout_wave_selfplay_from_starts_is_lockstep(game, fixed):
    """The one-launch rollout self-play (mode 6), both wave kernels, FixedMCTS(maxDepth 3) and DynamicMCTS."""
    n_slots, n_games, sims = 5, 9, 12
    starts = starts_of(game)
    runs = {}
    for wave in (True, False):
        eng = _lib.Engine(game, n_slots=n_slots, sims_per_move=sims, mcts_kind=_lib.MCTS_FIXED if fixed else _lib.MCTS_DYNAMIC,
                          max_depth=3, evaluator=_lib.EVAL_ROLLOUT, seed=31, max_games=n_games, first_game_id=1000,
                          max_plies=5 if game == DC else None)
        eng.selfplay_rollouts(wave)
        assert eng.selfplay_mode() == (6 if wave else 0)
        runs[wave] = SP.play_from_starts(eng, n_games, starts)
        eng.close()
    assert_first_records_are(game, runs[True], starts, 1000)
    SP.assert_same_runs(runs[True], runs[False], (game, fixed))
    assert {k: runs[True]["cnt"][k] for k in COUNTERS} == {k: runs[False]["cnt"][k] for k in COUNTERS}


# ---- 4. the default path is untouched ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", [C4, TTT, DC])
def test_no_table_cleared_table_and_initial_table_are_the_same_run(game):
    """Never set / set and cleared with n = 0 / a table that holds the initial position: the same records and counters.
    (That the first of them is what the parent commit plays is held by every existing self-play test.)"""
    n_slots, n_games, sims = 3, 7, 16
    kw = dict(n_slots=n_slots, sims_per_move=sims, evaluator=_lib.EVAL_HASH, hash_salt=77, seed=5, max_games=n_games,
              max_plies=6 if game == DC else None)
    runs = []
    for table in ("never", "cleared", "initial"):
        eng = _lib.Engine(game, **kw)
        if table == "cleared":
            eng.selfplay_set_starts(starts_of(game))
            eng.selfplay_set_starts(None)
        runs.append(SP.play_from_starts(eng, n_games, _lib.game_initial(game) if table == "initial" else "keep"))
        eng.close()
    assert_first_records_are(game, runs[0], _lib.game_initial(game))
    for other in runs[1:]:
        SP.assert_same_runs(runs[0], other, game)
        assert {k: runs[0]["cnt"][k] for k in COUNTERS} == {k: other["cnt"][k] for k in COUNTERS}


# ---- 5. validation ---------------------------------------------------------------------------------------------------------------
def _refused(eng, table, index, reason_words):
    with pytest.raises(ValueError) as err:
        eng.selfplay_set_starts(table)
    msg = str(err.value)
    assert ("state %d " % index) in msg and reason_words in msg, msg


def test_states_no_game_can_start_from_are_refused():
    # Connect4: four in a row for player 1 at the bottom (after 0 0 1 1 2 2 3); refused for reason 1, at index 2 of the table
    st = _lib.game_initial(C4)
    for a in (0, 0, 1, 1, 2, 2, 3):
        st = SP._apply(C4, st, a)
    assert _lib.game_winner(C4, st)[0] == 1
    good = starts_of(C4)
    eng = _lib.Engine(C4, n_slots=3, sims_per_move=16, evaluator=_lib.EVAL_HASH, hash_salt=1, seed=2, max_games=7,
                      launch=_lib.LAUNCH_LOCKSTEP)
    eng.selfplay_set_starts(good)
    _refused(eng, np.concatenate([good[:2], st, good[2:]]), 2, "already over")
    out = SP.play_from_starts(eng, 7)                      # after the refusal the previous table is still in force
    assert_first_records_are(C4, out, good)
    eng.close()
    # TicTacToe: a full board without a line (X O X / X O O / O X X) is a draw: Winner() == 0, so reason 1 (the game is over)
    # fires, before reason 2 (no legal move, which also holds) is looked at
    st = _lib.game_initial(TTT)
    for a in (0, 1, 2, 4, 3, 5, 7, 6, 8):
        st = SP._apply(TTT, st, a)
    assert _lib.game_winner(TTT, st)[0] == 0 and _lib.game_legal(TTT, st).sum() == 0
    eng = _lib.Engine(TTT, n_slots=3, sims_per_move=16, evaluator=_lib.EVAL_HASH, max_games=7)
    _refused(eng, st, 0, "already over")
    out = SP.play_from_starts(eng, 7)                      # there was no table before: initial positions
    assert_first_records_are(TTT, out, _lib.game_initial(TTT))
    eng.close()
    # DragonChess: the hand-built position with 148 legal moves (more than S = 144): reason 3
    over = WC.Positions("over_")
    i = int(np.flatnonzero(over.n_legal == 148)[0])
    wide = over.packed(_lib, [i])
    assert _lib.game_winner(DC, wide)[0] < 0 and _lib.game_legal(DC, wide).sum() == 148
    good = starts_of(DC)
    eng = _lib.Engine(DC, n_slots=3, sims_per_move=16, evaluator=_lib.EVAL_HASH, max_games=7, max_plies=6)
    eng.selfplay_set_starts(good)
    _refused(eng, np.concatenate([good, wide]), 4, "more legal moves")
    # a king is missing: the game is over (reason 1)
    dead = good[:1].copy()
    dead[0, :64][dead[0, :64] == 1] = 0
    _refused(eng, np.concatenate([good[:1], dead]), 1, "already over")
    out = SP.play_from_starts(eng, 7)
    assert_first_records_are(DC, out, good)
    eng.close()


# ---- 6. the front end ------------------------------------------------------------------------------------------------------------
def test_generate_training_samples_from_start_states(tmp_path, monkeypatch):
    from blackbird_amd import Blackbird, TicTacToe
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(Blackbird, "MAX_CONCURRENT_GAMES", 2)   # a 2-slot engine: 5 games refill its slots
    cls = TicTacToe.BoardState
    s0, s1 = cls(), cls()
    s0.ApplyAction(4)
    for a in (0, 4, 1):
        s1.ApplyAction(a)
    start_states = [s0, s1]

    def model(name):
        np.random.seed(11)  # weight initialisation draws from numpy's stream
        m = Blackbird.Model(cls, name, {"explorationRate": 0.85, "playLimit": 16}, M.net_config(blocks=1, eps=0.3))
        games = []
        inner = m.Conn.PutGames
        monkeypatch.setattr(m.Conn, "PutGames", lambda *a: (games.append(list(a[3])), inner(*a))[1])
        return m, games

    m, games = model("starts")
    np.random.seed(21)
    Blackbird.GenerateTrainingSamples(m, 5, 1.0, startStates=start_states)
    eng = m._batch_engine
    assert eng.n_slots == 2 and len(games) == 5
    rec, offs, _win = eng.fetch_examples(0, 5)
    used = set()
    for k in range(5):
        r = rec[offs[k]:offs[k + 1]]
        want0 = start_states[k % 2]
        assert r["state"][0].tobytes() == want0._packed().tobytes() and r["ply"][0] == 0
        planes = _lib.game_encode(TTT, SP.states_of(TTT, r))
        # the game's PutGames call: the blobs whose boards are the game's records, in ply order
        hit = [j for j, blobs in enumerate(games) if j not in used and len(blobs) == len(r) and all(
            np.array_equal(Blackbird.ExampleState.FromSerialized(b).Board, planes[i:i + 1]) for i, b in enumerate(blobs))]
        assert hit, k
        used.add(hit[0])
        first = Blackbird.ExampleState.FromSerialized(games[hit[0]][0])
        assert np.array_equal(first.Board, want0.AsInputArray())
    blobs_starts = m.Conn.GetGames(m.Name, m.Version)
    assert len(blobs_starts) == int(offs[5])
    # a terminal start: ValueError, nothing stored (and the previous table stays on the engine until the next call replaces it)
    over = cls()
    for a in (0, 3, 1, 4, 2):
        over.ApplyAction(a)
    assert over.Winner() == 1
    with pytest.raises(ValueError) as err:
        Blackbird.GenerateTrainingSamples(m, 5, 1.0, startStates=[s0, over])
    assert "state 1 " in str(err.value) and "already over" in str(err.value)
    assert m.Conn.GetGames(m.Name, m.Version) == blobs_starts
    # startStates=None on the engine that held a table == the two-argument call, under the same seeds: a second model plays the
    # first run from the initial position (the same game ids are then behind both), and the second runs are compared
    np.random.seed(33)
    Blackbird.GenerateTrainingSamples(m, 5, 1.0, startStates=None)
    after = m.Conn.GetGames(m.Name, m.Version)[len(blobs_starts):]
    m._batch_engine.close()
    m.Conn.Close()
    m2, _g2 = model("plain")
    np.random.seed(21)
    Blackbird.GenerateTrainingSamples(m2, 5, 1.0)
    n_first = len(m2.Conn.GetGames(m2.Name, m2.Version))
    np.random.seed(33)
    Blackbird.GenerateTrainingSamples(m2, 5, 1.0)
    plain = m2.Conn.GetGames(m2.Name, m2.Version)[n_first:]
    m2._batch_engine.close()
    m2.Conn.Close()
    assert sorted(after) == sorted(plain) and len(plain) >= 5 * 2
    init = cls().AsInputArray()
    assert sum(np.array_equal(Blackbird.ExampleState.FromSerialized(b).Board, init) for b in plain) == 5


def test_timed_selfplay_honours_start_states(tmp_path, monkeypatch):
    """mcts.timeLimit: the loop primes its own roots, so it takes the start states itself; a refused one raises ValueError."""
    from blackbird_amd import Blackbird, TicTacToe
    monkeypatch.chdir(tmp_path)
    cls = TicTacToe.BoardState
    s0, s1 = cls(), cls()
    s0.ApplyAction(4)
    for a in (0, 4, 1):
        s1.ApplyAction(a)
    np.random.seed(11)
    m = Blackbird.Model(cls, "timed", {"explorationRate": 0.85, "playLimit": 16, "timeLimit": 0.001}, M.net_config(blocks=1, eps=0.3))
    m._MAX_NODES = 4096      # (the lock-step engine's pool per slot: 9 plies of 16 simulations need far less)
    games = []
    inner = m.Conn.PutGames
    monkeypatch.setattr(m.Conn, "PutGames", lambda *a: (games.append(list(a[3])), inner(*a))[1])
    Blackbird.GenerateTrainingSamples(m, 3, 1.0, startStates=[s0, s1])
    assert len(games) == 3   # (this path stores its games in game order)
    for k, blobs in enumerate(games):
        assert np.array_equal(Blackbird.ExampleState.FromSerialized(blobs[0]).Board, [s0, s1][k % 2].AsInputArray())
    over = cls()
    for a in (0, 3, 1, 4, 2):
        over.ApplyAction(a)
    with pytest.raises(ValueError):
        Blackbird.GenerateTrainingSamples(m, 3, 1.0, startStates=[over])
    assert len(games) == 3
    m.Conn.Close()
