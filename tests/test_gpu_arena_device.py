"""-m gpu: the arena on the device (bb_arena_*, `_lib.Arena`, TestModelsBatched(loop='device')) against a stepwise statement of
the same match loop made from entry points the arena does not touch.

`statement` is the loop of blackbird_amd/arena.py written out -- set_roots on a side's first turn, run_sims(mask),
sample_moves(temp, None), game_apply, move_roots for every primed side, game_winner -- with u = None, so it draws the moves from
the same Philox streams as the device loop, and it records every move.  Everything compared is compared for exact equality:
results, plies, the move log, the final states, and both engines' sims / nodes / evals counters."""
import ctypes as C

import numpy as np
import pytest

from blackbird_amd import Blackbird, Connect4, DragonChess, TicTacToe, _lib, arena
from blackbird_amd.FixedMCTS import FixedMCTS

from tests import model_cases as M
from tests.arena_cases import HashPlayer as _HashPlayer, searcher_engines as _engines

pytestmark = pytest.mark.gpu

LOG = 64  # move log long enough for every dense game played here (Connect4: 42 plies at most)


def _model(game, name, seed, play_limit, eps=0.0):
    return M.model(game, name, seed=seed, play_limit=play_limit, eps=eps, blocks=2)


def statement(ea, eb, first, temp, starts=None, max_plies=None):
    """The host loop of arena.py over engines ea / eb with u = None; dict(result, plies, moves, states, overflow)."""
    game_id, n_slots = ea.game, ea.n_slots
    first = np.asarray(first, dtype=bool)
    n = len(first)
    states = np.repeat(_lib.game_initial(game_id), n, axis=0) if starts is None else np.array(starts, copy=True)
    alive = np.ones(n, dtype=bool)
    result = np.zeros(n, dtype=np.int8)
    plies = np.zeros(n, dtype=np.int32)
    moves = [[] for _ in range(n)]
    primed = [np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)]
    to_a = first.copy()
    a_player = np.where(first, 1, 2)
    done = 0
    while alive.any() and (max_plies is None or done < max_plies):
        actions = np.full(n, -1, dtype=np.int32)
        for k, eng in enumerate((ea, eb)):
            idx = np.nonzero(alive & (to_a if k == 0 else ~to_a))[0]
            if not len(idx):
                continue
            fresh = idx[~primed[k][idx]]
            if len(fresh):
                eng.set_roots(states[fresh], slots=fresh, game_ids=fresh)
                primed[k][fresh] = True
            mask = np.zeros(n_slots, dtype=np.uint8)
            mask[idx] = 1
            eng.run_sims(eng.cfg.sims_per_move, mask=mask)
            out = eng.sample_moves(temp, None)
            assert (out['action'][idx] >= 0).all()
            actions[idx] = out['action'][idx]
        idx = np.nonzero(alive)[0]
        new_states, status = _lib.game_apply(game_id, states[idx], actions[idx])
        assert (status == 0).all()
        states[idx] = new_states
        for k, eng in enumerate((ea, eb)):
            mv = np.full(n_slots, -1, dtype=np.int32)
            mv[:n] = np.where(alive & primed[k], actions, -1)
            eng.move_roots(mv)
        winners = _lib.game_winner(game_id, states[idx])
        to_a = ~to_a
        for i, w in zip(idx, winners):
            moves[i].append(int(actions[i]))
            plies[i] += 1
            if w >= 0:
                alive[i] = False
                result[i] = 0 if w == 0 else (1 if w == a_player[i] else -1)
        done += 1
    return dict(result=result, plies=plies, moves=moves, states=states, alive=int(alive.sum()),
                overflow=ea.counters()['overflow'] + eb.counters()['overflow'])


def device(ea, eb, first, temp, starts=None, log_plies=LOG, max_plies=None):
    """The same match through the arena: step(8) + status until nobody is alive (or max_plies in one step), then fetch."""
    ar = _lib.Arena(ea, eb, log_plies=log_plies)
    try:
        ar.begin(first, temp, starts)
        if max_plies is not None:
            ar.step(max_plies)
            alive = ar.status()
        else:
            alive = len(first)
            while alive:
                ar.step(8)
                alive = ar.status()
        out = ar.fetch()
        out['alive'] = alive
        return out
    finally:
        ar.close()


def _same(want, got, engines_want, engines_got, counters=('sims', 'nodes', 'evals'), log_plies=LOG):
    assert np.array_equal(got['result'], want['result']), (got['result'], want['result'])
    assert np.array_equal(got['plies'], want['plies']), (got['plies'], want['plies'])
    assert got['alive'] == want['alive']
    for i, mv in enumerate(want['moves']):
        row = np.full(log_plies, -1, dtype=np.int32)
        row[:min(len(mv), log_plies)] = mv[:log_plies]
        assert np.array_equal(got['moves'][i], row), (i, got['moves'][i], row)
    assert np.array_equal(got['states'], want['states'])
    for side, (ew, eg) in enumerate(zip(engines_want, engines_got)):
        cw, cg = ew.counters(), eg.counters()
        for name in counters:
            assert cw[name] == cg[name], (side, name, cw[name], cg[name])
        assert cg['overflow'] == 0


def _check(players, first, temp, n_slots=None, counters=('sims', 'nodes', 'evals'), structure=None, **kw):
    n_slots = n_slots or len(first)
    ew, eg = _engines(players, n_slots), _engines(players, n_slots)
    try:
        if structure is not None:                      # the case is about the structure it names
            assert [e.run_sims_structure() for e in eg] == list(structure)
        want = statement(ew[0], ew[1], first, temp, **kw)
        got = device(eg[0], eg[1], first, temp, **kw)
        _same(want, got, ew, eg, counters)
        return want, got
    finally:
        for e in ew + eg:
            e.close()


MIXED = [True, False, True, True, False, False, True, False]
SHAPES = {"mixed8": (MIXED, 8), "afirst8": ([True] * 8, 8), "one": ([False], 1), "five_of_8": (MIXED[:5], 8)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("temp", [0, 0.7, 0.1])
@pytest.mark.parametrize("game", [Connect4.BoardState, TicTacToe.BoardState], ids=["c4", "ttt"])
def test_hash_players_equal_the_stepwise_statement(game, temp, shape):
    """Two hash-evaluator searchers (two salts, two exploration rates), 24 simulations, lock-step: mixed first movers, side b's
    mask empty at ply 0, a single game, and fewer games than slots.  temp 0.1 is the exploitation temperature every evaluation
    game is played at (the law itself is held against the oracle in tests/test_gpu_arena.py and tests/test_gpu_sample_temp.py)."""
    first, n_slots = SHAPES[shape]
    players = (_HashPlayer(game, 11), _HashPlayer(game, 22, c_puct=1.3))
    want, _ = _check(players, first, temp, n_slots=n_slots, structure=(_lib.LAUNCH_LOCKSTEP,) * 2)
    assert want['alive'] == 0 and (want['plies'] >= (5 if game is TicTacToe.BoardState else 7)).all()


def test_hash_players_in_the_one_launch_structure():
    players = (_HashPlayer(Connect4.BoardState, 11), _HashPlayer(Connect4.BoardState, 22, c_puct=1.3))
    for p in players:
        p.SearchLaunch = 'wave'
    _check(players, MIXED, 0.7, structure=(_lib.LAUNCH_WAVE,) * 2)


@pytest.mark.parametrize("how", ["lockstep", "wave", "wave_cache"])
def test_two_models_equal_the_stepwise_statement(tmp_path, monkeypatch, how):
    """Two networks (2 blocks, 16 filters; prior noise off and on), Connect4, 8 games, 24 simulations, sampled moves."""
    monkeypatch.chdir(tmp_path)
    players = (_model(Connect4.BoardState, "a", 1, 24), _model(Connect4.BoardState, "b", 2, 24, eps=0.3))
    counters = ('sims', 'nodes', 'evals')
    for p in players:
        if how != "lockstep":
            p.SearchLaunch = 'wave'
        if how == "wave_cache":
            p.SearchEvalCache = True
            counters = ('sims', 'nodes')    # evals and the eval_cache_* counters depend on what the table held: by design
    structure = (_lib.LAUNCH_LOCKSTEP if how == "lockstep" else _lib.LAUNCH_WAVE,) * 2
    _check(players, MIXED, 0.7, counters=counters, structure=structure)


@pytest.mark.parametrize("how", ["lockstep", "wave_rollouts"])
def test_rollout_searcher_against_a_model(tmp_path, monkeypatch, how):
    """FixedMCTS(maxDepth=3), the rollout evaluator, against a network."""
    monkeypatch.chdir(tmp_path)
    fixed = FixedMCTS(maxDepth=3, explorationRate=0.85, playLimit=24)
    fixed.Game = Connect4.BoardState
    model = _model(Connect4.BoardState, "a", 1, 24)
    structure = (_lib.LAUNCH_LOCKSTEP,) * 2
    if how == "wave_rollouts":
        for p in (fixed, model):
            p.SearchLaunch = 'wave'
        fixed.SearchRollouts = True
        structure = (_lib.LAUNCH_WAVE,) * 2
    _check((fixed, model), MIXED, 0.7, structure=structure)


def test_dragonchess_six_plies_mid_run():
    """The callers alternate every ply although White moves twice in a row (W, W, B): six plies, looked at in the middle of the
    run, against six plies of the statement."""
    players = (_HashPlayer(DragonChess.BoardState, 11, playLimit=12), _HashPlayer(DragonChess.BoardState, 22, c_puct=1.3, playLimit=12))
    first = [True, False, False, True]
    ew, eg = _engines(players, 4), _engines(players, 4)
    try:
        want = statement(ew[0], ew[1], first, 0.7, max_plies=6)
        got = device(eg[0], eg[1], first, 0.7, log_plies=8, max_plies=6)
        assert want['alive'] == 4 and (want['plies'] == 6).all()
        _same(want, got, ew, eg, log_plies=8)
        players_to_move = _lib.unpack_dc(got['states'])[1]
        assert len(set(players_to_move.tolist())) == 1      # same turn order in every game, whoever started
    finally:
        for e in ew + eg:
            e.close()


def _near_end_connect4(n_empty_tops):
    """A Connect4 board without any run of four -- cell (r, c) holds player 1 + (r // 2 + c) % 2 -- with the top cell of the
    first `n_empty_tops` columns empty: that many moves from the end at most.  Player 1 to move."""
    board = np.zeros((6, 7, 2), dtype=np.int8)
    for r in range(6):
        for c in range(7):
            if r == 5 and c < n_empty_tops:
                continue
            board[r, c, (r // 2 + c) % 2] = 1
    return _lib.pack_grid(_lib.GAME_CONNECT4, board[None], [1], [2])


def test_start_states_finished_games_stay_untouched_and_short_log():
    """Games one, two and three moves from the end, and one from the initial position: they end at different plies.  Once a game
    is over, further steps leave both engines' slots of it bit-identical; with log_plies = 1 later moves are played, not logged."""
    starts = np.concatenate([_near_end_connect4(1), _near_end_connect4(2), _near_end_connect4(3), _lib.game_initial(_lib.GAME_CONNECT4)])
    first = [True, False, True, False]
    players = (_HashPlayer(Connect4.BoardState, 11), _HashPlayer(Connect4.BoardState, 22, c_puct=1.3))
    want, got = _check(players, first, 0, starts=starts)
    assert want['plies'][0] == 1 and 1 <= want['plies'][1] <= 2 and 1 <= want['plies'][2] <= 3 and want['plies'][3] >= 7
    assert len(set(want['plies'].tolist())) >= 3

    ew, eg = _engines(players, 4), _engines(players, 4)
    ar = _lib.Arena(eg[0], eg[1], log_plies=1)
    try:
        want = statement(ew[0], ew[1], first, 0, starts=starts)
        ar.begin(first, 0, starts)
        ar.step(3)
        assert ar.status() == 1                             # the three near-end games are over, the fourth runs
        mid = ar.fetch()
        assert (mid['plies'] == [want['plies'][0], want['plies'][1], want['plies'][2], 3]).all()

        def roots():
            return [e.node_edges(slot, -1) for e in eg for slot in range(3)]
        before = roots()
        while ar.status():
            ar.step(8)
        after = roots()
        for x, y in zip(before, after):
            for key in x:
                assert np.array_equal(x[key], y[key]), key
        end = ar.fetch()
        assert np.array_equal(end['result'], want['result']) and np.array_equal(end['plies'], want['plies'])
        assert np.array_equal(end['states'], want['states'])
        assert np.array_equal(end['moves'][:, 0], [m[0] for m in want['moves']])   # the first move only
    finally:
        ar.close()
        for e in ew + eg:
            e.close()


def test_begin_refuses_bad_arguments():
    players = (_HashPlayer(Connect4.BoardState, 11), _HashPlayer(Connect4.BoardState, 22))
    ea, eb = _engines(players, 4)
    other = _engines((_HashPlayer(TicTacToe.BoardState, 11),), 4)[0]
    wide = _engines((_HashPlayer(Connect4.BoardState, 11),), 8)[0]
    one_sim = _engines((_HashPlayer(Connect4.BoardState, 11, playLimit=1),), 4)[0]
    ar = None
    try:
        for a, b, log in ((ea, other, 4), (ea, wide, 4), (ea, eb, -1)):
            with pytest.raises(ValueError):
                _lib.Arena(a, b, log_plies=log)
        ar = _lib.Arena(ea, eb, log_plies=4)
        with pytest.raises(ValueError):
            ar.step(1)                                       # before begin
        with pytest.raises(ValueError):
            ar.begin([True] * 5, 0)                          # more games than slots
        with pytest.raises(ValueError):
            ar.begin([True] * 4, -0.5)
        assert _lib.lib().bb_arena_begin(ar.h, 4, None, None, C.c_double(0.0)) == _lib.ERR_ARG
        over = _near_end_connect4(0)                         # the full board: the game is over there
        with pytest.raises(ValueError, match="state 2"):
            ar.begin([True] * 4, 0, np.concatenate([_near_end_connect4(1)] * 2 + [over, over]))
        ar.begin([True, False], 0)                           # and it still works afterwards
        ar.step(2)
        assert ar.status() == 2
        ar.close()
        ar = _lib.Arena(ea, one_sim, log_plies=4)
        with pytest.raises(ValueError, match="NaN"):
            ar.begin([True] * 4, 0.7)                        # bb_selfplay_begin's rule: < 2 simulations and temp != 0
        ar.begin([True] * 4, 0)
    finally:
        if ar is not None:
            ar.close()
        for e in (ea, eb, other, wide, one_sim):
            e.close()


def test_python_device_loop_equals_the_host_loop(tmp_path, monkeypatch):
    """temp = 0 and no prior noise: nothing random is consumed, so TestModelsBatched(loop='device') returns the host loop's array;
    ArenaLoop = 'device' on the first side selects it too, and startStates= reaches the arena."""
    monkeypatch.chdir(tmp_path)
    m1, m2 = _model(Connect4.BoardState, "a", 1, 24), _model(Connect4.BoardState, "b", 2, 24)
    first = np.array(MIXED)
    host = arena.TestModelsBatched(m1, m2, 0, len(first), first=first)
    assert arena.last_loop == 'host'
    dev = arena.TestModelsBatched(m1, m2, 0, len(first), first=first, loop='device')
    assert arena.last_loop == 'device'
    assert dev.dtype == host.dtype and np.array_equal(dev, host), (dev, host)
    m1.ArenaLoop = 'device'
    assert np.array_equal(Blackbird.TestModelsBatched(m1, m2, 0, len(first), first=first), host)
    assert arena.last_loop == 'device'
    near = [Connect4.BoardState._from_packed(_near_end_connect4(k)) for k in (1, 2)]
    res = arena.TestModelsBatched(m1, m2, 0, 2, first=[True, False], startStates=near)
    assert res.shape == (2,) and set(np.unique(res)) <= {-1, 0, 1}


def test_node_pool_too_small_is_reported():
    """24 simulations per move into pools of 40 nodes: the statement's engines count overflow, the arena's status answers
    BB_ERR_CAPACITY and the Python loop raises."""
    players = (_HashPlayer(Connect4.BoardState, 11, node_capacity=40), _HashPlayer(Connect4.BoardState, 22, node_capacity=40))
    ew, eg = _engines(players, 4), _engines(players, 4)
    first = [True, False, True, False]
    ar = _lib.Arena(eg[0], eg[1], log_plies=0)
    try:
        assert statement(ew[0], ew[1], first, 0, max_plies=8)['overflow'] > 0
        ar.begin(first, 0)
        ar.step(8)
        alive = C.c_int()
        assert _lib.lib().bb_arena_status(ar.h, C.byref(alive)) == _lib.ERR_CAPACITY
        with pytest.raises(_lib.BlackbirdHipError):
            ar.status()
    finally:
        ar.close()
        for e in ew + eg:
            e.close()
    with pytest.raises(_lib.BlackbirdHipError):
        arena.TestModelsBatched(players[0], players[1], 0, 4, first=first, loop='device')
