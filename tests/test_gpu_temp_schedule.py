"""-m gpu: a temperature schedule by ply (bb_selfplay_set_temp_schedule, bb_arena_set_temp_schedule, Model.SelfPlayTempSchedule,
tempSchedule=) in every structure that chooses a self-play or arena move.

The move out of ply p is drawn at the run's `temp` while p < plies and at temp_late from there on; p is the ply in the record
header and in the draw's key.  The yardstick is tests/temp_schedule_cases.py: the oracle's self-play loop with the temperature
chosen per move, pinned to the constant-temperature yardstick in tests/test_temp_schedule_cpu.py, which also shows that every draw
compared here keeps 2^-40 from the boundaries of its cdf at its own temperature -- so every comparison is exact.

1. Lock-step engines of all three games against the oracle under every schedule of the cases module (7 games on 3 slots: a
   refilled slot starts again at the early temperature).
2. Every other structure against the lock-step engine's records, byte for byte, under two schedules; one case from caller-given
   start positions against the oracle: ply counts from the start position.
3. The default is untouched: never set, set and turned off, and temp_late == temp play the same bytes.
4. The NaN rule with two temperatures.
5. The arena on the device against the stepwise statement with sample_moves(temp_of(ply), None), and against the host loop.
6. GenerateTrainingSamples under Model.SelfPlayTempSchedule."""
import numpy as np
import pytest

from blackbird_amd import Blackbird, Connect4, DragonChess, TicTacToe, _lib, arena
from tests import arena_cases as AC
from tests import model_cases as M
from tests import selfplay_cases as SS
from tests import temp_cases as T
from tests import temp_schedule_cases as TS
from tests import test_gpu_arena_device as AD

pytestmark = pytest.mark.gpu
C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
OG = SS.OG
GAMES = pytest.mark.parametrize("game", [C4, TTT, DC], ids=["c4", "ttt", "dc"])


def _play(eng, n_games, name, starts="keep", step=3):
    """Play n_games to the end under SCHEDULES[name] (None: the engine's schedule is left as it is, at temp 0.5)."""
    temp = 0.5
    if name is not None:
        temp, plies, late = TS.SCHEDULES[name]
        eng.selfplay_set_temp_schedule(plies, late)
    return SS.play_from_starts(eng, n_games, starts, step=step, temp=temp)


def _hash_lockstep(game, sims=None, salt=None):
    L = T.LOCKSTEP
    eng = _lib.Engine(game, n_slots=L["n_slots"], sims_per_move=sims or L["sims"], evaluator=_lib.EVAL_HASH,
                      hash_salt=L["salt"] if salt is None else salt, salt_per_game=True, seed=TS.SEED, max_games=L["n_games"],
                      first_game_id=L["first_id"], launch=_lib.LAUNCH_LOCKSTEP, max_plies=T.DC_MAX_PLIES if game == DC else None)
    assert eng.selfplay_mode() == 0 and eng.max_plies == T.lockstep_max_plies(OG[game])
    return eng


# ---- 1. lock-step against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TS.SCHEDULES))
@GAMES
def test_lockstep_hash_selfplay_under_a_schedule_vs_oracle(orc, game, name):
    L = T.LOCKSTEP
    eng = _hash_lockstep(game)
    out = _play(eng, L["n_games"], name)
    eng.close()
    games = TS.lockstep_games(orc, OG[game], name)
    for k, o in enumerate(games):
        SS.assert_game_is_the_oracles(game, out, k, o, L["first_id"])
    assert out["cnt"]["sims"] == sum(o["stats"].sims for o in games) and out["cnt"]["examples"] == len(out["rec"])
    assert out["cnt"]["games_finished"] == L["n_games"] and out["cnt"]["plies"] == sum(o["n"] - 1 for o in games)


def test_lockstep_under_a_schedule_from_start_positions_vs_oracle(orc):
    """Games that start mid-game (the table of tests/selfplay_cases.py, wrapped by 7 games): their first move is ply 0 of the
    schedule, whatever the number of stones on the board."""
    S, L = TS.STARTS_CASE, T.LOCKSTEP
    eng = _hash_lockstep(C4, salt=S["salt"])
    starts = SS.starts_of(C4)
    out = _play(eng, L["n_games"], S["name"], starts)
    eng.close()
    SS.assert_first_records_are(C4, out, starts, S["first_id"])
    games = TS.starts_games(orc)
    for k, o in enumerate(games):
        SS.assert_game_is_the_oracles(C4, out, k, o, S["first_id"])
    assert out["cnt"]["sims"] == sum(o["stats"].sims for o in games)


# ---- 2. the other structures against lock-step -----------------------------------------------------------------------------------
_reference = {}


def _net_lockstep(game, n_slots, n_games, sims, name, **kw):
    """The lock-step run of the network engine of SS.net_engine under SCHEDULES[name]; played once per case, not to be changed."""
    key = (game, n_slots, n_games, sims, name, tuple(sorted(kw.items())))
    if key not in _reference:
        eng, _flat = SS.net_engine(game, n_slots, n_games, sims, 1, launch=_lib.LAUNCH_LOCKSTEP, **kw)
        assert eng.selfplay_mode() == 0
        _reference[key] = _play(eng, n_games, name, step=2)
        eng.close()
    return _reference[key]


@pytest.mark.parametrize("cache", [True, False], ids=["cache", "nocache"])
@pytest.mark.parametrize("name", TS.TWO)
def test_connect4_persistent_kernel_is_lockstep(monkeypatch, name, cache):
    """16-filter network, prior noise on, 24 games on 19 slots (one 16-game workgroup and a ragged one), evaluation cache on / off."""
    SS.cache_env(monkeypatch, cache, 12 if cache else None)
    eng, _flat = SS.net_engine(C4, 19, 24, 24, 1, seed=5, first_id=0)
    assert eng.selfplay_mode() == 3
    out = _play(eng, 24, name, step=2)
    eng.close()
    assert (out["cnt"]["eval_cache_probes"] > 0) == cache
    SS.assert_same_runs(out, _net_lockstep(C4, 19, 24, 24, name, seed=5, first_id=0), (name, cache))


@pytest.mark.parametrize("name", TS.TWO)
def test_tictactoe_persistent_kernel_is_lockstep(name):
    eng, _flat = SS.net_engine(TTT, 16, 21, 24, 1, seed=5, first_id=0)
    assert eng.selfplay_mode() == 3
    out = _play(eng, 21, name, step=2)
    eng.close()
    SS.assert_same_runs(out, _net_lockstep(TTT, 16, 21, 24, name, seed=5, first_id=0), name)


@pytest.mark.parametrize("name", TS.TWO)
def test_asynchronous_rounds_are_lockstep(name):
    eng, _flat = SS.net_engine(C4, 19, 24, 24, 1, launch=_lib.LAUNCH_ROUNDS, seed=5, first_id=0)
    assert eng.selfplay_mode() == 1
    out = _play(eng, 24, name, step=2)
    eng.close()
    SS.assert_same_runs(out, _net_lockstep(C4, 19, 24, 24, name, seed=5, first_id=0), name)


@pytest.mark.parametrize("name", TS.TWO)
def test_dragonchess_one_wave_kernel_is_lockstep(name):
    eng, _flat = SS.net_engine(DC, 5, 9, 12, 1, seed=7, first_id=0, max_plies=5)
    assert eng.selfplay_mode() == 5
    out = _play(eng, 9, name)
    eng.close()
    SS.assert_same_runs(out, _net_lockstep(DC, 5, 9, 12, name, seed=7, first_id=0, max_plies=5), name)


@pytest.mark.parametrize("name", TS.TWO)
@pytest.mark.parametrize("game,fixed", [(C4, True), (DC, False)], ids=["c4_fixed3", "dc_dynamic"])
def test_rollout_selfplay_in_one_launch_is_lockstep(game, fixed, name):
    runs = {}
    for wave in (True, False):
        eng = _lib.Engine(game, n_slots=5, sims_per_move=12, mcts_kind=_lib.MCTS_FIXED if fixed else _lib.MCTS_DYNAMIC, max_depth=3,
                          evaluator=_lib.EVAL_ROLLOUT, seed=31, max_games=9, first_game_id=1000, max_plies=5 if game == DC else None)
        eng.selfplay_rollouts(wave)
        assert eng.selfplay_mode() == (6 if wave else 0)
        runs[wave] = _play(eng, 9, name)
        eng.close()
    SS.assert_same_runs(runs[True], runs[False], (game, fixed, name))
    assert {k: runs[True]["cnt"][k] for k in SS.COUNTERS} == {k: runs[False]["cnt"][k] for k in SS.COUNTERS}


# ---- 3. the default is untouched -------------------------------------------------------------------------------------------------
@GAMES
def test_never_set_turned_off_and_equal_temperatures_are_the_same_run(game):
    """(That the first of them is what the parent commit plays is held by every existing self-play test.)"""
    L = T.LOCKSTEP
    runs = {}
    for how in ("never", "off", "equal", "scheduled"):
        eng = _hash_lockstep(game)
        if how == "off":
            eng.selfplay_set_temp_schedule(2, 0.0)
            eng.selfplay_set_temp_schedule(-1, 0.0)
        elif how == "equal":
            eng.selfplay_set_temp_schedule(5, 0.5)
        elif how == "scheduled":
            eng.selfplay_set_temp_schedule(2, 0.0)
        runs[how] = _play(eng, L["n_games"], None)
        eng.close()
    for how in ("off", "equal"):
        SS.assert_same_runs(runs["never"], runs[how], (game, how))
        assert {k: runs["never"]["cnt"][k] for k in SS.COUNTERS} == {k: runs[how]["cnt"][k] for k in SS.COUNTERS}
    assert runs["scheduled"]["rec"].tobytes() != runs["never"]["rec"].tobytes()      # (the comparison can tell)


# ---- 4. the NaN rule -------------------------------------------------------------------------------------------------------------
def test_begin_looks_at_both_temperatures():
    eng = _lib.Engine(C4, n_slots=3, sims_per_move=1, evaluator=_lib.EVAL_HASH, max_games=3, launch=_lib.LAUNCH_LOCKSTEP)
    eng.selfplay_begin(3, 0.0)                                    # one simulation and the arg-max move: fine
    eng.selfplay_set_temp_schedule(3, 0.5)
    assert _lib.lib().bb_selfplay_begin(eng.h, 3, 0.0) == _lib.ERR_NAN and "NaN" in _lib.last_error()
    with pytest.raises(ValueError, match="NaN"):
        eng.selfplay_begin(3, 0.0)
    eng.selfplay_set_temp_schedule(3, 0.0)
    with pytest.raises(ValueError, match="NaN"):
        eng.selfplay_begin(3, 0.5)
    eng.selfplay_begin(3, 0.0)
    eng.selfplay_set_temp_schedule(-1, 0.5)                       # off: the late temperature is nobody's
    eng.selfplay_begin(3, 0.0)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temp_late"):
            eng.selfplay_set_temp_schedule(2, bad)
    eng.close()


def test_an_overflowing_late_temperature_parks_the_slot_at_the_first_late_ply():
    """48 simulations: some child of every root has >= 7 visits and 7 ** 500 = inf.  Two plies at 0.5 are played; the third finds
    no probabilities: no record, one count per slot, and nothing more happens to the slot."""
    L = T.LOCKSTEP
    eng = _hash_lockstep(C4, sims=48)
    eng.reset_counters()
    eng.selfplay_set_temp_schedule(2, T.OVERFLOW_TEMP)
    eng.selfplay_begin(L["n_games"], 0.5)
    eng.selfplay_step(2)
    cnt = eng.counters()
    assert cnt["overflow"] == 0 and cnt["plies"] == 2 * L["n_slots"], cnt
    seen = []
    for steps in (1, 2):
        eng.selfplay_step(steps)
        assert eng.selfplay_done() == (False, 0)
        cnt = eng.counters()
        assert cnt["overflow"] == L["n_slots"] and cnt["plies"] == 2 * L["n_slots"], cnt
        assert cnt["games_finished"] == 0 and cnt["examples"] == 0 and not eng.selfplay_headers().any(), cnt
        seen.append(cnt)
    assert seen[0] == seen[1]
    eng.close()


def test_generate_training_samples_names_the_late_temperature(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    np.random.seed(11)
    m = Blackbird.Model(Connect4.BoardState, "hot", {"explorationRate": 0.85, "playLimit": 48}, M.net_config(blocks=1, eps=0.3))
    np.random.seed(21)
    m.SelfPlayTempSchedule = (2, T.OVERFLOW_TEMP)
    with pytest.raises(ValueError, match="NaN.*late temperature %r" % T.OVERFLOW_TEMP):
        Blackbird.GenerateTrainingSamples(m, 3, 1.0)
    assert len(m.Conn.GetGames(m.Name, m.Version)) == 0
    m._batch_engine.close()
    m.Conn.Close()


# ---- 5. the arena ----------------------------------------------------------------------------------------------------------------
def statement(ea, eb, first, sched, max_plies=None):
    """tests/test_gpu_arena_device.py::statement with sample_moves(temp_of(ply), None): the loop iteration is the ply."""
    temp_of = TS.temp_of(sched)
    game_id, n_slots = ea.game, ea.n_slots
    first = np.asarray(first, dtype=bool)
    n = len(first)
    states = np.repeat(_lib.game_initial(game_id), n, axis=0)
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
            out = eng.sample_moves(temp_of(done), None)
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


def device(ea, eb, first, sched, log_plies=AD.LOG, max_plies=None):
    """The same match through the arena under the schedule: steps of 3 plies, so that the schedule's boundary falls inside a step."""
    temp, plies, late = sched
    ar = _lib.Arena(ea, eb, log_plies=log_plies)
    try:
        ar.set_temp_schedule(plies, late)
        ar.begin(first, temp)
        if max_plies is not None:
            ar.step(max_plies)
            alive = ar.status()
        else:
            alive = len(first)
            while alive:
                ar.step(3)
                alive = ar.status()
        out = ar.fetch()
        out['alive'] = alive
        return out
    finally:
        ar.close()


def _check(players, first, sched, structure=None, counters=('sims', 'nodes', 'evals')):
    ew, eg = AC.searcher_engines(players, len(first)), AC.searcher_engines(players, len(first))
    try:
        if structure is not None:
            assert [e.run_sims_structure() for e in eg] == list(structure)
        want = statement(ew[0], ew[1], first, sched)
        got = device(eg[0], eg[1], first, sched)
        AD._same(want, got, ew, eg, counters)
        return want, got
    finally:
        for e in ew + eg:
            e.close()


@pytest.mark.parametrize("name", TS.TWO)
@pytest.mark.parametrize("game", [Connect4.BoardState, TicTacToe.BoardState], ids=["c4", "ttt"])
def test_arena_hash_players_equal_the_stepwise_statement(game, name):
    players = (AC.HashPlayer(game, 11), AC.HashPlayer(game, 22, c_puct=1.3))
    want, _ = _check(players, AD.MIXED, TS.SCHEDULES[name], structure=(_lib.LAUNCH_LOCKSTEP,) * 2)
    assert want['alive'] == 0 and (want['plies'] > TS.SCHEDULES[name][1]).all()      # every game reaches the late phase


def test_arena_two_models_in_the_wave_structure(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    players = (AD._model(Connect4.BoardState, "a", 1, 24), AD._model(Connect4.BoardState, "b", 2, 24, eps=0.3))
    for p in players:
        p.SearchLaunch = 'wave'
    _check(players, AD.MIXED, TS.SCHEDULES[TS.TWO[1]], structure=(_lib.LAUNCH_WAVE,) * 2)


def test_arena_dragonchess_six_plies():
    players = (AC.HashPlayer(DragonChess.BoardState, 11, playLimit=12), AC.HashPlayer(DragonChess.BoardState, 22, c_puct=1.3, playLimit=12))
    first = [True, False, False, True]
    sched = TS.SCHEDULES[TS.TWO[0]]
    ew, eg = AC.searcher_engines(players, 4), AC.searcher_engines(players, 4)
    try:
        want = statement(ew[0], ew[1], first, sched, max_plies=6)
        got = device(eg[0], eg[1], first, sched, log_plies=8, max_plies=6)
        assert want['alive'] == 4 and (want['plies'] == 6).all()
        AD._same(want, got, ew, eg, log_plies=8)
    finally:
        for e in ew + eg:
            e.close()


def test_arena_schedule_is_taken_at_begin_and_can_be_turned_off():
    players = (AC.HashPlayer(Connect4.BoardState, 11), AC.HashPlayer(Connect4.BoardState, 22, c_puct=1.3))
    first = AD.MIXED
    runs = {}
    for how in ("never", "off", "equal", "scheduled", "set_after_begin"):
        ea, eb = AC.searcher_engines(players, len(first))
        ar = _lib.Arena(ea, eb, log_plies=AD.LOG)
        try:
            if how == "off":
                ar.set_temp_schedule(2, 0.0)
                ar.set_temp_schedule(-1, 0.0)
            elif how == "equal":
                ar.set_temp_schedule(3, 0.7)
            elif how == "scheduled":
                ar.set_temp_schedule(2, 0.0)
            ar.begin(first, 0.7)
            if how == "set_after_begin":
                ar.set_temp_schedule(2, 0.0)                      # the next begin's; the run keeps what it began with
            while ar.status():
                ar.step(3)
            runs[how] = ar.fetch()
            for bad in (-0.5, float("nan"), float("inf")):
                with pytest.raises(ValueError, match="temp_late"):
                    ar.set_temp_schedule(2, bad)
        finally:
            ar.close()
            ea.close()
            eb.close()
    for how in ("off", "equal", "set_after_begin"):
        for k in ("result", "plies", "moves", "states"):
            assert np.array_equal(runs["never"][k], runs[how][k]), (how, k)
    assert not np.array_equal(runs["never"]["moves"], runs["scheduled"]["moves"])


def test_arena_begin_looks_at_both_temperatures():
    ea, eb = AC.searcher_engines((AC.HashPlayer(Connect4.BoardState, 11), AC.HashPlayer(Connect4.BoardState, 11, playLimit=1)), 4)
    ar = _lib.Arena(ea, eb, log_plies=0)
    try:
        ar.begin([True] * 4, 0)
        ar.set_temp_schedule(2, 0.5)
        with pytest.raises(ValueError, match="NaN"):
            ar.begin([True] * 4, 0)
        ar.set_temp_schedule(-1, 0.5)
        ar.begin([True] * 4, 0)
    finally:
        ar.close()
        ea.close()
        eb.close()


def _replayed_draws(orc, first, plies, sched, seed=77):
    """uniforms= for the host loop that hands it the draws the device loop takes from the engines' own streams: in the host loop's
    order (ply, then side), for the movers of that side that are alive, the draw of (seed, game, the side's own ply counter --
    a side primes its slot on its first turn, so the second mover's counter lags by one).  `plies`: per game, from the device run."""
    temp_of, first = TS.temp_of(sched), np.asarray(first, dtype=bool)
    batches = []
    for p in range(int(max(plies))):
        if temp_of(p) == 0:
            continue
        for k in (0, 1):
            mover_is_a = first ^ bool(p & 1)
            idx = np.nonzero((plies > p) & (mover_is_a if k == 0 else ~mover_is_a))[0]
            if len(idx):
                batches.append(np.array([orc.u53(seed, i, p - (0 if first[i] == (k == 0) else 1)) for i in idx]))
    it = iter(batches)

    def draw(n):
        u = next(it)
        assert len(u) == n, (len(u), n)
        return u
    draw.left = lambda: len(list(it))
    return draw


@pytest.mark.parametrize("name", TS.TWO)
def test_python_loops_agree_under_a_schedule(orc, name):
    """TestModelsBatched(tempSchedule=) in the device loop returns the stepwise statement's results, and the host loop returns them
    too when its uniforms are the draws of the engines' streams: the host loop asks for exactly those draws -- none for a ply at
    temperature 0 -- and in that order."""
    sched = TS.SCHEDULES[name]
    temp, plies, late = sched
    players = (AC.HashPlayer(Connect4.BoardState, 11), AC.HashPlayer(Connect4.BoardState, 22, c_puct=1.3))
    first = np.array(AD.MIXED)
    ew = AC.searcher_engines(players, len(first))
    try:
        want = statement(ew[0], ew[1], first, sched)
    finally:
        for e in ew:
            e.close()
    dev = arena.TestModelsBatched(players[0], players[1], temp, len(first), first=first, loop='device', tempSchedule=(plies, late))
    assert arena.last_loop == 'device' and np.array_equal(dev, want['result']), (dev, want['result'])
    draw = _replayed_draws(orc, first, want['plies'], sched)
    host = Blackbird.TestModelsBatched(players[0], players[1], temp, len(first), first=first, loop='host', uniforms=draw,
                                       tempSchedule=(plies, late))
    assert arena.last_loop == 'host' and np.array_equal(host, dev), (host, dev)
    assert draw.left() == 0


# ---- 6. the front end ------------------------------------------------------------------------------------------------------------
def test_generate_training_samples_under_a_schedule_and_then_without(tmp_path, monkeypatch):
    """With model.SelfPlayTempSchedule set, the call stores the examples of an engine-level run of the same stream under the same
    schedule; the next call, with the attribute back at None, plays unscheduled games on the engine the first call left a
    schedule on."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(Blackbird, "MAX_CONCURRENT_GAMES", 2)          # a 2-slot engine: 5 games refill its slots
    cls, n = TicTacToe.BoardState, 5
    np.random.seed(11)
    m = Blackbird.Model(cls, "sched", {"explorationRate": 0.85, "playLimit": 16}, M.net_config(blocks=1, eps=0.3))
    streams = []
    inner = _lib.Engine.set_rng_stream
    monkeypatch.setattr(_lib.Engine, "set_rng_stream", lambda self, seed, first=0: (streams.append((seed, first)), inner(self, seed, first))[1])

    def stored(before):
        out = []
        for b in m.Conn.GetGames(m.Name, m.Version)[before:]:
            e = Blackbird.ExampleState.FromSerialized(b)
            out.append((e.Board.tobytes(), np.asarray(e.MctsPolicy, dtype=np.float64).tobytes(), float(e.MctsEval[0])))
        return sorted(out)

    def of_records(rec):
        return sorted((e.Board.tobytes(), e.MctsPolicy.tobytes(), float(e.MctsEval)) for e in Blackbird._records_to_examples(cls, rec))

    def engine_level(eng, stream, schedule):
        inner(eng, *stream)
        if schedule != "keep":
            eng.selfplay_set_temp_schedule(*schedule)
        return SS.play_from_starts(eng, n, temp=1.0)["rec"]

    np.random.seed(21)
    assert m.SelfPlayTempSchedule is None
    m.SelfPlayTempSchedule = (1, 0.0)
    Blackbird.GenerateTrainingSamples(m, n, 1.0)
    eng = m._batch_engine
    assert eng.n_slots == 2 and len(streams) == 1
    first_call = stored(0)
    rec = eng.fetch_examples(0, n)[0]
    assert first_call == of_records(rec) and len(rec) >= 2 * n
    assert rec.tobytes() == engine_level(eng, streams[0], (1, 0.0)).tobytes()
    assert rec.tobytes() != engine_level(eng, streams[0], (-1, 0.0)).tobytes()     # (the schedule is seen in these games)
    eng.selfplay_set_temp_schedule(1, 0.0)                               # as the first call left the engine
    np.random.seed(33)
    m.SelfPlayTempSchedule = None
    Blackbird.GenerateTrainingSamples(m, n, 1.0)
    assert m._batch_engine is eng and len(streams) == 2
    rec2 = eng.fetch_examples(0, n)[0]
    assert stored(len(first_call)) == of_records(rec2)
    assert rec2.tobytes() == engine_level(eng, streams[1], "keep").tobytes()      # the call turned the schedule off ...
    assert rec2.tobytes() == engine_level(eng, streams[1], (-1, 0.0)).tobytes()   # ... these are unscheduled games
    assert rec2.tobytes() != engine_level(eng, streams[1], (1, 0.0)).tobytes()
    eng.close()
    m.Conn.Close()
