"""Support for the -m gpu tests that play self-play games to the end and compare what a caller can read of them (not collected).
A run is a dict: rec, offs, win (bb_fetch_examples), cnt (the counters) and, where asked for, hdr (bb_selfplay_headers)."""
import numpy as np

from blackbird_amd import _lib, weights as W
from tests.search_cases import assert_same_array

C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS

REPORTED_COUNTERS = ("sims", "evals", "eval_cache_hits", "eval_cache_probes")   # what assert_cache_counters prints
NET_UNDER_CACHE = dict(evaluator=_lib.EVAL_NET, c_puct=0.85, seed=1234, alpha=0.2, epsilon=0.3)


# ---- engines -----------------------------------------------------------------------------------------------------------------
def cache_env(monkeypatch, cache, log2):
    """BB_EVAL_CACHE / BB_EVAL_CACHE_LOG2 (log2 None: unset) as the next engine shall read them: bb_create reads them once."""
    monkeypatch.setenv("BB_EVAL_CACHE", "1" if cache else "0")
    if log2 is not None:
        monkeypatch.setenv("BB_EVAL_CACHE_LOG2", str(log2))
    else:
        monkeypatch.delenv("BB_EVAL_CACHE_LOG2", raising=False)


def net_engine_under_cache(monkeypatch, game, cache, log2, **kw):
    """A network engine (seed 1234, c_puct 0.85, noise parameters 0.2 / 0.3) created under cache_env(cache, log2)."""
    cache_env(monkeypatch, cache, log2)
    return _lib.Engine(game, **NET_UNDER_CACHE, **kw)


def c4_weights(filters, blocks, seed=0):
    return W.flatten(W.init_weights(3, filters, blocks, 16, 7, seed=seed))


def c4_engine_under_cache(monkeypatch, cache, slots, sims, max_games, log2=None, **kw):
    return net_engine_under_cache(monkeypatch, C4, cache, log2, n_slots=slots, sims_per_move=sims, noise_on=True,
                                  max_games=max_games, **kw)


# ---- playing -----------------------------------------------------------------------------------------------------------------
def step_bound(n_games, max_plies, step):
    """More selfplay_step(step) calls than any run needs: one slot playing all the games one after another, each game its
    ceil(max_plies / step) steps and one more in which it is found over."""
    return n_games * (-(-max_plies // step) + 1)


def play_to_end(eng, n_games, step, temp, *, begin=True, steps_below=None, between=None, headers=False,
                overflow_each_step=False):
    """bb_selfplay_begin(n_games, temp) unless begin=False (the caller has begun them), then steps of `step` plies until every
    game is over; between(k): called after step k -- the place to harvest finished games in mid-run: feed a
    tests/harvest_cases.py Ledger there (harvest(eng, ledger)) and hand it this function's result at the end (headers=True).
    The number of steps stays below step_bound() -- and below steps_below,
    a caller's own tighter count -- or the run fails; overflow_each_step: no node pool has overflowed after any step.
    Everything a caller can read (headers=True: hdr too)."""
    if begin:
        eng.selfplay_begin(n_games, temp)
    bound = step_bound(n_games, eng.max_plies, step)
    if steps_below is not None:
        bound = min(bound, steps_below)
    steps = 0
    while not eng.selfplay_done()[0]:
        eng.selfplay_step(step)
        if between:
            between(steps)
        steps += 1
        assert not overflow_each_step or eng.counters()["overflow"] == 0, ("overflow in step", steps)
        assert steps < bound, ("self-play is not over after", steps, "steps of", step, "plies", n_games, eng.max_plies)
    rec, offs, win = eng.fetch_examples()
    out = dict(rec=rec, offs=offs, win=win, cnt=eng.counters())
    if headers:
        out["hdr"] = eng.selfplay_headers()
    return out


def play_loaded(eng, flat, n_games, step, *, mode, steps_below=None, overflow_each_step=False):
    """Load `flat` (None: the engine has its weights), reset the counters, play n_games at temperature 1 to the end; mode: what
    bb_selfplay_mode must say with these weights (None: not asked).  No node pool may have overflowed."""
    if flat is not None:
        eng.load_weights(flat)
    if mode is not None:
        assert eng.selfplay_mode() == mode
    eng.reset_counters()
    out = play_to_end(eng, n_games, step, 1.0, steps_below=steps_below, overflow_each_step=overflow_each_step)
    assert out["cnt"]["overflow"] == 0
    return out


# ---- comparing ---------------------------------------------------------------------------------------------------------------
def assert_same_records(a, b, what="", counters=(), no_overflow=False):
    """Two runs: game offsets, winners, records and (where both have them) headers byte for byte, and the named counters.
    no_overflow: neither run's node pools overflowed."""
    for k in ("offs", "win", "rec") + (("hdr",) if "hdr" in a and "hdr" in b else ()):
        assert_same_array(a[k], b[k], (what, k))
    if no_overflow:
        assert a["cnt"]["overflow"] == 0 and b["cnt"]["overflow"] == 0, (what, a["cnt"], b["cnt"])
    for k in counters:
        assert a["cnt"][k] == b["cnt"][k], (what, k, a["cnt"][k], b["cnt"][k])


def assert_cache_counters(on, off, probed=True):
    """Counters of the same games with the cache (on) and without (off): the run without counts no probe; every probe is a
    tower run or a hit, and a hit is one tower run less (probed=False: an engine that keeps the cache out of it)."""
    print("on:", {k: on[k] for k in REPORTED_COUNTERS}, "off:", {k: off[k] for k in REPORTED_COUNTERS})
    assert off["eval_cache_hits"] == 0 and off["eval_cache_probes"] == 0, off
    if probed:
        assert on["eval_cache_probes"] == on["evals"] + on["eval_cache_hits"], on
    else:
        assert on["eval_cache_hits"] == 0 and on["eval_cache_probes"] == 0, on
    assert on["evals"] + on["eval_cache_hits"] == off["evals"], (on, off)
    assert on["sims"] == off["sims"], (on, off)


def pi_of(game, r):
    """visits / total of the example records r as [len(r), A]; DragonChess: the compact child list spread over 4032 actions."""
    gi = _lib.game_info(game)
    if gi.dense:
        return r["visits"][:, :gi.A] / np.maximum(r["total"].astype(np.float64), 1.0)[:, None]
    pi = np.zeros((len(r), gi.A))
    for k in range(len(r)):
        nch = int(r["n_children"][k])
        if r["total"][k] > 0:
            pi[k, r["action"][k][:nch]] = r["visits"][k][:nch] / float(r["total"][k])
    return pi


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def oracle_selfplay_from(orc, cfg, game_id, start, temp, play_limit, max_plies):
    """One self-play game of the oracle from `start` (an orc.State; not changed): the dict orc.selfplay_game returns, and per
    move the root's child visit counts (`plays`) and the keyed draw of (seed, game id, ply) (`u`; not consumed at temp 0)."""
    game = cfg.game
    A = orc.dims(game)[3]
    search = orc.Search(cfg, game_id)
    search.drop_root()
    st = start.copy()
    boards, pi, player, actions, plays, us = [], [], [], [], [], []
    winner, n = None, 0
    while winner is None and n < max_plies:
        o = search.find_move(st, temp, play_limit, u=-1.0, ply=n)
        boards.append(orc.encode(game, st)[0])   # ExampleState(..., state.AsInputArray(), player) of the state before the move
        pi.append(o["prob"])
        player.append(st.player)
        actions.append(o["action"])
        plays.append(o["plays"])
        us.append(orc.u53(cfg.seed, game_id, n))
        st = o["next"]
        search.move_root(st)
        winner = orc.winner(game, st)            # lastAction is always None (Blackbird.py:242,253)
        n += 1
    boards.append(orc.encode(game, st)[0])       # terminal example with pi = zeros (Blackbird.py:256-258)
    pi.append(np.zeros(A))
    player.append(st.player)
    player = np.array(player, dtype=np.int8)
    w = -1 if winner is None else int(winner)
    z = np.zeros(n + 1, dtype=np.float32) if w <= 0 else np.where(player == w, 1.0, -1.0).astype(np.float32)  # :260-264
    return dict(n=n + 1, boards=np.stack(boards), pi=np.stack(pi), player=player, z=z,
                actions=np.array(actions, dtype=np.int32), winner=w, stats=search.stats(), plays=np.array(plays).reshape(n, A),
                u=np.array(us))


def orc_state_from_packed(orc, og, game, packed):
    """One packed engine state (include/blackbird_hip.h) as the oracle's state."""
    if game == _lib.GAME_DRAGONCHESS:
        b, p, pv, c = _lib.unpack_dc(np.asarray(packed).view(np.uint8).reshape(1, 80))
        return orc.state_from_arrays(og, b[0], p[0], int(pv[0]) or None, c[0])
    b, p, pv = _lib.unpack_grid(game, np.asarray(packed).view(np.uint64).reshape(1, 2))
    return orc.state_from_arrays(og, b[0], p[0], int(pv[0]) or None)


# ---- self-play from caller-given start positions ------------------------------------------------------------------------------
OG = {C4: 0, TTT: 1, DC: 2}
ACTIONS = {C4: ([], [3], [3, 3, 2, 4], [0, 1, 0, 1, 0, 1]),   # the last: one move from a win for either side -> short games
           TTT: ([], [4], [4, 0, 8], [0, 4, 1])}
DC_FIRST_LEGAL_TIMES = (1, 2, 3, 5)                            # crosses White's double move
ALPHA, EPS = 0.2, 0.3
COUNTERS = ("sims", "sum_depth", "nodes", "terminal_leaves", "games_finished", "plies", "examples")


def _apply(game, st, a):
    nxt, status = _lib.game_apply(game, st, [int(a)])
    assert status[0] == 0
    return nxt


_starts = {}


def starts_of(game):
    """The game's start set as packed states [4, ...]; built once, the caller must not change it."""
    if game not in _starts:
        out = []
        if game == DC:
            for times in DC_FIRST_LEGAL_TIMES:
                st = _lib.game_initial(game)
                for _ in range(times):
                    st = _apply(game, st, int(np.flatnonzero(_lib.game_legal(game, st)[0])[0]))
                out.append(st)
        else:
            for acts in ACTIONS[game]:
                st = _lib.game_initial(game)
                for a in acts:
                    st = _apply(game, st, a)
                out.append(st)
        _starts[game] = np.ascontiguousarray(np.concatenate(out, axis=0))
        assert (_lib.game_winner(game, _starts[game]) < 0).all()
    return _starts[game]


def play_from_starts(eng, n_games, starts="keep", step=3, temp=1.0):
    """Play n_games to the end at `temp`; starts: a packed table to set first, None to clear, "keep" to leave the engine as it is."""
    if not isinstance(starts, str):
        eng.selfplay_set_starts(starts)
    eng.reset_counters()
    out = play_to_end(eng, n_games, step, temp, steps_below=400, headers=True)
    assert out["cnt"]["overflow"] == 0 and out["cnt"]["games_finished"] == n_games
    return out


def states_of(game, r):
    return np.ascontiguousarray(r["state"]).view(_lib.STATE_DTYPE[game]).reshape(len(r), -1)


def assert_first_records_are(game, out, starts, first_id=0):
    """The first record of game k holds starts[k % n] at ply 0."""
    for k in range(len(out["win"])):
        r = out["rec"][out["offs"][k]]
        assert r["ply"] == 0 and r["game_id"] == first_id + k
        assert r["state"].tobytes() == starts[k % len(starts)].tobytes(), k


def assert_game_is_the_oracles(game, out, k, o, first_id):
    """Game k's records, header and winner against one oracle game."""
    r = out["rec"][out["offs"][k]:out["offs"][k + 1]]
    assert len(r) == o["n"] and out["win"][k] == o["winner"], (k, len(r), o["n"], out["win"][k], o["winner"])
    assert out["hdr"][k].tolist() == [o["n"], o["winner"], o["n"] - 1, 1], k
    assert (r["game_id"] == first_id + k).all() and np.array_equal(r["ply"], np.arange(len(r))), k
    assert np.array_equal(_lib.game_encode(game, states_of(game, r)), o["boards"]), k
    assert np.array_equal(pi_of(game, r), o["pi"]), k
    assert np.array_equal(r["player"], o["player"]) and np.array_equal(r["z"].astype(np.float32), o["z"]), k


def assert_games_are_the_oracles(orc, game, out, starts, cfg_of, first_id, sims, max_plies):
    """Every game's records against oracle_selfplay_from(starts[k % n]); returns the oracle's simulation total."""
    og = OG[game]
    sims_total = 0
    for k in range(len(out["win"])):
        start = orc_state_from_packed(orc, og, game, starts[k % len(starts)])
        o = oracle_selfplay_from(orc, cfg_of(k), first_id + k, start, 1.0, sims, max_plies)
        assert_game_is_the_oracles(game, out, k, o, first_id)
        sims_total += o["stats"].sims
    return sims_total


def assert_same_runs(a, b, what):
    assert_same_records(a, b, what, counters=("sims", "sum_depth"), no_overflow=True)


def net_engine(game, n_slots, n_games, sims, blocks, launch=_lib.LAUNCH_AUTO, noise=True, seed=17, first_id=500, **kw):
    gi = _lib.game_info(game)
    flat = W.flatten(W.init_weights(gi.C, 16, blocks, 16, gi.A, seed=21, perturb=True))
    eng = _lib.Engine(game, n_slots=n_slots, sims_per_move=sims, evaluator=_lib.EVAL_NET, seed=seed, max_games=n_games,
                      first_game_id=first_id, noise_on=noise, alpha=ALPHA, epsilon=EPS, launch=launch, **kw)
    eng.load_weights(flat)
    return eng, flat
