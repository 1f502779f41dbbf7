"""Support for the -m gpu tests of the search API across launch structures (not collected): engines that differ in nothing but
bb_config.launch / search_cache, roots, and the comparison of everything a caller can read of their trees.  A constant in
which the test modules differ (node_capacity, max_plies, blocks) is an argument without a default."""
import functools
import os

import numpy as np
import pytest

from blackbird_amd import _lib
from blackbird_amd import weights as W
from blackbird_amd.DynamicMCTS import DynamicMCTS

C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
LOCK, WAVE = _lib.LAUNCH_LOCKSTEP, _lib.LAUNCH_WAVE
GAME_OF = {"c4": C4, "ttt": TTT}
CACHE_COUNTERS = ("evals", "eval_cache_hits", "eval_cache_probes")


# ---- positions ---------------------------------------------------------------------------------------------------------------
def pack_states(game, g):
    if game == DC:
        return _lib.pack_dc(g["board"].reshape(-1, 8, 8), g["player"], g["prev"], g["castle"])
    H, W_, _s = _lib.GRID[game]
    return _lib.pack_grid(game, g["board"].reshape(-1, H, W_, 2), g["player"], g["prev"])


def same_position(game, a, b):
    """GameState.__eq__: PreviousPlayer is ignored."""
    if game == DC:
        a, b = a.copy(), b.copy()
        a[:, 65] = 0
        b[:, 65] = 0
        return np.array_equal(a[:, :70], b[:, :70])
    m = np.uint64((1 << 58) - 1)
    return np.array_equal(a & m, b & m)


def openings(game, n):
    """n different positions two plies into a dense game."""
    A = _lib.game_info(game).A
    st = np.repeat(_lib.game_initial(game), n, axis=0)
    i = np.arange(n)
    for moves in (i % A, (i + 4) % A):
        st, status = _lib.game_apply(game, st, moves.astype(np.int32))
        assert (status == 0).all()
    return st


DC_PLIES = (2, 1, 2, 4, 3)   # White moves twice, then Black (W, W, B): after 1 and after 4 plies the pair of White moves is half played


def dc_openings(n):
    """n different DragonChess positions a few plies into the game: slot i plays DC_PLIES[i % 5] moves, each the
    (3 i + 2 ply)-th legal one."""
    out = []
    for i in range(n):
        st = _lib.game_initial(DC)
        for ply in range(DC_PLIES[i % len(DC_PLIES)]):
            legal = np.nonzero(_lib.game_legal(DC, st)[0])[0]
            st, status = _lib.game_apply(DC, st, np.array([legal[(3 * i + 2 * ply) % len(legal)]], dtype=np.int32))
            assert (status == 0).all()
        out.append(st)
    st = np.concatenate(out, axis=0)
    movers = [(int(s[64]), int(s[65])) for s in st]          # (player, previous player)
    assert n < 2 or (1, 1) in movers                          # a position between White's two moves is among them
    return st


def endgame_roots(golden_dir, key):
    """Five roots close to the end of recorded games: two and three plies before a full board (a drawn game: few legal moves,
    terminal leaves everywhere) and one or two plies before a win."""
    g = np.load(os.path.join(golden_dir, f"playouts_{key}.npz"), allow_pickle=False)
    st = pack_states(GAME_OF[key], g)
    gs = g["game_start"]
    last = gs[1:] - 1                      # a game's final position (no action follows)
    drawn = [i for i in range(len(last)) if g["win_none"][last[i]] == 0]
    won = [i for i in range(len(last)) if g["win_none"][last[i]] > 0 and last[i] - gs[i] >= 4]
    assert drawn and len(won) >= 2
    idx = [last[drawn[0]] - 2, last[drawn[0]] - 3, last[won[0]] - 1, last[won[1]] - 1, last[won[1]] - 2]
    return st[np.array(idx)]


def game_ids(n):
    return 7 * np.arange(n) + 3   # distinct, not the slot numbers


def set_roots_on(engines, states):
    for e in engines:
        e.set_roots(states, game_ids=game_ids(len(states)))


def close_all(*engines):
    for e in engines:
        e.close()


# ---- engines -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_weights(game, filters, blocks, seed=21):
    gi = _lib.game_info(game)
    return W.flatten(W.init_weights(gi.C, filters, blocks, 16, gi.A, seed=seed, perturb=True))


@functools.lru_cache(maxsize=None)
def dc_weights(blocks, seed=21):
    return W.flatten(W.init_weights(17, 16, blocks, 16, 4032, seed=seed, perturb=True))


SEARCH_KW = dict(sims_per_move=8, seed=17, first_game_id=1000)
NET_KW = dict(evaluator=_lib.EVAL_NET, noise_on=True, alpha=0.2, epsilon=0.3)    # the prior noise on


def dense_engine(game, n_slots, launch, ev, *, node_capacity, **kw):
    """ev: 'hash', 'rollout', or ('net', filters, blocks) with the prior noise on (epsilon 0.3)."""
    common = dict(SEARCH_KW, n_slots=n_slots, launch=launch, node_capacity=node_capacity, **kw)
    if ev == "hash":
        return _lib.Engine(game, evaluator=_lib.EVAL_HASH, hash_salt=4242, salt_per_game=True, **common)
    if ev == "rollout":
        return _lib.Engine(game, evaluator=_lib.EVAL_ROLLOUT, **common)
    eng = _lib.Engine(game, **NET_KW, **common)
    eng.load_weights(dense_weights(game, ev[1], ev[2]))
    return eng


def dc_engine(n_slots, launch, blocks, *, node_capacity, max_plies, **kw):
    """A DragonChess engine on the network evaluator with the prior noise on (epsilon 0.3)."""
    eng = _lib.Engine(DC, n_slots=n_slots, launch=launch, node_capacity=node_capacity, max_plies=max_plies, **SEARCH_KW,
                      **NET_KW, **kw)
    eng.load_weights(dc_weights(blocks))
    return eng


def lock_and_wave(make, want, cached=False):
    """make(launch, **kw): the lock-step engine, the wave engine and, cached, the wave engine with search_cache -- the same
    engine otherwise.  want: what the wave engines must report (LOCK: an engine the one-launch kernel does not cover)."""
    engines = [make(LOCK), make(WAVE)] + ([make(WAVE, search_cache=True)] if cached else [])
    assert engines[0].run_sims_structure() == LOCK
    assert all(e.run_sims_structure() == want for e in engines[1:])
    return tuple(engines)


# ---- everything of the trees a caller can read ---------------------------------------------------------------------------------
def view_rows(eng, slot, node):
    """Dense games: (bb_node_view of the node, its children)."""
    row = eng.node_view(slot, node)
    return row, row["child"]


def edge_rows(eng, slot, node):
    """DragonChess: (bb_node_edges of the node, its first n_children children)."""
    row = eng.node_edges(slot, node)
    return row, row["child"][:row["n_children"]]


def snapshot(eng, temp, u, rows):
    """bb_sample_moves' outputs, the rows of every root and of each of its children (rows: view_rows / edge_rows), the counters."""
    out = eng.sample_moves(temp, u)
    got = []
    for s in range(eng.n_slots):
        root, children = rows(eng, s, -1)
        got.append(root)
        got += [rows(eng, s, int(c) & 0x3FFFFFFF)[0] for c in children if c >= 0]
    return out, got, eng.counters()


def assert_same_array(x, y, what):
    """Same dtype, same shape, same bytes (tells -0.0 from 0.0) and np.array_equal (no NaN passes as equal to itself; records
    are compared by their bytes alone: they hold padding that numpy's == skips)."""
    x, y = np.asarray(x), np.asarray(y)
    assert x.dtype == y.dtype and x.shape == y.shape, (what, x.dtype, y.dtype, x.shape, y.shape)
    assert x.tobytes() == y.tobytes() and (x.dtype.names is not None or np.array_equal(x, y)), (what, x, y)


def assert_same_fields(x, y, what):
    assert set(x) == set(y), (what, sorted(x), sorted(y))
    for k in x:
        assert_same_array(x[k], y[k], what + (k,))


def assert_same(a, b, what, ignore_counters=()):
    """Two snapshots equal in everything, but for the counters named in ignore_counters."""
    (oa, ra, ca), (ob, rb, cb) = a, b
    assert_same_fields(oa, ob, (what,))
    assert len(ra) == len(rb), (what, "node rows", len(ra), len(rb))
    for i, (x, y) in enumerate(zip(ra, rb)):
        assert_same_fields(x, y, (what, "node row", i))
    rest = lambda c: {k: v for k, v in c.items() if k not in ignore_counters}
    assert rest(ca) == rest(cb), (what, ca, cb)


def same_as_first(snaps, what):
    for b in snaps[1:]:
        assert_same(snaps[0], b, what)


def same_trio(snaps, what, probing=True):
    """(lock-step, wave, cached wave) snapshots of one moment: same trees, and the counter identities.  probing=False: an
    engine whose search takes the flag and probes nothing."""
    a, b, c = snaps
    assert_same(a, b, what)
    assert_same(a, c, what, ignore_counters=CACHE_COUNTERS)
    ca, cc = a[2], c[2]
    assert ca["eval_cache_hits"] == 0 and ca["eval_cache_probes"] == 0, (what, ca)
    if probing:
        assert cc["eval_cache_probes"] == cc["evals"] + cc["eval_cache_hits"] == ca["evals"], (what, ca, cc)
    else:
        assert cc == ca, (what, ca, cc)


def step_and_compare(engines, sims, rng, rows, mask=None, what="", check=same_as_first):
    """One run_sims on every engine (the pair, or the trio with check=same_trio), compared by check(snapshots, what); returns
    the snapshots, the lock-step engine's first."""
    u = rng.random_sample(engines[0].n_slots)
    for e in engines:
        e.run_sims(sims, mask=mask)
    snaps = [snapshot(e, 1.0, u, rows) for e in engines]
    check(snaps, what)
    return snaps


def sampled_moves(snap):
    return np.where(snap[0]["action"] >= 0, snap[0]["action"], -1).astype(np.int32)


def counter_delta(after, before):
    return {k: after[k] - before[k] for k in CACHE_COUNTERS}


# ---- golden vectors of the reference -----------------------------------------------------------------------------------------
def replay_find_move_golden(golden_dir, fname, game, launch=None):
    """The recorded FindMove calls of one golden file on one engine, a slot per game: plays, win rates, root statistics, sampled
    action and probabilities, exactly.  launch: bb_config.launch, which the engine must then report (None: not passed)."""
    g = np.load(os.path.join(golden_dir, fname), allow_pickle=False)
    A = _lib.game_info(game).A
    dc = game == DC
    cells = 64 if dc else _lib.GRID[game][0] * _lib.GRID[game][1]
    sims, seed, salt, max_depth, fixed, reuse = [int(x) for x in g["meta"]]
    assert launch is None or not fixed
    c, temp = [float(x) for x in g["cfg"]]
    gs = g["game_start"]
    ng = len(gs) - 1
    lens = np.diff(gs)
    st_all = pack_states(game, g)
    eng = _lib.Engine(game, n_slots=ng, sims_per_move=sims, mcts_kind=_lib.MCTS_FIXED if fixed else _lib.MCTS_DYNAMIC,
                      max_depth=max_depth, evaluator=_lib.EVAL_HASH, c_puct=c, hash_salt=salt, salt_per_game=True,
                      node_capacity=sims * (cells + 1) * (max_depth if fixed else 1) + 8,
                      **({} if launch is None else dict(launch=launch)))
    assert launch is None or eng.run_sims_structure() == launch
    eng.set_roots(st_all[gs[:-1]], game_ids=np.arange(ng))
    for ply in range(int(lens.max())):
        live = lens > ply
        idx = gs[:-1] + np.minimum(ply, lens - 1)
        # FindMove asserts Root.State == state: the engine's root must be the fixture's position
        roots = eng.root_states()
        assert same_position(game, roots[live], st_all[idx][live])
        eng.run_sims(sims)
        out = eng.sample_moves(temp, u=g["u"][idx])
        for s in np.where(live)[0]:
            i = idx[s]
            if dc:  # compact child lists: (action, plays) pairs in ascending action order
                k = int((g["plays"][i][:, 0] >= 0).sum())
                assert np.array_equal(out["child_action"][s, :k], g["plays"][i][:k, 0].astype(np.int32)), (fname, s, ply)
                assert (out["child_action"][s, k:] == -1).all()
                plays = out["child_plays"][s, :k].astype(np.float64)
                assert np.array_equal(plays, g["plays"][i][:k, 1]), (fname, s, ply)
                n32 = out["child_plays"][s, :k].astype(np.float32)
                wr = np.where(n32 > 0, out["child_value"][s, :k] / np.maximum(n32, 1), 0).astype(np.float64)
                assert np.array_equal(wr, g["winrates"][i][:k])
                assert out["root_plays"][s] == g["root_plays"][i] and float(out["root_winrate"][s]) == g["v"][i]
                assert out["action"][s] == g["action"][i], (fname, s, ply)
                assert np.array_equal(plays / plays.sum(), g["prob"][i][:k])
                continue
            plays = out["child_plays"][s, :A].astype(np.float64)
            assert np.array_equal(plays, g["plays"][i]), (fname, s, ply, plays, g["plays"][i])
            n32 = out["child_plays"][s, :A].astype(np.float32)
            wr = np.where(n32 > 0, out["child_value"][s, :A] / np.maximum(n32, 1), 0).astype(np.float64)
            assert np.array_equal(wr, g["winrates"][i]), (fname, s, ply)
            assert out["root_plays"][s] == g["root_plays"][i]
            assert float(out["root_winrate"][s]) == g["v"][i]
            assert out["action"][s] == g["action"][i], (fname, s, ply)
            tot = plays.sum()
            assert np.array_equal(plays / tot if tot > 0 else plays, g["prob"][i])
        acts = np.where(live, g["action"][idx], -1).astype(np.int32)
        if reuse:
            eng.move_roots(acts)
        else:  # the fixture called DropRoot() after every move
            nxt_live = lens > ply + 1
            if nxt_live.any():
                sl = np.where(nxt_live)[0]
                eng.set_roots(st_all[gs[:-1][sl] + ply + 1], slots=sl, game_ids=sl)
    assert eng.counters()["overflow"] == 0
    eng.close()


# ---- the front end -----------------------------------------------------------------------------------------------------------
class HashSearch(DynamicMCTS):
    """DynamicMCTS on the validation evaluator, through the base class's _make_engine (which reads SearchLaunch)."""
    _EVALUATOR = _lib.EVAL_HASH
    salt = 0

    def __init__(self, game=None, salt=0, **kw):
        DynamicMCTS.__init__(self, **kw)
        self.Game, self.salt = game, salt

    def _make_engine(self, game_id, n_slots, sims, **kw):
        return DynamicMCTS._make_engine(self, game_id, n_slots, sims, hash_salt=self.salt, **kw)


class DirectHashSearch(DynamicMCTS):
    """DynamicMCTS on the validation evaluator with an engine of its own making (what the golden fixtures were generated with):
    unlike HashSearch it passes max_depth and no launch, so MCTS.SearchLaunch does not reach it."""
    _EVALUATOR = _lib.EVAL_HASH
    salt = 0

    def _make_engine(self, game_id, n_slots, sims, **kw):
        return _lib.Engine(game_id, n_slots=n_slots, sims_per_move=max(int(sims), 1), mcts_kind=self._KIND,
                           max_depth=self._max_depth(), evaluator=_lib.EVAL_HASH, hash_salt=self.salt,
                           c_puct=float(self.ExplorationRate), **kw)


@pytest.fixture
def launches(monkeypatch):
    """bb_config.launch and run_sims_structure() of every engine the front end creates and searches with."""
    seen = []
    real = _lib.Engine

    class Spy(real):
        def run_sims(self, sims, mask=None):
            seen.append((self.cfg.launch, self.run_sims_structure()))
            real.run_sims(self, sims, mask=mask)

    monkeypatch.setattr(_lib, "Engine", Spy)
    return seen
