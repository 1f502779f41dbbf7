"""-m gpu: the search API in one launch (bb_config.launch = BB_LAUNCH_WAVE, k_search_wave: one wave per slot) against the
lock-step loop it replaces.  Per slot the sequence of operations is the same, from the same device functions, so everything
a caller can see -- sampled moves, root statistics, the node rows of the root and of its children, the counters -- must be
the lock-step engine's bit for bit; engines the kernel does not cover must say so and search lock-step."""
import functools
import os

import numpy as np
import pytest

from blackbird_amd import Blackbird, Connect4, TicTacToe, _lib, arena
from blackbird_amd import weights as W
from blackbird_amd.DynamicMCTS import DynamicMCTS
from blackbird_amd.MCTS import MCTS
from tests.test_gpu_mcts import pack_states, same_position

pytestmark = pytest.mark.gpu
C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
LOCK, WAVE = _lib.LAUNCH_LOCKSTEP, _lib.LAUNCH_WAVE
GAME_OF = {"c4": C4, "ttt": TTT}
CLS_OF = {"c4": Connect4.BoardState, "ttt": TicTacToe.BoardState}


@functools.lru_cache(maxsize=None)
def _weights(game, filters, blocks):
    gi = _lib.game_info(game)
    return W.flatten(W.init_weights(gi.C, filters, blocks, 16, gi.A, seed=21, perturb=True))


def _engine(game, n_slots, launch, ev="hash", **kw):
    """ev: 'hash', 'rollout', or ('net', filters, blocks) with the prior noise on (epsilon 0.3)."""
    kw.setdefault("node_capacity", 512)
    common = dict(n_slots=n_slots, sims_per_move=8, seed=17, first_game_id=1000, launch=launch, **kw)
    if ev == "hash":
        return _lib.Engine(game, evaluator=_lib.EVAL_HASH, hash_salt=4242, salt_per_game=True, **common)
    if ev == "rollout":
        return _lib.Engine(game, evaluator=_lib.EVAL_ROLLOUT, **common)
    eng = _lib.Engine(game, evaluator=_lib.EVAL_NET, noise_on=True, alpha=0.2, epsilon=0.3, **common)
    eng.load_weights(_weights(game, ev[1], ev[2]))
    return eng


def _pair(game, n_slots, ev="hash", want=WAVE, **kw):
    lock, wave = _engine(game, n_slots, LOCK, ev, **kw), _engine(game, n_slots, WAVE, ev, **kw)
    assert lock.run_sims_structure() == LOCK and wave.run_sims_structure() == want
    return lock, wave


def _openings(game, n):
    """n different positions two plies into the game."""
    A = _lib.game_info(game).A
    st = np.repeat(_lib.game_initial(game), n, axis=0)
    i = np.arange(n)
    for moves in (i % A, (i + 4) % A):
        st, status = _lib.game_apply(game, st, moves.astype(np.int32))
        assert (status == 0).all()
    return st


def _set(engines, states):
    for e in engines:
        e.set_roots(states, game_ids=7 * np.arange(len(states)) + 3)


def _snap(eng, temp=1.0, u=None):
    """Everything of the trees a caller can read: bb_sample_moves' outputs, the node rows of every root and of its children
    (bb_node_view), the counters."""
    out = eng.sample_moves(temp, u)
    rows = []
    for s in range(eng.n_slots):
        root = eng.node_view(s, -1)
        rows.append(root)
        rows += [eng.node_view(s, int(c) & 0x3FFFFFFF) for c in root["child"] if c >= 0]
    return out, rows, eng.counters()


def _same(a, b, what=""):
    (oa, ra, ca), (ob, rb, cb) = a, b
    for k in oa:
        assert np.array_equal(oa[k], ob[k]), (what, k, oa[k], ob[k])
    assert len(ra) == len(rb), what
    for i, (x, y) in enumerate(zip(ra, rb)):
        for k in x:
            assert np.array_equal(x[k], y[k]), (what, "node row", i, k, x[k], y[k])
    assert ca == cb, (what, ca, cb)


def _step(lock, wave, sims, rng, mask=None, what=""):
    """One run_sims on both engines, compared; returns the lock-step snapshot."""
    u = rng.random_sample(lock.n_slots)
    for e in (lock, wave):
        e.run_sims(sims, mask=mask)
    a, b = _snap(lock, 1.0, u), _snap(wave, 1.0, u)
    _same(a, b, what)
    return a


def _moves(snapshot):
    return np.where(snapshot[0]["action"] >= 0, snapshot[0]["action"], -1).astype(np.int32)


EVALUATORS = {"hash": "hash", "net_r0": ("net", 16, 0), "net_r2": ("net", 16, 2)}


@pytest.mark.parametrize("sims", [1, 2, 50])
@pytest.mark.parametrize("n_slots", [1, 3, 5])   # never a multiple of the four waves of a workgroup
@pytest.mark.parametrize("ev", list(EVALUATORS))
@pytest.mark.parametrize("key", ["c4", "ttt"])
def test_same_bits_as_lockstep_over_three_moves(key, ev, n_slots, sims):
    """Three consecutive moves with tree reuse (move_roots); after every search the two engines agree on everything."""
    game = GAME_OF[key]
    lock, wave = _pair(game, n_slots, EVALUATORS[ev])
    _set((lock, wave), _openings(game, n_slots))
    rng = np.random.RandomState(5)
    for move in range(3):
        a = _step(lock, wave, sims, rng, what=(key, ev, n_slots, sims, move))
        assert a[2]["overflow"] == 0 and a[2]["sims"] == (move + 1) * sims * n_slots
        for e in (lock, wave):
            e.move_roots(_moves(a))
    for e in (lock, wave):
        e.close()


def _endgame_roots(golden_dir, key):
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


@pytest.mark.parametrize("ev", ["hash", "net_r2"])
@pytest.mark.parametrize("key", ["c4", "ttt"])
def test_roots_next_to_a_win_and_to_a_full_board(golden_dir, key, ev):
    game = GAME_OF[key]
    lock, wave = _pair(game, 5, EVALUATORS[ev])
    _set((lock, wave), _endgame_roots(golden_dir, key))
    rng = np.random.RandomState(6)
    for move in range(2):
        a = _step(lock, wave, 50, rng, what=(key, ev, move))
        assert a[2]["terminal_leaves"] > 0 and a[2]["overflow"] == 0
        for e in (lock, wave):
            e.move_roots(_moves(a))
    for e in (lock, wave):
        e.close()


@pytest.mark.parametrize("ev", ["hash", "net_r2"])
def test_masked_search_leaves_the_other_slots_alone(ev):
    lock, wave = _pair(C4, 5, EVALUATORS[ev])
    _set((lock, wave), _openings(C4, 5))
    rng = np.random.RandomState(7)
    even = np.array([1, 0, 1, 0, 1], dtype=np.uint8)
    before = None
    for k, mask in enumerate((even, 1 - even, even, 1 - even)):
        a = _step(lock, wave, 20, rng, mask=mask, what=(ev, k))
        for s in np.nonzero(mask == 0)[0]:   # a slot outside the mask: its tree is what it was
            now = wave.node_view(int(s), -1)
            if before is not None:
                assert all(np.array_equal(now[f], before[int(s)][f]) for f in now), (ev, k, s)
        before = {s: wave.node_view(s, -1) for s in range(5)}
        assert a[2]["sims"] == 20 * sum(int(m.sum()) for m in (even, 1 - even, even, 1 - even)[:k + 1])
    for e in (lock, wave):
        e.close()


@pytest.mark.parametrize("ev", ["hash", "net_r0"])
def test_three_short_calls_equal_one_long_call(ev):
    """run_sims(16) three times == run_sims(48) once: nothing of a call outlives its launch but the tree."""
    lock, once = _pair(C4, 3, EVALUATORS[ev])
    thrice = _engine(C4, 3, WAVE, EVALUATORS[ev])
    _set((lock, once, thrice), _openings(C4, 3))
    u = np.random.RandomState(8).random_sample(3)
    lock.run_sims(48)
    once.run_sims(48)
    for _ in range(3):
        thrice.run_sims(16)
    a = _snap(lock, 1.0, u)
    _same(a, _snap(once, 1.0, u), "48 at once")
    _same(a, _snap(thrice, 1.0, u), "3 x 16")
    for e in (lock, once, thrice):
        e.close()


@pytest.mark.parametrize("ev", ["hash", "net_r2"])
def test_ancestors_and_reset_roots(ev):
    """track_ancestors: every backup also walks the chain above the root (backup_path, not the store-only variants), so
    after two moves bb_reset_roots finds the same statistics at the top."""
    lock, wave = _pair(TTT, 3, EVALUATORS[ev], track_ancestors=True)
    _set((lock, wave), _openings(TTT, 3))
    rng = np.random.RandomState(9)
    for move in range(2):
        a = _step(lock, wave, 30, rng, what=(ev, move))
        for e in (lock, wave):
            e.move_roots(_moves(a))
    a = _step(lock, wave, 30, rng, what=(ev, "below"))
    for e in (lock, wave):
        e.reset_roots()
    top = _snap(lock, 0.0)
    _same(top, _snap(wave, 0.0), (ev, "after reset"))
    assert (top[0]["root_plays"] == 90).all()
    _step(lock, wave, 10, rng, what=(ev, "on the reset tree"))
    for e in (lock, wave):
        e.close()


@pytest.mark.parametrize("ev", ["hash", "net_r0"])
def test_full_node_pool_counts_the_same_overflow(ev):
    lock, wave = _pair(C4, 3, EVALUATORS[ev], node_capacity=24)
    _set((lock, wave), _openings(C4, 3))
    a = _step(lock, wave, 50, np.random.RandomState(10), what=ev)
    assert a[2]["overflow"] > 0 and a[2]["nodes"] <= 3 * 23   # (the root takes one of a pool's 24 rows)
    for e in (lock, wave):
        e.close()


# ---- golden vectors of the reference, replayed under the wave launch (as tests/test_gpu_mcts.py::test_find_move_golden) ----
@pytest.mark.parametrize("fname", ["mcts_c4_s50.npz", "mcts_ttt_s50.npz", "mcts_c4_s64_t0.npz"])
def test_find_move_golden_under_wave(golden_dir, fname):
    g = np.load(os.path.join(golden_dir, fname), allow_pickle=False)
    game = GAME_OF[fname.split("_")[1]]
    A = _lib.game_info(game).A
    cells = _lib.GRID[game][0] * _lib.GRID[game][1]
    sims, seed, salt, max_depth, fixed, reuse = [int(x) for x in g["meta"]]
    assert not fixed
    c, temp = [float(x) for x in g["cfg"]]
    gs = g["game_start"]
    ng = len(gs) - 1
    lens = np.diff(gs)
    st_all = pack_states(game, g)
    eng = _lib.Engine(game, n_slots=ng, sims_per_move=sims, mcts_kind=_lib.MCTS_DYNAMIC, max_depth=max_depth,
                      evaluator=_lib.EVAL_HASH, c_puct=c, hash_salt=salt, salt_per_game=True,
                      node_capacity=sims * (cells + 1) + 8, launch=WAVE)
    assert eng.run_sims_structure() == WAVE
    eng.set_roots(st_all[gs[:-1]], game_ids=np.arange(ng))
    for ply in range(int(lens.max())):
        live = lens > ply
        idx = gs[:-1] + np.minimum(ply, lens - 1)
        roots = eng.root_states()
        assert same_position(game, roots[live], st_all[idx][live])
        eng.run_sims(sims)
        out = eng.sample_moves(temp, u=g["u"][idx])
        for s in np.where(live)[0]:
            i = idx[s]
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
        else:
            nxt_live = lens > ply + 1
            if nxt_live.any():
                sl = np.where(nxt_live)[0]
                eng.set_roots(st_all[gs[:-1][sl] + ply + 1], slots=sl, game_ids=sl)
    assert eng.counters()["overflow"] == 0
    eng.close()


# ---- the front end: MCTS.SearchLaunch --------------------------------------------------------------------------------
class HashSearch(DynamicMCTS):
    """DynamicMCTS on the validation evaluator, through the base class's _make_engine (which reads SearchLaunch)."""
    _EVALUATOR = _lib.EVAL_HASH
    salt = 0

    def __init__(self, game=None, salt=0, **kw):
        DynamicMCTS.__init__(self, **kw)
        self.Game, self.salt = game, salt

    def _make_engine(self, game_id, n_slots, sims, **kw):
        return DynamicMCTS._make_engine(self, game_id, n_slots, sims, hash_salt=self.salt, **kw)


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


def test_resetroot_and_children_golden_under_wave(golden_dir, monkeypatch, launches):
    """tests/test_gpu_mirror.py::test_resetroot_and_children_golden with MCTS.SearchLaunch = 'wave'."""
    monkeypatch.setattr(MCTS, "SearchLaunch", "wave")
    g = np.load(os.path.join(golden_dir, "resetroot_c4.npz"), allow_pickle=False)
    cls = Connect4.BoardState
    sims, moves, sims_after, salt = [int(x) for x in g["meta"]]
    m = HashSearch(salt=salt, explorationRate=0.85, playLimit=sims)
    s = cls()
    for k in range(moves):
        nxt, _v, _p = m.FindMove(s, 0)
        want = s.Copy()
        want.ApplyAction(int(g["actions"][k]))
        assert nxt == want
        s = nxt
        m.MoveRoot(s)
    m.ResetRoot()
    node = m.Root
    assert node.State == cls() and node.Parent is None
    for depth in range(moves + 1):
        assert node.Plays == g[f"plays_{depth}"], depth
        assert np.float32(node.Value) == np.float32(g[f"value_{depth}"]), depth
        assert np.array_equal(node.ChildPlays(), g[f"child_plays_{depth}"]), depth
        assert np.array_equal(node.ChildWinRates(), g[f"child_winrates_{depth}"]), depth
        assert np.array_equal(node.LegalActions, g[f"legal_{depth}"]), depth
        assert [c is None for c in node.Children] == list(g[f"children_none_{depth}"]), depth
        if depth < moves:
            child = node.Children[int(g["actions"][depth])]
            assert child.Parent is node
            node = child
    nxt, v, prob = m.FindMove(cls(), 0, playLimit=sims_after)
    assert m.Root.Plays == g["after_plays"] and float(v) == float(g["after_v"])
    assert np.array_equal(m.Root.ChildPlays(), g["after_child_plays"])
    assert np.array_equal(m.Root.ChildWinRates(), g["after_child_winrates"])
    assert np.array_equal(prob, g["after_prob"])
    assert launches and all(x == (WAVE, WAVE) for x in launches)


def _model(game, name, seed):
    cfg = {"blocks": 2, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": {"optimizer": "adam"}}
    np.random.seed(seed)  # weight initialisation draws from numpy's stream
    return Blackbird.Model(game, name, {"explorationRate": 0.85, "playLimit": 32}, cfg)


@pytest.mark.parametrize("players", ["hash", "model"])
@pytest.mark.parametrize("temp", [0, 1.0])
def test_batched_arena_same_results_under_wave(tmp_path, monkeypatch, launches, players, temp):
    """TestModelsBatched, 6 games at 32 simulations, at temp 0 and at temp 1 with supplied uniforms: the result array of
    'lockstep' again under 'wave' (a Model's engines draw their prior noise from a seed taken from numpy's state: reseeded)."""
    monkeypatch.chdir(tmp_path)
    game = Connect4.BoardState
    if players == "hash":
        p1, p2 = HashSearch(game, 11, explorationRate=0.85, playLimit=32), HashSearch(game, 22, explorationRate=1.3, playLimit=32)
    else:
        p1, p2 = _model(game, "a", 1), _model(game, "b", 2)
    first = np.array([True, False, False, True, True, False])
    results = {}
    for launch in ("lockstep", "wave"):
        monkeypatch.setattr(MCTS, "SearchLaunch", launch)
        del launches[:]
        np.random.seed(3)
        results[launch] = arena.TestModelsBatched(p1, p2, temp, 6, playLimit=32, first=first,
                                                  uniforms=np.random.RandomState(5).random_sample)
        want = (WAVE, WAVE) if launch == "wave" else (_lib.LAUNCH_AUTO, LOCK)
        assert launches and all(x == want for x in launches), (launch, launches[:4])
    assert np.array_equal(results["lockstep"], results["wave"]), results
    assert set(np.unique(results["wave"])) <= {-1, 0, 1}


# ---- engines the kernel does not cover: visible, and lock-step ---------------------------------------------------------
FALLBACKS = {
    "dragonchess": (DC, "hash", dict(max_plies=24, node_capacity=128)),
    "rollout": (C4, "rollout", {}),
    "wide_network": (C4, ("net", 32, 2), {}),
    "net_form_f32": (C4, ("net", 16, 2), dict(net_form=_lib.NET_FORM_F32)),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_uncovered_engines_search_lockstep_and_say_so(case):
    game, ev, kw = FALLBACKS[case]
    lock, wave = _pair(game, 3, ev, want=LOCK, **kw)
    states = np.repeat(_lib.game_initial(game), 3, axis=0) if game == DC else _openings(game, 3)
    _set((lock, wave), states)
    u = np.random.RandomState(11).random_sample(3)
    for e in (lock, wave):
        e.run_sims(20)
    oa, ob = lock.sample_moves(1.0, u), wave.sample_moves(1.0, u)
    for k in oa:
        assert np.array_equal(oa[k], ob[k]), (case, k)
    for s in range(3):
        ra, rb = lock.node_edges(s, -1), wave.node_edges(s, -1)
        assert all(np.array_equal(ra[k], rb[k]) for k in ra), (case, s)
    assert lock.counters() == wave.counters()
    for e in (lock, wave):
        e.close()


def test_structure_entry_point_arguments():
    import ctypes as C
    eng = _engine(C4, 1, WAVE)
    assert _lib.lib().bb_run_sims_structure(eng.h, None) == _lib.ERR_ARG
    net = _lib.Engine(C4, n_slots=1, sims_per_move=8, evaluator=_lib.EVAL_NET, launch=WAVE)
    out = C.c_int32(-1)
    assert _lib.lib().bb_run_sims_structure(net.h, C.byref(out)) == _lib.ERR_WEIGHTS   # read it after bb_load_weights
    net.load_weights(_weights(C4, 16, 2))
    assert net.run_sims_structure() == WAVE and net.selfplay_mode() == 0   # self-play treats the value as lock-step
    with pytest.raises(ValueError):
        _lib.Engine(C4, n_slots=1, sims_per_move=8, evaluator=_lib.EVAL_HASH, launch=4)
    for e in (eng, net):
        e.close()
