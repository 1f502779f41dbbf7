"""-m gpu: the search API in one launch (bb_config.launch = BB_LAUNCH_WAVE, k_search_wave: one wave per slot) against the
lock-step loop it replaces.  Per slot the sequence of operations is the same, from the same device functions, so everything
a caller can see -- sampled moves, root statistics, the node rows of the root and of its children, the counters -- must be
the lock-step engine's bit for bit; engines the kernel does not cover must say so and search lock-step."""
import os

import numpy as np
import pytest

from blackbird_amd import Connect4, TicTacToe, _lib, arena
from blackbird_amd.MCTS import MCTS
from tests import model_cases as M
from tests import search_cases as S
from tests.search_cases import GAME_OF, HashSearch, launches  # noqa: F401  (launches: a fixture)

pytestmark = pytest.mark.gpu
C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
LOCK, WAVE = _lib.LAUNCH_LOCKSTEP, _lib.LAUNCH_WAVE
CLS_OF = {"c4": Connect4.BoardState, "ttt": TicTacToe.BoardState}


def _engine(game, n_slots, launch, ev="hash", node_capacity=512, **kw):
    return S.dense_engine(game, n_slots, launch, ev, node_capacity=node_capacity, **kw)


def _pair(game, n_slots, ev="hash", want=WAVE, **kw):
    return S.lock_and_wave(lambda launch: _engine(game, n_slots, launch, ev, **kw), want)


EVALUATORS = {"hash": "hash", "net_r0": ("net", 16, 0), "net_r2": ("net", 16, 2)}


@pytest.mark.parametrize("sims", [1, 2, 50])
@pytest.mark.parametrize("n_slots", [1, 3, 5])   # never a multiple of the four waves of a workgroup
@pytest.mark.parametrize("ev", list(EVALUATORS))
@pytest.mark.parametrize("key", ["c4", "ttt"])
def test_same_bits_as_lockstep_over_three_moves(key, ev, n_slots, sims):
    """Three consecutive moves with tree reuse (move_roots); after every search the two engines agree on everything."""
    game = GAME_OF[key]
    lock, wave = _pair(game, n_slots, EVALUATORS[ev])
    S.set_roots_on((lock, wave), S.openings(game, n_slots))
    rng = np.random.RandomState(5)
    for move in range(3):
        a = S.step_and_compare((lock, wave), sims, rng, S.view_rows, what=(key, ev, n_slots, sims, move))[0]
        assert a[2]["overflow"] == 0 and a[2]["sims"] == (move + 1) * sims * n_slots
        for e in (lock, wave):
            e.move_roots(S.sampled_moves(a))
    S.close_all(lock, wave)


@pytest.mark.parametrize("ev", ["hash", "net_r2"])
@pytest.mark.parametrize("key", ["c4", "ttt"])
def test_roots_next_to_a_win_and_to_a_full_board(golden_dir, key, ev):
    game = GAME_OF[key]
    lock, wave = _pair(game, 5, EVALUATORS[ev])
    S.set_roots_on((lock, wave), S.endgame_roots(golden_dir, key))
    rng = np.random.RandomState(6)
    for move in range(2):
        a = S.step_and_compare((lock, wave), 50, rng, S.view_rows, what=(key, ev, move))[0]
        assert a[2]["terminal_leaves"] > 0 and a[2]["overflow"] == 0
        for e in (lock, wave):
            e.move_roots(S.sampled_moves(a))
    S.close_all(lock, wave)


@pytest.mark.parametrize("ev", ["hash", "net_r2"])
def test_masked_search_leaves_the_other_slots_alone(ev):
    lock, wave = _pair(C4, 5, EVALUATORS[ev])
    S.set_roots_on((lock, wave), S.openings(C4, 5))
    rng = np.random.RandomState(7)
    even = np.array([1, 0, 1, 0, 1], dtype=np.uint8)
    before = None
    for k, mask in enumerate((even, 1 - even, even, 1 - even)):
        a = S.step_and_compare((lock, wave), 20, rng, S.view_rows, mask=mask, what=(ev, k))[0]
        for s in np.nonzero(mask == 0)[0]:   # a slot outside the mask: its tree is what it was
            now = wave.node_view(int(s), -1)
            if before is not None:
                assert all(np.array_equal(now[f], before[int(s)][f]) for f in now), (ev, k, s)
        before = {s: wave.node_view(s, -1) for s in range(5)}
        assert a[2]["sims"] == 20 * sum(int(m.sum()) for m in (even, 1 - even, even, 1 - even)[:k + 1])
    S.close_all(lock, wave)


@pytest.mark.parametrize("ev", ["hash", "net_r0"])
def test_three_short_calls_equal_one_long_call(ev):
    """run_sims(16) three times == run_sims(48) once: nothing of a call outlives its launch but the tree."""
    lock, once = _pair(C4, 3, EVALUATORS[ev])
    thrice = _engine(C4, 3, WAVE, EVALUATORS[ev])
    S.set_roots_on((lock, once, thrice), S.openings(C4, 3))
    u = np.random.RandomState(8).random_sample(3)
    lock.run_sims(48)
    once.run_sims(48)
    for _ in range(3):
        thrice.run_sims(16)
    a = S.snapshot(lock, 1.0, u, S.view_rows)
    S.assert_same(a, S.snapshot(once, 1.0, u, S.view_rows), "48 at once")
    S.assert_same(a, S.snapshot(thrice, 1.0, u, S.view_rows), "3 x 16")
    S.close_all(lock, once, thrice)


@pytest.mark.parametrize("ev", ["hash", "net_r2"])
def test_ancestors_and_reset_roots(ev):
    """track_ancestors: every backup also walks the chain above the root (backup_path, not the store-only variants), so
    after two moves bb_reset_roots finds the same statistics at the top."""
    lock, wave = _pair(TTT, 3, EVALUATORS[ev], track_ancestors=True)
    S.set_roots_on((lock, wave), S.openings(TTT, 3))
    rng = np.random.RandomState(9)
    for move in range(2):
        a = S.step_and_compare((lock, wave), 30, rng, S.view_rows, what=(ev, move))[0]
        for e in (lock, wave):
            e.move_roots(S.sampled_moves(a))
    a = S.step_and_compare((lock, wave), 30, rng, S.view_rows, what=(ev, "below"))[0]
    for e in (lock, wave):
        e.reset_roots()
    top = S.snapshot(lock, 0.0, None, S.view_rows)
    S.assert_same(top, S.snapshot(wave, 0.0, None, S.view_rows), (ev, "after reset"))
    assert (top[0]["root_plays"] == 90).all()
    S.step_and_compare((lock, wave), 10, rng, S.view_rows, what=(ev, "on the reset tree"))
    S.close_all(lock, wave)


@pytest.mark.parametrize("ev", ["hash", "net_r0"])
def test_full_node_pool_counts_the_same_overflow(ev):
    lock, wave = _pair(C4, 3, EVALUATORS[ev], node_capacity=24)
    S.set_roots_on((lock, wave), S.openings(C4, 3))
    a = S.step_and_compare((lock, wave), 50, np.random.RandomState(10), S.view_rows, what=ev)[0]
    assert a[2]["overflow"] > 0 and a[2]["nodes"] <= 3 * 23   # (the root takes one of a pool's 24 rows)
    S.close_all(lock, wave)


# ---- golden vectors of the reference, replayed under the wave launch (as tests/test_gpu_mcts.py::test_find_move_golden) ----
@pytest.mark.parametrize("fname", ["mcts_c4_s50.npz", "mcts_ttt_s50.npz", "mcts_c4_s64_t0.npz"])
def test_find_move_golden_under_wave(golden_dir, fname):
    S.replay_find_move_golden(golden_dir, fname, GAME_OF[fname.split("_")[1]], launch=WAVE)


# ---- the front end: MCTS.SearchLaunch --------------------------------------------------------------------------------
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
    return M.model(game, name, seed=seed, play_limit=32, eps=0.3, blocks=2)


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
    states = np.repeat(_lib.game_initial(game), 3, axis=0) if game == DC else S.openings(game, 3)
    S.set_roots_on((lock, wave), states)
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
    S.close_all(lock, wave)


def test_structure_entry_point_arguments():
    import ctypes as C
    eng = _engine(C4, 1, WAVE)
    assert _lib.lib().bb_run_sims_structure(eng.h, None) == _lib.ERR_ARG
    net = _lib.Engine(C4, n_slots=1, sims_per_move=8, evaluator=_lib.EVAL_NET, launch=WAVE)
    out = C.c_int32(-1)
    assert _lib.lib().bb_run_sims_structure(net.h, C.byref(out)) == _lib.ERR_WEIGHTS   # read it after bb_load_weights
    net.load_weights(S.dense_weights(C4, 16, 2))
    assert net.run_sims_structure() == WAVE and net.selfplay_mode() == 0   # self-play treats the value as lock-step
    with pytest.raises(ValueError):
        _lib.Engine(C4, n_slots=1, sims_per_move=8, evaluator=_lib.EVAL_HASH, launch=4)
    S.close_all(eng, net)
