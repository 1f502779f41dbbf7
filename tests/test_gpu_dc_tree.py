"""-m gpu: the DragonChess search tree behind the MCTS API -- Root statistics over the 4032 actions, Children, ResetRoot
(the ancestor chain of bb_config.track_ancestors) and bb_node_edges -- against the reference's own runs
(tests/make_golden.py gen_mcts, tests/make_golden_dc_tree.py) and against the engine without the chain."""
import os

import numpy as np
import pytest

from blackbird_amd import _lib, Connect4, DragonChess
from tests.search_cases import DirectHashSearch as HashSearch

pytestmark = pytest.mark.gpu
DC = _lib.GAME_DRAGONCHESS
A = 4032


def dense(idx, vals):
    out = np.zeros(A, dtype=np.float64)
    out[idx] = vals
    return out


def test_findmove_api_golden_dc(golden_dir, monkeypatch):
    """FindMove + MoveRoot through the Python mirror: Root.ChildPlays / ChildWinRates / ChildProbability over the 4032 actions,
    as the reference returns them (the fixture keeps the legal entries only, in ascending action order)."""
    g = np.load(os.path.join(golden_dir, "mcts_dc_s24.npz"), allow_pickle=False)
    sims, _seed, salt, _max_depth, _fixed, reuse = [int(x) for x in g["meta"]]
    c, temp = [float(x) for x in g["cfg"]]
    assert reuse
    gs = g["game_start"]
    for gi in range(len(gs) - 1):
        m = HashSearch(explorationRate=c, playLimit=sims)
        m.salt = salt + gi
        state = DragonChess.BoardState()
        m.DropRoot()
        for i in range(gs[gi], gs[gi + 1]):
            k = int((g["plays"][i][:, 0] >= 0).sum())
            legal = g["plays"][i][:k, 0].astype(np.int64)
            assert np.array_equal(np.where(state.LegalActions() == 1)[0], legal)
            monkeypatch.setattr(np.random, "random_sample", lambda *a, _u=float(g["u"][i]): _u)
            nxt, v, prob = m.FindMove(state, temp)
            assert prob.shape == (A,) and m.Root.ChildPlays().shape == (A,) and m.Root.ChildWinRates().shape == (A,)
            assert np.array_equal(prob, dense(legal, g["prob"][i][:k])), i
            assert np.array_equal(m.Root.ChildPlays(), dense(legal, g["plays"][i][:k, 1])), i
            assert np.array_equal(m.Root.ChildWinRates(), dense(legal, g["winrates"][i][:k])), i
            assert np.array_equal(m.Root.LegalActions, state.LegalActions())
            assert m.Root.Plays == g["root_plays"][i] and float(v) == g["v"][i]
            want = state.Copy()
            want.ApplyAction(int(g["action"][i]))
            assert nxt == want
            state = nxt
            m.MoveRoot(state)


def test_resetroot_and_children_golden_dc(golden_dir):
    """MCTS.ResetRoot (MCTS.py:214-225) after three FindMove + MoveRoot (White, White, Black: the chain crosses an edge where
    the player to move stays the same), then down the played line through Children, then FindMove on the tree it left."""
    g = np.load(os.path.join(golden_dir, "resetroot_dc.npz"), allow_pickle=False)
    cls = DragonChess.BoardState
    sims, moves, sims_after, salt = [int(x) for x in g["meta"]]
    m = HashSearch(explorationRate=0.85, playLimit=sims)
    m.salt = salt
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
    assert node.State == cls() and node.Parent is None and m._root_state == cls()
    for depth in range(moves + 1):
        assert node.Plays == g[f"plays_{depth}"], depth
        assert np.float32(node.Value) == np.float32(g[f"value_{depth}"]), depth
        assert np.array_equal(node.ChildPlays(), g[f"child_plays_{depth}"]), depth
        assert np.array_equal(node.ChildWinRates(), g[f"child_winrates_{depth}"]), depth
        assert np.array_equal(node.LegalActions, g[f"legal_{depth}"]), depth
        assert len(node.Children) == A
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
    want = cls()
    want.ApplyAction(int(g["after_action"]))
    assert nxt == want
    # ResetRoot on a tree that never moved, and on no tree at all, changes nothing
    m.ResetRoot()
    assert m.Root.Plays == g["after_plays"] and m._root_state == cls()
    fresh = HashSearch(explorationRate=0.85, playLimit=4)
    fresh.ResetRoot()
    assert fresh.Root is None


def dc_engine(track, sims=16, **kw):
    return _lib.Engine(DC, n_slots=1, sims_per_move=sims, evaluator=_lib.EVAL_HASH, hash_salt=4400, c_puct=0.85,
                       node_capacity=4096, track_ancestors=track, **kw)


def play_line(eng, sims, n_moves, actions=None):
    """run_sims + the most visited move (temp 0), n_moves times; returns the actions played."""
    played = []
    for k in range(n_moves):
        eng.run_sims(sims)
        a = int(eng.sample_moves(0.0)["action"][0]) if actions is None else int(actions[k])
        eng.move_roots([a])
        played.append(a)
    return played


def test_c_abi_reset_roots_and_node_edges_dc():
    s0 = _lib.game_initial(DC)
    eng = dc_engine(True)
    eng.set_roots(s0)
    acts = play_line(eng, 16, 3)
    eng.run_sims(16)
    below = eng.sample_moves(0.0)
    below_edges = eng.node_edges(0, -1)
    # the same search without the chain: the statistics at the current root are the same bits
    ref = dc_engine(False)
    ref.set_roots(s0)
    play_line(ref, 16, 3, acts)
    ref.run_sims(16)
    ref_out = ref.sample_moves(0.0)
    for key in ("action", "root_winrate", "root_plays", "child_action", "child_plays", "child_value"):
        assert below[key].tobytes() == ref_out[key].tobytes(), key
    ref_edges = ref.node_edges(0, -1)
    for key in ("action", "child", "plays", "value", "state"):
        assert below_edges[key].tobytes() == ref_edges[key].tobytes(), key
    with pytest.raises(AssertionError):
        ref.reset_roots()   # BB_ERR_STATE: no chain kept
    ref.close()
    # ResetRoot: back to the first position, with all 64 simulations
    eng.reset_roots()
    assert eng.root_states().tobytes() == s0.tobytes()
    top = eng.sample_moves(0.0)
    r = eng.node_edges(0, -1)
    n = r["n_children"]
    assert r["node"] == 0 and r["flags"] & 1
    legal = np.where(_lib.game_legal(DC, s0)[0] == 1)[0]
    assert n == len(legal) and np.array_equal(np.sort(r["action"][:n]), legal) and (r["action"][n:] == -1).all()
    assert np.array_equal(r["action"], top["child_action"][0]) and np.array_equal(r["plays"], top["child_plays"][0])
    assert np.array_equal(r["value"], top["child_value"][0])
    assert top["root_plays"][0] == 64 and r["plays"].sum() == 63   # (the first simulation expanded the root itself)
    # the played line hangs below: its first edge leads to the node the second search started from
    k = int(np.where(r["action"] == acts[0])[0][0])
    c1 = eng.node_edges(0, int(r["child"][k]) & 0x3FFFFFFF)
    assert c1["plays"].sum() + 1 >= 16 and c1["n_children"] > 0
    with pytest.raises(ValueError):
        eng.node_edges(0, 4000)   # not a node of the tree
    eng.close()


def test_node_edges_dense_matches_node_view():
    eng = _lib.Engine(_lib.GAME_CONNECT4, n_slots=1, sims_per_move=40, evaluator=_lib.EVAL_HASH, c_puct=0.85,
                      node_capacity=4096)
    s = Connect4.BoardState()
    for a in (3, 3, 2):
        s.ApplyAction(a)
    eng.set_roots(s._packed())
    eng.run_sims(40)
    v, e = eng.node_view(0, -1), eng.node_edges(0, -1)
    legal = [(v["legal_mask"] >> i) & 1 for i in range(7)] + [0]
    assert list(e["action"]) == [i if legal[i] else -1 for i in range(8)] and e["n_children"] == sum(legal)
    on = e["action"] >= 0
    assert np.array_equal(e["plays"][on], v["plays"][on]) and np.array_equal(e["value"][on], v["value"][on])
    assert np.array_equal(e["child"][on], v["child"][on]) and e["flags"] == v["flags"] and e["node"] == v["node"]
    assert e["state"].tobytes() == v["state"].tobytes()
    eng.close()


def test_restarted_tree_keeps_its_root_dc():
    """A move from an unexpanded root re-primes the tree at the new position: the chain above it is gone, so ResetRoot
    leaves the root where it is."""
    s0 = _lib.game_initial(DC)
    eng = dc_engine(True)
    eng.set_roots(s0)
    eng.run_sims(2)
    out = eng.sample_moves(0.0)
    k = int(np.where((out["child_action"][0] >= 0) & (out["child_plays"][0] == 0))[0][0])
    a = int(out["child_action"][0, k])
    eng.move_roots([a])       # an unvisited child: the new root is not expanded
    s1, _ = _lib.game_apply(DC, s0, [a])
    b = int(np.where(_lib.game_legal(DC, s1)[0] == 1)[0][0])
    eng.move_roots([b])       # from the unexpanded root: re-prime
    s2, _ = _lib.game_apply(DC, s1, [b])
    eng.reset_roots()
    assert eng.root_states()[:, :70].tobytes() == s2[:, :70].tobytes()   # (board, players, castling rights)
    eng.close()


class TinyPool(HashSearch):
    _MAX_NODES = 6


def test_resetroot_after_pool_restart_dc():
    """MoveRoot into a full node pool restarts the tree at the new position (MCTS.py's ResetRoot then finds no ancestor):
    the front end takes the root from the engine instead of assuming the first position."""
    m = TinyPool(explorationRate=0.85, playLimit=6)
    m.salt = 4500
    s0 = DragonChess.BoardState()
    m.FindMove(s0, 0)                       # 6 simulations: 6 nodes, the pool is full
    s1 = s0.Copy()
    s1.ApplyAction(int(np.argmax(m.Root.ChildPlays())))
    m.MoveRoot(s1)                          # a node that exists
    assert m.Root.Plays > 0 and m._engine.counters()["overflow"] == 0
    a = int(np.where((m.Root.LegalActions == 1) & (m.Root.ChildPlays() == 0))[0][0])
    s2 = s1.Copy()
    s2.ApplyAction(a)
    m.MoveRoot(s2)                          # a node that does not: no room, the tree restarts at s2
    assert m._engine.counters()["overflow"] == 1 and m.Root.Plays == 0
    m.ResetRoot()
    assert m._root_state == s2 and DragonChess.BoardState._from_packed(m._engine.root_states()) == s2


def test_chain_longer_than_max_plies_is_refused_dc():
    s0 = _lib.game_initial(DC)
    eng = dc_engine(True, max_plies=2)      # room for max_plies + 2 = 4 ancestors
    eng.set_roots(s0)
    play_line(eng, 8, 4)
    eng.reset_roots()                       # four fit
    assert eng.root_states().tobytes() == s0.tobytes()
    eng.set_roots(s0)
    play_line(eng, 8, 5)
    eng.run_sims(8)
    here = eng.root_states().tobytes()
    with pytest.raises(_lib.BlackbirdHipError, match="max_plies"):
        eng.reset_roots()
    assert eng.root_states().tobytes() == here   # nothing moved
    eng.close()


def test_selfplay_refused_with_ancestors_dc():
    eng = dc_engine(True)
    with pytest.raises(AssertionError, match="track_ancestors"):
        eng.selfplay_begin(1, 1.0)
    eng.close()
