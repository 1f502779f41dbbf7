"""Oracle tree search (oracle/orc_mcts.c) vs golden vectors produced by the reference's
MCTS.py / DynamicMCTS.py / FixedMCTS.py + Model.SampleValue/GetPriors bodies under the
deterministic hash evaluator (tests/make_golden.py part 'mcts')."""
import glob
import os

import numpy as np
import pytest

KEYS = {"c4": 0, "ttt": 1, "dc": 2}
FILES = sorted(os.path.basename(p) for p in glob.glob(
    os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mcts_*.npz")))


def dense(game_A, sparse_rows, vals):
    out = np.zeros(game_A)
    for (idx, _), v in zip(sparse_rows, vals):
        if idx >= 0:
            out[int(idx)] = v
    return out


@pytest.mark.parametrize("fname", FILES)
def test_mcts_golden(orc, golden_dir, fname):
    g = np.load(os.path.join(golden_dir, fname), allow_pickle=False)
    key = fname.split("_")[1]
    game = KEYS[key]
    A = orc.dims(game)[3]
    sims, seed, salt, max_depth, fixed, reuse = [int(x) for x in g["meta"]]
    c, temp = [float(x) for x in g["cfg"]]
    gs = g["game_start"]
    for gi in range(len(gs) - 1):
        cfg = orc.make_cfg(game, kind=orc.FIXED if fixed else orc.DYNAMIC, evaluator=orc.EVAL_HASH,
                           c_puct=c, max_depth=max_depth, salt=salt + gi, priors_ones=bool(fixed))
        s = orc.Search(cfg)
        for i in range(gs[gi], gs[gi + 1]):
            st = orc.state_from_arrays(game, g["board"][i], g["player"][i], g["prev"][i] or None,
                                       g["castle"][i])
            r = s.find_move(st, temp, sims, u=float(g["u"][i]))
            if key == "dc":
                plays = dense(A, g["plays"][i], g["plays"][i][:, 1])
                wr = dense(A, g["plays"][i], g["winrates"][i])
                prob = dense(A, g["plays"][i], g["prob"][i])
            else:
                plays, wr, prob = g["plays"][i], g["winrates"][i], g["prob"][i]
            assert np.array_equal(r["plays"], plays), (fname, gi, i, r["plays"], plays)
            assert np.array_equal(r["winrates"], wr), (fname, gi, i)
            assert np.array_equal(r["prob"], prob)
            assert r["root_plays"] == g["root_plays"][i]
            assert r["winrate"] == g["v"][i]
            assert r["action"] == g["action"][i], (fname, gi, i)
            if reuse:
                s.move_root(r["next"])
            else:
                s.drop_root()


def test_sampling_law(orc):
    # np.random.choice(len(p), p=p) == searchsorted(cumsum(p)/cumsum(p)[-1], u, 'right')
    rng = np.random.RandomState(3)
    for _ in range(300):
        A = int(rng.choice([7, 9]))
        plays = rng.randint(0, 50, A).astype(np.float64)
        if plays.sum() == 0:
            continue
        temp = float(rng.choice([1.0, 0.1, 0.5, 2.0]))
        st = rng.get_state()
        u = rng.random_sample()
        rng.set_state(st)
        allp = sum([p ** (1 / temp) for p in plays])
        p = [c ** (1 / temp) / allp for c in plays]
        want = rng.choice(len(plays), p=p)
        assert orc.sample_action(plays, temp, u) == want


def test_edge_cases(orc):
    # playLimit=1 on a fresh root -> 0/0 -> ValueError; 2 sims -> [1,0,...]; reuse adds playLimit
    cfg = orc.make_cfg(0, salt=7)
    s = orc.Search(cfg)
    st = orc.new_state(0)
    with pytest.raises(ValueError):
        s.find_move(st, 1.0, 1, u=0.5)
    s = orc.Search(cfg)
    r = s.find_move(st, 1.0, 2, u=0.0)
    assert r["root_plays"] == 2 and r["plays"].sum() == 1 and r["winrate"] == 0.0
    r = s.find_move(st, 1.0, 3, u=0.0)
    assert r["root_plays"] == 5 and r["plays"].sum() == 4
    # root mismatch -> AssertionError
    other = st.copy()
    orc.apply(0, other, 0)
    with pytest.raises(AssertionError):
        s.find_move(other, 1.0, 2, u=0.0)
    # FixedMCTS(maxDepth=3), 1 sim: root + 3 levels x 7 children = 22 nodes
    cfg = orc.make_cfg(0, kind=orc.FIXED, max_depth=3, evaluator=orc.EVAL_ROLLOUT)
    s = orc.Search(cfg)
    s.find_move(st, 1.0, 1, u=0.5)
    assert s.stats().nodes == 22


# ---- the rollout evaluator (MCTS.SampleValue, MCTS.py:360-383): what tests/test_gpu_rollout.py relies on ------------------
from tests import rollout_cases as RC  # noqa: E402


@pytest.mark.parametrize("name", sorted(RC.SELFPLAY))
def test_rollout_selfplay_stays_clear_of_cap_and_stalemate(orc, name):
    """The configurations and seeds the GPU comparison uses: no rollout reaches the HIP engine's 2048-ply cap or a position
    without a legal move -- the two places where engine and oracle score 0.5 where the reference would go on or raise -- and
    every move of every game ran exactly sims-per-move rollouts."""
    _key, _fixed, _depth, sims, n_games, _slots, max_plies = RC.SELFPLAY[name]
    games = RC.oracle_selfplay(orc, name)
    assert len(games) == n_games
    for o in games:
        RC.assert_rollouts_decided(o["stats"])
        assert 2 <= o["n"] <= max_plies + 1
        assert o["stats"].sims == (o["n"] - 1) * sims
        assert o["stats"].max_rollout_steps > 0 and o["stats"].nodes_reached <= o["stats"].nodes


def test_rollout_stats_count_steps(orc):
    """max_rollout_steps is the number of moves the longest rollout played: from TicTacToe's empty board with one
    simulation (DynamicMCTS: the root is the leaf) a rollout plays 5 to 9 moves; Connect4 7 to 42."""
    for game, lo, hi in ((RC.ORC_GAME["ttt"], 5, 9), (RC.ORC_GAME["c4"], 7, 42)):
        seen = set()
        for gid in range(40):
            s = orc.Search(orc.make_cfg(game, evaluator=orc.EVAL_ROLLOUT, seed=RC.SEED), gid)
            with pytest.raises(ValueError):  # one simulation on a fresh root: 0 / 0
                s.find_move(orc.new_state(game), 1.0, 1, u=0.5)
            st = s.stats()
            assert st.sims == 1 and st.rollouts_without_moves == 0 and lo <= st.max_rollout_steps <= hi
            seen.add(st.max_rollout_steps)
        assert len(seen) > 1


@pytest.mark.parametrize("fixed", [False, True])
def test_rollout_without_a_legal_move_scores_half(orc, fixed):
    """DragonChess, both kings present, the side to move has no pseudo-legal move: the reference's np.random.choice would
    raise; the oracle (like the HIP engine) ends the rollout with 0.5 and treats the node as a leaf.  Every simulation
    terminates and backs up exactly 0.5."""
    stuck, forced, after = (RC.orc_state(orc, p) for p in (RC.STUCK_ROOK, RC.FORCED, RC.STUCK_AFTER_FORCED))
    for st in (stuck, after):
        assert orc.legal(orc.DC, st).sum() == 0 and orc.winner(orc.DC, st) is None
    assert np.flatnonzero(orc.legal(orc.DC, forced)).tolist() == [RC.FORCED_ACTION] and orc.winner(orc.DC, forced) is None
    nxt = forced.copy()
    assert orc.apply(orc.DC, nxt, RC.FORCED_ACTION) == 0
    assert bytes(nxt) == bytes(after)
    cfg = RC.oracle_cfg(orc, "dc", fixed, 3)
    # reached as the only child of the root
    s = orc.Search(cfg, 5)
    r = s.find_move(forced, 0, 4)
    assert r["action"] == RC.FORCED_ACTION and r["root_plays"] == 4
    assert r["plays"].sum() == r["plays"][RC.FORCED_ACTION] == (4 if fixed else 3)  # (DynamicMCTS: the first leaf is the root)
    assert r["winrates"][RC.FORCED_ACTION] == 0.5
    st = s.stats()
    assert (st.sims, st.rollouts_without_moves, st.max_rollout_steps) == (4, 4, 0 if fixed else 1)
    # ... and as the root itself: it keeps its statistics, gets no children, and there is no move to choose
    assert s.move_root(r["next"]) == 1
    with pytest.raises(ValueError):
        s.find_move(after, 0, 4)
    st = s.stats()
    assert (st.sims, st.rollouts_without_moves, st.sum_depth) == (8, 8, 4 if fixed else 3)
    s2 = orc.Search(cfg, 6)
    with pytest.raises(ValueError):
        s2.find_move(stuck, 0, 4)
    st = s2.stats()
    assert (st.sims, st.rollouts_without_moves, st.max_rollout_steps, st.sum_depth) == (4, 4, 0, 0)
