"""What tests/test_oracle_mcts.py (no GPU) and tests/test_gpu_rollout.py (-m gpu) share about the rollout evaluator
(MCTS.SampleValue, MCTS.py:360-383): the self-play configurations, the oracle's games for them (played once per session),
the DragonChess positions in which the side to move has its king and no legal move, and the stepwise FindMove comparison of
the -m gpu tests (this module imports blackbird_amd._lib for it; the no-GPU test makes no call into the library through it)."""
import os

import numpy as np

from blackbird_amd import _lib
from tests.selfplay_cases import pi_of

SEED = 31
FIRST_GAME_ID = 1000
C_PUCT = 0.85  # TestGood's FixedMCTS(maxDepth=10, explorationRate=0.85, ...), Blackbird.py:164
ROLLOUT_CAP = 2048  # the HIP DragonChess rollout stops there and scores 0.5; no compared value may come from that

# name: (game key, Fixed?, max depth, sims per move, games, slots, max plies)
SELFPLAY = {
    "c4_fixed10": ("c4", True, 10, 50, 24, 7, 42),
    "c4_fixed3": ("c4", True, 3, 60, 12, 5, 42),   # leaves are mid-game nodes that already have children
    "c4_dynamic": ("c4", False, 10, 60, 12, 5, 42),
    "ttt_dynamic": ("ttt", False, 10, 30, 40, 16, 9),
    "dc_fixed3": ("dc", True, 3, 16, 6, 5, 12),
    "dc_dynamic": ("dc", False, 10, 16, 6, 5, 12),
}
ORC_GAME = {"c4": 0, "ttt": 1, "dc": 2}
GAMES = {"c4": _lib.GAME_CONNECT4, "ttt": _lib.GAME_TICTACTOE, "dc": _lib.GAME_DRAGONCHESS}


def oracle_cfg(orc, key, fixed, max_depth):
    return orc.make_cfg(ORC_GAME[key], kind=orc.FIXED if fixed else orc.DYNAMIC, max_depth=max_depth,
                        evaluator=orc.EVAL_ROLLOUT, c_puct=C_PUCT, seed=SEED)


_games = {}


def oracle_selfplay(orc, name):
    """The oracle's games FIRST_GAME_ID .. of one SELFPLAY case; the caller must not change them."""
    if name not in _games:
        key, fixed, max_depth, sims, n_games, _slots, max_plies = SELFPLAY[name]
        cfg = oracle_cfg(orc, key, fixed, max_depth)
        _games[name] = [orc.selfplay_game(cfg, FIRST_GAME_ID + g, 1.0, sims, max_plies) for g in range(n_games)]
    return _games[name]


def assert_rollouts_decided(stats, allow_without_moves=False):
    """No rollout behind a compared value ran into the engine's ply cap or ended for want of a legal move."""
    assert stats.max_rollout_steps < ROLLOUT_CAP, stats.max_rollout_steps
    if not allow_without_moves:
        assert stats.rollouts_without_moves == 0, stats.rollouts_without_moves


# ---- DragonChess: both kings on the board, the side to move without a pseudo-legal move ----------------------------------
# A White pawn on row 6 never moves (its promotion branches return a falsy 0, DragonChess.py:282-319), nor does a pawn on
# row 7, and a king moves to no square that holds a piece of its own colour.
K, P, R = 1, 2, 5


def _board(pieces):
    b = np.zeros((8, 8), dtype=np.int8)
    for (r, c), v in pieces.items():
        b[r, c] = v
    return b


_WHITE_BOXED = {(7, 0): K, (7, 1): P, (6, 0): P, (6, 1): P}
_BLACK_BOXED = {(0, 7): -K, (0, 6): -P, (1, 6): -P, (1, 7): -P}
# White to move after Black's move: the row-6 pawn with a rook diagonally ahead of it
STUCK_ROOK = dict(board=_board({**_WHITE_BOXED, (7, 2): -R, (0, 7): -K}), player=1, prev=2)
# Black to move, one legal move (the pawn 3,3 -> 2,3); after it White is to move and has none
FORCED = dict(board=_board({**_WHITE_BOXED, **_BLACK_BOXED, (3, 3): -P}), player=2, prev=1)
FORCED_ACTION = (3 * 8 + 3) * 63 + (2 * 8 + 3)  # sq1 * 63 + sq2 - (sq2 > sq1), DragonChess.py:26-34
STUCK_AFTER_FORCED = dict(board=_board({**_WHITE_BOXED, **_BLACK_BOXED, (2, 3): -P}), player=1, prev=2)


def orc_state(orc, pos):
    return orc.state_from_arrays(orc.DC, pos["board"], pos["player"], pos["prev"], (0, 0, 0, 0))


# ---- FindMove in its steps, from mid-game positions, with tree reuse (tests/test_gpu_rollout.py's docstring says what) -------
def _positions(golden_dir, key, every):
    g = np.load(os.path.join(golden_dir, f"playouts_{key}.npz"), allow_pickle=False)
    idx = np.flatnonzero(g["win_none"] < 0)[::every]
    return g, idx


def _dense(out, s, gi):
    """Slot s of bb_sample_moves as (plays [A], child values [A])."""
    plays, value = np.zeros(gi.A), np.zeros(gi.A)
    if gi.dense:
        plays[:] = out["child_plays"][s, :gi.A]
        value[:] = out["child_value"][s, :gi.A]
    else:
        k = int((out["child_action"][s] >= 0).sum())
        assert (out["child_action"][s, k:] == -1).all() and (np.diff(out["child_action"][s, :k]) > 0).all()
        plays[out["child_action"][s, :k]] = out["child_plays"][s, :k]
        value[out["child_action"][s, :k]] = out["child_value"][s, :k]
    return plays, value


def find_move_steps_vs_oracle(orc, golden_dir, key, fixed, max_depth, every, masked):
    game, og = GAMES[key], ORC_GAME[key]
    gi = _lib.game_info(game)
    g, idx = _positions(golden_dir, key, every)
    n = len(idx)
    assert (60 <= n <= 70) if key == "c4" else (44 <= n <= 52)
    turns = set(zip(g["player"][idx].tolist(), g["prev"][idx].tolist()))
    assert {p for p, _ in turns} == {1, 2} and (key != "dc" or {(1, 1), (1, 2), (2, 1)} <= turns)
    if key == "dc":
        packed = _lib.pack_dc(g["board"][idx].reshape(-1, 8, 8), g["player"][idx], g["prev"][idx], g["castle"][idx])
    else:
        H, W, _s = _lib.GRID[game]
        packed = _lib.pack_grid(game, g["board"][idx].reshape(-1, H, W, 2), g["player"][idx], g["prev"][idx])
    lids = 7 + 3 * np.arange(n)  # distinct, not the slot numbers
    eng = _lib.Engine(game, n_slots=n, sims_per_move=9, mcts_kind=_lib.MCTS_FIXED if fixed else _lib.MCTS_DYNAMIC,
                      max_depth=max_depth, evaluator=_lib.EVAL_ROLLOUT, c_puct=C_PUCT, seed=SEED,
                      first_game_id=FIRST_GAME_ID, max_plies=42 if key == "c4" else 64)
    eng.set_roots(packed, game_ids=lids)
    cfg = oracle_cfg(orc, key, fixed, max_depth)
    search = [orc.Search(cfg, FIRST_GAME_ID + int(lids[s])) for s in range(n)]
    state = [orc.state_from_arrays(og, g["board"][i], g["player"][i], g["prev"][i] or None, g["castle"][i]) for i in idx]
    alive = np.ones(n, dtype=bool)  # (a game that ends drops out)
    for rnd, sims in enumerate((2, 5, 9)):
        run = alive & ((np.arange(n) % 3 != 2) if (masked and rnd == 1) else True)
        if masked and rnd == 1:
            before = eng.sample_moves(0)
            eng.run_sims(sims, mask=run.astype(np.uint8))
        else:
            eng.run_sims(sims, mask=None if alive.all() else run.astype(np.uint8))
        out = eng.sample_moves(0)
        acts = np.full(n, -1, dtype=np.int32)
        for s in range(n):
            if not run[s]:
                if alive[s]:  # left out of this round: nothing of the slot has changed
                    for f in ("root_plays", "root_winrate", "child_action", "child_plays", "child_value", "action"):
                        assert np.array_equal(out[f][s], before[f][s]), (f, s)
                continue
            o = search[s].find_move(state[s], 0, sims)
            where = (key, fixed, rnd, s)
            plays, value = _dense(out, s, gi)
            assert out["root_plays"][s] == o["root_plays"], where
            assert out["root_winrate"][s] == np.float32(o["winrate"]), where
            assert np.array_equal(plays, o["plays"]), where
            assert out["action"][s] == o["action"], where
            assert np.array_equal(np.where(plays > 0, value / np.maximum(plays, 1), 0.0), o["winrates"]), where
            acts[s] = o["action"]
            state[s] = o["next"]
            search[s].move_root(state[s])
            if orc.winner(og, state[s]) is not None:
                alive[s] = False
        eng.move_roots(acts)
    cnt = eng.counters()
    eng.close()
    stats = [sr.stats() for sr in search]
    for st in stats:
        assert_rollouts_decided(st)
    assert cnt["overflow"] == 0
    assert cnt["sims"] == sum(st.sims for st in stats) and cnt["sum_depth"] == sum(st.sum_depth for st in stats)
    assert cnt["nodes"] == sum(st.nodes_reached for st in stats)
    assert cnt["terminal_leaves"] == sum(st.terminal_leaves for st in stats)


def assert_selfplay_is_the_oracles(orc, name, rec, offs, win, cnt):
    """The engine's games of one SELFPLAY case against the oracle's serial games, example by example, and the counters."""
    key = SELFPLAY[name][0]
    game = GAMES[key]
    tot = dict(sims=0, sum_depth=0, nodes=0, terminal_leaves=0)
    for gidx, o in enumerate(oracle_selfplay(orc, name)):
        assert_rollouts_decided(o["stats"])
        r = rec[offs[gidx]:offs[gidx + 1]]
        assert len(r) == o["n"] and win[gidx] == o["winner"], (gidx, len(r), o["n"], win[gidx], o["winner"])
        assert (r["game_id"] == FIRST_GAME_ID + gidx).all() and np.array_equal(r["ply"], np.arange(len(r)))
        assert np.array_equal(pi_of(game, r), o["pi"]), gidx
        assert np.array_equal(r["player"], o["player"]) and np.array_equal(r["z"].astype(np.float32), o["z"]), gidx
        st = np.ascontiguousarray(r["state"])
        if key != "dc":
            st = st.view(np.uint64).reshape(-1, 2)
        assert np.array_equal(_lib.game_encode(game, st), o["boards"]), gidx
        tot["sims"] += o["stats"].sims
        tot["sum_depth"] += o["stats"].sum_depth
        tot["nodes"] += o["stats"].nodes_reached  # (the engine builds a child when a descent first selects it)
        tot["terminal_leaves"] += o["stats"].terminal_leaves
    assert {k: cnt[k] for k in tot} == tot
