"""What tests/test_oracle_mcts.py (no GPU) and tests/test_gpu_rollout.py (-m gpu) share about the rollout evaluator
(MCTS.SampleValue, MCTS.py:360-383): the self-play configurations, the oracle's games for them (played once per session),
and the DragonChess positions in which the side to move has its king and no legal move."""
import numpy as np

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
