"""What tests/test_sample_temp_cpu.py (no GPU) and the -m gpu tests of move choice at temperatures other than 1 share: the
reference's sampling law written in numpy, the temperatures, visit vectors and draws of the sweep, the oracle games the GPU
self-play is compared with, and `draw_margins`, which says how far a game's move draws stay from the boundaries of their cdfs.

The law (MCTS.py:335-338 + np.random.choice(p=...)):
    allPlays = sum(p ** (1 / temp));  p = c ** (1 / temp) / allPlays;  cdf = cumsum(p);  cdf /= cdf[-1];  searchsorted(cdf, u, 'right')

MARGIN = 2^-40, derived and not measured: pow on the host and in the device library are each good to about an ulp (2^-52), and a
cdf over at most 144 terms then moves by less than 2^-44 relative.  A draw that keeps a relative distance of 2^-40 from every
boundary of its cdf lands in the same interval whichever pow computed it, so the GPU tests may demand exact agreement."""
import numpy as np

from tests import selfplay_cases as SC

# 1 / 0.1 is exactly 10.0 and 1 / 0.5, 1 / 2.0, 1 / 50.0 are exact too; 0.3 and 0.7 give NON-INTEGER exponents (3.33.., 1.42..):
# pow has no integer shortcut there.  That is why they are in the list.
TEMPS = (0.1, 0.3, 0.5, 0.7, 2.0, 50.0)
MARGIN = 2.0 ** -40
MIN_SHARE = 2.0 ** -30
OVERFLOW_TEMP = 0.002   # 7 ** 500 overflows, 4 ** 500 does not


def probabilities(plays, temp):
    """The reference's p, term by term in numpy float64 scalars (an overflow gives inf / nan, as there)."""
    plays = np.asarray(plays, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        all_plays = sum([p ** (1 / temp) for p in plays])
        return np.array([c ** (1 / temp) / all_plays for c in plays], dtype=np.float64)


def choice(p, u):
    """np.random.choice(len(p), p=p) for the uniform draw u."""
    cdf = np.cumsum(p)
    cdf /= cdf[-1]
    return int(np.searchsorted(cdf, u, side="right"))


def draws(plays, temp):
    """The sweep's draws for one visit vector: [(kind, child, u)].  Per child whose share is >= 2^-30 and whose neighbours in
    the cdf -- the nearest children with a non-zero share on either side; a child without visits has no interval -- also have
    shares >= 2^-30: the middle of its interval, and its upper boundary times (1 -+ 2^-40).  u stays inside [0, 1)."""
    p = probabilities(plays, temp)
    cum = np.cumsum(p)
    nz = np.flatnonzero(p > 0)
    out = []
    for i, k in enumerate(nz):
        near = [p[k]] + ([p[nz[i - 1]]] if i > 0 else []) + ([p[nz[i + 1]]] if i + 1 < len(nz) else [])
        if min(near) < MIN_SHARE:
            continue
        for kind, u in (("mid", cum[k] - 0.5 * p[k]), ("below", cum[k] * (1 - MARGIN)), ("above", cum[k] * (1 + MARGIN))):
            if 0.0 <= u < 1.0:
                out.append((kind, int(k), float(u)))
    return out


def margin(plays, temp, u):
    """Smallest relative distance between the draw u and an inner boundary of the cdf of `plays` at `temp` (inf: no boundary).
    Children in front of the first visited one have the boundary 0, which no draw is below; the last boundary is 1, which every
    draw is below: neither can change the answer."""
    p = probabilities(plays, temp)
    cdf = np.cumsum(p)
    cdf /= cdf[-1]
    inner = cdf[:-1][cdf[:-1] > 0]
    return float(np.min(np.abs(u - inner) / inner)) if len(inner) else float("inf")


def draw_margins(o, temp):
    """For an oracle game (SC.oracle_selfplay_from: per move `plays` and the keyed draw `u`): the smallest margin of any move."""
    if temp == 0:
        return float("inf")   # PUCT argmax: no draw is consumed
    return min([margin(c, temp, u) for c, u in zip(o["plays"], o["u"])], default=float("inf"))


# ---- the sweep's visit vectors --------------------------------------------------------------------------------------------------
def visit_vectors(A):
    rng = np.random.RandomState(1000 + A)
    last = [0] * (A - 1)
    out = [[0, 12, 0, 7, 3, 0, 25] + [0, 4][:A - 7],           # zeros among the legal children
           [0, 0, 47] + [0] * (A - 3),                          # a single non-zero child
           last + [48], last + [800],                           # all visits on the last child
           [800, 790, 3, 0, 1, 799, 650] + [777, 2][:A - 7],    # N ** 10 > 2 ** 53: the terms are no longer exact integers
           [1] * A, [6, 7, 7, 7, 7, 7, 6] + [7, 7][:A - 7]]     # 47 or 48 visits, nearly even
    for hi in (8, 50, 800):
        for _ in range(12):
            v = rng.randint(0, hi + 1, A)
            v[rng.random_sample(A) < 0.25] = 0
            if v.sum() > 0:
                out.append(v.tolist())
    return [np.array(v, dtype=np.float64) for v in out]


# ---- bb_sample_moves on the dense games (tests/test_gpu_sample_temp.py) -------------------------------------------------------
SAMPLE = dict(n_slots=5, sims=48, salt=606, seed=23)   # slot i: game id i, salt + i, root kind i % 3
SAMPLE_MIN_DRAWS = 200                                 # draws over the five roots and six temperatures, at the least
# root kinds as action lists from the initial position: the initial position, a root with a full column (TicTacToe: taken
# cells), and a root with one legal move (c4_one_move_board / TTT_ONE_MOVE)
ROOT_ACTIONS = {0: ([], [3, 3, 3, 3, 3, 3]), 1: ([], [4, 0, 8])}
TTT_ONE_MOVE = [0, 1, 2, 4, 3, 5, 7, 6]                # X O X / X O O / O X . : cell 8 is left, nobody has a line


def c4_one_move_board():
    """Connect4 without any run of four -- cell (r, c) holds player 1 + (r // 2 + c) % 2 -- and the top cell of column 0 empty."""
    board = np.zeros((6, 7, 2), dtype=np.int8)
    for r in range(6):
        for c in range(7):
            if not (r == 5 and c == 0):
                board[r, c, (r // 2 + c) % 2] = 1
    return board


def sample_roots(orc, og):
    """The oracle states of the three root kinds of game og (0 Connect4, 1 TicTacToe)."""
    out = []
    for acts in ROOT_ACTIONS[og]:
        st = orc.new_state(og)
        for a in acts:
            assert orc.apply(og, st, a) == 0
        out.append(st)
    if og == 0:
        one = orc.state_from_arrays(og, c4_one_move_board(), 1, 2)
    else:
        one = orc.new_state(og)
        for a in TTT_ONE_MOVE:
            assert orc.apply(og, one, a) == 0
    assert orc.legal(og, one).sum() == 1 and orc.winner(og, one) is None
    return out + [one]


def root_arrays(orc, og, st):
    """(board [H, W, 2], player, previous player) of an oracle state of a dense game: what _lib.pack_grid takes."""
    H, W, _c, _a = orc.dims(og)
    return np.array(st.b[:H * W * 2], dtype=np.int8).reshape(H, W, 2), int(st.player), int(st.prev)


_searched = {}


def sample_oracle(orc, og):
    """Per slot of SAMPLE: the oracle's search of its root (find_move's dict at temp 1, u = 0.5) -- searched once, not to be
    changed -- and its state."""
    if og not in _searched:
        roots = sample_roots(orc, og)
        rows = []
        for i in range(SAMPLE["n_slots"]):
            cfg = orc.make_cfg(og, evaluator=orc.EVAL_HASH, salt=SAMPLE["salt"] + i, seed=SAMPLE["seed"])
            st = roots[i % 3]
            rows.append((st, orc.Search(cfg, i).find_move(st, 1.0, SAMPLE["sims"], u=0.5)))
        _searched[og] = rows
    return _searched[og]


# ---- self-play against the oracle (lock-step, hash evaluator) ------------------------------------------------------------------
SELFPLAY_TEMPS = (0.1, 0.5, 0.0)
LOCKSTEP = dict(n_games=7, n_slots=3, sims=24, salt=4242, seed=99, first_id=1000)
DC_MAX_PLIES = 6


def lockstep_max_plies(og):
    return {0: 42, 1: 9, 2: DC_MAX_PLIES}[og]


def lockstep_cfg(orc, og, k, seed=None):
    return orc.make_cfg(og, evaluator=orc.EVAL_HASH, salt=LOCKSTEP["salt"] + k, seed=LOCKSTEP["seed"] if seed is None else seed)


_games = {}


def lockstep_games(orc, og, temp):
    """The oracle's games first_id .. first_id + 6 of the lock-step case at `temp`, played once; not to be changed."""
    if (og, temp) not in _games:
        _games[og, temp] = [SC.oracle_selfplay_from(orc, lockstep_cfg(orc, og, k), LOCKSTEP["first_id"] + k, orc.new_state(og), temp,
                                                    LOCKSTEP["sims"], lockstep_max_plies(og)) for k in range(LOCKSTEP["n_games"])]
    return _games[og, temp]
