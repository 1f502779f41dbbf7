"""What tests/test_gpu_dc_wide_nodes.py (-m gpu) needs about the wide DragonChess positions of tests/golden/boards_dc_wide.npz:
the positions as engine and oracle states, the oracle's searches of them (run once per session and shared), and the draws u that
make np.random.choice's cumulative sum stop at an edge past index 64."""
import functools
import os

import numpy as np

S = 144            # DragonChess::S, edges per tree node
C_PUCT = 0.85
SEED = 31
FIRST_GAME_ID = 1000
SALT = 7700
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, "boards_dc_wide.npz"), allow_pickle=False)


class Positions:
    """The fixture's positions (pre = "over_": the two with more than S legal moves)."""

    def __init__(self, pre=""):
        g = fixture()
        self.names = g[pre + "name"].tolist()
        self.board, self.player, self.prev, self.castle = (g[pre + k] for k in ("board", "player", "prev", "castle"))
        off = g[pre + "legal_off"]
        self.legal = [g[pre + "legal_idx"][off[i]:off[i + 1]].astype(np.int32) for i in range(len(self.names))]
        self.n_legal = np.diff(off)
        self.lids = 7 + 3 * np.arange(len(self.names))   # game ids: distinct, not the slot numbers

    def __len__(self):
        return len(self.names)

    def packed(self, _lib, which=None):
        w = slice(None) if which is None else which
        return _lib.pack_dc(self.board[w].reshape(-1, 8, 8), self.player[w], self.prev[w], self.castle[w])

    def orc_state(self, orc, i):
        return orc.state_from_arrays(orc.DC, self.board[i], self.player[i], self.prev[i] or None, self.castle[i])


def sims_for(n_legal, kind):
    """Simulations per position: Fixed with uniform priors visits every edge once in n_legal simulations (+ 10 more); the
    dynamic searches get twice the edges of the widest node, so edges of every pass of 64 are visited."""
    return int(n_legal) + 10 if kind == "fixed" else 2 * S + 2


_runs = {}


def oracle_run(orc, key, cfg, sims, positions=None, which=None):
    """orc.Search(cfg).find_move(temp 0) of every position (or of `which`), once per `key`: a list of dicts with the oracle's
    result `o`, its `stats` and the Search itself (for move_root); the caller must not change them."""
    if key not in _runs:
        P = positions or Positions()
        out = []
        for i in (range(len(P)) if which is None else which):
            sr = orc.Search(cfg, FIRST_GAME_ID + int(P.lids[i]))
            st = P.orc_state(orc, i)
            o = sr.find_move(st, 0, sims[i] if hasattr(sims, "__len__") else sims)
            out.append(dict(o=o, stats=sr.stats(), search=sr, state=st, cfg=cfg))
        _runs[key] = out
    return _runs[key]


def u_for_edges_past(plays, temp, first=64):
    """Two draws u at which np.random.choice's cumulative sum over plays ** (1 / temp) stops at an edge with index >= first --
    the first and the last such edge that holds a share of at least 1e-9 -- as [(u, edge), ...]; fewer when there are none."""
    w = np.asarray(plays, dtype=np.float64)
    w = w if temp == 1.0 else w ** (1.0 / temp)
    p = w / w.sum()
    cum = np.cumsum(p)
    ks = [k for k in range(first, len(p)) if p[k] >= 1e-9]
    return [(float(cum[k] - 0.5 * p[k]), k) for k in sorted({ks[0], ks[-1]})] if ks else []
