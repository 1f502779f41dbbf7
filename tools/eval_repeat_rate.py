"""How many network evaluations of Connect4 self-play repeat a position evaluated before (CPU only, the oracle).

Plays n full games at the bench's settings (weights seed 0, 800 simulations, prior noise alpha 0.2 / eps 0.3 per (game, node
serial)) through the oracle's keyed evaluator callback and counts, among the FIRST evaluation of every node, those whose
position (network input) was already evaluated: in the same game, and in the same game or any earlier one.  This is the
hit rate an unbounded evaluation cache would reach with that many games sharing it (the persistent kernel's table is bounded
and is shared by 4096 concurrent games).

usage: python tools/eval_repeat_rate.py [games] [sims]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blackbird_amd import weights as W  # noqa: E402
from oracle import orc  # noqa: E402

ALPHA, EPS, SEED = 0.2, 0.3, 1234


def main():
    n_games = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    sims = int(sys.argv[2]) if len(sys.argv) > 2 else 800
    orc.build()
    L = orc.lib()
    L.orc_beta_noise.restype = C.c_float
    L.orc_beta_noise.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float]
    flat = W.flatten(W.init_weights(3, 16, 4, 16, 7, seed=0))
    net = orc.NetWeights(6, 7, 3, 16, 4, 16, 7, flat)
    seen_all, seen_game, first = set(), set(), set()
    rows = []  # per game: first visits, repeats in the game, repeats in this or an earlier game

    def evaluate(_ctx, stp, gid, serial, vp, pp):
        planes = orc.encode(orc.C4, stp.contents)
        v, _l, p = orc.net_forward(net, planes)
        vp[0] = float(v[0])
        if pp:
            q = [(1.0 - EPS) * float(p[0, a]) + EPS * L.orc_beta_noise(SEED, gid, serial, a, ALPHA) for a in range(7)]
            t = sum(q)
            for a in range(7):
                pp[a] = q[a] / t
        if (gid, serial) in first:
            return
        first.add((gid, serial))
        key = planes.tobytes()
        r = rows[-1]
        r[0] += 1
        r[1] += key in seen_game
        r[2] += key in seen_all
        seen_game.add(key)
        seen_all.add(key)

    cfg = orc.make_cfg(orc.C4, evaluator=orc.EVAL_CALLBACK_KEYED, seed=SEED, noise_on=True, alpha=ALPHA, eps=EPS,
                       cb2=orc.EVAL_CB2(evaluate))
    sims_total = 0
    for g in range(n_games):
        rows.append([0, 0, 0])
        seen_game.clear()
        o = orc.selfplay_game(cfg, g, 1.0, sims, 42)
        sims_total += o["stats"].sims
        n, same, shared = rows[-1]
        print("game %3d: %5d first visits, repeats: same game %.3f, with the %d earlier games %.3f"
              % (g, n, same / max(n, 1), g, shared / max(n, 1)), flush=True)
    a = np.array(rows, dtype=np.float64)
    print("all %d games: first visits / simulations %.3f, repeats: same game %.3f, shared table %.3f"
          % (n_games, a[:, 0].sum() / max(sims_total, 1), a[:, 1].sum() / a[:, 0].sum(), a[:, 2].sum() / a[:, 0].sum()))


if __name__ == "__main__":
    main()
