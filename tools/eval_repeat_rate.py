"""How many network evaluations of self-play repeat a position evaluated before (CPU only, the oracle).

Plays n games at the bench's settings (random weights seed 0, prior noise alpha 0.2 / eps 0.3 per (game, node serial))
through the oracle's keyed evaluator callback and counts, among the FIRST evaluation of every node, those whose position
(network input) was already evaluated: in the same game, and in the same game or any earlier one.  This is the hit rate an
unbounded evaluation cache would reach with that many games sharing it (the persistent kernels' tables are bounded and are
shared by 4096 concurrent Connect4 games / 1024 DragonChess games).

  --game c4 (default): Connect4, R4/F16 on 3 planes, 800 simulations, full games.
  --game dc: DragonChess (bench.py --workload dc), R4/F16 on 17 planes, 4032-wide policy, 400 simulations; the CPU oracle
             plays ~30 plies a minute there, so --plies caps every game (default 40).  The noise is drawn for the legal
             moves only (the priors are renormalised over them anyway; only their rounding differs from the oracle's own).

  --search: the search API instead (bb_config.search_cache: the evaluation cache of the one-launch search).  The share of ALL
             leaf evaluations (a node evaluated again counts again: the search probes every leaf it posts) whose position was
             evaluated before, in two cases: ONE GAME played through by FindMove with tree reuse, table empty at the first
             move (game 0 alone), and an ARENA of `games` games (default 64) from the start position on one table.  The
             oracle plays each game move by move with tree reuse, which is FindMove + MoveRoot; its arena stand-in is one
             network playing both sides, where a real arena has two engines that each search every other ply with a table
             of their own -- a real side sees fewer of a game's positions, so its share is at most the one reported.

usage: python tools/eval_repeat_rate.py [games] [sims] [--game c4|dc] [--plies N] [--search]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blackbird_amd import weights as W  # noqa: E402
from oracle import orc  # noqa: E402

ALPHA, EPS, SEED = 0.2, 0.3, 1234
GAMES = {  # game, H, W, planes, actions, simulations, ply cap
    "c4": (orc.C4, 6, 7, 3, 7, 800, 42),
    "dc": (orc.DC, 8, 8, 17, 4032, 400, 40),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("games", type=int, nargs="?", default=20)
    ap.add_argument("sims", type=int, nargs="?", default=None)
    ap.add_argument("--game", choices=sorted(GAMES), default="c4")
    ap.add_argument("--plies", type=int, default=None, help="ply cap of every game")
    ap.add_argument("--search", action="store_true", help="the search API: one FindMove game, and an arena of `games` games")
    args = ap.parse_args()
    if args.search and len([x for x in sys.argv[1:] if not x.startswith("-") and x.isdigit()]) == 0:
        args.games = 64
    game, H, Wd, Cc, A, sims, plies = GAMES[args.game]
    sims = args.sims or sims
    plies = args.plies or plies
    orc.build()
    L = orc.lib()
    L.orc_beta_noise.restype = C.c_float
    L.orc_beta_noise.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float]
    flat = W.flatten(W.init_weights(Cc, 16, 4, 16, A, seed=0))
    net = orc.NetWeights(H, Wd, Cc, 16, 4, 16, A, flat)
    seen_all, seen_game, first = set(), set(), set()
    rows = []  # per game: first visits, repeats in the game, repeats in this or an earlier game, all evaluations, their repeats

    def evaluate(_ctx, stp, gid, serial, vp, pp):
        planes = orc.encode(game, stp.contents)
        v, _l, p = orc.net_forward(net, planes)
        vp[0] = float(v[0])
        if pp:
            acts = np.nonzero(orc.legal(game, stp.contents))[0] if game == orc.DC else range(A)
            q = np.zeros(A, dtype=np.float64)
            for a in acts:
                q[a] = (1.0 - EPS) * float(p[0, a]) + EPS * L.orc_beta_noise(SEED, gid, serial, int(a), ALPHA)
            q /= max(q.sum(), 1e-30)
            for a in acts:
                pp[a] = q[a]
        key = planes.tobytes()
        r = rows[-1]
        r[3] += 1
        r[4] += key in seen_all
        if (gid, serial) not in first:
            first.add((gid, serial))
            r[0] += 1
            r[1] += key in seen_game
            r[2] += key in seen_all
        seen_game.add(key)
        seen_all.add(key)

    cfg = orc.make_cfg(game, evaluator=orc.EVAL_CALLBACK_KEYED, seed=SEED, noise_on=True, alpha=ALPHA, eps=EPS,
                       cb2=orc.EVAL_CB2(evaluate))
    sims_total = 0
    print("%s: %d simulations per move, games capped at %d plies" % (args.game, sims, plies), flush=True)
    for g in range(args.games):
        rows.append([0, 0, 0, 0, 0])
        seen_game.clear()
        o = orc.selfplay_game(cfg, g, 1.0, sims, plies)
        sims_total += o["stats"].sims
        n, same, shared, _ne, _nr = rows[-1]
        print("game %3d: %3d plies, %5d first visits, repeats: same game %.3f, with the %d earlier games %.3f"
              % (g, o["n"] - 1, n, same / max(n, 1), g, shared / max(n, 1)), flush=True)
    a = np.array(rows, dtype=np.float64)
    if args.search:
        print("search API, %s at %d simulations: one FindMove game (%d evaluations) repeat share %.3f; arena of %d games on one "
              "table (%d evaluations) repeat share %.3f"
              % (args.game, sims, a[0, 3], a[0, 4] / max(a[0, 3], 1), args.games, a[:, 3].sum(), a[:, 4].sum() / a[:, 3].sum()))
        return
    print("all %d games: first visits / simulations %.3f, repeats: same game %.3f, shared table %.3f; "
          "every evaluation (first visits or not): %d, repeats %.3f"
          % (args.games, a[:, 0].sum() / max(sims_total, 1), a[:, 1].sum() / a[:, 0].sum(), a[:, 2].sum() / a[:, 0].sum(),
             a[:, 3].sum(), a[:, 4].sum() / a[:, 3].sum()))


if __name__ == "__main__":
    main()
