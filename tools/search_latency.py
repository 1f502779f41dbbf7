"""Latency of the search API, lock-step against the one-launch search (MCTS.SearchLaunch = 'wave'), on one box.

Two figures per structure, each from the calls a user makes:
  * `model.FindMove(state, temp)` on the game's start position -- Connect4 at 800 simulations, or with `--game dc` DragonChess
    at 400 (k_dc_search_wave; a 4-block network either way) --, a fresh tree every time;
  * one arena ply of 64 games: what `arena._Searcher.search` does for a side that is to move in all of them
    (`run_sims(sims, mask)` on an engine with one slot per game) plus the `sample_moves` that follows it.
Every measurement is a process of its own (a fresh child; nothing warmed up by the other structure), and the two structures
alternate -- heat-up run first, then lockstep, wave, lockstep, wave, ... -- in the manner of tools/ab.sh.  `--tree DIR` adds one
lock-step run per alternation from another checkout of the project with its library built (the parent commit's: lock-step
itself must not have moved).
Prints the runs and ONE JSON line with medians and spreads (milliseconds).

usage: python tools/search_latency.py [--game c4|dc] [--rounds 5] [--sims 800|400] [--games 64] [--reps 20] [--tree other/checkout]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    os.chdir(tempfile.mkdtemp())   # (a Model opens its sqlite sink in the working directory)
    import numpy as np
    from blackbird_amd import Blackbird, Connect4, DragonChess, _lib
    from blackbird_amd.MCTS import MCTS
    if not a.tree:   # (another checkout searches the way it always did)
        MCTS.SearchLaunch = a.child
    cfg = {"blocks": 4, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": {"optimizer": "adam"}}
    np.random.seed(0)
    cls, game_id, plies = (DragonChess.BoardState, _lib.GAME_DRAGONCHESS, 64) if a.game == "dc" else (Connect4.BoardState, _lib.GAME_CONNECT4, 43)
    model = Blackbird.Model(cls, "t", {"explorationRate": 0.85, "playLimit": a.sims}, cfg)
    start = cls()
    for _ in range(3):   # heat-up: code objects, clocks
        model.DropRoot()
        model.FindMove(start, 1.0)
    find = []
    for _ in range(a.reps):
        model.DropRoot()
        t = time.perf_counter()
        model.FindMove(start, 1.0)   # (ends in bb_sample_moves, which synchronises)
        find.append((time.perf_counter() - t) * 1e3)
    structure = None
    if hasattr(model._engine, "run_sims_structure"):
        structure = model._engine.run_sims_structure()
    # one arena ply: a searcher's engine with one slot per game, every game at its first move
    eng = model._make_engine(game_id, a.games, a.sims, node_capacity=a.sims * plies + 64)   # (arena._Searcher's sizing)
    model._after_engine_created(eng)
    states = np.repeat(_lib.game_initial(game_id), a.games, axis=0)
    mask = np.ones(a.games, dtype=np.uint8)
    ply = []
    for k in range(3 + max(a.reps // 2, 3)):
        eng.set_roots(states, game_ids=np.arange(a.games))
        t = time.perf_counter()
        eng.run_sims(a.sims, mask=mask)
        eng.sample_moves(1.0, np.full(a.games, 0.5))
        if k >= 3:
            ply.append((time.perf_counter() - t) * 1e3)
    assert eng.counters()["overflow"] == 0
    eng.close()
    print(json.dumps({"run": a.child, "game": a.game, "tree": a.tree or "-", "structure": structure, "findmove_ms": statistics.median(find),
                      "findmove_min_ms": min(find), "arena_ply_ms": statistics.median(ply), "arena_ply_min_ms": min(ply)}))


def run(a, which, tree=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--game", a.game, "--sims", str(a.sims), "--games", str(a.games),
           "--reps", str(a.reps)] + (["--tree", tree] if tree else [])
    out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout, check=True).stdout.decode()
    r = json.loads(out.strip().splitlines()[-1])
    print(json.dumps(r), flush=True)
    return r


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--game", choices=["c4", "dc"], default="c4")
    p.add_argument("--sims", type=int, default=None, help="simulations per move (default: 800 for c4, 400 for dc)")
    p.add_argument("--games", type=int, default=64)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--tree", default=None)
    p.add_argument("--timeout", type=int, default=240, help="seconds one measurement process may take")
    p.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.sims is None:
        a.sims = 400 if a.game == "dc" else 800
    if a.child:
        return child(a)
    run(a, "lockstep")   # heat-up, not counted
    runs = {"lockstep": [], "wave": [], "other_lockstep": []}
    for _ in range(a.rounds):
        runs["lockstep"].append(run(a, "lockstep"))
        runs["wave"].append(run(a, "wave"))
        if a.tree:
            runs["other_lockstep"].append(run(a, "lockstep", a.tree))
    res = {"game": a.game, "sims": a.sims, "games": a.games, "rounds": a.rounds}
    for name, rs in runs.items():
        for key in ("findmove_ms", "arena_ply_ms"):
            v = [r[key] for r in rs]
            if v:
                res[f"{name}_{key}"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
