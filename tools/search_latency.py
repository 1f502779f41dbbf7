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

`--cache` measures the evaluation cache of the one-launch search instead (MCTS.SearchEvalCache): the wave with the cache against
the wave without it in the same build, and with `--tree` against the other checkout's wave (the parent commit's: the uncached
path must not have moved), alternating, a fresh process per run.  Repeating one search on a warm table would hit every time and
measure nothing, so a run times what fills its own table: a WHOLE GAME played through (FindMove + MoveRoot from the start
position to the end, table cold at the first move) and a WHOLE ARENA of `--games` games (arena.TestModelsBatched between two
networks; DragonChess, whose games outlast the arena's node pools at 400 simulations: the same loop for `--plies` plies), and
reports the share of leaf evaluations the cache answered (eval_cache_hits / eval_cache_probes of the engines).

`--evaluator rollout` measures the searchers of the rollout evaluator instead (MCTS.SearchRollouts): `FixedMCTS(maxDepth=--depth)`
or, with `--kind dynamic`, a plain DynamicMCTS, on the same two figures at the same simulation counts -- lock-step against wave in
this build, against the other checkout's lock-step with `--tree`, and for a dense game against `wave_plain`: the wave kernel whose
lane 0 alone plays the leaf out (BB_SW_ROLLOUT_PLAIN=1) instead of the lane-parallel draws.

`--arena-loop host|device` measures the WHOLE ARENA of `--games` games between two networks through the two loops of
blackbird_amd/arena.py: `host` (moves read back every ply) and `device` (the match loop enqueued on the GPU, bb_arena_*), with the
engines searching through `--launch lockstep|wave`.  `device` alternates the device loop with the host loop of this build, `host`
runs the host loop alone; `--tree` adds the other checkout's host loop (the parent commit's: untouched code must not have moved).
The games are played at `--temp 0` by default: no move is drawn, so every loop plays the very same games and the times compare
like for like (the loops draw their moves from different streams otherwise, and an arena is as long as its longest game).
DragonChess plays `--plies` plies (default 40) of every game, as in `--cache`.

usage: python tools/search_latency.py [--game c4|dc] [--rounds 5] [--sims 800|400] [--games 64] [--reps 20] [--tree other/checkout]
       python tools/search_latency.py --cache [--game c4|dc] [--rounds 5] [--sims ..] [--games 64] [--plies 40] [--tree other/checkout]
       python tools/search_latency.py --evaluator rollout [--game c4|dc] [--kind fixed|dynamic] [--depth 10] [--rounds 5] [--reps 20] [--tree ..]
       python tools/search_latency.py --arena-loop host|device [--launch lockstep|wave] [--game c4|dc] [--rounds 5] [--sims ..] [--games 64] [--temp 0] [--tree ..]
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


def child_rollout(a):
    """One run of the --evaluator rollout leg; a.child is 'lockstep', 'wave' or 'wave_plain' (the environment makes the difference)."""
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import numpy as np
    from blackbird_amd import Connect4, DragonChess, _lib
    from blackbird_amd.DynamicMCTS import DynamicMCTS
    from blackbird_amd.FixedMCTS import FixedMCTS
    from blackbird_amd.MCTS import MCTS
    if not a.tree:   # (another checkout searches the way it always did)
        MCTS.SearchLaunch = "lockstep" if a.child == "lockstep" else "wave"
        MCTS.SearchRollouts = a.child != "lockstep"
    np.random.seed(0)
    cls, game_id, plies = (DragonChess.BoardState, _lib.GAME_DRAGONCHESS, 64) if a.game == "dc" else (Connect4.BoardState, _lib.GAME_CONNECT4, 43)
    if a.kind == "fixed":
        m = FixedMCTS(maxDepth=a.depth, explorationRate=0.85, playLimit=a.sims)
    else:
        m = DynamicMCTS(explorationRate=0.85, playLimit=a.sims)
    start = cls()
    find = []
    for k in range(3 + a.reps):   # (three heat-up calls: code objects, clocks)
        m.DropRoot()
        t = time.perf_counter()
        m.FindMove(start, 1.0)   # (ends in bb_sample_moves, which synchronises)
        if k >= 3:
            find.append((time.perf_counter() - t) * 1e3)
    structure = m._engine.run_sims_structure() if hasattr(m._engine, "run_sims_structure") else None
    eng = m._make_engine(game_id, a.games, a.sims, node_capacity=a.sims * plies * m._max_depth() + 64)   # (arena._Searcher's sizing)
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
    print(json.dumps({"run": a.child, "game": a.game, "kind": a.kind, "tree": a.tree or "-", "structure": structure,
                      "findmove_ms": statistics.median(find), "findmove_min_ms": min(find), "arena_ply_ms": statistics.median(ply),
                      "arena_ply_min_ms": min(ply)}))


def child_cache(a):
    """One run of the --cache leg: a whole game and a whole arena; a.child is 'wave' or 'wave_cache'."""
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    os.chdir(tempfile.mkdtemp())
    import numpy as np
    from blackbird_amd import Blackbird, Connect4, DragonChess, _lib, arena
    from blackbird_amd.MCTS import MCTS
    MCTS.SearchLaunch = "wave"
    if a.child == "wave_cache":
        MCTS.SearchEvalCache = True
    made, real = [], _lib.Engine

    class Spy(real):
        def __init__(self, *args, **kw):
            real.__init__(self, *args, **kw)
            self.final = None
            made.append(self)

        def close(self):   # (the arena closes its engines: keep what they counted)
            if self.h.value:
                self.final = self.counters()
            real.close(self)

    _lib.Engine = Spy
    cfg = {"blocks": 4, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": {"optimizer": "adam"}}
    cls = DragonChess.BoardState if a.game == "dc" else Connect4.BoardState
    np.random.seed(0)
    p1 = Blackbird.Model(cls, "p1", {"explorationRate": 0.85, "playLimit": a.sims}, cfg)
    p2 = Blackbird.Model(cls, "p2", {"explorationRate": 0.85, "playLimit": a.sims}, cfg)

    def share():
        c = [e.final or e.counters() for e in made]
        hits, probes, evals = (sum(x[k] for x in c) for k in ("eval_cache_hits", "eval_cache_probes", "evals"))
        for e in made:
            if e.h.value:
                e.reset_counters()
        made[:] = [e for e in made if e.h.value]
        return (hits / probes if probes else 0.0), evals

    warm = Blackbird.Model(cls, "w", {"explorationRate": 0.85, "playLimit": 16}, cfg)   # heat-up: code objects, clocks; its own engine
    for _ in range(3):
        warm.DropRoot()
        warm.FindMove(cls(), 1.0)
    share()
    np.random.seed(1)
    s, plies = cls(), 0
    t = time.perf_counter()
    while s.Winner() is None and plies < a.plies:
        s, _v, _p = p1.FindMove(s, 1.0)
        p1.MoveRoot(s)
        plies += 1
    game_ms = (time.perf_counter() - t) * 1e3
    game_share, game_evals = share()
    np.random.seed(2)
    t = time.perf_counter()
    if a.game == "dc":   # (a DragonChess game outlasts the 64 plies arena._Searcher sizes its pools for: the same loop, capped)
        capped_arena(np, _lib, (p1, p2), a.games, a.sims, a.plies)
    else:
        arena.TestModelsBatched(p1, p2, 1.0, a.games, playLimit=a.sims, uniforms=np.random.RandomState(5).random_sample)
    arena_ms = (time.perf_counter() - t) * 1e3
    arena_share, arena_evals = share()
    print(json.dumps({"run": a.child, "game": a.game, "tree": a.tree or "-", "plies": plies, "game_ms": game_ms, "game_hit_share": game_share,
                      "game_evals": game_evals, "arena_ms": arena_ms, "arena_hit_share": arena_share, "arena_evals": arena_evals}))


def child_arena(a):
    """One run of the --arena-loop leg: a whole arena through the loop a.child names ('host' or 'device')."""
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    os.chdir(tempfile.mkdtemp())
    import numpy as np
    from blackbird_amd import Blackbird, Connect4, DragonChess, _lib, arena
    from blackbird_amd.MCTS import MCTS
    MCTS.SearchLaunch = a.launch
    cfg = {"blocks": 4, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": {"optimizer": "adam"}}
    cls = DragonChess.BoardState if a.game == "dc" else Connect4.BoardState
    np.random.seed(0)
    p1 = Blackbird.Model(cls, "p1", {"explorationRate": 0.85, "playLimit": a.sims}, cfg)
    p2 = Blackbird.Model(cls, "p2", {"explorationRate": 0.85, "playLimit": a.sims}, cfg)
    warm = Blackbird.Model(cls, "w", {"explorationRate": 0.85, "playLimit": 16}, cfg)   # heat-up: code objects, clocks; its own engine
    for _ in range(3):
        warm.DropRoot()
        warm.FindMove(cls(), 1.0)
    first = np.arange(a.games) % 2 == 0
    np.random.seed(2)   # (the engines' seeds come from numpy's state: the same in every run)
    t = time.perf_counter()
    if a.game == "dc":   # (a DragonChess game outlasts the arena's node pools: a.plies plies of every game)
        if a.child == "device":
            plies = device_capped_arena(np, _lib, (p1, p2), a.games, a.sims, a.plies, a.temp)
        else:
            capped_arena(np, _lib, (p1, p2), a.games, a.sims, a.plies, a.temp)
            plies = a.plies
        results = None
    else:
        kw = {"loop": a.child} if a.child == "device" else {}   # (another checkout has the host loop only, and no such argument)
        res = arena.TestModelsBatched(p1, p2, a.temp, a.games, playLimit=a.sims, first=first, **kw)
        plies, results = None, [int((res == v).sum()) for v in (1, 0, -1)]
    arena_ms = (time.perf_counter() - t) * 1e3
    print(json.dumps({"run": a.child, "game": a.game, "launch": a.launch, "tree": a.tree or "-", "arena_ms": arena_ms, "plies": plies,
                      "wins_draws_losses": results}))


def device_capped_arena(np, _lib, players, games, sims, plies, temp):
    """capped_arena through the arena on the device: the first side moves first in every game."""
    game_id = players[0].Game.GAME_ID
    engines = []
    for m in players:
        eng = m._make_engine(game_id, games, sims, node_capacity=sims * (plies // 2 + 2) + 64)
        m._after_engine_created(eng)
        engines.append(eng)
    ar = _lib.Arena(engines[0], engines[1])
    ar.begin(np.ones(games, dtype=bool), temp)
    ar.step(plies)
    ar.status()
    done = int(ar.fetch()["plies"].max())
    ar.close()
    for e in engines:
        e.close()
    return done


def main_arena(a):
    run(a, "host")   # heat-up, not counted
    runs = {"device": [], "host": [], "other_host": []}
    order = ([("device", "device", None)] if a.arena_loop == "device" else []) + [("host", "host", None)]
    order += [("other_host", "host", a.tree)] if a.tree else []
    for k in range(a.rounds):   # (the order rotates: no loop always runs right after the same other one)
        for name, which, tree in order[k % len(order):] + order[:k % len(order)]:
            runs[name].append(run(a, which, tree))
    res = {"game": a.game, "sims": a.sims, "games": a.games, "rounds": a.rounds, "launch": a.launch, "temp": a.temp,
           "plies_cap": a.plies if a.game == "dc" else None}
    for name, rs in runs.items():
        v = [r["arena_ms"] for r in rs]
        if v:
            res[f"{name}_arena_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(json.dumps(res))


def capped_arena(np, _lib, players, games, sims, plies, temp=1.0):
    """What arena.TestModelsBatched does with its two engines, for at most `plies` plies: the side to move searches all its
    games (run_sims under a mask), samples its moves, and both sides follow with move_roots."""
    game_id = players[0].Game.GAME_ID
    engines = []
    for m in players:
        eng = m._make_engine(game_id, games, sims, node_capacity=sims * (plies // 2 + 2) + 64)
        m._after_engine_created(eng)
        eng.set_roots(np.repeat(_lib.game_initial(game_id), games, axis=0), game_ids=np.arange(games))
        engines.append(eng)
    rng = np.random.RandomState(5)
    for ply in range(plies):
        eng = engines[ply % 2]
        eng.run_sims(sims, mask=np.ones(games, dtype=np.uint8))
        act = eng.sample_moves(temp, rng.random_sample(games))["action"]
        act = np.where(act >= 0, act, -1).astype(np.int32)
        if (act < 0).all():
            break
        for e in engines:
            e.move_roots(act)
    assert all(e.counters()["overflow"] == 0 for e in engines)
    for e in engines:
        e.close()


def main_cache(a):
    run(a, "wave")   # heat-up, not counted
    runs = {"wave_cache": [], "wave": [], "other_wave": []}
    order = [("wave_cache", "wave_cache", None), ("wave", "wave", None)] + ([("other_wave", "wave", a.tree)] if a.tree else [])
    for k in range(a.rounds):   # (the order rotates: no structure always runs right after the same other one)
        for name, which, tree in order[k % len(order):] + order[:k % len(order)]:
            runs[name].append(run(a, which, tree))
    res = {"game": a.game, "sims": a.sims, "games": a.games, "rounds": a.rounds, "plies_cap": a.plies}
    for name, rs in runs.items():
        for key in ("game_ms", "arena_ms", "game_hit_share", "arena_hit_share", "plies"):
            v = [r[key] for r in rs]
            if v:
                res[f"{name}_{key}"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(json.dumps(res))


def run(a, which, tree=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--game", a.game, "--sims", str(a.sims), "--games", str(a.games),
           "--reps", str(a.reps), "--plies", str(a.plies), "--evaluator", a.evaluator, "--kind", a.kind, "--depth", str(a.depth)]
    cmd += (["--tree", tree] if tree else []) + (["--cache"] if a.cache else [])
    cmd += ["--arena-loop", a.arena_loop, "--launch", a.launch, "--temp", str(a.temp)] if a.arena_loop else []
    env = dict(os.environ, BB_SW_ROLLOUT_PLAIN="1" if which == "wave_plain" else "0")
    out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout, check=True, env=env).stdout.decode()
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
    p.add_argument("--cache", action="store_true", help="the evaluation cache of the one-launch search: whole game, whole arena")
    p.add_argument("--plies", type=int, default=None, help="--cache: cap on the plies of the whole game (default: 43 for c4, 40 for dc)")
    p.add_argument("--evaluator", choices=["net", "rollout"], default="net", help="rollout: FixedMCTS / DynamicMCTS instead of a Model")
    p.add_argument("--kind", choices=["fixed", "dynamic"], default="fixed", help="--evaluator rollout: the searcher")
    p.add_argument("--depth", type=int, default=10, help="--evaluator rollout --kind fixed: maxDepth")
    p.add_argument("--arena-loop", choices=["host", "device"], default=None, help="the whole arena through the host / the device loop")
    p.add_argument("--launch", choices=["lockstep", "wave"], default="lockstep", help="--arena-loop: MCTS.SearchLaunch of the engines")
    p.add_argument("--temp", type=float, default=0.0, help="--arena-loop: TestModels' temp (0: every loop plays the same games)")
    p.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.sims is None:
        a.sims = 400 if a.game == "dc" else 800
    if a.plies is None:
        a.plies = 40 if a.game == "dc" else 43
    if a.arena_loop and not a.cache:
        return child_arena(a) if a.child else main_arena(a)
    if a.child:
        return child_cache(a) if a.cache else child_rollout(a) if a.evaluator == "rollout" else child(a)
    if a.cache:
        return main_cache(a)
    run(a, "lockstep")   # heat-up, not counted
    runs = {"lockstep": [], "wave": [], "wave_plain": [], "other_lockstep": []}
    for _ in range(a.rounds):
        runs["lockstep"].append(run(a, "lockstep"))
        runs["wave"].append(run(a, "wave"))
        if a.evaluator == "rollout" and a.game != "dc":   # (DragonChess has one form: its playout is a wave's already)
            runs["wave_plain"].append(run(a, "wave_plain"))
        if a.tree:
            runs["other_lockstep"].append(run(a, "lockstep", a.tree))
    res = {"game": a.game, "sims": a.sims, "games": a.games, "rounds": a.rounds}
    if a.evaluator == "rollout":
        res.update(evaluator="rollout", kind=a.kind, depth=a.depth if a.kind == "fixed" else None)
    for name, rs in runs.items():
        for key in ("findmove_ms", "arena_ply_ms"):
            v = [r[key] for r in rs]
            if v:
                res[f"{name}_{key}"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
