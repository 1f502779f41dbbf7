"""Whole self-play runs with the rollout evaluator, lock-step against the one-launch structure (bb_selfplay_rollouts), on one box.

A run is what a user of the C ABI does: bb_selfplay_begin(n_games), bb_selfplay_step(--step plies) until bb_selfplay_done, on an
engine with evaluator = BB_EVAL_ROLLOUT; it reports games/s and milliseconds per bb_selfplay_step (wall clock from begin to done,
the last step synchronised by bb_selfplay_done), after a small heat-up game set in the same process (code objects, clocks).
Every run is a process of its own (a fresh child), and the structures alternate in the manner of tools/search_latency.py --
heat-up run first, then lockstep, wave, [other_lockstep], lockstep, wave, ... --: `lockstep` and `wave` are this build,
`other_lockstep` is lock-step from another checkout of the project with its library built (`--tree DIR`: the parent commit's,
which is the comparison base and must not have moved).  Prints the runs and ONE JSON line per case with medians and min-max.

Cases (`--case`, default all):
  ttt64 / ttt4096   TicTacToe FixedMCTS(maxDepth=10), 50 simulations, c_puct 0.85 (BASELINE configs[0]) at 64 / 4096 slots
  c4_64             Connect4 FixedMCTS(maxDepth=10), 800 simulations at 64 slots (the 4096-slot case is not here: its node
                    pools do not fit the device at the engine's own sizing, and with smaller pools the lock-step run did not
                    finish within the tool's 120 s per process on an MI355X -- cause not found, not measured)
  dc                DragonChess DynamicMCTS rollouts: 64 slots, 16 simulations, games capped at 16 plies (under a minute per run)
Each slot plays `--games-per-slot` games one after another (slots are refilled).  A node pool smaller than the engine's own
sizing (`--node-capacity`, for slot counts whose default pools do not fit the device) can overflow: the count is reported, and a
run with overflow > 0 did not play the games the others played.

usage: python tools/selfplay_rollout_time.py [--case c4_64 ...] [--rounds 3] [--step 8] [--games-per-slot 2] [--tree other/checkout]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: (game, Fixed?, max depth, simulations, slots, max plies, node capacity or 0 = the engine's sizing)
CASES = {
    "ttt64": ("ttt", True, 10, 50, 64, 9, 0),
    "ttt4096": ("ttt", True, 10, 50, 4096, 9, 0),
    "c4_64": ("c4", True, 10, 800, 64, 42, 0),
    "dc": ("dc", False, 10, 16, 64, 16, 0),
}


def child(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    from blackbird_amd import _lib
    game_key, fixed, depth, sims, slots, max_plies, cap = CASES[a.case]
    game = {"c4": _lib.GAME_CONNECT4, "ttt": _lib.GAME_TICTACTOE, "dc": _lib.GAME_DRAGONCHESS}[game_key]
    cap = a.node_capacity if a.node_capacity is not None else cap

    def play(n_slots, n_games):
        eng = _lib.Engine(game, n_slots=n_slots, sims_per_move=sims, mcts_kind=_lib.MCTS_FIXED if fixed else _lib.MCTS_DYNAMIC,
                          max_depth=depth, evaluator=_lib.EVAL_ROLLOUT, c_puct=0.85, seed=31, max_games=n_games, max_plies=max_plies,
                          first_game_id=1000, node_capacity=cap)
        if a.child == "wave":   # (another checkout plays the way it always did)
            eng.selfplay_rollouts(True)
        mode = eng.selfplay_mode()
        eng.synchronize()
        t = time.perf_counter()
        eng.selfplay_begin(n_games, 1.0)
        steps = 0
        while not eng.selfplay_done()[0]:
            eng.selfplay_step(a.step)
            steps += 1
        wall = time.perf_counter() - t
        cnt = eng.counters()
        eng.close()
        return mode, wall, steps, cnt

    play(min(slots, 8), min(slots, 8))   # heat-up
    n_games = slots * a.games_per_slot
    mode, wall, steps, cnt = play(slots, n_games)
    assert cnt["games_finished"] == n_games
    print(json.dumps({"run": a.child, "case": a.case, "tree": a.tree or "-", "mode": mode, "games": n_games, "steps": steps,
                      "wall_s": round(wall, 4), "games_per_s": n_games / wall, "ms_per_step": wall * 1e3 / steps, "sims": cnt["sims"],
                      "plies": cnt["plies"], "overflow": cnt["overflow"]}))


def run(a, case, which, tree=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--case", case, "--step", str(a.step),
           "--games-per-slot", str(a.games_per_slot)]
    cmd += (["--tree", tree] if tree else []) + (["--node-capacity", str(a.node_capacity)] if a.node_capacity is not None else [])
    out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout, check=True).stdout.decode()
    r = json.loads(out.strip().splitlines()[-1])
    print(json.dumps(r), flush=True)
    return r


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--case", nargs="*", choices=sorted(CASES), default=None)
    p.add_argument("--rounds", type=int, default=3, help="alternations (at least three for a figure that goes into the documents)")
    p.add_argument("--step", type=int, default=8, help="plies per bb_selfplay_step")
    p.add_argument("--games-per-slot", type=int, default=2)
    p.add_argument("--node-capacity", type=int, default=None, help="nodes per slot instead of the case's")
    p.add_argument("--tree", default=None)
    p.add_argument("--timeout", type=int, default=120, help="seconds one measurement process may take")
    p.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        a.case = a.case[0]
        return child(a)
    for case in a.case or ["ttt64", "ttt4096", "c4_64", "dc"]:
        run(a, case, "lockstep")   # heat-up, not counted
        runs = {"lockstep": [], "wave": [], "other_lockstep": []}
        for _ in range(a.rounds):
            runs["lockstep"].append(run(a, case, "lockstep"))
            runs["wave"].append(run(a, case, "wave"))
            if a.tree:
                runs["other_lockstep"].append(run(a, case, "lockstep", a.tree))
        game_key, fixed, depth, sims, slots, max_plies, _cap = CASES[case]
        res = {"case": case, "game": game_key, "kind": "fixed" if fixed else "dynamic", "sims": sims, "slots": slots, "step": a.step,
               "rounds": a.rounds, "games": slots * a.games_per_slot}
        for name, rs in runs.items():
            if rs:
                assert len({(r["sims"], r["plies"]) for r in rs}) == 1   # (every run of a structure played the same games)
                res[f"{name}_overflow"] = rs[0]["overflow"]
            for key in ("games_per_s", "ms_per_step"):
                v = [r[key] for r in rs]
                if v:
                    res[f"{name}_{key}"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        if runs["wave"] and runs["lockstep"]:
            res["same_games"] = (runs["wave"][0]["sims"], runs["wave"][0]["plies"]) == (runs["lockstep"][0]["sims"], runs["lockstep"][0]["plies"])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
