"""-m gpu: the recorded descent of the persistent self-play kernel (async_game<G, true>, tree.hip.h) requests a level's row one
level ahead and creates a new child behind its loop.  Self-play through that kernel (mode 3) must give the bytes of the lock-step
structure (mode 0), whose descent is phase_select: example records, game offsets, headers, winners, simulation and depth counts.

The shapes aim at the edges the loop has:
  * BB_LEVEL_BUDGET 2 and 3 (the engine's opt-in, read by bb_create): a descent parks between the request of a row and its use,
    and the resumed call requests the row again;
  * 3 and 19 slots with 12 and 48 simulations per move: every move starts at a fresh root, so the first level's child is
    CHILD_NONE and the clamped request is the common case; 19 slots are one full 16-game workgroup and one with 3 games;
  * Connect4 from a board with 36 stones (6 cells left, no winner yet; LATE_C4): on the CPU oracle (hash evaluator, 25 games of
    48 simulations from that board) 3 763 of 3 888 simulations, 96.8 %, end on a terminal leaf, and 175 nodes are created in all,
    so at least 143 simulations per game revisit a terminal leaf whose value is cached -- the NODE_CACHED exit, which reads pad0.
    The test repeats that count on the oracle (5 games) and requires at least one such revisit per game on average.
All comparisons are exact."""
import numpy as np
import pytest

from blackbird_amd import _lib
from tests import selfplay_cases as SP

pytestmark = pytest.mark.gpu
C4, TTT = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE
LATE_C4 = (3, 0, 1, 4, 0, 5, 5, 3, 6, 0, 4, 1, 0, 2, 3, 4, 5, 6, 4, 3, 5, 6, 0, 4, 3, 0, 3, 5, 4, 6, 6, 6, 1, 1, 1, 5)


def _late_c4():
    st = _lib.game_initial(C4)
    for a in LATE_C4:
        st = SP._apply(C4, st, a)
    assert _lib.game_winner(C4, st)[0] < 0 and int(_lib.game_legal(C4, st).sum()) >= 2
    return st


def _queue_and_lockstep(monkeypatch, game, n_slots, n_games, sims, budget, starts=None):
    if budget is None:
        monkeypatch.delenv("BB_LEVEL_BUDGET", raising=False)
    else:
        monkeypatch.setenv("BB_LEVEL_BUDGET", str(budget))
    runs, modes = {}, {}
    for name, launch in (("queue", _lib.LAUNCH_AUTO), ("lockstep", _lib.LAUNCH_LOCKSTEP)):
        eng, _flat = SP.net_engine(game, n_slots, n_games, sims, 1, launch=launch, seed=23, first_id=100)
        modes[name] = eng.selfplay_mode()
        runs[name] = SP.play_from_starts(eng, n_games, starts, step=2)
        eng.close()
    assert modes == {"queue": 3, "lockstep": 0}
    SP.assert_same_runs(runs["queue"], runs["lockstep"], (game, n_slots, sims, budget))
    assert {k: runs["queue"]["cnt"][k] for k in SP.COUNTERS} == {k: runs["lockstep"]["cnt"][k] for k in SP.COUNTERS}
    return runs["queue"]


@pytest.mark.parametrize("game,n_slots,n_games,sims,budget", [
    (C4, 3, 7, 12, 2), (C4, 19, 25, 48, 3), (C4, 19, 25, 12, None),
    (TTT, 3, 7, 48, 3), (TTT, 19, 30, 12, 2),
])
def test_queue_kernel_is_lockstep_under_small_level_budgets(monkeypatch, game, n_slots, n_games, sims, budget):
    out = _queue_and_lockstep(monkeypatch, game, n_slots, n_games, sims, budget)
    assert out["cnt"]["sims"] >= n_games * sims


@pytest.mark.parametrize("budget", [2, None])
def test_late_connect4_boards_end_on_cached_terminals(monkeypatch, orc, budget):
    n_slots, n_games, sims = 19, 25, 48
    start = _late_c4()
    # the oracle alone: every node is first reached once, so terminal-leaf simulations beyond the number of nodes ever created
    # revisited a terminal leaf whose value is cached -- a lower bound on those revisits, not their count
    cfg = orc.make_cfg(0, evaluator=orc.EVAL_HASH, salt=11, seed=5)
    ostart = SP.orc_state_from_packed(orc, 0, C4, start[0])
    term = nodes = 0
    for gid in range(5):
        s = SP.oracle_selfplay_from(orc, cfg, gid, ostart, 1.0, sims, 43)["stats"]
        term, nodes = term + s.terminal_leaves, nodes + s.nodes
    assert term - nodes >= 5, (term, nodes)
    out = _queue_and_lockstep(monkeypatch, C4, n_slots, n_games, sims, budget, starts=start)
    cnt = out["cnt"]
    assert cnt["terminal_leaves"] - cnt["nodes"] >= n_games, cnt   # the engine met them too
    assert np.all(np.diff(out["offs"]) >= 2) and np.all(np.diff(out["offs"]) <= 7)
