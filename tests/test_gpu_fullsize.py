"""-m gpu: size-independent properties of the hot path at BASELINE.json's full sizes, where the oracle would need hours.

configs[1] (Connect4, 4096 concurrent games, 800 simulations per move, the default persistent kernel) and configs[3]
(DragonChess, 1024 concurrent games, 400 simulations per move, ply cap 512, the one-wave-per-game kernel on the 161 GB
edge pool + 27 GB node pool):

* every example's visit counts add up to the root's play count, which is >= playLimit - 1 on a game's first move and grows by
  the re-used subtree afterwards (MCTS.py:146-199 playLimit semantics, _moveRoot :260-282);
* pi is the normalised visit vector over LEGAL moves only; the terminal example of every finished game has pi = 0 and the
  z of all its examples follows the winner found on the final board (Blackbird.py:253-264);
* replaying a game's recorded positions with the game kernels reproduces each next position (the move is legal and is the
  one the visit counts allow: visited at least once); DragonChess: the side to move follows W, W, B (DragonChess.py:192-197);
* schedule independence: the same games played on fewer slots (every slot plays several games) are byte-identical to the
  run with one slot per game -- RNG streams are keyed by game id / ply / node, never by slot or time."""
import numpy as np
import pytest

from blackbird_amd import _lib, weights as W
from tests import selfplay_cases as SP

pytestmark = pytest.mark.gpu
SIMS = 800


def _play(n_slots, n_games, plies):
    eng = _lib.Engine(_lib.GAME_CONNECT4, n_slots=n_slots, sims_per_move=SIMS, evaluator=_lib.EVAL_NET, seed=4242,
                      noise_on=True, alpha=0.2, epsilon=0.3, max_games=n_games)
    eng.load_weights(W.flatten(W.init_weights(3, 16, 4, 16, 7, seed=0)))
    eng.selfplay_begin(n_games, 1.0)
    for _ in range(plies):
        eng.selfplay_step(1)
        if eng.selfplay_done()[0]:
            break
    done, finished = eng.selfplay_done()
    rec, offs, win = eng.fetch_examples()
    cnt = eng.counters()
    eng.close()
    return rec, offs, win, cnt, finished


def test_full_size_selfplay_properties():
    n = 4096
    rec, offs, win, cnt, finished = _play(n, n, 30)   # 30 steps of all 4096 games: ~100 M simulations, ~3 s
    assert cnt["overflow"] == 0 and cnt["sims"] >= n * SIMS * 20
    assert finished >= n // 2 and cnt["games_finished"] == finished  # most games are over after 30+ plies
    game = _lib.GAME_CONNECT4
    checked_terminal = checked_records = 0
    fin = np.nonzero(np.diff(offs) > 0)[0]
    assert len(fin) == finished
    for g in fin[::13]:                                # a spread of finished games (python loop cost), all plies of each
        r = rec[offs[g]:offs[g + 1]]
        states = np.ascontiguousarray(r["state"]).view(_lib.STATE_DTYPE[game]).reshape(len(r), -1)
        legal = _lib.game_legal(game, states)
        vis = r["visits"][:, :7].astype(np.int64)
        tot = r["total"].astype(np.int64)
        nonterm = vis.sum(1) > 0
        assert nonterm[:-1].all() and not nonterm[-1]  # exactly one terminal example (pi = 0), the last one
        assert np.array_equal(vis.sum(1)[nonterm], tot[nonterm])
        assert tot[0] >= SIMS - 1                      # first move: playLimit simulations, the first one expands the root
        assert (tot[:-1] >= SIMS - 1).all()            # later moves: playLimit more on top of the re-used subtree
        assert (np.diff(r["ply"].astype(np.int64)) == 1).all() and r["ply"][0] == 0
        assert ((vis > 0) <= (legal > 0)).all()        # visits only on legal moves
        assert (r["player"][:-1] == 1 + (np.arange(len(r) - 1) % 2)).all()  # players alternate from player 1
        # the recorded next position is reachable by a visited move
        for k in range(len(r) - 1):
            cand = np.nonzero(vis[k])[0]
            nxt, status = _lib.game_apply(game, np.repeat(states[k:k + 1], len(cand), 0), cand.astype(np.int32))
            assert any(status[i] == 0 and nxt[i].tobytes() == states[k + 1].tobytes() for i in range(len(cand)))
        # finished game: the final board decides z for every example (Blackbird.py:260-264)
        w = int(_lib.game_winner(game, states[-1:])[0])
        assert w == win[g] and w >= 0
        z = r["z"].astype(np.int64)
        expect = np.where(w == 0, 0, np.where(r["player"] == w, 1, -1))
        assert np.array_equal(z, expect)
        checked_terminal += 1
        checked_records += len(r)
    assert checked_terminal >= 150 and checked_records >= 150 * 8, (checked_terminal, checked_records)


def test_results_do_not_depend_on_the_slot_count():
    a = _play(1024, 1536, 100)   # at most 2 games of <= 42 plies per slot
    b = _play(512, 1536, 140)    # 3 games per slot
    # compare the games that finished in both runs (all of them, given enough plies)
    assert a[4] == b[4] == 1536
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[0].tobytes() == b[0].tobytes()


# ---- BASELINE configs[3]: DragonChess, 1024 concurrent games x 400 simulations per move ---------------------------
DC_SIMS = 400


def _play_dc(n_slots, n_games, prefill_plies, plies, max_plies=512, first_id=0, to_the_end=False):
    game = _lib.GAME_DRAGONCHESS
    eng = _lib.Engine(game, n_slots=n_slots, sims_per_move=DC_SIMS, evaluator=_lib.EVAL_NET, seed=777, noise_on=True,
                      alpha=0.2, epsilon=0.3, max_games=n_games, max_plies=max_plies, first_game_id=first_id)
    eng.load_weights(W.flatten(W.init_weights(17, 16, 4, 16, 4032, seed=0)))
    mode = eng.selfplay_mode()
    eng.selfplay_begin(n_games, 1.0)
    if prefill_plies:
        eng.set_sims_per_move(6)                      # a quick stretch of weak play so that games END inside the test
        eng.selfplay_step(prefill_plies)
        eng.set_sims_per_move(DC_SIMS)
        eng.synchronize()
        eng.reset_counters()                          # the counters then describe the full-strength plies only
    for _ in range(plies):
        eng.selfplay_step(1)
    guard = 0
    while to_the_end and not eng.selfplay_done()[0]:  # (a launch hands out simulations, not whole moves: play on until every game is over)
        eng.selfplay_step(2)
        guard += 1
        assert guard < 200
    eng.synchronize()
    cnt = eng.counters()
    done, finished = eng.selfplay_done()
    rec, offs, win = eng.fetch_examples()
    eng.close()
    return rec, offs, win, cnt, finished, mode


def _dc_pi(r, k):
    pi = np.zeros(4032, dtype=np.int64)
    n = int(r["n_children"][k])
    pi[r["action"][k][:n]] = r["visits"][k][:n]
    return pi


def test_dragonchess_full_size_properties():
    """configs[3] at full size: 1024 waves on 1024 slots, pools of 512 plies x 400 simulations per slot (188 GB), slot
    recycling when games end.  200 plies of weak play bring many games to their end; then 6 plies at the full 400
    simulations per move follow (records whose root play count says 400-strength search; the counters cover these plies)."""
    n = 1024
    rec, offs, win, cnt, finished, mode = _play_dc(n, 8 * n, 200, 6)
    assert mode == 5 and cnt["overflow"] == 0
    assert cnt["sims"] == 6 * n * DC_SIMS                # six plies' worth of 400 simulations for each of the 1024 slots
    # (a wave owns 7/8 of its game's simulations and draws the rest from one pool per launch in chunks: a quick game may be ahead
    # of a slow one, and a launch ends wherever a game is inside its move -- at most one unfinished move per game)
    assert 6 * n - n <= cnt["plies"] <= 6 * n + n // 16 and cnt["evals"] <= cnt["sims"]
    assert finished >= 200, finished                     # kings do get captured under weak play
    game = _lib.GAME_DRAGONCHESS
    fin = np.nonzero(np.diff(offs) > 0)[0]
    # every record of every finished game at once: the visits of the listed children add up to the root's play count
    live = np.arange(rec["visits"].shape[1])[None, :] < rec["n_children"][:, None]
    assert np.array_equal((rec["visits"] * live).sum(1), rec["total"])
    strong = (rec["n_children"] > 0) & (rec["total"] >= DC_SIMS - 1)   # searched with the full 400 simulations
    assert strong.sum() >= 20, int(strong.sum())                        # games that ended during the six strong plies
    checked_games = capped = 0
    for g in fin[::7]:
        r = rec[offs[g]:offs[g + 1]]
        states = np.ascontiguousarray(r["state"])
        legal = _lib.game_legal(game, states)
        assert (np.diff(r["ply"].astype(np.int64)) == 1).all() and r["ply"][0] == 0 and (r["game_id"] == g).all()
        tot = r["total"].astype(np.int64)
        # W, W, B turn order (DragonChess.py:192-197), checked on the recorded side to move
        pl = r["player"].astype(np.int64)
        assert (pl[:-1] == np.array([1, 1, 2])[np.arange(len(r) - 1) % 3]).all()
        for k in range(len(r) - 1):
            pi = _dc_pi(r, k)
            nch = int(r["n_children"][k])
            assert nch == int(legal[k].sum()) and pi.sum() == tot[k] and tot[k] >= 5
            assert ((pi > 0) <= (legal[k] > 0)).all()
            assert sorted(r["action"][k][:nch].tolist()) == np.nonzero(legal[k])[0].tolist()  # one child per legal move
        # replay: the next recorded position follows from a visited move (spot-check three plies per game)
        for k in sorted(set([0, (len(r) - 1) // 2, len(r) - 2]) & set(range(len(r) - 1))):
            cand = np.nonzero(_dc_pi(r, k))[0]
            nxt, status = _lib.game_apply(game, np.repeat(states[k:k + 1], len(cand), 0), cand.astype(np.int32))
            assert any(status[i] == 0 and nxt[i][:70].tobytes() == states[k + 1][:70].tobytes() for i in range(len(cand)))
        # terminal example + z
        assert int(r["n_children"][-1]) == 0 and tot[-1] == 0
        w = int(_lib.game_winner(game, states[-1:])[0])
        if w < 0:                                        # ply cap reached (documented deviation: z = 0)
            assert len(r) == 513 and (r["z"] == 0).all() and win[g] == -1
            capped += 1
        else:
            assert w == win[g] and w in (1, 2)           # never a draw: win by king capture (DragonChess.py:161-167)
            assert np.array_equal(r["z"].astype(np.int64), np.where(r["player"] == w, 1, -1))
        checked_games += 1
    assert checked_games >= 25, checked_games


def test_dragonchess_results_do_not_depend_on_the_slot_count():
    """1024 games on 1024 slots vs the same games on 256 slots (4 games per slot, 4x smaller pools): byte-identical
    records.  Ply cap 24 and full 400-simulation searches throughout, so every game ends (at the cap) and is compared."""
    a = _play_dc(1024, 1024, 0, 24, max_plies=24, to_the_end=True)
    b = _play_dc(256, 1024, 0, 96, max_plies=24, to_the_end=True)
    assert a[5] == b[5] == 5 and a[3]["overflow"] == 0 and b[3]["overflow"] == 0
    assert a[4] == b[4] == 1024
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[0].tobytes() == b[0].tobytes()
    assert a[3]["sims"] == b[3]["sims"] and a[3]["sum_depth"] == b[3]["sum_depth"]
    r = a[0]
    assert (r["total"][r["n_children"] > 0] >= DC_SIMS - 1).all()  # every search had the full 400 simulations


def test_every_slot_advances_when_workgroups_outnumber_the_chip():
    """More 16-game workgroups than the persistent kernel can keep resident (one per CU): the first-resident ones must not
    drain the launch's visits.  Every workgroup owns 7/8 of its slots' visits (mega2.hip.h), so after one step of two moves'
    worth of search every slot has moved at least once -- and the games are still the ones a one-slot-per-game run on few
    slots plays (schedule independence at this size is test_results_do_not_depend_on_the_slot_count's subject)."""
    n_cu = 256
    n_slots = 16 * n_cu * 2 + 16 * 5 + 3   # 517 workgroups of 16, the last one ragged
    sims = 16
    eng = _lib.Engine(_lib.GAME_CONNECT4, n_slots=n_slots, sims_per_move=sims, evaluator=_lib.EVAL_NET, seed=99, noise_on=True,
                      max_games=n_slots)
    eng.load_weights(W.flatten(W.init_weights(3, 16, 4, 16, 7, seed=0)))
    assert eng.selfplay_mode() == 3
    eng.selfplay_begin(n_slots, 1.0)
    eng.selfplay_step(2)
    eng.synchronize()
    cnt = eng.counters()
    assert cnt["overflow"] == 0
    roots = eng.root_states().reshape(n_slots, -1).view(np.uint64)
    stones = np.array([bin(int(a & 0x00FFFFFFFFFFFFFF)).count("1") + bin(int(b & 0x00FFFFFFFFFFFFFF)).count("1") for a, b in roots[:, :2]])
    assert stones.min() >= 1, f"{int((stones == 0).sum())} of {n_slots} slots did not move"
    # the visits handed out are the launch's: 2 moves' worth per slot (a visit completes >= 1 simulation)
    assert cnt["sims"] >= n_slots * 2 * sims * 7 // 8
    eng.close()


def test_c5_network_full_size_in_search():
    """BASELINE configs[4] on one GPU: 4096 concurrent Connect4 games searched with the 20-block x 256-filter network (the
    launch-per-layer kernels, tower layers in the split-operand form, inside the asynchronous-round search).  A handful of
    simulations per move and a ply cap of 3 keep it to seconds; what is checked does not depend on either:
    * every record's visit counts add up to its root play count (>= playLimit - 1 on a game's first move), pi > 0 only on
      legal moves, the terminal record has pi = 0, replaying a visited move gives the next recorded position;
    * schedule independence: the same 4096 games on 1024 slots (four games per slot, four times smaller evaluation batches:
      another launch shape of every conv layer) are byte-identical to the one-slot-per-game run."""
    game, sims, cap, n = _lib.GAME_CONNECT4, 8, 3, 4096
    flat = W.flatten(W.init_weights(3, 256, 20, 16, 7, seed=0))

    def play(n_slots):
        eng = _lib.Engine(game, n_slots=n_slots, sims_per_move=sims, evaluator=_lib.EVAL_NET, seed=31, noise_on=True, alpha=0.2,
                          epsilon=0.3, max_games=n, max_plies=cap)
        eng.load_weights(flat)
        assert eng.net_form() == 3 and eng.selfplay_mode() == 1
        out = SP.play_to_end(eng, n, 1, 1.0, steps_below=64)
        rec, offs, win = out["rec"], out["offs"], out["win"]
        cnt = eng.counters()
        eng.close()
        return rec, offs, win, cnt

    rec, offs, win, cnt = play(n)
    assert cnt["overflow"] == 0 and cnt["games_finished"] == n and len(rec) == n * (cap + 1)
    assert cnt["evals"] <= cnt["sims"] and cnt["sims"] >= n * cap * (sims - 1)
    r = rec.reshape(n, cap + 1)
    assert (r["ply"] == np.arange(cap + 1)[None, :]).all() and (r["z"] == 0).all() and (win == -1).all()   # ply cap: z = 0
    vis = r["visits"][:, :, :7].astype(np.int64)
    assert np.array_equal(vis.sum(2), r["total"]) and (r["total"][:, cap] == 0).all()
    assert (r["total"][:, 0] == sims - 1).all() and (r["total"][:, 1:cap] >= sims - 1).all()   # fresh root / re-used subtree
    states = np.ascontiguousarray(rec["state"])
    legal = _lib.game_legal(game, states).reshape(n, cap + 1, 7)
    assert ((vis > 0) <= (legal > 0)).all()
    for k in range(cap):   # the next recorded position follows from a visited move
        st_k = np.ascontiguousarray(r["state"][:, k])
        ok = np.zeros(n, dtype=bool)
        for a in range(7):
            nxt, status = _lib.game_apply(game, st_k.copy(), np.full(n, a, dtype=np.int32))
            same = (nxt.reshape(n, -1) == np.ascontiguousarray(r["state"][:, k + 1]).reshape(n, -1)).all(1)
            ok |= same & (status == 0) & (vis[:, k, a] > 0)
        assert ok.all(), k
    rec_b, offs_b, win_b, cnt_b = play(1024)
    assert np.array_equal(offs, offs_b) and np.array_equal(win, win_b) and rec.tobytes() == rec_b.tobytes()
    assert cnt_b["sims"] == cnt["sims"] and cnt_b["sum_depth"] == cnt["sum_depth"]
