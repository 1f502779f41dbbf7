"""-m gpu: the random-rollout evaluator (BB_EVAL_ROLLOUT: k_rollout<Connect4 / TicTacToe>, k_dc_rollout) and the tree branches
only rollouts take, against the oracle's restatement of MCTS.SampleValue (MCTS.py:360-383; oracle/orc_mcts.c sample_value).
Both sides draw move k of a rollout from Philox(seed, game id, simulation serial, 'ROLL', k) and pick x0 * n >> 32, so
every comparison is exact.  Every compared search also asserts, on the oracle's side, that no rollout reached the engine's
2048-ply cap or a position without a legal move (tests/rollout_cases.py), except where that is what is tested."""
import numpy as np
import pytest

from blackbird_amd import _lib
from tests import rollout_cases as RC
from tests import selfplay_cases as SP

pytestmark = pytest.mark.gpu
GAMES = RC.GAMES


def _selfplay(name, n_slots=None):
    key, fixed, max_depth, sims, n_games, slots, max_plies = RC.SELFPLAY[name]
    eng = _lib.Engine(GAMES[key], n_slots=n_slots or slots, sims_per_move=sims,
                      mcts_kind=_lib.MCTS_FIXED if fixed else _lib.MCTS_DYNAMIC, max_depth=max_depth,
                      evaluator=_lib.EVAL_ROLLOUT, c_puct=RC.C_PUCT, seed=RC.SEED, max_games=n_games, max_plies=max_plies,
                      first_game_id=RC.FIRST_GAME_ID)
    out = SP.play_to_end(eng, n_games, 8, 1.0, steps_below=200)    # (SP.step_bound: 24 Connect4 games on one slot, 168)
    rec, offs, win, cnt = out["rec"], out["offs"], out["win"], out["cnt"]
    eng.close()
    assert cnt["overflow"] == 0 and cnt["games_finished"] == n_games and cnt["examples"] == len(rec)
    return rec, offs, win, cnt


@pytest.mark.parametrize("name", sorted(RC.SELFPLAY))
def test_rollout_selfplay_vs_oracle(orc, name):
    """Batched self-play with rollouts == the oracle's serial games, example by example.  Fewer slots than games (slots are
    reused), slot counts that do not fill the workgroups' four waves, game ids from 1000."""
    rec, offs, win, cnt = _selfplay(name)
    RC.assert_selfplay_is_the_oracles(orc, name, rec, offs, win, cnt)


@pytest.mark.parametrize("name", ["c4_fixed10", "dc_dynamic"])
def test_rollout_selfplay_does_not_depend_on_the_schedule(name):
    """The streams are keyed by game id and simulation serial, never by slot or launch: 1, 5 and 64 slots give the same bytes."""
    runs = [_selfplay(name, n_slots=n) for n in (1, 5, 64)]
    for rec, offs, win, _cnt in runs[1:]:
        assert np.array_equal(offs, runs[0][1]) and np.array_equal(win, runs[0][2])
        assert rec.tobytes() == runs[0][0].tobytes()


# ---- FindMove in its steps, from mid-game positions, with tree reuse -------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("key,fixed,max_depth,every", [("c4", True, 10, 67), ("c4", False, 10, 67),
                                                       ("dc", True, 3, 26), ("dc", False, 10, 26)])
def test_rollout_find_move_steps_vs_oracle(orc, golden_dir, key, fixed, max_depth, every, masked):
    """bb_set_roots, then three rounds of bb_run_sims(2, 5, 9) / bb_sample_moves(temp 0) / bb_move_roots, one slot per
    position (every `every`-th non-terminal position of the golden playouts: either side to move, both halves of White's
    double move), against one oracle search per slot.  Pins the rollout's value from arbitrary positions (the value is
    PreviousPlayer's), and that the simulation serial -- the rollout stream's key -- carries on across MoveRoot.
    masked: the second round searches through bb_run_sims_masked with every third slot left out; those slots keep their
    statistics and their later rollouts use the serials of an oracle search that skipped the round.
    root_winrate is the float32 the ABI returns: the oracle's float64 WinRate rounded once."""
    RC.find_move_steps_vs_oracle(orc, golden_dir, key, fixed, max_depth, every, masked)


# ---- DragonChess: a position without a legal move --------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [False, True], ids=["dynamic", "fixed3"])
def test_rollout_position_without_a_legal_move(orc, fixed):
    """Both kings on the board and the side to move without a pseudo-legal move (the reference would raise inside
    np.random.choice): the rollout scores 0.5, the node is expanded to zero edges and stays a leaf, bb_sample_moves on it
    answers BB_ERR_NAN.  Slot 0 reaches the position as the only child of its root (one forced move), then moves its root
    there; slot 1 starts on such a position.  The oracle follows the same rule (oracle/orc_mcts.c sample_value)."""
    game = _lib.GAME_DRAGONCHESS
    pos = [RC.FORCED, RC.STUCK_ROOK]
    packed = _lib.pack_dc(np.stack([p["board"] for p in pos]), [p["player"] for p in pos], [p["prev"] for p in pos])
    ost = [RC.orc_state(orc, p) for p in pos]
    for p, st, n_legal in zip(packed, ost, (1, 0)):
        assert orc.legal(orc.DC, st).sum() == n_legal and orc.winner(orc.DC, st) is None
        assert _lib.game_legal(game, p[None]).sum() == n_legal and _lib.game_winner(game, p[None])[0] == -1
    eng = _lib.Engine(game, n_slots=2, sims_per_move=4, mcts_kind=_lib.MCTS_FIXED if fixed else _lib.MCTS_DYNAMIC,
                      max_depth=3, evaluator=_lib.EVAL_ROLLOUT, c_puct=RC.C_PUCT, seed=RC.SEED, max_plies=8)
    eng.set_roots(packed, game_ids=[5, 6])
    cfg = RC.oracle_cfg(orc, "dc", fixed, 3)
    search = [orc.Search(cfg, 5), orc.Search(cfg, 6)]
    eng.run_sims(4)
    assert eng.counters()["overflow"] == 0
    out = eng.sample_moves(0)
    o = search[0].find_move(ost[0], 0, 4)
    with pytest.raises(ValueError):
        search[1].find_move(ost[1], 0, 4)
    n_child = int(o["plays"][RC.FORCED_ACTION])
    assert n_child == (4 if fixed else 3) and o["winrates"][RC.FORCED_ACTION] == 0.5
    assert out["action"].tolist() == [RC.FORCED_ACTION, _lib.ERR_NAN] and out["root_plays"].tolist() == [4, 4]
    assert out["child_action"][0, 0] == RC.FORCED_ACTION and (out["child_action"][0, 1:] == -1).all()
    assert out["child_plays"][0, 0] == n_child and out["child_value"][0, 0] == 0.5 * n_child  # every backup was 0.5
    assert (out["child_action"][1] == -1).all() and (out["child_plays"][1] == 0).all()
    eng.move_roots(np.array([RC.FORCED_ACTION, -1], dtype=np.int32))
    assert search[0].move_root(o["next"]) == 1
    after = _lib.pack_dc(RC.STUCK_AFTER_FORCED["board"][None], [1], [2])
    assert np.array_equal(eng.root_states()[0], after[0])
    out = eng.sample_moves(0)
    assert out["root_plays"][0] == n_child and out["root_winrate"][0] == 0.5
    eng.run_sims(4)
    for s in range(2):
        with pytest.raises(ValueError):
            search[s].find_move(o["next"] if s == 0 else ost[1], 0, 4)
    out = eng.sample_moves(0)
    assert out["action"].tolist() == [_lib.ERR_NAN, _lib.ERR_NAN]
    assert out["root_plays"].tolist() == [n_child + 4, 8] and out["root_winrate"][0] == 0.5
    assert (out["child_action"] == -1).all()
    cnt = eng.counters()
    eng.close()
    stats = [sr.stats() for sr in search]
    assert [st.sims for st in stats] == [8, 8] and all(st.rollouts_without_moves == 8 for st in stats)
    assert all(st.max_rollout_steps <= 1 for st in stats)
    assert cnt["overflow"] == 0 and cnt["sims"] == 16
    assert cnt["sum_depth"] == sum(st.sum_depth for st in stats) and cnt["nodes"] == sum(st.nodes_reached for st in stats)
    assert cnt["terminal_leaves"] == 0
