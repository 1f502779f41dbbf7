"""-m gpu: the one-launch search with the rollout evaluator (bb_search_rollouts: k_search_wave_rollout, k_dc_search_wave_rollout)
against the lock-step loop it replaces.  A rollout's draws are keyed (game id, simulation serial, 'ROLL', step), never by who
computes them, so a wave that plays out its own leaf must leave what k_tree_step + k_rollout leave: every case is a pair of
engines with the same seed and first game id, lock-step and wave, compared on everything a caller can read -- sampled moves,
root rows, child rows, counters -- bit for bit.  Lock-step itself is held to the CPU oracle by tests/test_gpu_rollout.py."""
import numpy as np
import pytest

from blackbird_amd import Connect4, _lib, arena
from blackbird_amd.FixedMCTS import FixedMCTS
from blackbird_amd.MCTS import MCTS
from tests import rollout_cases as RC
from tests import search_cases as S
from tests.search_cases import HashSearch, launches  # noqa: F401  (launches: a fixture)

pytestmark = pytest.mark.gpu
C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
LOCK, WAVE = _lib.LAUNCH_LOCKSTEP, _lib.LAUNCH_WAVE
KINDS = {"dynamic": dict(mcts_kind=_lib.MCTS_DYNAMIC),
         "fixed3": dict(mcts_kind=_lib.MCTS_FIXED, max_depth=3),     # leaves that already have children
         "fixed10": dict(mcts_kind=_lib.MCTS_FIXED, max_depth=10)}
DC_KW = dict(max_plies=24, node_capacity=128)


def _rollout_engine(game, n_slots, launch, kind="dynamic", node_capacity=512, **kw):
    return S.dense_engine(game, n_slots, launch, "rollout", node_capacity=node_capacity, **dict(KINDS[kind], **kw))


def _searching(game, n_slots, launch, kind, **kw):
    eng = _rollout_engine(game, n_slots, launch, kind, **kw)
    if launch == WAVE:
        eng.search_rollouts(True)
    return eng


def _pair(game, n_slots, kind="dynamic", **kw):
    return S.lock_and_wave(lambda launch: _searching(game, n_slots, launch, kind, **kw), WAVE)


# ---- structure ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dynamic", "fixed10"])
@pytest.mark.parametrize("game", [C4, TTT, DC], ids=["c4", "ttt", "dc"])
def test_structure_follows_the_setter(game, kind):
    kw = DC_KW if game == DC else {}
    wave, lock = _rollout_engine(game, 3, WAVE, kind, **kw), _rollout_engine(game, 3, LOCK, kind, **kw)
    assert wave.run_sims_structure() == LOCK          # without the call: as before
    wave.search_rollouts(True)
    assert wave.run_sims_structure() == WAVE
    wave.search_rollouts(False)
    assert wave.run_sims_structure() == LOCK
    wave.search_rollouts()                            # (on=True is the default)
    assert wave.run_sims_structure() == WAVE and wave.selfplay_mode() == 0   # self-play stays lock-step
    lock.search_rollouts(True)                        # launch = LOCKSTEP: the call changes nothing
    assert lock.run_sims_structure() == LOCK
    for bad in (2, -1):
        assert _lib.lib().bb_search_rollouts(wave.h, bad) == _lib.ERR_ARG
    assert wave.run_sims_structure() == WAVE
    S.close_all(wave, lock)


def test_setter_changes_nothing_for_another_evaluator():
    hashed = S.dense_engine(DC, 1, WAVE, "hash", **DC_KW)      # no one-launch kernel for DragonChess's hash evaluator
    hashed.search_rollouts(True)
    assert hashed.run_sims_structure() == LOCK
    dense = S.dense_engine(C4, 1, WAVE, "hash", node_capacity=512)
    dense.search_rollouts(False)
    assert dense.run_sims_structure() == WAVE
    S.close_all(hashed, dense)


# ---- dense games -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sims", [1, 2, 50])
@pytest.mark.parametrize("n_slots", [1, 3, 5])   # never a multiple of the four waves of a workgroup
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("key", ["c4", "ttt"])
def test_same_bits_as_lockstep_over_three_moves(key, kind, n_slots, sims):
    game = S.GAME_OF[key]
    lock, wave = _pair(game, n_slots, kind, node_capacity=2048)
    S.set_roots_on((lock, wave), S.openings(game, n_slots))
    rng = np.random.RandomState(5)
    for move in range(3):
        a = S.step_and_compare((lock, wave), sims, rng, S.view_rows, what=(key, kind, n_slots, sims, move))[0]
        assert a[2]["overflow"] == 0 and a[2]["sims"] == (move + 1) * sims * n_slots
        for e in (lock, wave):
            e.move_roots(S.sampled_moves(a))
    S.close_all(lock, wave)


@pytest.mark.parametrize("kind", ["dynamic", "fixed10"])
@pytest.mark.parametrize("key", ["c4", "ttt"])
def test_roots_next_to_a_win_and_to_a_full_board(golden_dir, key, kind):
    """Terminal leaves (rollouts of zero steps) and playouts that fill the board (0.5)."""
    game = S.GAME_OF[key]
    lock, wave = _pair(game, 5, kind, node_capacity=2048)
    S.set_roots_on((lock, wave), S.endgame_roots(golden_dir, key))
    rng = np.random.RandomState(6)
    halves = 0
    for move in range(2):
        a = S.step_and_compare((lock, wave), 50, rng, S.view_rows, what=(key, kind, move))[0]
        assert a[2]["terminal_leaves"] > 0 and a[2]["overflow"] == 0
        # a child every one of whose backups was 0.5: a drawn playout (or a drawn terminal leaf)
        halves += int(((a[0]["child_plays"] > 0) & (a[0]["child_value"] == 0.5 * a[0]["child_plays"])).sum())
        for e in (lock, wave):
            e.move_roots(S.sampled_moves(a))
    assert halves > 0
    S.close_all(lock, wave)


@pytest.mark.parametrize("kind", ["dynamic", "fixed10"])
def test_masked_search_leaves_the_other_slots_alone(kind):
    lock, wave = _pair(C4, 5, kind, node_capacity=2048)
    S.set_roots_on((lock, wave), S.openings(C4, 5))
    rng = np.random.RandomState(7)
    even = np.array([1, 0, 1, 0, 1], dtype=np.uint8)
    before = None
    masks = (even, 1 - even, even, 1 - even)
    for k, mask in enumerate(masks):
        a = S.step_and_compare((lock, wave), 20, rng, S.view_rows, mask=mask, what=(kind, k))[0]
        for s in np.nonzero(mask == 0)[0]:   # a slot outside the mask: its tree is what it was
            now = wave.node_view(int(s), -1)
            if before is not None:
                assert all(np.array_equal(now[f], before[int(s)][f]) for f in now), (kind, k, s)
        before = {s: wave.node_view(s, -1) for s in range(5)}
        assert a[2]["sims"] == 20 * sum(int(m.sum()) for m in masks[:k + 1])
    S.close_all(lock, wave)


@pytest.mark.parametrize("kind", ["dynamic", "fixed10"])
def test_three_short_calls_equal_one_long_call(kind):
    """run_sims(16) three times == run_sims(48) once: the simulation serial, the rollout stream's key, carries on."""
    lock, once = _pair(C4, 3, kind, node_capacity=2048)
    thrice = _rollout_engine(C4, 3, WAVE, kind, node_capacity=2048)
    thrice.search_rollouts(True)
    S.set_roots_on((lock, once, thrice), S.openings(C4, 3))
    u = np.random.RandomState(8).random_sample(3)
    lock.run_sims(48)
    once.run_sims(48)
    for _ in range(3):
        thrice.run_sims(16)
    a = S.snapshot(lock, 1.0, u, S.view_rows)
    S.assert_same(a, S.snapshot(once, 1.0, u, S.view_rows), "48 at once")
    S.assert_same(a, S.snapshot(thrice, 1.0, u, S.view_rows), "3 x 16")
    S.close_all(lock, once, thrice)


@pytest.mark.parametrize("kind", ["dynamic", "fixed3"])
def test_ancestors_and_reset_roots(kind):
    lock, wave = _pair(TTT, 3, kind, track_ancestors=True)
    S.set_roots_on((lock, wave), S.openings(TTT, 3))
    rng = np.random.RandomState(9)
    for move in range(2):
        a = S.step_and_compare((lock, wave), 30, rng, S.view_rows, what=(kind, move))[0]
        for e in (lock, wave):
            e.move_roots(S.sampled_moves(a))
    S.step_and_compare((lock, wave), 30, rng, S.view_rows, what=(kind, "below"))
    for e in (lock, wave):
        e.reset_roots()
    top = S.snapshot(lock, 0.0, None, S.view_rows)
    S.assert_same(top, S.snapshot(wave, 0.0, None, S.view_rows), (kind, "after reset"))
    assert (top[0]["root_plays"] == 90).all()
    S.step_and_compare((lock, wave), 10, rng, S.view_rows, what=(kind, "on the reset tree"))
    S.close_all(lock, wave)


@pytest.mark.parametrize("kind", ["dynamic", "fixed10"])
def test_full_node_pool_counts_the_same_overflow(kind):
    lock, wave = _pair(C4, 3, kind, node_capacity=24)
    S.set_roots_on((lock, wave), S.openings(C4, 3))
    a = S.step_and_compare((lock, wave), 50, np.random.RandomState(10), S.view_rows, what=kind)[0]
    assert a[2]["overflow"] > 0 and a[2]["nodes"] <= 3 * 23   # (the root takes one of a pool's 24 rows)
    S.close_all(lock, wave)


# ---- DragonChess (<= 16 simulations, <= 5 slots: 2048-ply playouts at worst) -----------------------------------------------------
@pytest.mark.parametrize("kind", ["dynamic", "fixed3"])
def test_dragonchess_same_bits_as_lockstep_over_two_moves(kind):
    lock, wave = _pair(DC, 3, kind, **DC_KW)
    S.set_roots_on((lock, wave), S.dc_openings(3))
    rng = np.random.RandomState(12)
    for move in range(2):
        a = S.step_and_compare((lock, wave), 12, rng, S.edge_rows, what=(kind, move))[0]      # (bb_node_edges of every root and of its children)
        assert a[2]["overflow"] == 0 and a[2]["sims"] == (move + 1) * 12 * 3
        for e in (lock, wave):
            e.move_roots(S.sampled_moves(a))
    S.close_all(lock, wave)


@pytest.mark.parametrize("kind", ["dynamic", "fixed3"])
def test_dragonchess_rollout_without_a_legal_move(kind):
    """Roots of tests/rollout_cases.py: one forced move into a position without a legal move, and such a position itself.
    A playout that finds no legal move scores 0.5 in both structures."""
    pos = [RC.FORCED, RC.STUCK_ROOK]
    packed = _lib.pack_dc(np.stack([p["board"] for p in pos]), [p["player"] for p in pos], [p["prev"] for p in pos])
    lock, wave = _pair(DC, 2, kind, **DC_KW)
    S.set_roots_on((lock, wave), packed)
    rng = np.random.RandomState(13)
    a = S.step_and_compare((lock, wave), 12, rng, S.edge_rows, what=(kind, "first"))[0]
    out = a[0]
    assert out["action"].tolist() == [RC.FORCED_ACTION, _lib.ERR_NAN] and out["root_plays"].tolist() == [12, 12]
    assert out["child_plays"][0, 0] > 0 and out["child_value"][0, 0] == 0.5 * out["child_plays"][0, 0]   # every backup was 0.5
    for e in (lock, wave):
        e.move_roots(S.sampled_moves(a))
    b = S.step_and_compare((lock, wave), 12, rng, S.edge_rows, what=(kind, "after the forced move"))[0]
    assert b[0]["action"].tolist() == [_lib.ERR_NAN, _lib.ERR_NAN] and b[2]["overflow"] == 0 and b[2]["terminal_leaves"] == 0
    assert b[0]["root_winrate"][0] == 0.5   # (the root that was moved to has a previous player; a root that was set counts no value)
    S.close_all(lock, wave)


# ---- against the oracle directly -------------------------------------------------------------------------------------------------
def test_connect4_fixed10_under_wave_vs_oracle(orc, golden_dir, monkeypatch):
    """tests/test_gpu_rollout.py::test_rollout_find_move_steps_vs_oracle[c4 Fixed 10, masked] with the engine it creates searching
    through the wave launch: one oracle search per slot, exact."""
    real, made = _lib.Engine, []

    class WaveEngine(real):
        def __init__(self, game, **kw):
            real.__init__(self, game, launch=WAVE, **kw)
            self.search_rollouts(True)
            made.append(self.run_sims_structure())

    monkeypatch.setattr(_lib, "Engine", WaveEngine)
    RC.find_move_steps_vs_oracle(orc, golden_dir, "c4", True, 10, 67, True)
    assert made == [WAVE]


# ---- the front end: MCTS.SearchRollouts ----------------------------------------------------------------------------------------
def _switch(monkeypatch, launch):
    monkeypatch.setattr(MCTS, "SearchLaunch", launch)
    monkeypatch.setattr(MCTS, "SearchRollouts", launch == "wave")
    return (WAVE, WAVE) if launch == "wave" else (_lib.LAUNCH_AUTO, LOCK)


def test_fixed_mcts_find_move_and_move_root(monkeypatch, launches):  # noqa: F811
    """TestGood's opponent on a play limit: three FindMove / MoveRoot steps give the same successors, win rates and
    probabilities under both launches (the engine's seed and FindMove's draw come from numpy's state: reseeded)."""
    runs = {}
    for launch in ("lockstep", "wave"):
        want = _switch(monkeypatch, launch)
        del launches[:]
        np.random.seed(3)
        m = FixedMCTS(maxDepth=10, explorationRate=0.85, playLimit=50)
        s, rec = Connect4.BoardState(), []
        for _ in range(3):
            nxt, v, prob = m.FindMove(s, 1.0)
            rec.append((nxt, float(v), np.array(prob), int(m.Root.Plays), np.array(m.Root.ChildPlays())))
            s = nxt
            m.MoveRoot(s)
        runs[launch] = rec
        assert len(launches) == 3 and all(x == want for x in launches), (launch, launches)
    for (s1, v1, p1, n1, c1), (s2, v2, p2, n2, c2) in zip(runs["lockstep"], runs["wave"]):
        assert s1 == s2 and v1 == v2 and np.array_equal(p1, p2) and n1 == n2 and np.array_equal(c1, c2)
        assert p1.sum() > 0


@pytest.mark.parametrize("temp", [0, 1.0])
def test_batched_arena_same_results_under_wave(monkeypatch, launches, temp):  # noqa: F811
    game = Connect4.BoardState
    p1 = HashSearch(game, 11, explorationRate=0.85, playLimit=32)
    p2 = FixedMCTS(maxDepth=10, explorationRate=0.85, playLimit=32)
    first = np.array([True, False, False, True, True, False])
    results = {}
    for launch in ("lockstep", "wave"):
        want = _switch(monkeypatch, launch)
        del launches[:]
        np.random.seed(3)
        results[launch] = arena.TestModelsBatched(p1, p2, temp, 6, playLimit=32, first=first,
                                                  uniforms=np.random.RandomState(5).random_sample)
        assert launches and all(x == want for x in launches), (launch, launches[:4])
    assert np.array_equal(results["lockstep"], results["wave"]), results
    assert set(np.unique(results["wave"])) <= {-1, 0, 1}
