"""-m gpu: the search API of a DragonChess engine in one launch (bb_config.launch = BB_LAUNCH_WAVE, k_dc_search_wave: one wave per
slot, the policy head kept as five numbers in LDS) against the lock-step loop it replaces (k_dc_tree_step + k_net_x3 per simulation,
a 4032-float policy row through memory).  Per slot the sequence of operations is the same, so everything a caller can see --
sampled moves, root statistics, the edges of every root and of its children, the counters -- must be the lock-step engine's bit
for bit; engines the kernel does not cover must say so and search lock-step."""
import numpy as np
import pytest

from blackbird_amd import DragonChess, _lib
from blackbird_amd.MCTS import MCTS
from tests import model_cases as M
from tests import search_cases as S
from tests.search_cases import launches  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
DC = _lib.GAME_DRAGONCHESS
LOCK, WAVE = _lib.LAUNCH_LOCKSTEP, _lib.LAUNCH_WAVE


def _engine(n_slots, launch, blocks=2, node_capacity=256, max_plies=24, **kw):
    return S.dc_engine(n_slots, launch, blocks, node_capacity=node_capacity, max_plies=max_plies, **kw)


def _pair(n_slots, blocks=2, want=WAVE, **kw):
    """want = WAVE: what an engine without k_dc_search_wave cannot say"""
    return S.lock_and_wave(lambda launch: _engine(n_slots, launch, blocks, **kw), want)


@pytest.mark.parametrize("sims", [1, 2, 24])
@pytest.mark.parametrize("n_slots", [1, 3, 5])   # never a multiple of the four waves of a workgroup
@pytest.mark.parametrize("blocks", [0, 2])
def test_same_bits_as_lockstep_over_three_moves(blocks, n_slots, sims):
    """Three consecutive moves with tree reuse (move_roots); after every search the two engines agree on everything."""
    lock, wave = _pair(n_slots, blocks)
    S.set_roots_on((lock, wave), S.dc_openings(n_slots))
    rng = np.random.RandomState(5)
    for move in range(3):
        a = S.step_and_compare((lock, wave), sims, rng, S.edge_rows, what=(blocks, n_slots, sims, move))[0]
        assert a[2]["overflow"] == 0 and a[2]["sims"] == (move + 1) * sims * n_slots   # every slot searched, every time
        for e in (lock, wave):
            e.move_roots(S.sampled_moves(a))
    S.close_all(lock, wave)


def _king_captured():
    """A finished game: the start position without Black's king."""
    st = _lib.game_initial(DC).copy()
    assert st[0, 60] == np.uint8(-1 & 0xFF)
    st[0, 60] = 0
    assert _lib.game_winner(DC, st)[0] == 1
    return st


def test_masks_carry_over_and_a_finished_game():
    """A slot outside the mask keeps its tree and its simulations for a later call; a root whose game is over searches the
    same way under both launches."""
    lock, wave = _pair(5)
    states = S.dc_openings(5)
    states[3] = _king_captured()[0]
    S.set_roots_on((lock, wave), states)
    rng = np.random.RandomState(7)
    but2 = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    calls = (but2, 1 - but2, but2, np.ones(5, dtype=np.uint8), 1 - but2)
    before = None
    for k, mask in enumerate(calls):
        a = S.step_and_compare((lock, wave), 12, rng, S.edge_rows, mask=mask, what=k)[0]
        for s in np.nonzero(mask == 0)[0]:   # a slot outside the mask: its tree is what it was
            now = wave.node_edges(int(s), -1)
            if before is not None:
                assert all(np.asarray(now[f]).tobytes() == np.asarray(before[int(s)][f]).tobytes() for f in now), (k, s)
        before = {s: wave.node_edges(s, -1) for s in range(5)}
        assert a[2]["sims"] == 12 * sum(int(m.sum()) for m in calls[:k + 1])
    S.close_all(lock, wave)


def test_three_short_calls_equal_one_long_call():
    """run_sims(8) three times == run_sims(24) once: nothing of a call outlives its launch but the tree."""
    lock, once = _pair(3)
    thrice = _engine(3, WAVE)
    S.set_roots_on((lock, once, thrice), S.dc_openings(3))
    u = np.random.RandomState(8).random_sample(3)
    lock.run_sims(24)
    once.run_sims(24)
    for _ in range(3):
        thrice.run_sims(8)
    a = S.snapshot(lock, 1.0, u, S.edge_rows)
    assert a[2]["sims"] == 3 * 24
    S.assert_same(a, S.snapshot(once, 1.0, u, S.edge_rows), "24 at once")
    S.assert_same(a, S.snapshot(thrice, 1.0, u, S.edge_rows), "3 x 8")
    S.close_all(lock, once, thrice)


def _walk_down(eng, slot, actions):
    """The edges of the root and of the nodes below it along `actions`."""
    rows = [eng.node_edges(slot, -1)]
    for a in actions:
        k = np.nonzero(rows[-1]["action"] == a)[0]
        if a < 0 or len(k) == 0 or rows[-1]["child"][k[0]] < 0:
            break
        rows.append(eng.node_edges(slot, int(rows[-1]["child"][k[0]]) & 0x3FFFFFFF))
    return rows


def test_ancestors_and_reset_roots():
    """track_ancestors: every backup also walks the chain above the root (dc_phase_apply's ANC half), so after two moves
    bb_reset_roots finds the same statistics at the top and all the way down to the old root."""
    lock, wave = _pair(3, track_ancestors=True)
    S.set_roots_on((lock, wave), S.dc_openings(3))
    rng = np.random.RandomState(9)
    played = []
    for move in range(2):
        a = S.step_and_compare((lock, wave), 24, rng, S.edge_rows, what=move)[0]
        played.append(S.sampled_moves(a))
        for e in (lock, wave):
            e.move_roots(played[-1])
    a = S.step_and_compare((lock, wave), 24, rng, S.edge_rows, what="below")[0]
    assert a[2]["sims"] == 3 * 3 * 24
    for e in (lock, wave):
        e.reset_roots()
    top = S.snapshot(lock, 0.0, None, S.edge_rows)
    S.assert_same(top, S.snapshot(wave, 0.0, None, S.edge_rows), "after reset")
    assert (top[0]["root_plays"] == 72).all()
    for s in range(3):
        line = [int(p[s]) for p in played]
        ra, rb = _walk_down(lock, s, line), _walk_down(wave, s, line)
        assert len(ra) == len(rb) == 3, s
        for x, y in zip(ra, rb):
            assert all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in x), s
    S.step_and_compare((lock, wave), 8, rng, S.edge_rows, what="on the reset tree")
    S.close_all(lock, wave)


def test_broken_ancestor_chain_is_refused_by_both():
    """More moves than max_plies + 2 ancestors: the searches below the broken chain agree, and both engines refuse ResetRoot."""
    lock, wave = _pair(1, track_ancestors=True, max_plies=2)
    S.set_roots_on((lock, wave), S.dc_openings(1))
    rng = np.random.RandomState(12)
    for move in range(5):
        a = S.step_and_compare((lock, wave), 8, rng, S.edge_rows, what=move)[0]
        for e in (lock, wave):
            e.move_roots(S.sampled_moves(a))
    a = S.step_and_compare((lock, wave), 8, rng, S.edge_rows, what="below the broken chain")[0]
    assert a[2]["sims"] == 6 * 8
    for e in (lock, wave):
        here = e.root_states().tobytes()
        with pytest.raises(_lib.BlackbirdHipError, match="max_plies"):
            e.reset_roots()
        assert e.root_states().tobytes() == here
    S.close_all(lock, wave)


def test_full_pools_count_the_same_overflow():
    """12 node rows (and 12 x 24 edges) per slot: 24 simulations outgrow them."""
    lock, wave = _pair(3, node_capacity=12)
    S.set_roots_on((lock, wave), S.dc_openings(3))
    a = S.step_and_compare((lock, wave), 24, np.random.RandomState(10), S.edge_rows)[0]
    assert a[2]["overflow"] > 0 and a[2]["nodes"] <= 3 * 11 and a[2]["sims"] == 3 * 24   # (the root takes one of a pool's 12 rows)
    S.close_all(lock, wave)


@pytest.mark.parametrize("case", ["nine_blocks", "net_form_f32"])
def test_uncovered_networks_search_lockstep_and_say_so(case):
    """A tower whose constants do not fit the kernel's LDS copy (R > 8) and the float32-MFMA form: lock-step, visibly."""
    kw = dict(blocks=9) if case == "nine_blocks" else dict(net_form=_lib.NET_FORM_F32)
    lock, wave = _pair(3, want=LOCK, **kw)
    S.set_roots_on((lock, wave), S.dc_openings(3))
    a = S.step_and_compare((lock, wave), 8, np.random.RandomState(11), S.edge_rows, what=case)[0]
    assert a[2]["sims"] == 3 * 8
    S.close_all(lock, wave)


# ---- the front end: MCTS.SearchLaunch --------------------------------------------------------------------------------
def _model(name, seed):
    return M.model(DragonChess.BoardState, name, seed=seed, play_limit=16, eps=0.3, blocks=2)


def _node_facts(node):
    return (node.State, node.Plays, np.float32(node.Value).tobytes(), node.ChildPlays().tobytes(), node.ChildWinRates().tobytes())


def _front_end_run():
    """FindMove x 3 with MoveRoot, ResetRoot, then down the played line through Children: everything the API returned."""
    m = _model("dcw", 1)
    np.random.seed(3)    # the engine's noise seed and FindMove's draws come from numpy's state
    s = DragonChess.BoardState()
    facts, line = [], []
    for k in range(3):
        nxt, v, prob = m.FindMove(s, 1.0 if k == 1 else 0)
        facts.append((nxt, np.float32(v).tobytes(), prob.tobytes()) + _node_facts(m.Root))
        line.append(next(int(a) for a in np.nonzero(m.Root.LegalActions == 1)[0] if m._applyAction(s, int(a)) == nxt))
        s = nxt
        m.MoveRoot(s)
        facts.append(_node_facts(m.Root))
    m.ResetRoot()
    node = m.Root
    assert node.State == DragonChess.BoardState() and node.Parent is None and node.Plays == 3 * 16
    for a in line:
        facts.append(_node_facts(node))
        node = node.Children[a]
        assert node is not None
    facts.append(_node_facts(node))
    return facts


def test_model_findmove_moveroot_resetroot_children_under_wave(tmp_path, monkeypatch, launches):
    monkeypatch.chdir(tmp_path)
    runs = {}
    for launch in ("lockstep", "wave"):
        monkeypatch.setattr(MCTS, "SearchLaunch", launch)
        del launches[:]
        runs[launch] = _front_end_run()
        want = (WAVE, WAVE) if launch == "wave" else (_lib.LAUNCH_AUTO, LOCK)
        assert len(launches) == 3 and all(x == want for x in launches), (launch, launches)
    assert len(runs["wave"]) == len(runs["lockstep"])
    for i, (x, y) in enumerate(zip(runs["lockstep"], runs["wave"])):
        assert x == y, i
