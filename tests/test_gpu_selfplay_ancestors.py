"""-m gpu: ancestor chains under self-play.  bb_config.track_ancestors promises that every simulation is backed up through the
edges above the current root (MCTS._backProp recurses past the root, MCTS.py:238-258) and bb_reset_roots (MCTS.ResetRoot,
:214-225) depends on it; advance_root grows the chain during self-play in every launch structure.  Here engines that keep the
chain PLAY, in every structure, and the whole tree of every slot is then held against the invariants of tests/tree_cases.py
from its top-most root down; lock-step self-play is compared with the search path that the reference's golden vectors pin; and
a dense chain that outgrows its max_plies + 2 entries is refused as DragonChess's is."""
import numpy as np
import pytest

from blackbird_amd import _lib
from tests import search_cases as S
from tests import selfplay_cases as SP
from tests import tree_cases as T

pytestmark = pytest.mark.gpu
C4, TTT = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE
LOCK, WAVE = _lib.LAUNCH_LOCKSTEP, _lib.LAUNCH_WAVE
N_SLOTS = 17      # the queue kernel holds 16 games per workgroup: one full workgroup and one with a single game
SIMS = 16
BLOCKS = 2        # 16 filters x 2 blocks
NODE_CAP = 512    # cannot fill: a tree takes at most one node per simulation and one per move, and no slot gets near 30 moves' worth
FIRST_STEPS, MORE_STEPS = 3, 2   # TicTacToe cannot end before ply 5, Connect4 not before ply 7


def _net(game, launch, **kw):
    return SP.net_engine(game, N_SLOTS, 2 * N_SLOTS, SIMS, BLOCKS, launch=launch, noise=True, node_capacity=NODE_CAP,
                         track_ancestors=True, **kw)[0]


def _dense(game, launch, ev, n_slots=N_SLOTS, **kw):
    return S.dense_engine(game, n_slots, launch, ev, node_capacity=NODE_CAP, track_ancestors=True, sims_per_move=SIMS,
                          max_games=2 * n_slots, **kw)


def _rollout(game, wave):
    eng = _dense(game, LOCK, "rollout")
    eng.selfplay_rollouts(wave)
    return eng


# structure -> (engine, what bb_selfplay_mode must say)
STRUCTURES = {
    "lockstep_hash": (lambda g: _dense(g, LOCK, "hash"), _lib.PLAY_LOCKSTEP),
    "lockstep_net": (lambda g: _net(g, LOCK), _lib.PLAY_LOCKSTEP),
    "rounds_hash": (lambda g: _dense(g, _lib.LAUNCH_ROUNDS, "hash"), _lib.PLAY_ROUNDS),
    # LAUNCH_AUTO with a 16-filter network is the persistent queue kernel -- in the split-operand form with store-only backups
    # that never walk the chain, and in either form with per-slot rows indexed by the workgroup's local slot number, which the
    # chain's rows are not made for.  An engine that keeps the chain is sent to the rounds instead (selfplay_plan).
    "auto_net_split": (lambda g: _net(g, _lib.LAUNCH_AUTO), _lib.PLAY_ROUNDS),
    "auto_net_f32": (lambda g: _net(g, _lib.LAUNCH_AUTO, net_form=_lib.NET_FORM_F32), _lib.PLAY_ROUNDS),
    "rollout_lockstep": (lambda g: _rollout(g, False), _lib.PLAY_LOCKSTEP),
    "rollout_wave": (lambda g: _rollout(g, True), _lib.PLAY_WAVE_ROLLOUT),
}


def _stones(game, states):
    """Plies played from an empty board, read off the board alone."""
    boards = _lib.unpack_grid(game, states)[0]
    return boards.reshape(len(boards), -1).astype(np.int64).sum(axis=1)


def _reset_and_check(eng, game, what):
    """bb_reset_roots, then every slot: its root is the game's first position and its whole tree keeps the invariants.
    Returns (stones on every slot's board before the reset, root plays after it, nodes seen)."""
    assert not eng.selfplay_done()[0], what
    before = _stones(game, eng.root_states())
    eng.reset_roots()
    roots = eng.root_states()
    start = np.repeat(_lib.game_initial(game), eng.n_slots, axis=0)
    assert S.same_position(game, roots, start), (what, "a root is not its game's first position", _stones(game, roots))
    plays = eng.sample_moves(0.0)["root_plays"]
    nodes = 0
    for s in range(eng.n_slots):
        st = T.check_tree(lambda node: S.view_rows(eng, s, node), -1, int(plays[s]), "%s slot %d" % (what, s))
        assert st["depth"] >= before[s], (what, s, st, before[s])   # the line the game took hangs below the top
        nodes += st["nodes"]
    assert eng.counters()["overflow"] == 0, what
    return before, plays, nodes


@pytest.mark.parametrize("structure", list(STRUCTURES))
@pytest.mark.parametrize("key", ["ttt", "c4"])
def test_every_selfplay_structure_keeps_the_chain(key, structure):
    """Play three plies, go back to the top, check every slot's whole tree; play two more from there, go back, check again.
    A slot that moved m times since its game began has had 16 m .. 16 m + 16 simulations applied (a move is made once 16 are, the
    next 16 lead to the next move; one in flight is not counted), and with the chain kept the top's plays are that number --
    whatever the structure, and for a slot that went on to its next game too (reset_slot starts chain and count anew)."""
    game = S.GAME_OF[key]
    make, mode = STRUCTURES[structure]
    eng = make(game)
    assert eng.selfplay_mode() == mode
    eng.selfplay_begin(2 * N_SLOTS, 1.0)
    eng.selfplay_step(FIRST_STEPS)
    moved, plays, nodes = _reset_and_check(eng, game, (key, structure, "first"))
    print(key, structure, "plies before the reset", moved.tolist(), "top plays", plays.tolist(), "nodes walked", nodes)
    assert (moved >= 2).sum() * 2 >= N_SLOTS, ("too few slots two plies deep: the check is vacuous", moved)
    assert ((plays >= SIMS * moved) & (plays <= SIMS * moved + SIMS)).all(), (moved, plays)
    if mode in (_lib.PLAY_LOCKSTEP, _lib.PLAY_WAVE_ROLLOUT):   # every slot makes exactly `plies` moves per call
        assert (moved == FIRST_STEPS).all() and (plays == SIMS * FIRST_STEPS).all(), (moved, plays)
    finished = eng.selfplay_done()[1]
    eng.selfplay_step(MORE_STEPS)   # play resumes from the reset root
    more, plays2, nodes2 = _reset_and_check(eng, game, (key, structure, "second"))
    print(key, structure, "plies after it", more.tolist(), "top plays", plays2.tolist(), "nodes walked", nodes2)
    assert (more >= 1).sum() * 2 >= N_SLOTS and nodes2 > nodes, (more, nodes, nodes2)
    if finished == 0 and eng.selfplay_done()[1] == 0:   # every slot still in its first game: the count goes on
        total = moved + more
        assert ((plays2 >= SIMS * total) & (plays2 <= SIMS * total + SIMS)).all(), (total, plays2)
    eng.close()


@pytest.mark.parametrize("key", ["ttt", "c4"])
def test_track_ancestors_plays_the_rounds_not_the_queue(key):
    game = S.GAME_OF[key]
    plain = SP.net_engine(game, N_SLOTS, N_SLOTS, SIMS, BLOCKS)[0]
    kept = SP.net_engine(game, N_SLOTS, N_SLOTS, SIMS, BLOCKS, track_ancestors=True)[0]
    assert (plain.selfplay_mode(), kept.selfplay_mode()) == (_lib.PLAY_QUEUE, _lib.PLAY_ROUNDS)
    S.close_all(plain, kept)


def _action_between(game, a, b):
    """The one action that leads from packed state a to b."""
    found = [k for k in np.flatnonzero(_lib.game_legal(game, a)[0])
             if S.same_position(game, _lib.game_apply(game, a, np.array([k], dtype=np.int32))[0], b)]
    assert len(found) == 1, (a, b, found)
    return int(found[0])


@pytest.mark.parametrize("key", ["ttt", "c4"])
def test_lockstep_selfplay_builds_the_search_paths_tree(key):
    """Three plies of lock-step self-play (hash evaluator, no noise) against set_roots + run_sims(16) + move_roots of the moves
    it made, on the same game ids and seed: after bb_reset_roots the whole trees are the same rows byte for byte, with 48 plays at
    the top.  The two paths differ by design in the counters that only self-play keeps -- plies and examples -- and in nothing
    else: the slot's random streams are keyed by (seed, game id, ply / node serial) on both."""
    game, n, plies = S.GAME_OF[key], 3, 3
    play, search = _dense(game, LOCK, "hash", n_slots=n), _dense(game, LOCK, "hash", n_slots=n)
    start = np.repeat(_lib.game_initial(game), n, axis=0)
    play.selfplay_begin(n, 1.0)                       # slot s plays game s
    search.set_roots(start, game_ids=np.arange(n))
    at = play.root_states().copy()
    assert S.same_position(game, at, start)
    for ply in range(plies):
        play.selfplay_step(1)
        now = play.root_states().copy()
        actions = np.array([_action_between(game, at[s:s + 1], now[s:s + 1]) for s in range(n)], dtype=np.int32)
        search.run_sims(SIMS)
        search.move_roots(actions)
        assert S.same_position(game, search.root_states(), now), ply
        at = now
    for e in (play, search):
        e.reset_roots()
    a, b = (S.snapshot(e, 0.0, None, S.view_rows) for e in (play, search))
    S.assert_same(a, b, key, ignore_counters=("plies", "examples"))
    assert (a[0]["root_plays"] == SIMS * plies).all() and a[2]["overflow"] == 0
    for s in range(n):
        ra, rb = (T.collect_rows(lambda node: S.view_rows(e, s, node), -1) for e in (play, search))
        assert len(ra) == len(rb) > SIMS * plies // 2, (s, len(ra), len(rb))
        for i, (x, y) in enumerate(zip(ra, rb)):
            S.assert_same_fields(x, y, (key, s, "row", i))
        T.check_tree(lambda node: S.view_rows(search, s, node), -1, SIMS * plies, "%s search slot %d" % (key, s))
    S.close_all(play, search)


def test_broken_ancestor_chain_is_refused_by_both():
    """More moves than max_plies + 2 ancestors (tests/test_gpu_search_wave_dc.py has DragonChess's): the searches below the
    broken chain agree bit for bit, both engines refuse ResetRoot, and nothing moves."""
    lock, wave = S.lock_and_wave(lambda launch: S.dense_engine(TTT, 3, launch, "hash", node_capacity=NODE_CAP, max_plies=2,
                                                               track_ancestors=True), WAVE)
    S.set_roots_on((lock, wave), np.repeat(_lib.game_initial(TTT), 3, axis=0))
    rng = np.random.RandomState(12)
    for move in range(5):   # five stones: no game is over before the last of them
        a = S.step_and_compare((lock, wave), 8, rng, S.view_rows, what=move)[0]
        for e in (lock, wave):
            e.move_roots(S.sampled_moves(a))
    assert (_stones(TTT, lock.root_states()) == 5).all()
    a = S.step_and_compare((lock, wave), 8, rng, S.view_rows, what="below the broken chain")[0]
    assert a[2]["sims"] == 3 * 6 * 8 and a[2]["overflow"] == 0   # every slot searched, every time (a finished game's root too)
    for e in (lock, wave):
        here = e.root_states().tobytes()
        with pytest.raises(_lib.BlackbirdHipError, match="max_plies"):
            e.reset_roots()
        assert e.root_states().tobytes() == here
    S.set_roots_on((lock, wave), np.repeat(_lib.game_initial(TTT), 3, axis=0))   # a new chain: whole again
    for e in (lock, wave):
        e.run_sims(8)
        e.move_roots(np.zeros(3, dtype=np.int32))
        e.reset_roots()
        assert _stones(TTT, e.root_states()).tolist() == [0, 0, 0]
    S.close_all(lock, wave)
