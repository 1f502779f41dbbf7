"""-m gpu: the evaluation cache in the one-launch search (bb_config.search_cache with BB_LAUNCH_WAVE; k_search_wave<G, true, true>)
against the lock-step loop and the one-launch search without it.  A hit leaves in the mailbox the bits the tower would have --
the cached value and pre-noise priors through the same prior-noise tail, with the node's own noise key -- so everything a caller
can see is the lock-step engine's bit for bit; only the counters evals / eval_cache_hits / eval_cache_probes tell the engines
apart, and they obey  probes == evals + hits == the evals of the same search without the cache.

(A terminal leaf is posted to the evaluator like any other, by the lock-step engine too -- its `evals` counts it -- so the cached
search probes it like any other: that is what keeps the identity above.)"""
import numpy as np
import pytest

from blackbird_amd import Connect4, _lib, arena
from blackbird_amd import weights as W
from blackbird_amd.MCTS import MCTS
from tests.test_gpu_search_wave import _endgame_roots, _engine, _model, _openings, _snap

pytestmark = pytest.mark.gpu
C4, TTT = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE
AUTO, LOCK, WAVE = _lib.LAUNCH_AUTO, _lib.LAUNCH_LOCKSTEP, _lib.LAUNCH_WAVE
NET = ("net", 16, 2)
CACHE_COUNTERS = ("evals", "eval_cache_hits", "eval_cache_probes")


def _trio(game, n_slots, ev=NET, **kw):
    """Lock-step, wave, wave with search_cache: the same engine otherwise."""
    lock, wave = _engine(game, n_slots, LOCK, ev, **kw), _engine(game, n_slots, WAVE, ev, **kw)
    cached = _engine(game, n_slots, WAVE, ev, search_cache=True, **kw)
    assert lock.run_sims_structure() == LOCK and wave.run_sims_structure() == WAVE and cached.run_sims_structure() == WAVE
    return lock, wave, cached


def _set(engines, states):
    for e in engines:
        e.set_roots(states, game_ids=7 * np.arange(len(states)) + 3)


def _close(*engines):
    for e in engines:
        e.close()


def _same_trees(a, b, what=""):
    """Snapshots (tests/test_gpu_search_wave.py::_snap) equal in everything but the three counters the cache may change."""
    (oa, ra, ca), (ob, rb, cb) = a, b
    for k in oa:
        assert np.array_equal(oa[k], ob[k]), (what, k, oa[k], ob[k])
    assert len(ra) == len(rb), what
    for i, (x, y) in enumerate(zip(ra, rb)):
        for k in x:
            assert np.array_equal(x[k], y[k]), (what, "node row", i, k, x[k], y[k])
    rest = lambda c: {k: v for k, v in c.items() if k not in CACHE_COUNTERS}
    assert rest(ca) == rest(cb), (what, ca, cb)


def _check(snaps, what=""):
    """(lock-step, wave, cached wave) snapshots of one moment: same trees, and the counter identities."""
    a, b, c = snaps
    _same_trees(a, b, what)
    _same_trees(a, c, what)
    ca, cb, cc = a[2], b[2], c[2]
    assert ca == cb, (what, ca, cb)
    assert ca["eval_cache_hits"] == 0 and ca["eval_cache_probes"] == 0, (what, ca)
    assert cc["eval_cache_probes"] == cc["evals"] + cc["eval_cache_hits"] == ca["evals"], (what, ca, cc)


def _step(engines, sims, rng, mask=None, what=""):
    u = rng.random_sample(engines[0].n_slots)
    for e in engines:
        e.run_sims(sims, mask=mask)
    snaps = [_snap(e, 1.0, u) for e in engines]
    _check(snaps, what)
    return snaps


def _moves(snapshot):
    return np.where(snapshot[0]["action"] >= 0, snapshot[0]["action"], -1).astype(np.int32)


@pytest.mark.parametrize("sims", [2, 50])
@pytest.mark.parametrize("n_slots", [1, 3, 5])   # never a multiple of the four waves of a workgroup
def test_same_bits_over_three_moves(n_slots, sims):
    engines = _trio(C4, n_slots)
    _set(engines, _openings(C4, n_slots))
    rng = np.random.RandomState(5)
    for move in range(3):
        snaps = _step(engines, sims, rng, what=(n_slots, sims, move))
        assert snaps[0][2]["overflow"] == 0 and snaps[0][2]["sims"] == (move + 1) * sims * n_slots
        for e in engines:
            e.move_roots(_moves(snaps[0]))
    _close(*engines)


def _delta(after, before):
    return {k: after[k] - before[k] for k in CACHE_COUNTERS}


def test_second_pass_is_all_hits_and_a_reload_empties_the_table():
    """The same roots searched twice: the second pass finds every position of the first.  (Assumes that nothing is evicted in
    between: at most 150 distinct positions in 2^26 two-way buckets -- a third position of one bucket is what it would take.)
    Then other weights: no entry of the first network may answer, so every position's first evaluation is a tower run and the
    trees are those of a fresh lock-step engine with the second weights."""
    cached = _engine(C4, 3, WAVE, NET, search_cache=True)
    st, ids = _openings(C4, 3), 7 * np.arange(3) + 3
    u = np.random.RandomState(12).random_sample(3)
    zero = cached.counters()
    cached.set_roots(st, game_ids=ids)
    cached.run_sims(50)
    first = _snap(cached, 1.0, u)
    d1 = _delta(first[2], zero)
    assert d1["eval_cache_probes"] == d1["evals"] + d1["eval_cache_hits"] > 0
    cached.set_roots(st, game_ids=ids)
    cached.run_sims(50)
    second = _snap(cached, 1.0, u)
    d2 = _delta(second[2], first[2])
    assert d2["evals"] == 0 and d2["eval_cache_hits"] == d2["eval_cache_probes"] == d1["eval_cache_probes"], (d1, d2)
    (oa, ra, _), (ob, rb, _) = first, second
    assert all(np.array_equal(oa[k], ob[k]) for k in oa) and len(ra) == len(rb)
    assert all(np.array_equal(x[k], y[k]) for x, y in zip(ra, rb) for k in x)

    gi = _lib.game_info(C4)
    other = W.flatten(W.init_weights(gi.C, 16, 2, 16, gi.A, seed=22, perturb=True))
    cached.load_weights(other)
    cached.set_roots(st, game_ids=ids)
    cached.run_sims(1)    # each slot's first simulation evaluates its root: three positions the table held before the reload
    d3 = _delta(cached.counters(), second[2])
    assert d3 == {"evals": 3, "eval_cache_hits": 0, "eval_cache_probes": 3}, d3
    cached.run_sims(49)
    third = _snap(cached, 1.0, u)
    fresh = _lib.Engine(C4, evaluator=_lib.EVAL_NET, noise_on=True, alpha=0.2, epsilon=0.3, n_slots=3, sims_per_move=8, seed=17,
                        first_game_id=1000, launch=LOCK, node_capacity=512)
    fresh.load_weights(other)
    fresh.set_roots(st, game_ids=ids)
    fresh.run_sims(50)
    want = _snap(fresh, 1.0, u)
    (oa, ra, ca), (ob, rb, _) = want, third
    assert all(np.array_equal(oa[k], ob[k]) for k in oa) and len(ra) == len(rb)
    assert all(np.array_equal(x[k], y[k]) for x, y in zip(ra, rb) for k in x)
    assert not np.array_equal(want[0]["child_value"], first[0]["child_value"])   # (the second network is another one)
    d4 = _delta(third[2], second[2])
    assert d4["eval_cache_probes"] == d4["evals"] + d4["eval_cache_hits"] == ca["evals"], (d4, ca)
    _close(cached, fresh)


def test_masked_slots():
    engines = _trio(C4, 3)
    _set(engines, _openings(C4, 3))
    rng = np.random.RandomState(7)
    for k, mask in enumerate((np.array([1, 0, 1], dtype=np.uint8), np.array([1, 1, 0], dtype=np.uint8))):
        before = engines[2].node_view(int(np.nonzero(mask == 0)[0][0]), -1)
        _step(engines, 20, rng, mask=mask, what=k)
        now = engines[2].node_view(int(np.nonzero(mask == 0)[0][0]), -1)
        assert all(np.array_equal(now[f], before[f]) for f in now), k
    _close(*engines)


def test_endgame_roots(golden_dir):
    engines = _trio(C4, 5)
    _set(engines, _endgame_roots(golden_dir, "c4"))
    rng = np.random.RandomState(6)
    for move in range(2):
        snaps = _step(engines, 50, rng, what=move)
        assert snaps[0][2]["terminal_leaves"] > 0 and snaps[0][2]["overflow"] == 0
        for e in engines:
            e.move_roots(_moves(snaps[0]))
    _close(*engines)


NO_PROBE = {
    "tictactoe_network": (TTT, NET, WAVE, {}, None),          # no cache key
    "connect4_hash": (C4, "hash", WAVE, {}, None),            # nothing to cache
    "cache_switched_off": (C4, NET, WAVE, {}, "0"),           # BB_EVAL_CACHE=0: no table
    "lockstep_search": (C4, NET, AUTO, {}, None),             # owns a table (self-play's), searches lock-step
}


@pytest.mark.parametrize("case", list(NO_PROBE))
def test_engines_without_table_or_wave_take_the_flag_and_probe_nothing(monkeypatch, case):
    game, ev, launch, kw, env = NO_PROBE[case]
    if env is not None:
        monkeypatch.setenv("BB_EVAL_CACHE", env)
    off, on = _engine(game, 3, launch, ev, **kw), _engine(game, 3, launch, ev, search_cache=True, **kw)
    assert off.run_sims_structure() == on.run_sims_structure() == (LOCK if launch == AUTO else WAVE)
    _set((off, on), _openings(game, 3))
    u = np.random.RandomState(11).random_sample(3)
    for e in (off, on):
        e.run_sims(50)
    a, b = _snap(off, 1.0, u), _snap(on, 1.0, u)
    _same_trees(a, b, case)
    assert a[2] == b[2] and b[2]["eval_cache_probes"] == 0 and b[2]["evals"] > 0, (case, a[2], b[2])
    _close(off, on)


def test_any_other_value_is_refused():
    with pytest.raises(ValueError):
        _lib.Engine(C4, n_slots=1, sims_per_move=8, evaluator=_lib.EVAL_HASH, launch=WAVE, search_cache=2)


# ---- the front end: MCTS.SearchEvalCache --------------------------------------------------------------------------------
@pytest.fixture
def engines_made(monkeypatch):
    made = []
    real = _lib.Engine

    class Spy(real):
        def __init__(self, *a, **kw):
            real.__init__(self, *a, **kw)
            self.final = None
            made.append(self)

        def close(self):   # (the arena closes its engines: keep what they counted)
            if self.h.value:
                self.final = self.counters()
            real.close(self)

    monkeypatch.setattr(_lib, "Engine", Spy)
    return made


def _hits(engines):
    return sum((e.final or e.counters())["eval_cache_hits"] for e in engines)


def test_findmove_same_moves_and_root_statistics(tmp_path, monkeypatch, engines_made):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(MCTS, "SearchLaunch", "wave")
    runs = {}
    for on in (False, True):
        monkeypatch.setattr(MCTS, "SearchEvalCache", on)
        del engines_made[:]
        m = _model(Connect4.BoardState, "f%d" % on, 1)
        np.random.seed(3)    # the engine's noise seed and FindMove's draws come from numpy's state
        s, facts = Connect4.BoardState(), []
        for k in range(3):
            nxt, v, prob = m.FindMove(s, 1.0 if k == 1 else 0)
            r = m.Root
            facts.append((nxt, np.float32(v).tobytes(), prob.tobytes(), r.Plays, np.float32(r.Value).tobytes(),
                          r.ChildPlays().tobytes(), r.ChildWinRates().tobytes()))
            s = nxt
            m.MoveRoot(s)
        runs[on] = facts
        assert engines_made and all(e.run_sims_structure() == WAVE for e in engines_made)
        assert (_hits(engines_made) > 0) == on
    assert runs[False] == runs[True]


def test_batched_arena_same_results(tmp_path, monkeypatch, engines_made):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(MCTS, "SearchLaunch", "wave")
    game = Connect4.BoardState
    p1, p2 = _model(game, "a", 1), _model(game, "b", 2)
    first = np.array([True, False, False, True, True, False])
    results = {}
    for on in (False, True):
        monkeypatch.setattr(MCTS, "SearchEvalCache", on)
        del engines_made[:]
        np.random.seed(3)
        results[on] = arena.TestModelsBatched(p1, p2, 1.0, 6, playLimit=32, first=first,
                                              uniforms=np.random.RandomState(5).random_sample)
        assert engines_made and (_hits(engines_made) > 0) == on     # six games share their first positions
    assert np.array_equal(results[False], results[True]), results
