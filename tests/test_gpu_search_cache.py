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
from blackbird_amd.MCTS import MCTS
from tests import model_cases as M
from tests import search_cases as S

pytestmark = pytest.mark.gpu
C4, TTT = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE
AUTO, LOCK, WAVE = _lib.LAUNCH_AUTO, _lib.LAUNCH_LOCKSTEP, _lib.LAUNCH_WAVE
NET = ("net", 16, 2)


def _engine(game, n_slots, launch, ev, **kw):
    return S.dense_engine(game, n_slots, launch, ev, node_capacity=512, **kw)


def _trio(game, n_slots):
    """Lock-step, wave, wave with search_cache: the same engine otherwise."""
    return S.lock_and_wave(lambda launch, **kw: _engine(game, n_slots, launch, NET, **kw), WAVE, cached=True)


def _model(game, name, seed):
    return M.model(game, name, seed=seed, play_limit=32, eps=0.3, blocks=2)


def _equal_trees(a, b, what):
    S.assert_same(a, b, what, ignore_counters=tuple(a[2]))


@pytest.mark.parametrize("sims", [2, 50])
@pytest.mark.parametrize("n_slots", [1, 3, 5])   # never a multiple of the four waves of a workgroup
def test_same_bits_over_three_moves(n_slots, sims):
    engines = _trio(C4, n_slots)
    S.set_roots_on(engines, S.openings(C4, n_slots))
    rng = np.random.RandomState(5)
    for move in range(3):
        snaps = S.step_and_compare(engines, sims, rng, S.view_rows, what=(n_slots, sims, move), check=S.same_trio)
        assert snaps[0][2]["overflow"] == 0 and snaps[0][2]["sims"] == (move + 1) * sims * n_slots
        for e in engines:
            e.move_roots(S.sampled_moves(snaps[0]))
    S.close_all(*engines)


def test_second_pass_is_all_hits_and_a_reload_empties_the_table():
    """The same roots searched twice: the second pass finds every position of the first.  (Assumes that nothing is evicted in
    between: at most 150 distinct positions in 2^26 two-way buckets -- a third position of one bucket is what it would take.)
    Then other weights: no entry of the first network may answer, so every position's first evaluation is a tower run and the
    trees are those of a fresh lock-step engine with the second weights."""
    cached = _engine(C4, 3, WAVE, NET, search_cache=True)
    st, ids = S.openings(C4, 3), S.game_ids(3)
    u = np.random.RandomState(12).random_sample(3)
    zero = cached.counters()
    cached.set_roots(st, game_ids=ids)
    cached.run_sims(50)
    first = S.snapshot(cached, 1.0, u, S.view_rows)
    d1 = S.counter_delta(first[2], zero)
    assert d1["eval_cache_probes"] == d1["evals"] + d1["eval_cache_hits"] > 0
    cached.set_roots(st, game_ids=ids)
    cached.run_sims(50)
    second = S.snapshot(cached, 1.0, u, S.view_rows)
    d2 = S.counter_delta(second[2], first[2])
    assert d2["evals"] == 0 and d2["eval_cache_hits"] == d2["eval_cache_probes"] == d1["eval_cache_probes"], (d1, d2)
    _equal_trees(first, second, "second pass")

    other = S.dense_weights(C4, 16, 2, seed=22)
    cached.load_weights(other)
    cached.set_roots(st, game_ids=ids)
    cached.run_sims(1)    # each slot's first simulation evaluates its root: three positions the table held before the reload
    d3 = S.counter_delta(cached.counters(), second[2])
    assert d3 == {"evals": 3, "eval_cache_hits": 0, "eval_cache_probes": 3}, d3
    cached.run_sims(49)
    third = S.snapshot(cached, 1.0, u, S.view_rows)
    fresh = _lib.Engine(C4, n_slots=3, launch=LOCK, node_capacity=512, **S.SEARCH_KW, **S.NET_KW)   # has seen no other weights
    fresh.load_weights(other)
    fresh.set_roots(st, game_ids=ids)
    fresh.run_sims(50)
    want = S.snapshot(fresh, 1.0, u, S.view_rows)
    _equal_trees(want, third, "other weights")
    ca = want[2]
    assert not np.array_equal(want[0]["child_value"], first[0]["child_value"])   # (the second network is another one)
    d4 = S.counter_delta(third[2], second[2])
    assert d4["eval_cache_probes"] == d4["evals"] + d4["eval_cache_hits"] == ca["evals"], (d4, ca)
    S.close_all(cached, fresh)


def test_masked_slots():
    engines = _trio(C4, 3)
    S.set_roots_on(engines, S.openings(C4, 3))
    rng = np.random.RandomState(7)
    for k, mask in enumerate((np.array([1, 0, 1], dtype=np.uint8), np.array([1, 1, 0], dtype=np.uint8))):
        before = engines[2].node_view(int(np.nonzero(mask == 0)[0][0]), -1)
        S.step_and_compare(engines, 20, rng, S.view_rows, mask=mask, what=k, check=S.same_trio)
        now = engines[2].node_view(int(np.nonzero(mask == 0)[0][0]), -1)
        assert all(np.array_equal(now[f], before[f]) for f in now), k
    S.close_all(*engines)


def test_endgame_roots(golden_dir):
    engines = _trio(C4, 5)
    S.set_roots_on(engines, S.endgame_roots(golden_dir, "c4"))
    rng = np.random.RandomState(6)
    for move in range(2):
        snaps = S.step_and_compare(engines, 50, rng, S.view_rows, what=move, check=S.same_trio)
        assert snaps[0][2]["terminal_leaves"] > 0 and snaps[0][2]["overflow"] == 0
        for e in engines:
            e.move_roots(S.sampled_moves(snaps[0]))
    S.close_all(*engines)


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
    S.set_roots_on((off, on), S.openings(game, 3))
    u = np.random.RandomState(11).random_sample(3)
    for e in (off, on):
        e.run_sims(50)
    a, b = S.snapshot(off, 1.0, u, S.view_rows), S.snapshot(on, 1.0, u, S.view_rows)
    S.assert_same(a, b, case, ignore_counters=S.CACHE_COUNTERS)
    assert a[2] == b[2] and b[2]["eval_cache_probes"] == 0 and b[2]["evals"] > 0, (case, a[2], b[2])
    S.close_all(off, on)


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
