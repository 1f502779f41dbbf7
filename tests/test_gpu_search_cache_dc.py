"""-m gpu: the evaluation cache in the one-launch search of a DragonChess engine (bb_config.search_cache with BB_LAUNCH_WAVE;
k_dc_search_wave<true>) against the lock-step loop and the one-launch search without it.  The entry is the network's WideHead --
the prior noise of the wide game is mixed in at expansion, per node -- so a hit leaves the wave what the tower would have, and
everything a caller can see is the lock-step engine's bit for bit; only evals / eval_cache_hits / eval_cache_probes differ:
probes == evals + hits == the evals of the same search without the cache."""
import numpy as np
import pytest

from blackbird_amd import _lib
from tests import search_cases as S

pytestmark = pytest.mark.gpu
DC = _lib.GAME_DRAGONCHESS
LOCK, WAVE = _lib.LAUNCH_LOCKSTEP, _lib.LAUNCH_WAVE


def _engine(n_slots, launch, blocks=2, **kw):
    return S.dc_engine(n_slots, launch, blocks, node_capacity=256, max_plies=24, **kw)


def _trio(n_slots, blocks=2, want=WAVE, **kw):
    return S.lock_and_wave(lambda launch, **k: _engine(n_slots, launch, blocks, **kw, **k), want, cached=True)


def _probing_nothing(snaps, what):
    S.same_trio(snaps, what, probing=False)


@pytest.mark.parametrize("n_slots", [1, 3])
def test_same_bits_over_two_moves(n_slots):
    engines = _trio(n_slots)
    S.set_roots_on(engines, S.dc_openings(n_slots))
    rng = np.random.RandomState(5)
    for move in range(2):
        snaps = S.step_and_compare(engines, 24, rng, S.edge_rows, what=(n_slots, move), check=S.same_trio)
        assert snaps[0][2]["overflow"] == 0 and snaps[0][2]["sims"] == (move + 1) * 24 * n_slots
        for e in engines:
            e.move_roots(S.sampled_moves(snaps[0]))
    S.close_all(*engines)


def _equal(a, b):
    try:
        S.assert_same(a, b, "", ignore_counters=tuple(a[2]))
    except AssertionError:
        return False
    return True


def test_second_pass_is_all_hits_and_a_reload_empties_the_table():
    """As tests/test_gpu_search_cache.py's: the same roots twice (nothing is evicted in between: at most 72 positions in 2^24
    entries -- two of them with the same 24 top bits of their digest is what it would take), then other weights."""
    cached = _engine(3, WAVE, search_cache=True)
    st, ids = S.dc_openings(3), S.game_ids(3)
    u = np.random.RandomState(12).random_sample(3)
    zero = cached.counters()
    cached.set_roots(st, game_ids=ids)
    cached.run_sims(24)
    first = S.snapshot(cached, 1.0, u, S.edge_rows)
    d1 = S.counter_delta(first[2], zero)
    assert d1["eval_cache_probes"] == d1["evals"] + d1["eval_cache_hits"] > 0
    cached.set_roots(st, game_ids=ids)
    cached.run_sims(24)
    second = S.snapshot(cached, 1.0, u, S.edge_rows)
    d2 = S.counter_delta(second[2], first[2])
    assert d2["evals"] == 0 and d2["eval_cache_hits"] == d2["eval_cache_probes"] == d1["eval_cache_probes"], (d1, d2)
    assert _equal(first, second)

    other = S.dc_weights(2, seed=22)
    cached.load_weights(other)
    cached.set_roots(st, game_ids=ids)
    cached.run_sims(1)    # each slot's first simulation evaluates its root: three positions the table held before the reload
    d3 = S.counter_delta(cached.counters(), second[2])
    assert d3 == {"evals": 3, "eval_cache_hits": 0, "eval_cache_probes": 3}, d3
    cached.run_sims(23)
    third = S.snapshot(cached, 1.0, u, S.edge_rows)
    fresh = _lib.Engine(DC, n_slots=3, launch=LOCK, node_capacity=256, max_plies=24, **S.SEARCH_KW, **S.NET_KW)   # has seen no other weights
    fresh.load_weights(other)
    fresh.set_roots(st, game_ids=ids)
    fresh.run_sims(24)
    want = S.snapshot(fresh, 1.0, u, S.edge_rows)
    assert _equal(want, third) and not _equal(want, first)
    d4 = S.counter_delta(third[2], second[2])
    assert d4["eval_cache_probes"] == d4["evals"] + d4["eval_cache_hits"] == want[2]["evals"], (d4, want[2])
    S.close_all(cached, fresh)


@pytest.mark.parametrize("case", ["nine_blocks", "net_form_f32"])
def test_uncovered_networks_search_lockstep_and_probe_nothing(case):
    kw = dict(blocks=9) if case == "nine_blocks" else dict(net_form=_lib.NET_FORM_F32)
    engines = _trio(3, want=LOCK, **kw)
    S.set_roots_on(engines, S.dc_openings(3))
    snaps = S.step_and_compare(engines, 8, np.random.RandomState(11), S.edge_rows, what=case, check=_probing_nothing)
    assert snaps[2][2]["sims"] == 3 * 8 and snaps[2][2]["evals"] > 0
    S.close_all(*engines)


def test_ancestors_and_reset_roots():
    engines = _trio(3, track_ancestors=True)
    S.set_roots_on(engines, S.dc_openings(3))
    rng = np.random.RandomState(9)
    for move in range(2):
        snaps = S.step_and_compare(engines, 24, rng, S.edge_rows, what=move, check=S.same_trio)
        for e in engines:
            e.move_roots(S.sampled_moves(snaps[0]))
    S.step_and_compare(engines, 24, rng, S.edge_rows, what="below", check=S.same_trio)
    for e in engines:
        e.reset_roots()
    top = [S.snapshot(e, 0.0, None, S.edge_rows) for e in engines]
    S.assert_same(top[0], top[1], "after reset", ignore_counters=S.CACHE_COUNTERS)
    S.assert_same(top[0], top[2], "after reset", ignore_counters=S.CACHE_COUNTERS)
    assert (top[0][0]["root_plays"] == 72).all()
    S.step_and_compare(engines, 8, rng, S.edge_rows, what="on the reset tree", check=S.same_trio)
    S.close_all(*engines)
