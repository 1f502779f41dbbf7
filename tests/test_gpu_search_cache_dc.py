"""-m gpu: the evaluation cache in the one-launch search of a DragonChess engine (bb_config.search_cache with BB_LAUNCH_WAVE;
k_dc_search_wave<true>) against the lock-step loop and the one-launch search without it.  The entry is the network's WideHead --
the prior noise of the wide game is mixed in at expansion, per node -- so a hit leaves the wave what the tower would have, and
everything a caller can see is the lock-step engine's bit for bit; only evals / eval_cache_hits / eval_cache_probes differ:
probes == evals + hits == the evals of the same search without the cache."""
import numpy as np
import pytest

from blackbird_amd import _lib
from blackbird_amd import weights as W
from tests.test_gpu_search_wave_dc import _engine, _openings, _snap

pytestmark = pytest.mark.gpu
DC = _lib.GAME_DRAGONCHESS
LOCK, WAVE = _lib.LAUNCH_LOCKSTEP, _lib.LAUNCH_WAVE
CACHE_COUNTERS = ("evals", "eval_cache_hits", "eval_cache_probes")


def _trio(n_slots, blocks=2, want=WAVE, **kw):
    lock, wave = _engine(n_slots, LOCK, blocks, **kw), _engine(n_slots, WAVE, blocks, **kw)
    cached = _engine(n_slots, WAVE, blocks, search_cache=True, **kw)
    assert lock.run_sims_structure() == LOCK and wave.run_sims_structure() == want and cached.run_sims_structure() == want
    return lock, wave, cached


def _set(engines, states):
    for e in engines:
        e.set_roots(states, game_ids=7 * np.arange(len(states)) + 3)


def _close(*engines):
    for e in engines:
        e.close()


def _same_trees(a, b, what=""):
    (oa, ra, ca), (ob, rb, cb) = a, b
    for k in oa:
        assert oa[k].tobytes() == ob[k].tobytes(), (what, k, oa[k], ob[k])
    assert len(ra) == len(rb), what
    for i, (x, y) in enumerate(zip(ra, rb)):
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), (what, "node", i, k, x[k], y[k])
    rest = lambda c: {k: v for k, v in c.items() if k not in CACHE_COUNTERS}
    assert rest(ca) == rest(cb), (what, ca, cb)


def _step(engines, sims, rng, what="", probing=True):
    u = rng.random_sample(engines[0].n_slots)
    for e in engines:
        e.run_sims(sims)
    a, b, c = snaps = [_snap(e, 1.0, u) for e in engines]
    _same_trees(a, b, what)
    _same_trees(a, c, what)
    assert a[2] == b[2] and a[2]["eval_cache_hits"] == 0 and a[2]["eval_cache_probes"] == 0, (what, a[2], b[2])
    if probing:
        assert c[2]["eval_cache_probes"] == c[2]["evals"] + c[2]["eval_cache_hits"] == a[2]["evals"], (what, a[2], c[2])
    else:
        assert c[2] == a[2], (what, a[2], c[2])
    return snaps


def _moves(snapshot):
    return np.where(snapshot[0]["action"] >= 0, snapshot[0]["action"], -1).astype(np.int32)


@pytest.mark.parametrize("n_slots", [1, 3])
def test_same_bits_over_two_moves(n_slots):
    engines = _trio(n_slots)
    _set(engines, _openings(n_slots))
    rng = np.random.RandomState(5)
    for move in range(2):
        snaps = _step(engines, 24, rng, what=(n_slots, move))
        assert snaps[0][2]["overflow"] == 0 and snaps[0][2]["sims"] == (move + 1) * 24 * n_slots
        for e in engines:
            e.move_roots(_moves(snaps[0]))
    _close(*engines)


def _delta(after, before):
    return {k: after[k] - before[k] for k in CACHE_COUNTERS}


def _equal(a, b):
    (oa, ra, _), (ob, rb, _) = a, b
    return (all(oa[k].tobytes() == ob[k].tobytes() for k in oa) and len(ra) == len(rb) and
            all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for x, y in zip(ra, rb) for k in x))


def test_second_pass_is_all_hits_and_a_reload_empties_the_table():
    """As tests/test_gpu_search_cache.py's: the same roots twice (nothing is evicted in between: at most 72 positions in 2^24
    entries -- two of them with the same 24 top bits of their digest is what it would take), then other weights."""
    cached = _engine(3, WAVE, search_cache=True)
    st, ids = _openings(3), 7 * np.arange(3) + 3
    u = np.random.RandomState(12).random_sample(3)
    zero = cached.counters()
    cached.set_roots(st, game_ids=ids)
    cached.run_sims(24)
    first = _snap(cached, 1.0, u)
    d1 = _delta(first[2], zero)
    assert d1["eval_cache_probes"] == d1["evals"] + d1["eval_cache_hits"] > 0
    cached.set_roots(st, game_ids=ids)
    cached.run_sims(24)
    second = _snap(cached, 1.0, u)
    d2 = _delta(second[2], first[2])
    assert d2["evals"] == 0 and d2["eval_cache_hits"] == d2["eval_cache_probes"] == d1["eval_cache_probes"], (d1, d2)
    assert _equal(first, second)

    other = W.flatten(W.init_weights(17, 16, 2, 16, 4032, seed=22, perturb=True))
    cached.load_weights(other)
    cached.set_roots(st, game_ids=ids)
    cached.run_sims(1)    # each slot's first simulation evaluates its root: three positions the table held before the reload
    d3 = _delta(cached.counters(), second[2])
    assert d3 == {"evals": 3, "eval_cache_hits": 0, "eval_cache_probes": 3}, d3
    cached.run_sims(23)
    third = _snap(cached, 1.0, u)
    fresh = _lib.Engine(DC, n_slots=3, sims_per_move=8, seed=17, first_game_id=1000, launch=LOCK, evaluator=_lib.EVAL_NET,
                        noise_on=True, alpha=0.2, epsilon=0.3, node_capacity=256, max_plies=24)
    fresh.load_weights(other)
    fresh.set_roots(st, game_ids=ids)
    fresh.run_sims(24)
    want = _snap(fresh, 1.0, u)
    assert _equal(want, third) and not _equal(want, first)
    d4 = _delta(third[2], second[2])
    assert d4["eval_cache_probes"] == d4["evals"] + d4["eval_cache_hits"] == want[2]["evals"], (d4, want[2])
    _close(cached, fresh)


@pytest.mark.parametrize("case", ["nine_blocks", "net_form_f32"])
def test_uncovered_networks_search_lockstep_and_probe_nothing(case):
    kw = dict(blocks=9) if case == "nine_blocks" else dict(net_form=_lib.NET_FORM_F32)
    engines = _trio(3, want=LOCK, **kw)
    _set(engines, _openings(3))
    snaps = _step(engines, 8, np.random.RandomState(11), what=case, probing=False)
    assert snaps[2][2]["sims"] == 3 * 8 and snaps[2][2]["evals"] > 0
    _close(*engines)


def test_ancestors_and_reset_roots():
    engines = _trio(3, track_ancestors=True)
    _set(engines, _openings(3))
    rng = np.random.RandomState(9)
    for move in range(2):
        snaps = _step(engines, 24, rng, what=move)
        for e in engines:
            e.move_roots(_moves(snaps[0]))
    _step(engines, 24, rng, what="below")
    for e in engines:
        e.reset_roots()
    top = [_snap(e, 0.0) for e in engines]
    _same_trees(top[0], top[1], "after reset")
    _same_trees(top[0], top[2], "after reset")
    assert (top[0][0]["root_plays"] == 72).all()
    _step(engines, 8, rng, what="on the reset tree")
    _close(*engines)
