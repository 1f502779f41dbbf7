"""The evaluation cache of the persistent self-play kernel (Connect4, net.hip.h EvalCache) changes no result.

A hit replaces the tower and the heads by the value and priors stored when the same position was evaluated (before the
prior noise, which is drawn anew per node), so a batch played with the cache must store the very same bytes as one played
without it.  BB_EVAL_CACHE is read when an engine is created: one process compares both settings."""
import numpy as np
import pytest

from blackbird_amd import _lib, weights as W

pytestmark = pytest.mark.gpu

C4 = _lib.GAME_CONNECT4


def _weights(seed):
    return W.flatten(W.init_weights(3, 16, 4, 16, 7, seed=seed))


def _engine(monkeypatch, cache, slots, sims, max_games, log2=None):
    monkeypatch.setenv("BB_EVAL_CACHE", "1" if cache else "0")
    if log2 is not None:
        monkeypatch.setenv("BB_EVAL_CACHE_LOG2", str(log2))
    else:
        monkeypatch.delenv("BB_EVAL_CACHE_LOG2", raising=False)
    return _lib.Engine(C4, n_slots=slots, sims_per_move=sims, evaluator=_lib.EVAL_NET, c_puct=0.85, seed=1234,
                       noise_on=True, alpha=0.2, epsilon=0.3, max_games=max_games)


def _play(eng, flat, n_games):
    """load `flat`, play n_games to the end; (records, winners, counters)"""
    eng.load_weights(flat)
    eng.reset_counters()
    eng.selfplay_begin(n_games, 1.0)
    while not eng.selfplay_done()[0]:
        eng.selfplay_step(8)
    rec, offs, win = eng.fetch_examples()
    cnt = eng.counters()
    assert cnt["overflow"] == 0
    return rec, offs, win, cnt


def _same(a, b):
    ra, oa, wa, _ = a
    rb, ob, wb, _ = b
    assert np.array_equal(oa, ob) and np.array_equal(wa, wb)
    assert ra.tobytes() == rb.tobytes()


@pytest.mark.parametrize("slots,sims,n_games", [(256, 800, 256), (8192, 64, 8192)])
def test_same_records(monkeypatch, slots, sims, n_games):
    # (8192 slots: more workgroups than the chip holds at once)
    flat = _weights(0)
    res = {}
    for cache in (True, False):
        eng = _engine(monkeypatch, cache, slots, sims, n_games)
        try:
            res[cache] = _play(eng, flat, n_games)
        finally:
            eng.close()
    _same(res[True], res[False])
    on, off = res[True][3], res[False][3]
    assert off["eval_cache_hits"] == 0 and off["eval_cache_probes"] == 0
    assert on["eval_cache_hits"] > 0
    assert on["eval_cache_probes"] == on["evals"] + on["eval_cache_hits"]
    assert on["evals"] + on["eval_cache_hits"] == off["evals"]
    assert on["sims"] == off["sims"]


def test_small_table(monkeypatch):
    # a table of 1024 entries: most probes land on an entry of another position (a miss), results unchanged
    flat = _weights(0)
    res = {}
    for cache in (True, False):
        eng = _engine(monkeypatch, cache, 128, 200, 128, log2=10)
        try:
            res[cache] = _play(eng, flat, 128)
        finally:
            eng.close()
    _same(res[True], res[False])
    on = res[True][3]
    assert on["eval_cache_probes"] == on["evals"] + on["eval_cache_hits"]


def test_no_stale_entries(monkeypatch):
    # entries made with weights A must not answer for weights B
    fa, fb = _weights(0), _weights(1)
    eng = _engine(monkeypatch, True, 256, 200, 256)
    try:
        _play(eng, fa, 256)
        after = _play(eng, fb, 256)
    finally:
        eng.close()
    fresh = _engine(monkeypatch, True, 256, 200, 256)
    try:
        ref = _play(fresh, fb, 256)
    finally:
        fresh.close()
    _same(after, ref)
