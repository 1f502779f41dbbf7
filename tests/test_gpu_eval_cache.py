"""The evaluation cache of the persistent self-play kernel (Connect4, net.hip.h EvalCache) changes no result.

A hit replaces the tower and the heads by the value and priors stored when the same position was evaluated (before the
prior noise, which is drawn anew per node), so a batch played with the cache must store the very same bytes as one played
without it.  BB_EVAL_CACHE is read when an engine is created: one process compares both settings."""
import pytest

from blackbird_amd import _lib
from tests import selfplay_cases as SP

pytestmark = pytest.mark.gpu

C4 = _lib.GAME_CONNECT4


def _play(eng, flat, n_games):
    return SP.play_loaded(eng, flat, n_games, 8, mode=None)


@pytest.mark.parametrize("slots,sims,n_games", [(256, 800, 256), (8192, 64, 8192)])
def test_same_records(monkeypatch, slots, sims, n_games):
    # (8192 slots: more workgroups than the chip holds at once)
    flat = SP.c4_weights(16, 4, 0)
    res = {}
    for cache in (True, False):
        eng = SP.c4_engine_under_cache(monkeypatch, cache, slots, sims, n_games)
        try:
            res[cache] = _play(eng, flat, n_games)
        finally:
            eng.close()
    SP.assert_same_records(res[True], res[False], (slots, sims, n_games))
    on, off = res[True]["cnt"], res[False]["cnt"]
    SP.assert_cache_counters(on, off)
    assert on["eval_cache_hits"] > 0


def test_small_table(monkeypatch):
    # a table of 1024 entries: most probes land on an entry of another position (a miss), results unchanged
    flat = SP.c4_weights(16, 4, 0)
    res = {}
    for cache in (True, False):
        eng = SP.c4_engine_under_cache(monkeypatch, cache, 128, 200, 128, log2=10)
        try:
            res[cache] = _play(eng, flat, 128)
        finally:
            eng.close()
    SP.assert_same_records(res[True], res[False], "small table")
    on = res[True]["cnt"]
    assert on["eval_cache_probes"] == on["evals"] + on["eval_cache_hits"]


def test_no_stale_entries(monkeypatch):
    # entries made with weights A must not answer for weights B
    fa, fb = SP.c4_weights(16, 4, 0), SP.c4_weights(16, 4, 1)
    eng = SP.c4_engine_under_cache(monkeypatch, True, 256, 200, 256)
    try:
        _play(eng, fa, 256)
        after = _play(eng, fb, 256)
    finally:
        eng.close()
    fresh = SP.c4_engine_under_cache(monkeypatch, True, 256, 200, 256)
    try:
        ref = _play(fresh, fb, 256)
    finally:
        fresh.close()
    SP.assert_same_records(after, ref, "after a reload")
